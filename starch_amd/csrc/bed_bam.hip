// starch_amd/csrc/bed_bam.hip -- bam2bed on MI355X: inflated BAM into the BED lines
// that sam2bed (bed_align.hip) writes for its SAM text (the definition:
// include/starch_amd.h; the argument for the framing: DESIGN.md section 21).
//   1. header: the one round trip.  The header's bytes are read back and its short
//      serial chain (text, reference names) is walked on the host; the reference
//      names return to HBM as offsets and bytes, a kept header line as its place
//      in the input and in the output.
//   2. framing.  Records are length-prefixed and aligned to nothing, so record k's
//      offset depends on every record before it.  The file is cut into tiles of
//      T = kTileBytes.  k_bam_table, one block per tile: next(i) = i + 4 + u32(i)
//      for EVERY byte offset i of the tile (itself where that u32 is below 32 or
//      next leaves the tile), pointer-doubled in LDS to last(i), the last offset
//      in the tile on the chain from i; 16 bits per byte, written to HBM for
//      kBatchTiles tiles at a time.  k_bam_tiles, one thread: the entry of the
//      next tile is next(last(entry)), one table load and one input load per
//      TILE; it carries its place from batch to batch in device memory and checks
//      the record that leaves each tile.  k_bam_chain, one wave per tile: the
//      tile staged in LDS and its chain walked from its entry, once to count the
//      records and, after an exclusive sum, once to write their 64-bit offsets.
//      Every stage is a launch of its own on the stream: no workgroup waits for
//      another.
//   3. k_bam_classify, one thread per record: the record against its own counts,
//      its CIGAR and the grammar of its tags; start, stop and the runs of a split
//      record; the bytes of its SAM columns from CIGAR on.  k_bam_write, after
//      br::place: its output lines, round after round across the wave as in
//      k_al_write.  The walks over CIGAR and tags are the same code in both
//      (Emit: count or write).  A record whose l_seq or largest B count reaches
//      W = kWaveThreshold leaves those columns to its whole wave in both kernels:
//      SEQ and QUAL a lane per base, an array a lane per element with a wave scan.
// All arithmetic is integer.  A thread reads only bytes of its own record, which
// the framing has shown to lie inside the input, and writes only its placed range.
#include "bed_bam.hpp"

#include <string.h>

#include <algorithm>
#include <vector>

namespace bam {
namespace {

using br::S_BAD, br::S_FLAG, br::S_OWN, br::S_HDR, br::S_REC, br::S_LINES, br::S_BYTES, br::C_BAD, br::C_TOOL;
using br::K_ZERO, br::K_TOOL;
using br::dec_digits, br::Writer, br::reset_and_bind, br::first_of, br::First, br::place, br::Placed;

enum : int { S_WAVE = S_FLAG, S_DROPPED = S_OWN };   // records left to a wave; unmapped records left out
enum : uint8_t { C_REC = C_TOOL, C_SPLIT, C_UNMAPPED, C_DROPPED };
enum : uint32_t { K_SHORT = K_TOOL, K_PAST, K_COUNTS, K_NAME, K_REF, K_CIGAR, K_TAGTYPE, K_TAGS, K_RNAME };
enum : uint32_t { O_CG = 0, O_BIG = 1, kSlots = 2 };   // Rec::fo: where the CG tag that holds the CIGAR starts (0: none); left to a wave
enum : int { F_CUR = 0, F_STOP, F_KIND, F_COUNT = 4 };   // the tile walk's state: where it stands, where the chain ends and how
constexpr uint32_t T = kTileBytes;
constexpr uint32_t kNoEntry = 0xffffffffu;

constexpr int doubling_rounds()   // 2^rounds hops reach the end of the longest chain in a tile
{
    int r = 0;
    while ((1u << r) < (T + kMinRecord - 1) / kMinRecord) ++r;
    return r;
}
constexpr int kRounds = doubling_rounds();
static_assert(T <= 65536 && T % kTableThreads == 0 && T % 16 == 0, "a 16-bit index per byte of a tile");
static_assert(kRounds == 9, "16 KiB of records of 36 bytes or more: at most 456 hops");

struct Rec : br::Rec {     // line_end and hflag are unused: records are found through rec_off, header lines written apart
    const uint64_t* rec_off;
    uint64_t* rest;        // bytes of the columns from CIGAR on
    const uint32_t* name_off;
    const uint8_t* names;
    int32_t n_ref;
    uint32_t split, split_deletions, all_reads, reduced;
    uint64_t out_base;     // the bytes of the kept header lines, which come first
};

struct Tally {             // what k_br_tally counts
    static constexpr uint32_t kOwn = C_DROPPED;
    static __device__ bool record(uint32_t c) { return c >= C_REC; }
};

__device__ __forceinline__ uint32_t ld16(const uint8_t* __restrict__ s) { return (uint32_t)s[0] | ((uint32_t)s[1] << 8); }
__device__ __forceinline__ uint32_t ld32(const uint8_t* __restrict__ s) { return ld16(s) | (ld16(s + 2) << 16); }

// ---- 2. framing ---------------------------------------------------------------------------
// The bytes [base, base + avail) of the input into LDS by aligned dwords: byte i
// is byte mis + i of lds.  (A dword that holds one byte of the input is read whole.)
__device__ __forceinline__ uint32_t stage_tile(const uint8_t* __restrict__ in, uint64_t base, uint32_t avail, uint32_t* lds, int tid,
                                               int threads)
{
    const uint8_t* b = in + base;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(b) & 3u);
    const uint32_t* ap = reinterpret_cast<const uint32_t*>(b - mis);
    const uint32_t ndw = (mis + avail + 3) / 4;
    for (uint32_t k = tid; k < ndw; k += threads) lds[k] = ap[k];
    return mis;
}

__device__ __forceinline__ uint32_t lds32(const uint32_t* lds, uint32_t at)   // the u32 at byte `at`, which need not be aligned
{
    const uint64_t w = (uint64_t)lds[at >> 2] | ((uint64_t)lds[(at >> 2) + 1] << 32);
    return (uint32_t)(w >> ((at & 3u) * 8));
}

__device__ __forceinline__ uint32_t tile_avail(uint64_t base, uint64_t n) { return (uint32_t)(n - base < T + 3 ? n - base : T + 3); }

// last(i) for every offset i of the tiles t0 + blockIdx.x
__global__ void __launch_bounds__(kTableThreads) k_bam_table(const uint8_t* __restrict__ in, uint64_t n, uint64_t t0,
                                                            uint16_t* __restrict__ tab)
{
    // the staged tile (T + 3 bytes and up to 3 before them), and then, over it, the table
    __shared__ uint32_t lds[T / 2];
    constexpr int kPer = T / kTableThreads;
    const int tid = threadIdx.x;
    const uint64_t base = (t0 + blockIdx.x) * T;
    const uint32_t avail = tile_avail(base, n), len = avail < T ? avail : T;
    const uint32_t mis = stage_tile(in, base, avail, lds, tid, kTableThreads);
    __syncthreads();
    uint16_t nx[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const uint32_t i = tid + k * kTableThreads;
        uint32_t v = i;
        if (i + 4 <= avail && i < len) {
            const uint32_t bs = lds32(lds, mis + i);
            const uint64_t nxt = (uint64_t)i + 4 + bs;
            if (bs >= kMinRecord - 4 && nxt < len) v = (uint32_t)nxt;
        }
        nx[k] = (uint16_t)v;
    }
    __syncthreads();
    uint16_t* t16 = reinterpret_cast<uint16_t*>(lds);
#pragma unroll
    for (int k = 0; k < kPer; ++k) t16[tid + k * kTableThreads] = nx[k];
    __syncthreads();
    for (int round = 0; round < kRounds; ++round) {
#pragma unroll
        for (int k = 0; k < kPer; ++k) nx[k] = t16[nx[k]];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPer; ++k) t16[tid + k * kTableThreads] = nx[k];
        __syncthreads();
    }
    uint16_t* o = tab + (uint64_t)blockIdx.x * T;
#pragma unroll
    for (int k = 0; k < kPer; ++k) o[tid + k * kTableThreads] = nx[k];
}

// The walk over the tiles [t0, t1), whose tables are in tab: one thread.  fs
// carries it from batch to batch.  The record that leaves a tile (or ends the
// chain) is checked here: the others have their next inside the tile.
__global__ void k_bam_tiles(const uint8_t* __restrict__ in, uint64_t n, uint64_t t0, uint64_t t1, const uint16_t* __restrict__ tab,
                            uint32_t* __restrict__ entry, unsigned long long* __restrict__ fs)
{
    if (threadIdx.x || fs[F_STOP] != ~0ull) return;
    uint64_t cur = fs[F_CUR], kind = 0;
    for (;;) {
        if (cur == n) break;                       // the chain ends exactly at the end of the input
        const uint64_t tile = cur / T;
        if (tile >= t1) { fs[F_CUR] = cur; return; }
        const uint32_t i = (uint32_t)(cur % T);
        entry[tile] = i;
        cur = tile * T + tab[(tile - t0) * T + i];
        if (cur + 4 > n) { kind = K_PAST; break; }
        const uint32_t bs = ld32(in + cur);
        if (bs < kMinRecord - 4) { kind = K_SHORT; break; }
        if (cur + 4 + bs > n) { kind = K_PAST; break; }
        cur += 4 + (uint64_t)bs;
    }
    fs[F_STOP] = cur;                              // the first offset that is not a good record's
    fs[F_KIND] = kind;
}

// One wave per tile: the records that start in it, from its entry and before the
// chain's end; counted, or with kWrite their offsets written from place[tile] on.
template <bool kWrite>
__global__ void __launch_bounds__(64) k_bam_chain(const uint8_t* __restrict__ in, uint64_t n, const uint32_t* __restrict__ entry,
                                                  const unsigned long long* __restrict__ fs, uint32_t* __restrict__ count,
                                                  const uint64_t* __restrict__ place, uint64_t* __restrict__ rec_off)
{
    __shared__ uint32_t lds[T / 4 + 2];
    const uint64_t tile = blockIdx.x, base = tile * T;
    const uint32_t e = entry[tile];
    if (e == kNoEntry) {
        if (!kWrite && threadIdx.x == 0) count[tile] = 0;
        return;
    }
    const uint32_t mis = stage_tile(in, base, tile_avail(base, n), lds, threadIdx.x, 64);
    __syncthreads();
    if (threadIdx.x) return;
    const uint64_t stop = fs[F_STOP], at = kWrite ? place[tile] : 0;
    uint32_t c = 0;
    for (uint64_t p = e; p < T && base + p < stop; ++c) {
        if (kWrite) rec_off[at + c] = base + p;
        p += 4 + (uint64_t)lds32(lds, mis + (uint32_t)p);
    }
    if (!kWrite) count[tile] = c;
}

// ---- 3. a record ----------------------------------------------------------------------------
struct Head {              // the fixed fields of a record and where its parts begin
    const uint8_t *s, *name, *cigar, *seq, *qual, *tags, *end;
    int32_t ref, pos, next_ref, next_pos, tlen;
    uint32_t l_name, mapq, n_cigar, flag, l_seq;
};

// the record at s; 0, or K_COUNTS when it does not hold what its counts announce
__device__ __forceinline__ uint32_t read_head(const uint8_t* __restrict__ s, Head& h)
{
    const uint32_t bs = ld32(s);
    h.s = s;
    h.ref = (int32_t)ld32(s + 4);
    h.pos = (int32_t)ld32(s + 8);
    h.l_name = s[12];
    h.mapq = s[13];
    h.n_cigar = ld16(s + 16);
    h.flag = ld16(s + 18);
    h.l_seq = ld32(s + 20);
    h.next_ref = (int32_t)ld32(s + 24);
    h.next_pos = (int32_t)ld32(s + 28);
    h.tlen = (int32_t)ld32(s + 32);
    h.name = s + 36;
    h.cigar = h.name + h.l_name;
    h.seq = h.cigar + 4ull * h.n_cigar;
    h.qual = h.seq + ((uint64_t)h.l_seq + 1) / 2;
    h.tags = h.qual + h.l_seq;
    h.end = s + 4 + (uint64_t)bs;
    return 32ull + h.l_name + 4ull * h.n_cigar + ((uint64_t)h.l_seq + 1) / 2 + h.l_seq > bs ? (uint32_t)K_COUNTS : 0u;
}

__device__ __forceinline__ uint32_t elem_size(uint32_t t)   // bytes of a value of type t; 0: no such type
{
    return t == 'c' || t == 'C' || t == 'A' ? 1u : (t == 's' || t == 'S' ? 2u : (t == 'i' || t == 'I' || t == 'f' ? 4u : 0u));
}

struct Tag {
    const uint8_t *at, *val;   // the tag's first byte; its value, a B array's first element
    uint32_t type, sub, count; // sub and count of a B array; count of Z and H: their bytes without the NUL
};

// the tag at p, which is below end; p moves past it.  0, or K_TAGTYPE, K_TAGS
__device__ __forceinline__ uint32_t tag_next(const uint8_t*& p, const uint8_t* end, Tag& t)
{
    if (end - p < 4) return K_TAGS;
    t.at = p;
    t.type = p[2];
    t.val = p += 3;
    t.sub = t.count = 0;
    uint64_t bytes = elem_size(t.type);
    if (t.type == 'Z' || t.type == 'H') {
        while (p < end && *p) ++p;
        if (p == end) return K_TAGS;
        t.count = (uint32_t)(p - t.val);
        ++p;
        return 0;
    }
    if (t.type == 'B') {
        if (end - p < 5) return K_TAGS;
        t.sub = p[0];
        t.count = ld32(p + 1);
        t.val = p += 5;
        const uint32_t es = t.sub == 'A' ? 0u : elem_size(t.sub);
        if (!es) return K_TAGTYPE;
        bytes = (uint64_t)es * t.count;
    } else if (!bytes) return K_TAGTYPE;
    if ((uint64_t)(end - p) < bytes) return K_TAGS;
    p += bytes;
    return 0;
}

// the text of one value of type t at v into b (12 bytes at most); returns its length
__device__ __forceinline__ uint32_t value_text(uint32_t t, const uint8_t* __restrict__ v, uint8_t* b)
{
    if (t == 'f') return float_g(ld32(v), b);
    int64_t x;
    switch (t) {
        case 'c': x = (int8_t)v[0]; break;
        case 'C': x = v[0]; break;
        case 's': x = (int16_t)ld16(v); break;
        case 'S': x = ld16(v); break;
        case 'i': x = (int32_t)ld32(v); break;
        default: x = ld32(v); break;
    }
    uint32_t n = 0;
    if (x < 0) { b[n++] = '-'; x = -x; }
    const uint32_t d = dec_digits((uint64_t)x);
    bt::put_dec(b + n, (uint64_t)x, d);
    return n + d;
}

constexpr uint32_t kCigarElem = 'G';   // an element of a CIGAR: count and operator, no comma
__device__ __forceinline__ uint32_t elem_text(uint32_t t, const uint8_t* __restrict__ v, uint8_t* b)
{
    if (t == kCigarElem) {
        const uint32_t x = ld32(v), d = dec_digits(x >> 4);
        bt::put_dec(b, x >> 4, d);
        b[d] = (uint8_t)"MIDNSHP=X???????"[x & 15u];
        return d + 1;
    }
    b[0] = ',';
    return 1 + value_text(t, v, b + 1);
}

// The cursor of the walks over a record's text: it counts, or with kWrite writes.
// kWave: every lane of the wave runs the same walk on one record; single bytes
// are lane 0's, the bases and the elements of an array go a lane each.
template <bool kWave, bool kWrite>
struct Emit {
    uint8_t* out;
    uint64_t o;
    int lane;
    __device__ __forceinline__ void ch(uint8_t c)
    {
        if (kWrite && (!kWave || lane == 0)) out[o] = c;
        ++o;
    }
    __device__ __forceinline__ void bytes(const uint8_t* __restrict__ s, uint64_t n)
    {
        if (kWrite)
            for (uint64_t p = kWave ? lane : 0; p < n; p += kWave ? 64 : 1) out[o + p] = s[p];
        o += n;
    }
    __device__ __forceinline__ void sdec(int64_t x)
    {
        if (x < 0) { ch('-'); x = -x; }
        const uint32_t d = dec_digits((uint64_t)x);
        if (kWrite && (!kWave || lane == 0)) bt::put_dec(out + o, (uint64_t)x, d);
        o += d;
    }
    __device__ __forceinline__ void seq(const uint8_t* __restrict__ s, uint32_t n)
    {
        if (kWrite)
            for (uint32_t p = kWave ? lane : 0; p < n; p += kWave ? 64 : 1)
                out[o + p] = (uint8_t)"=ACMGRSVTWYHKDBN"[(s[p >> 1] >> ((~p & 1u) * 4)) & 15u];
        o += n;
    }
    __device__ __forceinline__ void qual(const uint8_t* __restrict__ s, uint32_t n)
    {
        if (kWrite)
            for (uint32_t p = kWave ? lane : 0; p < n; p += kWave ? 64 : 1) out[o + p] = (uint8_t)(s[p] + 33);
        o += n;
    }
    // count elements of type t (or kCigarElem) from v on
    __device__ __forceinline__ void array(uint32_t t, const uint8_t* __restrict__ v, uint32_t count)
    {
        const uint32_t es = t == kCigarElem ? 4u : elem_size(t);
        uint8_t b[16];
        if (kWave) {
            for (uint32_t k0 = 0; k0 < count; k0 += 64) {   // (count is the same in every lane)
                const uint32_t k = k0 + lane;
                const uint32_t len = k < count ? elem_text(t, v + (uint64_t)k * es, b) : 0u;
                const uint32_t incl = wave_incl_scan_add<uint32_t>(len);
                if (kWrite)
                    for (uint32_t j = 0; j < len; ++j) out[o + incl - len + j] = b[j];
                o += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
        } else {
            for (uint32_t k = 0; k < count; ++k) {
                const uint32_t len = elem_text(t, v + (uint64_t)k * es, b);
                if (kWrite)
                    for (uint32_t j = 0; j < len; ++j) out[o + j] = b[j];
                o += len;
            }
        }
    }
};

// the CIGAR of a record: its own operators, or the array of the CG tag at h.s + cg
__device__ __forceinline__ const uint8_t* cigar_of(const Head& h, uint32_t cg, uint32_t* count)
{
    if (!cg) { *count = h.n_cigar; return h.cigar; }
    *count = ld32(h.s + cg + 4);
    return h.s + cg + 8;
}

// The SAM columns of a checked record from CIGAR on, without the TAB before them
// and the '\n' after: returns their bytes.
template <bool kWave, bool kWrite>
__device__ __forceinline__ uint64_t rest_text(const Rec& r, const Head& h, uint32_t cg, uint8_t* out, uint64_t at, int lane)
{
    Emit<kWave, kWrite> w{out, at, lane};
    uint32_t nc = 0;
    const uint8_t* c = cigar_of(h, cg, &nc);
    if (nc) w.array(kCigarElem, c, nc);
    else w.ch('*');
    w.ch('\t');
    if (h.next_ref < 0) w.ch('*');
    else if (h.next_ref == h.ref) w.ch('=');
    else w.bytes(r.names + r.name_off[h.next_ref], r.name_off[h.next_ref + 1] - r.name_off[h.next_ref]);
    w.ch('\t');
    w.sdec((int64_t)h.next_pos + 1);
    w.ch('\t');
    w.sdec(h.tlen);
    w.ch('\t');
    if (h.l_seq) w.seq(h.seq, h.l_seq);
    else w.ch('*');
    w.ch('\t');
    if (h.l_seq && h.qual[0] != 0xff) w.qual(h.qual, h.l_seq);
    else w.ch('*');
    Tag t;
    for (const uint8_t* p = h.tags; p < h.end;) {
        (void)tag_next(p, h.end, t);   // checked when the record was classified
        if (cg && t.at == h.s + cg) continue;
        w.ch('\t');
        w.ch(t.at[0]);
        w.ch(t.at[1]);
        w.ch(':');
        const bool integer = t.type != 'A' && t.type != 'f' && t.type != 'Z' && t.type != 'H' && t.type != 'B';
        w.ch(integer ? 'i' : (uint8_t)t.type);
        w.ch(':');
        if (t.type == 'A') w.ch(t.val[0]);
        else if (t.type == 'Z' || t.type == 'H') w.bytes(t.val, t.count);
        else if (t.type == 'B') {
            w.ch((uint8_t)t.sub);
            w.array(t.sub, t.val, t.count);
        } else {
            uint8_t b[16];
            const uint32_t len = value_text(t.type, t.val, b);
            if (kWrite && (!kWave || lane == 0))
                for (uint32_t j = 0; j < len; ++j) w.out[w.o + j] = b[j];
            w.o += len;
        }
    }
    return w.o - at;
}

struct RunWalk {           // where the walk over the CIGAR stands: the next operator, and the run of M D = X it is in
    uint32_t k;
    uint64_t at, len;
};

// The next maximal run of M D = X with positive length: [*a, *b), or false at the
// end of the CIGAR (then w.at is the position after its last reference base).  N
// ends a run, D too with split_deletions.  (sam_next_run of bed_align.hip on
// binary operators, which were checked before.)
__device__ __forceinline__ bool next_run(const uint8_t* __restrict__ c, uint32_t nc, RunWalk& w, bool split_deletions, uint64_t* a,
                                         uint64_t* b)
{
    for (;;) {
        const bool last = w.k == nc;
        const uint32_t x = last ? 0u : ld32(c + 4ull * w.k), op = x & 15u;
        const uint64_t n = x >> 4;
        if (!last) ++w.k;
        if (last || op == 3 || (split_deletions && op == 2)) {
            const bool run = w.len != 0;
            *a = w.at;
            *b = w.at + w.len;
            w.at += w.len + (last ? 0 : n);   // a position below 2^31 and fewer than 2^30 counts below 2^28: below 2^59
            w.len = 0;
            if (run) return true;
            if (last) return false;
        } else if (op == 0 || op == 2 || op == 7 || op == 8) {
            w.len += n;
        }
    }
}

// the reference name of a mapped record, its length in *n
__device__ __forceinline__ const uint8_t* rname_of(const Rec& r, int32_t ref, uint32_t* n)
{
    *n = r.name_off[ref + 1] - r.name_off[ref];
    return r.names + r.name_off[ref];
}

struct Line : br::Line<kSlots> {
    uint64_t rest = 0;
};

// a record against the definition; what it writes, except the bytes of a wave record's columns
__device__ __forceinline__ void classify(const Rec& r, const uint8_t* __restrict__ s, Head& h, Line& ln)
{
    if ((ln.kind = read_head(s, h))) return;
    if (h.l_name < 1 || h.name[h.l_name - 1] != 0) { ln.kind = K_NAME; return; }
    if (h.ref < -1 || h.ref >= r.n_ref || h.next_ref < -1 || h.next_ref >= r.n_ref) { ln.kind = K_REF; return; }
    for (uint32_t k = 0; k < h.n_cigar; ++k)
        if ((h.cigar[4ull * k] & 15u) > 8u) { ln.kind = K_CIGAR; return; }
    // the grammar of the tags; the first CG:B:I; the largest array
    uint32_t cg = 0, most = 0;
    Tag t;
    for (const uint8_t* p = h.tags; p < h.end;) {
        if ((ln.kind = tag_next(p, h.end, t))) return;
        if (t.type == 'B' && t.count > most) most = t.count;
        if (!cg && t.type == 'B' && t.sub == 'I' && t.at[0] == 'C' && t.at[1] == 'G') cg = (uint32_t)(t.at - s);
    }
    if (!(cg && h.n_cigar == 2 && ld32(h.cigar) == ((h.l_seq << 4) | 4u) && h.l_seq < (1u << 28) && (h.cigar[4] & 15u) == 3u)) cg = 0;
    uint32_t nc = 0;
    const uint8_t* c = cigar_of(h, cg, &nc);
    if (cg)
        for (uint32_t k = 0; k < nc; ++k)
            if ((c[4ull * k] & 15u) > 8u) { ln.kind = K_CIGAR; return; }
    ln.fo[O_CG] = cg;
    ln.fo[O_BIG] = h.l_seq >= kWaveThreshold || most >= kWaveThreshold;
    uint64_t start = 0, stop = 1, digits = 0;
    uint32_t cnt = 1, cls = C_REC, rname = 9;   // _unmapped
    if (h.flag & 4u) {
        if (!r.all_reads) { ln.cls = C_DROPPED; return; }
        cls = C_UNMAPPED;
    } else {
        if (h.ref < 0) { ln.kind = K_RNAME; return; }
        const uint8_t* name = rname_of(r, h.ref, &rname);
        if (rname == 0 || (rname == 1 && name[0] == '*')) { ln.kind = K_RNAME; return; }
        if (h.pos < 0) { ln.kind = K_ZERO; return; }
        start = (uint64_t)h.pos;
        uint32_t runs = 0;
        RunWalk w{0, start, 0};
        uint64_t ra = 0, rb = 0;
        while (next_run(c, nc, w, r.split_deletions != 0, &ra, &rb)) {
            ++runs;
            digits += dec_digits(ra) + dec_digits(rb);
        }
        stop = w.at > start ? w.at : start + 1;
        if (r.split && runs) {
            cls = C_SPLIT;
            cnt = runs;
        }
    }
    if (cls != C_SPLIT) digits = dec_digits(start) + dec_digits(stop);
    ln.cls = cls;
    ln.a = start;
    ln.b = stop;
    ln.cnt = cnt;
    // RNAME start stop QNAME FLAG strand: five TABs, the strand, and '\n'; the rest is added when it is known
    ln.ob = (uint64_t)cnt * ((uint64_t)rname + (h.l_name - 1) + dec_digits(h.flag) + 7) + digits;
}

// bytes of a line after the strand, without the '\n': TAB MAPQ TAB and the columns from CIGAR on
__device__ __forceinline__ uint64_t tail_bytes(const Head& h, uint64_t rest) { return 2ull + dec_digits(h.mapq) + rest; }

__global__ void __launch_bounds__(kThreads) k_bam_classify(const Rec r)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < r.L;
    const uint8_t* s = valid ? r.in + r.rec_off[i] : nullptr;
    Head h{};
    Line ln;
    if (valid) classify(r, s, h, ln);
    const bool text = valid && !ln.kind && !r.reduced && ln.cls >= C_REC && ln.cls != C_DROPPED;
    const bool big = text && ln.fo[O_BIG];
    if (text && !big) ln.rest = rest_text<false, false>(r, h, ln.fo[O_CG], nullptr, 0, lane);
    unsigned long long m = __ballot(big);
    const uint32_t nbig = __popcll(__ballot(valid && !ln.kind && ln.fo[O_BIG]));
    if (lane == 0 && nbig) atomicAdd(&r.scal[S_WAVE], (unsigned long long)nbig);
    while (m) {            // a wave record: its columns measured by the whole wave
        const int l = __ffsll(m) - 1;
        m &= m - 1;
        const uint64_t at = __shfl(valid ? r.rec_off[i] : 0ull, l, 64);
        const uint32_t cg = __shfl(ln.fo[O_CG], l, 64);
        Head hw;
        (void)read_head(r.in + at, hw);
        const uint64_t bytes = rest_text<true, false>(r, hw, cg, nullptr, 0, lane);
        if (lane == l) ln.rest = bytes;
    }
    if (text) ln.ob += (uint64_t)ln.cnt * tail_bytes(h, ln.rest);
    if (valid) {
        br::drop_bad(r, i, ln);
        br::store_line<kSlots>(r, i, ln);
        r.rest[i] = ln.rest;
    }
}

// A thread writes the output lines of its record, one per round; the columns
// from CIGAR on of a wave record are written by the whole wave, record after record.
__global__ void __launch_bounds__(kThreads)
k_bam_write(const Rec r, const uint64_t* __restrict__ off, uint64_t out_bytes, uint8_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < r.L;
    uint32_t nout = valid ? r.cnt[i] : 0u;
    if (nout && r.out_base + off[i] + r.ob[i] > out_bytes) nout = 0;
    const uint64_t at = nout ? r.rec_off[i] : 0;
    Head h{};
    if (nout) (void)read_head(r.in + at, h);
    const uint32_t cls = nout ? r.cls[i] : (uint32_t)C_BAD;
    const uint32_t cg = nout ? r.fo[(uint64_t)O_CG * r.L + i] : 0u;
    const bool big = nout && r.fo[(uint64_t)O_BIG * r.L + i];
    const uint64_t rest = nout ? r.rest[i] : 0;
    uint64_t start = nout ? r.a[i] : 0, stop = nout ? r.b[i] : 0;
    Writer<> w{out, r.out_base + (nout ? off[i] : 0)};
    uint32_t nc = 0, rname = 0;
    const uint8_t* c = nout ? cigar_of(h, cg, &nc) : nullptr;
    const uint8_t* name = nout && cls != C_UNMAPPED ? rname_of(r, h.ref, &rname) : nullptr;
    RunWalk cw{0, start, 0};
    for (uint32_t round = 0; __ballot(round < nout) != 0; ++round) {
        uint64_t rest_at = ~0ull;
        if (round < nout) {
            if (cls == C_SPLIT) (void)next_run(c, nc, cw, r.split_deletions != 0, &start, &stop);
            if (cls == C_UNMAPPED) w.bytes(reinterpret_cast<const uint8_t*>("_unmapped"), 9);
            else w.bytes(name, rname);
            w.tab();
            w.dec(start);
            w.tab();
            w.dec(stop);
            w.tab();
            w.bytes(h.name, h.l_name - 1);
            w.tab();
            w.dec(h.flag);
            w.tab();
            w.out[w.o++] = (h.flag & 16u) ? '-' : '+';
            if (!r.reduced) {
                w.tab();
                w.dec(h.mapq);
                w.tab();
                if (big) rest_at = w.o;
                else (void)rest_text<false, true>(r, h, cg, out, w.o, lane);
                w.o += rest;
            }
            w.out[w.o++] = '\n';
        }
        unsigned long long m = __ballot(rest_at != ~0ull);
        while (m) {
            const int l = __ffsll(m) - 1;
            m &= m - 1;
            const uint64_t wat = __shfl(at, l, 64), dst = __shfl(rest_at, l, 64);
            const uint32_t wcg = __shfl(cg, l, 64);
            Head hw;
            (void)read_head(r.in + wat, hw);
            (void)rest_text<true, true>(r, hw, wcg, out, dst, lane);
        }
    }
}

// kept header line k is in[hd[3k], ...) of hd[3k + 1] bytes and goes to out + hd[3k + 2]
__global__ void __launch_bounds__(kThreads) k_bam_header(const uint8_t* __restrict__ in, const uint64_t* __restrict__ hd, uint64_t H,
                                                         uint8_t* __restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    Writer<> w{out, 0};
    if (k < H) {
        w.o = hd[3 * k + 2];
        br::header_line(w, k, in + hd[3 * k], (uint32_t)hd[3 * k + 1]);
    }
    bt::wave_copy_tails(w, out, threadIdx.x & 63);
}

const char* bad_text(uint32_t k)
{
    switch (k) {
        case K_SHORT: return "block_size below 32";
        case K_PAST: return "the record runs past the end of the input";
        case K_COUNTS: return "block_size is below what l_read_name, n_cigar_op and l_seq announce";
        case K_NAME: return "the read name is empty or does not end in NUL";
        case K_REF: return "refID or next_refID is not -1 or a reference of the header";
        case K_CIGAR: return "CIGAR operator above 8";
        case K_TAGTYPE: return "unknown tag type";
        case K_TAGS: return "the tags do not parse exactly to the end of the record";
        case K_RNAME: return "mapped record without a reference name";
        default: return br::bad_text(k);
    }
}

[[noreturn]] void throw_record(uint64_t record, uint32_t kind)
{
    throw StarchError(STARCH_ERR_DATA, "bam2bed: record " + std::to_string(record + 1) + ": " + bad_text(kind));
}

[[noreturn]] void throw_header(const char* what) { throw StarchError(STARCH_ERR_DATA, std::string("bam2bed: ") + what); }

struct HeaderInfo {        // what the host's walk over the header leaves
    uint64_t body = 0;     // where the records begin
    std::vector<uint32_t> name_off;
    std::vector<uint8_t> names;
    std::vector<uint64_t> lines;   // per header line: its place in the input, its bytes
};

uint32_t host32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// The header in b[0, have) of an input of n bytes: 0 and *hi, or how many bytes
// the walk needs when it needs more than have.  Throws for a bad header.
uint64_t walk_header(const uint8_t* b, uint64_t have, uint64_t n, HeaderInfo* hi)
{
    uint64_t want = 0;
    auto need = [&](uint64_t end) {
        if (end > n) throw_header("the header is truncated");
        if (end > have) { want = end; return false; }
        return true;
    };
    if (!need(12)) return want;
    if (!(b[0] == 'B' && b[1] == 'A' && b[2] == 'M' && b[3] == 1)) throw_header("the input is neither gzip nor BAM (it does not begin BAM\\1)");
    const uint64_t l_text = host32(b + 4);
    if (!need(12 + l_text)) return want;
    const uint32_t n_ref = host32(b + 8 + l_text);
    if (n_ref > 0x7fffffffu) throw_header("n_ref is negative");
    uint64_t p = 12 + l_text;
    *hi = HeaderInfo{};
    hi->name_off.push_back(0);
    for (uint32_t k = 0; k < n_ref; ++k) {
        if (!need(p + 4)) return want;
        const uint64_t l_name = host32(b + p);
        if (l_name == 0) throw_header("a reference name has l_name 0");
        if (!need(p + 4 + l_name + 4)) return want;
        if (b[p + 4 + l_name - 1] != 0) throw_header("a reference name does not end in NUL");
        if (hi->names.size() + l_name - 1 > 0xffffffffull) throw_header("the reference names have 2^32 bytes or more");
        hi->names.insert(hi->names.end(), b + p + 4, b + p + 4 + l_name - 1);
        hi->name_off.push_back((uint32_t)hi->names.size());
        p += 4 + l_name + 4;
    }
    hi->body = p;
    uint64_t e = 8 + l_text;   // trailing NUL bytes are no text
    while (e > 8 && b[e - 1] == 0) --e;
    for (uint64_t at = 8; at < e;) {
        const void* nl = memchr(b + at, '\n', e - at);
        const uint64_t end = nl ? (uint64_t)(static_cast<const uint8_t*>(nl) - b) : e;
        hi->lines.push_back(at);
        hi->lines.push_back(end - at);
        at = end + 1;
    }
    return 0;
}

uint32_t digits_of(uint64_t v)
{
    uint32_t d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}

}  // namespace

void BamWorkspace::run(const BamOptions& opt, const uint8_t* d_in, uint64_t n, hipStream_t st, DevBuf& out, BamResult& res)
{
    res = BamResult{};
    (void)out.as<uint8_t>(64);
    timer.start(st);
    auto finish = [&](int from) { timer.finish(from, st, {&res.ms_frame, &res.ms_parse, &res.ms_write}); };

    // 1. the header: the one round trip of input bytes.  (A header longer than
    // the first read-back costs a second one, of what the walk then asks for.)
    HeaderInfo hi;
    {
        std::vector<uint8_t> hb;
        for (uint64_t have = std::min<uint64_t>(n, 256u << 10);;) {
            hb.resize(have);
            if (have) HIP_CHECK(hipMemcpyAsync(hb.data(), d_in, have, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            const uint64_t want = walk_header(hb.data(), have, n, &hi);
            if (!want) break;
            have = std::min<uint64_t>(n, std::max<uint64_t>(want, 2 * have));
        }
    }
    const uint64_t H = hi.lines.size() / 2, n_ref = hi.name_off.size() - 1;
    res.references = n_ref;
    res.header_lines = H;
    // the names as offsets and bytes; the kept header lines with their places in the output
    uint64_t header_bytes = 0;
    const uint64_t name_words = (n_ref + 1 + 1) / 2 * 2;   // (the bytes begin at a multiple of 8)
    uint8_t* d_names = names.as<uint8_t>(name_words * 4 + hi.names.size() + 8);
    HIP_CHECK(hipMemcpyAsync(d_names, hi.name_off.data(), (n_ref + 1) * 4, hipMemcpyHostToDevice, st));
    if (!hi.names.empty()) HIP_CHECK(hipMemcpyAsync(d_names + name_words * 4, hi.names.data(), hi.names.size(), hipMemcpyHostToDevice, st));
    std::vector<uint64_t> hd;
    if (opt.keep_header && H) {
        hd.resize(3 * H);
        for (uint64_t k = 0; k < H; ++k) {
            hd[3 * k] = hi.lines[2 * k];
            hd[3 * k + 1] = hi.lines[2 * k + 1];
            hd[3 * k + 2] = header_bytes;
            header_bytes += 8 + digits_of(k) + 1 + digits_of(k + 1) + 1 + hi.lines[2 * k + 1] + 1;   // _header K K+1 line
        }
        HIP_CHECK(hipMemcpyAsync(header.as<uint64_t>(3 * H), hd.data(), 3 * H * 8, hipMemcpyHostToDevice, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));   // (the host vectors are free again)

    // 2. framing
    const uint64_t tiles = ceil_div(n, T), first = hi.body / T;
    res.tiles = tiles;
    unsigned long long* fs = reinterpret_cast<unsigned long long*>(fstate.as<uint64_t>(F_COUNT));
    const unsigned long long fs0[F_COUNT] = {hi.body, ~0ull, 0, 0};
    HIP_CHECK(hipMemcpyAsync(fs, fs0, sizeof fs0, hipMemcpyHostToDevice, st));
    uint32_t* d_entry = entry.as<uint32_t>(tiles);
    HIP_CHECK(hipMemsetAsync(d_entry, 0xff, tiles * sizeof(uint32_t), st));
    uint16_t* tab = table.as<uint16_t>(std::min<uint64_t>(tiles - first, kBatchTiles) * T);
    for (uint64_t t0 = first; t0 < tiles; t0 += kBatchTiles) {
        const uint64_t t1 = std::min<uint64_t>(tiles, t0 + kBatchTiles);
        hipLaunchKernelGGL(k_bam_table, dim3((unsigned)(t1 - t0)), dim3(kTableThreads), 0, st, d_in, n, t0, tab);
        hipLaunchKernelGGL(k_bam_tiles, dim3(1), dim3(64), 0, st, d_in, n, t0, t1, tab, d_entry, fs);
        HIP_CHECK(hipGetLastError());
    }
    uint32_t* d_count = count.as<uint32_t>(tiles + 1);
    uint64_t* d_base = base.as<uint64_t>(tiles + 1);
    hipLaunchKernelGGL(k_bam_chain<false>, dim3((unsigned)tiles), dim3(64), 0, st, d_in, n, d_entry, fs, d_count, nullptr, nullptr);
    HIP_CHECK(hipGetLastError());
    scan::excl_sum_u32_to_u64(d_count, d_base, tiles, reinterpret_cast<uint64_t*>(fs) + 3, rb.tmp, st);
    unsigned long long fsh[F_COUNT];
    HIP_CHECK(hipMemcpyAsync(fsh, fs, sizeof fsh, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t R = fsh[3];   // the good records before the chain's end
    const uint32_t frame_kind = (uint32_t)fsh[F_KIND];
    if (R >= (1ull << 32)) throw StarchError(STARCH_ERR_ARG, "bam2bed: 2^32 records or more");
    uint64_t* d_rec = rec_off.as<uint64_t>(R);
    if (R) {
        hipLaunchKernelGGL(k_bam_chain<true>, dim3((unsigned)tiles), dim3(64), 0, st, d_in, n, d_entry, fs, nullptr, d_base, d_rec);
        HIP_CHECK(hipGetLastError());
    }
    timer.mark(1, st);

    // 3. classify and measure; the lowest bad record, which the chain's end is when no record before it is bad
    Rec r{};
    reset_and_bind(rb, r, d_in, nullptr, R, kSlots, st);
    r.rec_off = d_rec;
    r.rest = rest.as<uint64_t>(R);
    r.name_off = reinterpret_cast<const uint32_t*>(d_names);
    r.names = d_names + name_words * 4;
    r.n_ref = (int32_t)n_ref;
    r.split = opt.split;
    r.split_deletions = opt.split_deletions;
    r.all_reads = opt.all_reads;
    r.reduced = opt.reduced;
    r.keep_header = 0;     // (the header lines are not among the records)
    r.out_base = header_bytes;
    if (R) {
        hipLaunchKernelGGL(k_bam_classify, dim3(blocks_for(R, kThreads)), dim3(kThreads), 0, st, r);
        HIP_CHECK(hipGetLastError());
    }
    const First f = first_of(rb, st);
    if (f.bad != ~0ull) throw_record(f.bad >> 8, (uint32_t)(f.bad & 255));
    if (frame_kind) throw_record(R, frame_kind);
    const Placed p = place<Tally>(rb, r, R, "bam2bed", st);
    res.records = p.tot[S_REC];
    res.unmapped_dropped = p.tot[S_DROPPED];
    res.wave_records = p.tot[S_WAVE];
    timer.mark(2, st);

    // 4. output: the kept header lines, then the records
    const uint64_t bytes = header_bytes + p.tot[S_BYTES];
    if (bytes) {
        uint8_t* o = out.as<uint8_t>(bytes + 64);
        if (header_bytes) {
            hipLaunchKernelGGL(k_bam_header, dim3(blocks_for(H, kThreads)), dim3(kThreads), 0, st, d_in,
                               static_cast<const uint64_t*>(header.p), H, o);
            HIP_CHECK(hipGetLastError());
        }
        if (p.tot[S_BYTES]) {
            hipLaunchKernelGGL(k_bam_write, dim3(blocks_for(R, kThreads)), dim3(kThreads), 0, st, r, p.off, bytes, o);
            HIP_CHECK(hipGetLastError());
        }
    }
    res.lines_out = p.tot[S_LINES] + (opt.keep_header ? H : 0);
    res.out_bytes = bytes;
    if (res.lines_out >= (1ull << 32)) throw StarchError(STARCH_ERR_ARG, "bam2bed: 2^32 output lines or more");
    finish(3);
}

}  // namespace bam
