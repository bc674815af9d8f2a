// starch_amd/csrc/sort_bed.hip -- sort-bed on MI355X: BED lines into
// (chromosome, start, stop) order, equal keys in input order.
//
// Stages (all per-line arrays are struct-of-arrays, indexed by input line):
//   1. k_sb_count_nl / k_sb_index_nl   line ends (u64), a last line without
//      '\n' gets a virtual one; k_sb_parse: one thread per line -> chromosome
//      length, start, stop; the first malformed line by atomicMin.
//   2. chromosome ranks: k_sb_insert puts every name's 64-bit hash into an
//      open-addressing table (a slot's first claimant is its representative
//      line), k_sb_lookup finds each line's slot and compares its name bytes
//      with the representative's -- two names with one hash raise a flag and
//      the stage runs again under another seed, never merged.  The distinct
//      names go to the host once, are ordered there (memcmp, shorter first)
//      and their ranks come back through the table.
//   3. k_sb_check: is every key >= its predecessor's (first descent by
//      atomicMin), plus the OR and AND of every key word: a byte of the
//      160-bit key whose OR equals its AND is the same in every line and gets
//      no radix pass.
//   4. stable LSD radix sort of a 32-bit line index, one byte per pass:
//      k_sb_hist (gathers the pass's digit of every line through the index,
//      keeps it as a byte, per-tile histogram), a scan over (digit, tile), and
//      k_sb_scatter (ranks inside a tile from wave ballots, wave after wave).
//   5. gather: line lengths in sorted order, their exclusive sum, then
//      k_sb_copy (a thread per short line; long lines are listed) and
//      k_sb_copy_long (a wave per listed line).
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/starch_amd.h"
#include "bed_text.hpp"
#include "sort_bed.hpp"

namespace sb {
namespace {

constexpr int kTileBytes = 16384;   // 256 threads x 64 B
constexpr int kThreads = 256;
constexpr uint32_t kMaxProbe = 1024;
static_assert(kSortThreads == 256, "k_sb_hist and k_sb_scatter give one thread to each digit value");

// device scalars (u64 each); [0, 16) start as 0, [16, 32) as all ones
enum : int {
    S_NL = 0, S_NAMES, S_OVERFLOW, S_COLLISION, S_ENT, S_LONG, S_OR_RANK, S_OR_START, S_OR_STOP, S_GATHERED,
    S_BAD = 16, S_DESC, S_AND_RANK, S_AND_START, S_AND_STOP, S_COUNT = 32
};

enum : uint32_t {
    B_EMPTY = 1, B_HASH, B_TRACK, B_NOCHROM, B_FIELDS, B_START_EMPTY, B_START_DIGIT, B_START_RANGE, B_STOP_EMPTY,
    B_STOP_DIGIT, B_STOP_RANGE, B_LONG
};

struct Ent {            // one distinct chromosome name
    uint64_t off;       // its bytes in the input (the representative line's)
    uint32_t len, slot;
};

// ---- 1. framing and parse ---------------------------------------------------
__device__ __forceinline__ uint32_t nl_flags(uint32_t w)   // bit 7 of every byte that is '\n'
{
    const uint32_t x = w ^ 0x0a0a0a0au;
    const uint32_t t = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;
    return ~t & 0x80808080u;
}

// '\n' flags of the 64 bytes from base on (bytes at or past n: none)
__device__ __forceinline__ void load_flags(const uint8_t* __restrict__ bed, uint64_t n, uint64_t base, uint32_t* fl)
{
    if (base + 64 <= n && ((reinterpret_cast<uintptr_t>(bed) & 15u) == 0)) {
        const uint4* p = reinterpret_cast<const uint4*>(bed + base);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 v = p[k];
            fl[4 * k + 0] = nl_flags(v.x);
            fl[4 * k + 1] = nl_flags(v.y);
            fl[4 * k + 2] = nl_flags(v.z);
            fl[4 * k + 3] = nl_flags(v.w);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            uint32_t f = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint64_t i = base + 4 * j + b;
                if (i < n && bed[i] == '\n') f |= 0x80u << (8 * b);
            }
            fl[j] = f;
        }
    }
}

__global__ void __launch_bounds__(kThreads)
k_sb_count_nl(const uint8_t* __restrict__ bed, uint64_t n, uint32_t* __restrict__ tile_cnt)
{
    const uint64_t base = (uint64_t)blockIdx.x * kTileBytes + (uint64_t)threadIdx.x * 64;
    uint32_t fl[16];
    load_flags(bed, n, base, fl);
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) c += __popc(fl[j]);
    __shared__ uint32_t sh[kThreads / 64 + 1];
    uint32_t tot;
    (void)block_excl_scan_add<uint32_t>(c, sh, &tot);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kThreads)
k_sb_index_nl(const uint8_t* __restrict__ bed, uint64_t n, const uint64_t* __restrict__ tile_off,
              uint64_t* __restrict__ line_end)
{
    const uint64_t base = (uint64_t)blockIdx.x * kTileBytes + (uint64_t)threadIdx.x * 64;
    uint32_t fl[16];
    load_flags(bed, n, base, fl);
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) c += __popc(fl[j]);
    __shared__ uint32_t sh[kThreads / 64 + 1];
    const uint32_t pre = block_excl_scan_add<uint32_t>(c, sh, (uint32_t*)nullptr);
    uint64_t o = tile_off[blockIdx.x] + pre;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        uint32_t m = fl[j];
        while (m) {
            const uint32_t bpos = (uint32_t)__builtin_ctz(m) >> 3;
            line_end[o++] = base + 4 * j + bpos + 1;
            m &= m - 1;
        }
    }
}

__global__ void k_sb_set_u64(uint64_t* p, uint64_t v) { *p = v; }

// decimal field bed[b, e): 0 ok, 1 empty, 2 non-digit, 3 too long / above 2^63-1
__device__ __forceinline__ uint32_t parse_coord(const uint8_t* __restrict__ bed, uint64_t b, uint64_t e, uint64_t* v)
{
    if (b == e) return 1;
    for (uint64_t p = b; p < e; ++p)
        if ((uint32_t)bed[p] - '0' > 9u) return 2;
    if (e - b > 19) return 3;
    uint64_t x = 0;
    for (uint64_t p = b; p < e; ++p) x = x * 10 + ((uint32_t)bed[p] - '0');   // 19 digits: below 10^19 < 2^64
    if (x > 0x7fffffffffffffffull) return 3;
    *v = x;
    return 0;
}

// line i is bed[beg, end): end excludes its '\n' (line_end holds one past it;
// the entry of a last line without '\n' is n + 1)
using bt::line_beg;

__global__ void __launch_bounds__(kThreads)
k_sb_parse(const uint8_t* __restrict__ bed, const uint64_t* __restrict__ line_end, uint64_t L,
           uint64_t* __restrict__ start, uint64_t* __restrict__ stop, uint32_t* __restrict__ chr_len,
           unsigned long long* __restrict__ bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= L) return;
    const uint64_t b = line_beg(line_end, i), e = line_end[i] - 1;
    uint32_t kind = 0;
    uint64_t s = 0, t = 0, p = b;
    if (e - b >= 0xffffffffull) kind = B_LONG;
    else if (e == b) kind = B_EMPTY;
    else if (bed[b] == '#') kind = B_HASH;
    else {
        while (p < e && bed[p] != '\t') ++p;
        const uint64_t clen = p - b;
        if (e - b >= 5 && bed[b] == 't' && bed[b + 1] == 'r' && bed[b + 2] == 'a' && bed[b + 3] == 'c' &&
            bed[b + 4] == 'k' && (b + 5 == e || bed[b + 5] == '\t' || bed[b + 5] == ' '))
            kind = B_TRACK;
        else if (clen == 0) kind = B_NOCHROM;
        else if (p == e) kind = B_FIELDS;
        else {
            const uint64_t s0 = p + 1;
            uint64_t q = s0;
            while (q < e && bed[q] != '\t') ++q;
            if (q == e) kind = B_FIELDS;
            else {
                const uint64_t t0 = q + 1;
                uint64_t r = t0;
                while (r < e && bed[r] != '\t') ++r;
                const uint32_t a = parse_coord(bed, s0, q, &s);
                const uint32_t c = a ? 0 : parse_coord(bed, t0, r, &t);
                if (a) kind = B_START_EMPTY + a - 1;
                else if (c) kind = B_STOP_EMPTY + c - 1;
            }
        }
    }
    start[i] = s;
    stop[i] = t;
    chr_len[i] = kind ? 0u : (uint32_t)(p - b);
    if (kind) atomicMin(bad, (unsigned long long)((i << 8) | kind));
}

// ---- 2. chromosome ranks ----------------------------------------------------
__device__ __forceinline__ uint64_t name_hash(const uint8_t* __restrict__ p, uint32_t len, uint64_t seed)
{
    uint64_t h = 0xcbf29ce484222325ull ^ (seed * 0x9e3779b97f4a7c15ull);
    for (uint32_t k = 0; k < len; ++k) h = (h ^ p[k]) * 0x100000001b3ull;
    h ^= h >> 32;
    h *= 0x9e3779b97f4a7c15ull;
    h ^= h >> 29;
    return h ? h : 1;   // 0 marks an empty slot
}

__device__ __forceinline__ bool same_bytes(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint32_t len)
{
    for (uint32_t k = 0; k < len; ++k)
        if (a[k] != b[k]) return false;
    return true;
}

__global__ void __launch_bounds__(kThreads)
k_sb_insert(const uint8_t* __restrict__ bed, const uint64_t* __restrict__ line_end, const uint32_t* __restrict__ chr_len,
            uint64_t L, uint64_t seed, uint64_t* __restrict__ hash, unsigned long long* keys, uint32_t* rep,
            uint64_t mask, unsigned long long* scal)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= L) return;
    const uint64_t b = line_beg(line_end, i);
    const uint32_t len = chr_len[i];
    const uint64_t h = name_hash(bed + b, len, seed);
    hash[i] = h;
    // a line whose name is its predecessor's leaves the insert to that line
    if (i && chr_len[i - 1] == len && same_bytes(bed + line_beg(line_end, i - 1), bed + b, len)) return;
    if (__atomic_load_n(&scal[S_OVERFLOW], __ATOMIC_RELAXED)) return;
    uint64_t slot = h & mask;
    for (uint32_t probe = 0; probe < kMaxProbe; ++probe, slot = (slot + 1) & mask) {
        unsigned long long k = __atomic_load_n(&keys[slot], __ATOMIC_RELAXED);
        if (k == 0) {
            k = atomicCAS(&keys[slot], 0ull, (unsigned long long)h);
            if (k == 0) {
                rep[slot] = (uint32_t)i;
                atomicAdd(&scal[S_NAMES], 1ull);
                return;
            }
        }
        if (k == h) return;
    }
    atomicOr(&scal[S_OVERFLOW], 1ull);
}

// slot of every line (into slot_of); a name that differs from its slot's
// representative has met another name's hash
__global__ void __launch_bounds__(kThreads)
k_sb_lookup(const uint8_t* __restrict__ bed, const uint64_t* __restrict__ line_end, const uint32_t* __restrict__ chr_len,
            uint64_t L, const uint64_t* __restrict__ hash, const unsigned long long* __restrict__ keys,
            const uint32_t* __restrict__ rep, uint64_t mask, uint32_t* __restrict__ slot_of, unsigned long long* scal)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= L) return;
    const uint64_t h = hash[i];
    uint64_t slot = h & mask;
    bool found = false;
    for (uint32_t probe = 0; probe < kMaxProbe; ++probe, slot = (slot + 1) & mask) {
        const unsigned long long k = keys[slot];
        if (k == h) { found = true; break; }
        if (k == 0) break;
    }
    bool ok = found;
    if (found) {
        const uint32_t r = rep[slot];
        const uint32_t len = chr_len[i];
        if (r != (uint32_t)i)
            ok = (uint64_t)r < L && chr_len[r] == len &&
                 same_bytes(bed + line_beg(line_end, r), bed + line_beg(line_end, i), len);
    }
    slot_of[i] = found ? (uint32_t)slot : 0u;
    if (!ok) atomicOr(&scal[S_COLLISION], 1ull);
}

__global__ void __launch_bounds__(kThreads)
k_sb_collect(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ rep, uint64_t cap,
             const uint64_t* __restrict__ line_end, const uint32_t* __restrict__ chr_len, Ent* __restrict__ ent,
             uint64_t ent_cap, unsigned long long* scal)
{
    const uint64_t s = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= cap || keys[s] == 0) return;
    const unsigned long long k = atomicAdd(&scal[S_ENT], 1ull);
    if (k >= ent_cap) return;
    const uint32_t r = rep[s];
    ent[k] = Ent{line_beg(line_end, r), chr_len[r], (uint32_t)s};
}

// one wave per name: its bytes to names[dst[k] ...)
__global__ void __launch_bounds__(kThreads)
k_sb_names(const uint8_t* __restrict__ bed, const Ent* __restrict__ ent, const uint64_t* __restrict__ dst, uint64_t cnt,
           uint8_t* __restrict__ names)
{
    const uint64_t k = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    if (k >= cnt) return;
    const Ent e = ent[k];
    for (uint32_t j = threadIdx.x & 63; j < e.len; j += 64) names[dst[k] + j] = bed[e.off + j];
}

__global__ void __launch_bounds__(kThreads)
k_sb_slot_ranks(const Ent* __restrict__ ent, const uint32_t* __restrict__ rank_of, uint64_t cnt, uint32_t* __restrict__ rep)
{
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k < cnt) rep[ent[k].slot] = rank_of[k];
}

__global__ void __launch_bounds__(kThreads)
k_sb_assign(const uint32_t* __restrict__ slot_rank, uint32_t* __restrict__ rank, uint64_t L)   // rank: slots in, ranks out
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < L) rank[i] = slot_rank[rank[i]];
}

// ---- 3. order check, key reduction --------------------------------------------
__global__ void __launch_bounds__(kThreads)
k_sb_check(const uint32_t* __restrict__ rank, const uint64_t* __restrict__ start, const uint64_t* __restrict__ stop,
           uint64_t L, unsigned long long* scal)
{
    uint64_t o_r = 0, o_s = 0, o_t = 0, a_r = ~0ull, a_s = ~0ull, a_t = ~0ull, desc = ~0ull;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < L; i += stride) {
        const uint64_t r = rank[i], s = start[i], t = stop[i];
        o_r |= r; a_r &= r;
        o_s |= s; a_s &= s;
        o_t |= t; a_t &= t;
        if (i && desc == ~0ull) {
            const uint64_t pr = rank[i - 1], ps = start[i - 1], pt = stop[i - 1];
            if (r < pr || (r == pr && (s < ps || (s == ps && t < pt)))) desc = i;
        }
    }
    o_r = wave_reduce_or64(o_r); a_r = ~wave_reduce_or64(~a_r);
    o_s = wave_reduce_or64(o_s); a_s = ~wave_reduce_or64(~a_s);
    o_t = wave_reduce_or64(o_t); a_t = ~wave_reduce_or64(~a_t);
    if ((threadIdx.x & 63) == 0) {
        atomicOr(&scal[S_OR_RANK], (unsigned long long)o_r);
        atomicOr(&scal[S_OR_START], (unsigned long long)o_s);
        atomicOr(&scal[S_OR_STOP], (unsigned long long)o_t);
        atomicAnd(&scal[S_AND_RANK], (unsigned long long)a_r);
        atomicAnd(&scal[S_AND_START], (unsigned long long)a_s);
        atomicAnd(&scal[S_AND_STOP], (unsigned long long)a_t);
    }
    if (desc != ~0ull) atomicMin(&scal[S_DESC], (unsigned long long)desc);
}

// ---- 4. radix passes -----------------------------------------------------------
// digit of every position of the current order (src == nullptr: input order),
// kept in dig; hist[d * ntiles + tile] = lines of the tile with digit d
__global__ void __launch_bounds__(kSortThreads)
k_sb_hist(const uint32_t* __restrict__ src, const uint64_t* __restrict__ k64, const uint32_t* __restrict__ k32,
          uint32_t shift, uint64_t L, uint64_t ntiles, uint8_t* __restrict__ dig, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kSortTile;
#pragma unroll 4
    for (int k = 0; k < kSortItems; ++k) {
        const uint64_t e = base + (uint64_t)k * kSortThreads + threadIdx.x;
        if (e < L) {
            const uint64_t i = src ? src[e] : e;
            const uint32_t d = k64 ? (uint32_t)(k64[i] >> shift) & 255u : (k32[i] >> shift) & 255u;
            dig[e] = (uint8_t)d;
            atomicAdd(&h[d], 1u);
        }
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// stable scatter of a tile: wave w owns positions [w, w + 1) * kSortTile / 4 of
// the tile, 64 at a time; a line's place among its wave's equal digits comes
// from ballots, earlier rounds and earlier waves add their counts
__global__ void __launch_bounds__(kSortThreads)
k_sb_scatter(const uint32_t* __restrict__ src, const uint8_t* __restrict__ dig, const uint64_t* __restrict__ off,
             uint64_t L, uint64_t ntiles, uint32_t* __restrict__ dst)
{
    constexpr int kWaves = kSortThreads / 64;
    constexpr int kRounds = kSortTile / kSortThreads;
    __shared__ uint32_t wcnt[kWaves][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < kWaves * 256; k += kSortThreads) (&wcnt[0][0])[k] = 0;
    __syncthreads();
    volatile uint32_t* mine = wcnt[w];
    const uint64_t wbase = (uint64_t)blockIdx.x * kSortTile + (uint64_t)w * (kSortTile / kWaves);
    const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    uint32_t place[kRounds], digit[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint64_t e = wbase + (uint64_t)r * 64 + lane;
        const bool valid = e < L;
        const uint32_t d = valid ? dig[e] : 0u;
        uint64_t m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bal = __ballot(bit);
            m &= bit ? bal : ~bal;
        }
        const uint32_t cnt = mine[d];
        place[r] = cnt + (uint32_t)__popcll(m & lt);
        digit[r] = d;
        const bool last = valid && (lane == 63 || (m >> (lane + 1)) == 0);
        if (last) mine[d] = cnt + (uint32_t)__popcll(m);
    }
    __syncthreads();
    {
        const int d = threadIdx.x;
        uint32_t base = (uint32_t)off[(uint64_t)d * ntiles + blockIdx.x];   // below L < 2^32
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            const uint32_t c = wcnt[k][d];
            wcnt[k][d] = base;
            base += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint64_t e = wbase + (uint64_t)r * 64 + lane;
        if (e < L) {
            const uint64_t to = (uint64_t)wcnt[w][digit[r]] + place[r];
            if (to < L) dst[to] = src ? src[e] : (uint32_t)e;
        }
    }
}

// ---- 5. gather -------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
k_sb_len(const uint32_t* __restrict__ idx, const uint64_t* __restrict__ line_end, uint64_t L, uint32_t* __restrict__ len)
{
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= L) return;
    const uint64_t i = idx[j];
    len[j] = (uint32_t)(line_end[i] - line_beg(line_end, i));   // with its '\n'
}

__global__ void __launch_bounds__(kThreads)
k_sb_copy(const uint8_t* __restrict__ bed, const uint64_t* __restrict__ line_end, const uint32_t* __restrict__ idx,
          const uint32_t* __restrict__ len, const uint64_t* __restrict__ out_off, uint64_t L, uint8_t* __restrict__ out,
          uint32_t* __restrict__ long_list, unsigned long long* scal)
{
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= L) return;
    const uint32_t l = len[j];
    if (l >= kWaveCopyBytes) {
        long_list[atomicAdd(&scal[S_LONG], 1ull)] = (uint32_t)j;   // at most L entries
        return;
    }
    const uint8_t* s = bed + line_beg(line_end, idx[j]);
    uint8_t* d = out + out_off[j];
    for (uint32_t k = 0; k + 1 < l; ++k) d[k] = s[k];
    d[l - 1] = '\n';
}

__global__ void __launch_bounds__(kThreads)
k_sb_copy_long(const uint8_t* __restrict__ bed, const uint64_t* __restrict__ line_end, const uint32_t* __restrict__ idx,
               const uint32_t* __restrict__ len, const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out,
               const uint32_t* __restrict__ long_list, const unsigned long long* __restrict__ scal)
{
    const uint64_t nlong = scal[S_LONG];
    const uint64_t nwaves = (uint64_t)gridDim.x * (kThreads / 64);
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t k = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); k < nlong; k += nwaves) {
        const uint64_t j = long_list[k];
        const uint32_t l = len[j];
        const uint8_t* s = bed + line_beg(line_end, idx[j]);
        uint8_t* d = out + out_off[j];
        for (uint32_t q = lane; q + 1 < l; q += 64) d[q] = s[q];
        if (lane == 0) d[l - 1] = '\n';
    }
}

__global__ void __launch_bounds__(kThreads) k_sb_iota(uint32_t* idx, uint64_t L)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < L) idx[i] = (uint32_t)i;
}

}  // namespace

const char* bad_text(uint32_t k)
{
    switch (k) {
        case B_EMPTY: return "empty line";
        case B_HASH: return "'#' header line";
        case B_TRACK: return "'track' header line";
        case B_NOCHROM: return "empty chromosome field";
        case B_FIELDS: return "fewer than three tab-separated fields";
        case B_START_EMPTY: return "empty start coordinate";
        case B_START_DIGIT: return "non-digit in the start coordinate";
        case B_START_RANGE: return "start coordinate has 20 or more digits or is above 2^63-1";
        case B_STOP_EMPTY: return "empty stop coordinate";
        case B_STOP_DIGIT: return "non-digit in the stop coordinate";
        case B_STOP_RANGE: return "stop coordinate has 20 or more digits or is above 2^63-1";
        case B_LONG: return "line of 2^32 bytes or more";
        default: return "malformed line";
    }
}


uint64_t SortWorkspace::stage_frame(const uint8_t* d_bed, uint64_t n, hipStream_t st)
{
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    HIP_CHECK(hipMemsetAsync(scal, 0, 16 * sizeof(uint64_t), st));
    HIP_CHECK(hipMemsetAsync(scal + 16, 0xff, 16 * sizeof(uint64_t), st));
    const uint64_t ntile = ceil_div(n, kTileBytes);
    uint32_t* tile_cnt = b_tile_cnt.as<uint32_t>(ntile + 1);
    uint64_t* tile_off = b_tile_off.as<uint64_t>(ntile + 1);
    hipLaunchKernelGGL(k_sb_count_nl, dim3((unsigned)ntile), dim3(kThreads), 0, st, d_bed, n, tile_cnt);
    scan::excl_sum_u32_to_u64(tile_cnt, tile_off, ntile, scal + S_NL, b_tmp, st);
    uint64_t nl = 0;
    uint8_t last = 0;
    HIP_CHECK(hipMemcpyAsync(&nl, scal + S_NL, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&last, d_bed + (n - 1), 1, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const bool open_end = last != '\n';
    const uint64_t L = nl + (open_end ? 1 : 0);
    if (L > 0xffffffffull) throw StarchError(STARCH_ERR_ARG, "sort-bed: more than 2^32-1 lines in one call");
    ln = Lines{};
    ln.L = L;
    ln.open_end = open_end;
    ln.line_end = b_line_end.as<uint64_t>(L + 1);
    if (nl) hipLaunchKernelGGL(k_sb_index_nl, dim3((unsigned)ntile), dim3(kThreads), 0, st, d_bed, n, tile_off, ln.line_end);
    if (open_end) hipLaunchKernelGGL(k_sb_set_u64, dim3(1), dim3(1), 0, st, ln.line_end + nl, n + 1);
    HIP_CHECK(hipGetLastError());
    return L;
}

uint64_t SortWorkspace::stage_parse(const uint8_t* d_bed, uint64_t n, hipStream_t st, uint64_t* bad)
{
    const uint64_t L = stage_frame(d_bed, n, st);
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    unsigned long long* uscal = reinterpret_cast<unsigned long long*>(scal);
    ln.start = b_start.as<uint64_t>(L);
    ln.stop = b_stop.as<uint64_t>(L);
    ln.chr_len = b_chr_len.as<uint32_t>(L);
    hipLaunchKernelGGL(k_sb_parse, dim3(blocks_for(L, kThreads)), dim3(kThreads), 0, st, d_bed, ln.line_end, L, ln.start,
                       ln.stop, ln.chr_len, uscal + S_BAD);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(bad, scal + S_BAD, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return L;
}

void SortWorkspace::stage_rank(const uint8_t* d_bed, hipStream_t st)
{
    const uint64_t L = ln.L;
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    unsigned long long* uscal = reinterpret_cast<unsigned long long*>(scal);
    const uint64_t* line_end = ln.line_end;
    const uint32_t* chr_len = ln.chr_len;
    const unsigned lblocks = blocks_for(L, kThreads);
    uint64_t* hash = b_hash.as<uint64_t>(L);
    uint32_t* rank = b_rank.as<uint32_t>(L);
    uint64_t cap_max = 1ull << 16;
    while (cap_max < 8 * L) cap_max <<= 1;
    uint64_t cap = 1ull << 16, seed = 1, names = 0;
    unsigned long long* keys = nullptr;
    uint32_t* rep = nullptr;
    for (int attempt = 0;; ++attempt) {
        if (attempt >= 12) throw StarchError(STARCH_ERR_INTERNAL, "sort-bed: the chromosome table did not settle");
        keys = reinterpret_cast<unsigned long long*>(b_keys.as<uint64_t>(cap));
        rep = b_rep.as<uint32_t>(cap);
        HIP_CHECK(hipMemsetAsync(keys, 0, cap * sizeof(uint64_t), st));
        HIP_CHECK(hipMemsetAsync(scal + S_NAMES, 0, 4 * sizeof(uint64_t), st));   // names, overflow, collision, entries
        hipLaunchKernelGGL(k_sb_insert, dim3(lblocks), dim3(kThreads), 0, st, d_bed, line_end, chr_len, L, seed, hash, keys,
                           rep, cap - 1, uscal);
        uint64_t h[3];
        HIP_CHECK(hipMemcpyAsync(h, scal + S_NAMES, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (h[1] || h[0] * 2 > cap) {          // too full (or a probe ran long): a larger table
            if (cap >= cap_max) ++seed;
            cap = std::min(cap * 16, cap_max);
            continue;
        }
        names = h[0];
        hipLaunchKernelGGL(k_sb_lookup, dim3(lblocks), dim3(kThreads), 0, st, d_bed, line_end, chr_len, L, hash, keys, rep,
                           cap - 1, rank, uscal);
        HIP_CHECK(hipMemcpyAsync(h, scal + S_COLLISION, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (h[0] == 0) break;
        ++seed;                                 // two names under one hash: hash again
    }
    n_chromosomes = names;
    {
        Ent* ent = b_ent.as<Ent>(names);
        hipLaunchKernelGGL(k_sb_collect, dim3(blocks_for(cap, kThreads)), dim3(kThreads), 0, st, keys, rep, cap, line_end,
                           chr_len, ent, names, uscal);
        std::vector<Ent> he(names);
        HIP_CHECK(hipMemcpyAsync(he.data(), ent, names * sizeof(Ent), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        std::vector<uint64_t> dst(names);
        uint64_t nbytes = 0;
        for (uint64_t k = 0; k < names; ++k) { dst[k] = nbytes; nbytes += he[k].len; }
        uint64_t* d_dst = b_name_dst.as<uint64_t>(names);
        uint8_t* d_names = b_names.as<uint8_t>(nbytes);
        HIP_CHECK(hipMemcpyAsync(d_dst, dst.data(), names * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_sb_names, dim3(blocks_for(names * 64, kThreads)), dim3(kThreads), 0, st, d_bed, ent, d_dst,
                           names, d_names);
        std::vector<uint8_t> hn(nbytes ? nbytes : 1);
        if (nbytes) HIP_CHECK(hipMemcpyAsync(hn.data(), d_names, nbytes, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        std::vector<uint32_t> order(names), rank_of(names);
        for (uint64_t k = 0; k < names; ++k) order[k] = (uint32_t)k;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            const uint32_t la = he[a].len, lb = he[b].len;
            const int c = memcmp(hn.data() + dst[a], hn.data() + dst[b], std::min(la, lb));
            return c ? c < 0 : la < lb;        // (distinct names never tie)
        });
        chrom_off.resize(names);
        chrom_len.resize(names);
        for (uint64_t k = 0; k < names; ++k) {
            rank_of[order[k]] = (uint32_t)k;
            chrom_off[k] = he[order[k]].off;
            chrom_len[k] = he[order[k]].len;
        }
        uint32_t* d_rank_of = b_slot_rank.as<uint32_t>(names);
        HIP_CHECK(hipMemcpyAsync(d_rank_of, rank_of.data(), names * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_sb_slot_ranks, dim3(blocks_for(names, kThreads)), dim3(kThreads), 0, st, ent, d_rank_of, names,
                           rep);
        hipLaunchKernelGGL(k_sb_assign, dim3(lblocks), dim3(kThreads), 0, st, rep, rank, L);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));   // the host vectors above were copy sources
    }
    ln.rank = rank;
}

KeyBits SortWorkspace::stage_check(const uint32_t* rank, const uint64_t* start, const uint64_t* stop, uint64_t L,
                                   hipStream_t st)
{
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    unsigned long long* uscal = reinterpret_cast<unsigned long long*>(scal);
    HIP_CHECK(hipMemsetAsync(scal + S_OR_RANK, 0, 3 * sizeof(uint64_t), st));
    HIP_CHECK(hipMemsetAsync(scal + S_DESC, 0xff, 4 * sizeof(uint64_t), st));
    const unsigned cblocks = (unsigned)std::min<uint64_t>(blocks_for(L, kThreads), 2048);
    hipLaunchKernelGGL(k_sb_check, dim3(cblocks), dim3(kThreads), 0, st, rank, start, stop, L, uscal);
    uint64_t hs[S_COUNT];
    HIP_CHECK(hipMemcpyAsync(hs, scal, sizeof(hs), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    KeyBits kb;
    kb.or_rank = hs[S_OR_RANK];   kb.and_rank = hs[S_AND_RANK];
    kb.or_start = hs[S_OR_START]; kb.and_start = hs[S_AND_START];
    kb.or_stop = hs[S_OR_STOP];   kb.and_stop = hs[S_AND_STOP];
    kb.desc = hs[S_DESC];
    return kb;
}

const uint32_t* SortWorkspace::stage_radix(const uint32_t* rank, const uint64_t* start, const uint64_t* stop, uint64_t L,
                                           const KeyBits& kb, hipStream_t st, uint32_t* passes_out)
{
    // one pass per key byte that is not the same in every line, least significant first
    struct Pass { const uint64_t* k64; const uint32_t* k32; uint32_t shift; };
    std::vector<Pass> passes;
    if (stop)
        for (uint32_t b = 0; b < 8; ++b)
            if (((kb.or_stop ^ kb.and_stop) >> (8 * b)) & 255) passes.push_back(Pass{stop, nullptr, 8 * b});
    for (uint32_t b = 0; b < 8; ++b)
        if (((kb.or_start ^ kb.and_start) >> (8 * b)) & 255) passes.push_back(Pass{start, nullptr, 8 * b});
    for (uint32_t b = 0; b < 4; ++b)
        if (((kb.or_rank ^ kb.and_rank) >> (8 * b)) & 255) passes.push_back(Pass{nullptr, rank, 8 * b});
    *passes_out = (uint32_t)passes.size();
    if (passes.empty()) return nullptr;
    const uint64_t ntiles = ceil_div(L, kSortTile);
    uint32_t* idx[2] = {b_idx[0].as<uint32_t>(L), b_idx[1].as<uint32_t>(L)};
    uint8_t* dig = b_digit.as<uint8_t>(L);
    uint32_t* hist = b_hist.as<uint32_t>(256 * ntiles);
    uint64_t* hist_off = b_hist_off.as<uint64_t>(256 * ntiles);
    int cur = 0;
    bool first = true;
    for (const Pass& p : passes) {
        const uint32_t* src = first ? nullptr : idx[cur];
        hipLaunchKernelGGL(k_sb_hist, dim3((unsigned)ntiles), dim3(kSortThreads), 0, st, src, p.k64, p.k32, p.shift, L,
                           ntiles, dig, hist);
        scan::excl_sum_u32_to_u64(hist, hist_off, 256 * ntiles, (uint64_t*)nullptr, b_tmp, st);
        hipLaunchKernelGGL(k_sb_scatter, dim3((unsigned)ntiles), dim3(kSortThreads), 0, st, src, dig, hist_off, L, ntiles,
                           idx[cur ^ 1]);
        cur ^= 1;
        first = false;
    }
    HIP_CHECK(hipGetLastError());
    return idx[cur];
}

uint64_t SortWorkspace::stage_gather(const uint8_t* d_bed, const uint32_t* order, uint64_t K, uint64_t bytes,
                                     uint32_t* long_list, hipStream_t st, DevBuf& out)
{
    if (K == 0) {
        (void)out.as<uint8_t>(64);
        return 0;
    }
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    unsigned long long* uscal = reinterpret_cast<unsigned long long*>(scal);
    const unsigned kblocks = blocks_for(K, kThreads);
    const uint64_t* line_end = ln.line_end;
    uint32_t* len = b_len.as<uint32_t>(K);
    uint64_t* out_off = b_out_off.as<uint64_t>(K);
    if (!long_list) long_list = b_long.as<uint32_t>(K);
    HIP_CHECK(hipMemsetAsync(scal + S_LONG, 0, sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_sb_len, dim3(kblocks), dim3(kThreads), 0, st, order, line_end, K, len);
    if (bytes == ~0ull) {
        scan::excl_sum_u32_to_u64(len, out_off, K, scal + S_GATHERED, b_tmp, st);
        HIP_CHECK(hipMemcpyAsync(&bytes, scal + S_GATHERED, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    } else {
        scan::excl_sum_u32_to_u64(len, out_off, K, (uint64_t*)nullptr, b_tmp, st);
    }
    uint8_t* o = out.as<uint8_t>(bytes + 64);
    hipLaunchKernelGGL(k_sb_copy, dim3(kblocks), dim3(kThreads), 0, st, d_bed, line_end, order, len, out_off, K, o, long_list,
                       uscal);
    hipLaunchKernelGGL(k_sb_copy_long, dim3((unsigned)std::min<uint64_t>(kblocks, 1024)), dim3(kThreads), 0, st, d_bed,
                       line_end, order, len, out_off, o, long_list, uscal);
    HIP_CHECK(hipGetLastError());
    return bytes;
}

void SortWorkspace::run(const uint8_t* d_bed, uint64_t n, hipStream_t st, bool check_only, DevBuf& out, SortResult& res)
{
    res = SortResult{};
    if (n == 0) return;
    timer.start(st);

    // 1. line index and parse
    uint64_t bad = 0;
    const uint64_t L = stage_parse(d_bed, n, st, &bad);
    res.n_lines = L;
    timer.mark(1, st);
    if (bad != ~0ull)
        throw StarchError(STARCH_ERR_DATA, "sort-bed: line " + std::to_string((bad >> 8) + 1) + ": " +
                                               bad_text((uint32_t)(bad & 255)));

    // 2. chromosome ranks
    stage_rank(d_bed, st);
    res.n_chromosomes = n_chromosomes;
    timer.mark(2, st);

    // 3. order check
    const KeyBits kb = stage_check(ln.rank, ln.start, ln.stop, L, st);
    res.already_sorted = kb.desc == ~0ull;
    res.first_unsorted_line = res.already_sorted ? 0 : kb.desc + 1;
    if (check_only) {
        timer.mark(3, st);
        timer.mark(4, st);
    } else {
        const bool open_end = ln.open_end;
        unsigned long long* uscal = reinterpret_cast<unsigned long long*>(b_scal.as<uint64_t>(S_COUNT));
        res.out_bytes = n + (open_end ? 1 : 0);
        uint8_t* o = out.as<uint8_t>(res.out_bytes + 64);
        if (res.already_sorted) {
            timer.mark(3, st);
            HIP_CHECK(hipMemcpyAsync(o, d_bed, n, hipMemcpyDeviceToDevice, st));
            if (open_end) HIP_CHECK(hipMemsetAsync(o + n, '\n', 1, st));
        } else {
            // 4. radix passes
            const unsigned lblocks = blocks_for(L, kThreads);
            const uint32_t* order = stage_radix(ln.rank, ln.start, ln.stop, L, kb, st, &res.radix_passes);
            uint32_t* spare = b_idx[0].as<uint32_t>(L);
            if (!order) {   // (an unsorted input has a varying byte; kept for safety)
                hipLaunchKernelGGL(k_sb_iota, dim3(lblocks), dim3(kThreads), 0, st, spare, L);
                order = spare;
                spare = b_idx[1].as<uint32_t>(L);
            } else if (order == spare) {
                spare = b_idx[1].as<uint32_t>(L);
            }
            HIP_CHECK(hipGetLastError());
            timer.mark(3, st);
            // 5. gather
            (void)stage_gather(d_bed, order, L, res.out_bytes, spare, st, out);
        }
        timer.mark(4, st);
    }
    timer.finish(5, st, {&res.ms_parse, &res.ms_rank, &res.ms_sort, &res.ms_gather});   // (every event is recorded)
    res.ms_total = timer.elapsed(0, 4);
}

}  // namespace sb
