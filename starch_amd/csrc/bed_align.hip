// starch_amd/csrc/bed_align.hip -- sam2bed, psl2bed and rmsk2bed on MI355X: SAM,
// PSL and RepeatMasker .out text into BED lines (the definitions:
// include/starch_amd.h).  The stages are those of bed_convert.hip, over the same
// skeleton (bed_records.hpp):
//   1. framing: the sort's line-end pass (sb::SortWorkspace::stage_frame).
//   2. PSL alone, k_al_psl_head: whether line 1 begins with psLayout, and the
//      first line that begins with ----- (an atomicMin), so that the
//      classification knows the header's end before it counts anything.
//   3. k_al_classify<format>, one thread per line: the line's class, the offsets
//      of its fields (relative to the line, 32 bits; a RepeatMasker line keeps
//      none, its tokens are found again when it is written), its parsed
//      coordinates, its number of output lines and their bytes.  A SAM line is
//      read up to the end of its CIGAR; a PSL line to its end (a 22nd field is an
//      error); a RepeatMasker line to its 17th token.  The lowest bad line is an
//      atomicMin of (line << 8) | kind.
//   4. br::place (k_br_tally): class counts, and with keep_header the bytes of
//      the header lines from the exclusive sum of (is header).  An exclusive sum of
//      the bytes places every line; k_al_write<format>, one thread per input line,
//      writes its output lines: several in the split modes, round after round
//      across the wave, from the same walk over the CIGAR (sam_next_run) or over
//      blockSizes and tStarts in step (list_next) that measured them.  A copied
//      tail (CIGAR to the end of a SAM line, blockCount to the end of a PSL line,
//      a kept header line) of sb::kWaveCopyBytes or more is left to the whole wave.
// All arithmetic is unsigned 64-bit integer.  A thread reads only bytes of its
// own line and writes only its own placed range.
#include "bed_align.hpp"

namespace al {
namespace {

using br::S_BAD, br::S_MARK, br::S_FLAG, br::S_OWN, br::S_HDR, br::S_REC, br::S_LINES, br::S_BYTES, br::C_BAD, br::C_HEADER, br::C_TOOL;
using br::K_LONG, br::K_ZERO, br::K_OVER, br::K_END, br::K_STOP, br::K_TOOL;
using br::dec_digits, br::is_blank, br::is_word, br::line_beg, br::Writer, br::parse_coord, br::token_is, br::tokens;
using br::drop_bad, br::store_line, br::header_line, br::reset_and_bind, br::first_of, br::First, br::throw_bad, br::place, br::Placed;
using bt::kLimit;

// PSL: the first line that begins with -----, whether line 1 begins with psLayout; SAM: the unmapped records left out
enum : int { S_DASH = S_MARK, S_PSL = S_FLAG, S_DROPPED = S_OWN };
// C_SPLIT: a SAM record written run by run; C_UNMAPPED: written as _unmapped; C_DROPPED: unmapped and left out
enum : uint8_t { C_REC = C_TOOL, C_SPLIT, C_UNMAPPED, C_DROPPED };
enum : uint32_t {
    K_FEW6 = K_TOOL, K_FLAG, K_RNAME, K_CIGAR, K_NODASH, K_FEW21, K_MANY21, K_FIELD, K_STRAND, K_LIST, K_BLOCK0, K_UNDER, K_TOKENS,
    K_RSTRAND
};
// slots of a line (Rec::fo).  SAM: the starts of fields 2 to 6 (FLAG, RNAME, POS,
// MAPQ, CIGAR), then the value of FLAG.  PSL: the starts of fields 2 to 21.
enum : uint32_t { O_FLAG = 5 };
enum : uint32_t { P_STRAND = 8, P_QNAME = 9, P_QSIZE = 10, P_QSTART = 11, P_TNAME = 13, P_TSIZE = 14, P_TSTART = 15, P_TEND = 16,
                  P_BLOCKS = 17, P_SIZES = 18, P_QSTARTS = 19, P_TSTARTS = 20, P_FIELDS = 21 };
constexpr uint32_t kMaxSlots = kSlotsPsl;

constexpr uint32_t slots_of(int format) { return format == STARCH_ALIGN_SAM ? kSlotsSam : (format == STARCH_ALIGN_PSL ? kSlotsPsl : 0u); }

struct Rec : br::Rec {     // a of a split PSL record: tSize
    uint32_t split, split_deletions, all_reads, reduced;
};

struct Tally {             // what k_br_tally counts
    static constexpr uint32_t kOwn = C_DROPPED;
    static __device__ bool record(uint32_t c) { return c == C_REC || c == C_SPLIT || c == C_UNMAPPED || c == C_DROPPED; }
};

// ---- the walks that the measuring and the writing pass share ----------------------------
// The next piece of the CIGAR at s[p, ...), which ends at a TAB or at n: its
// operator with its count in *c, 0 at the end, 0xff for anything else.
__device__ __forceinline__ uint32_t cigar_piece(const uint8_t* __restrict__ s, uint32_t n, uint32_t& p, uint64_t* c)
{
    if (p == n || s[p] == '\t') return 0;
    uint32_t d = 0;
    uint64_t x = 0;
    while (p < n && (uint32_t)s[p] - '0' <= 9u) {
        if (++d > 9) return 0xff;
        x = x * 10 + ((uint32_t)s[p] - '0');
        ++p;
    }
    if (d == 0 || p == n) return 0xff;
    const uint32_t op = s[p++];
    if (op == 'M' || op == 'I' || op == 'D' || op == 'N' || op == 'S' || op == 'H' || op == 'P' || op == '=' || op == 'X') {
        *c = x;
        return op;
    }
    return 0xff;
}

struct CigarWalk {         // where the walk stands: the next piece, and the run of M D = X it is in
    uint32_t p;
    uint64_t at, len;      // the run's start on the reference and its length so far
    bool bad = false;
};

// The next maximal run of M D = X with positive length: [*a, *b), or false at the
// end of the CIGAR (then w.at is the position after its last reference base) or
// with w.bad at a malformed piece.  N ends a run, D too with split_deletions.
__device__ __forceinline__ bool sam_next_run(const uint8_t* __restrict__ s, uint32_t n, CigarWalk& w, bool split_deletions,
                                             uint64_t* a, uint64_t* b)
{
    for (;;) {
        uint64_t c = 0;
        const uint32_t op = cigar_piece(s, n, w.p, &c);
        if (op == 0xff) { w.bad = true; return false; }
        const bool last = op == 0;
        if (last || op == 'N' || (split_deletions && op == 'D')) {
            const bool run = w.len != 0;
            *a = w.at;
            *b = w.at + w.len;
            w.at += w.len + c;   // sums of counts below 10^9 in a line below 2^32 bytes: below 2^62
            w.len = 0;
            if (run) return true;
            if (last) return false;
        } else if (op == 'M' || op == 'D' || op == '=' || op == 'X') {
            w.len += c;
        }
    }
}

// The next number of a comma-terminated list s[p, end): 0 with the number in *v, 1
// at the end of the list, 2 for anything else.
__device__ __forceinline__ uint32_t list_next(const uint8_t* __restrict__ s, uint32_t end, uint32_t& p, uint64_t* v)
{
    if (p == end) return 1;
    const uint32_t b = p;
    while (p < end && s[p] != ',') ++p;
    if (p == end) return 2;
    if (bt::parse_coord<2u, 2u, 2u>(s, b, p, v)) return 2;
    ++p;
    return 0;
}

// block k of a PSL record from its size and tStart: 0 and [*a, *b), or a kind
__device__ __forceinline__ uint32_t psl_block(uint64_t size, uint64_t t, bool reverse, uint64_t tsize, uint64_t* a, uint64_t* b)
{
    if (size == 0) return K_BLOCK0;
    if (reverse) {
        if (t + size > tsize) return K_UNDER;   // both below 2^63
        *a = tsize - t - size;
        *b = tsize - t;
    } else {
        *a = t;
        *b = t + size;
        if (*b > kLimit) return K_OVER;
    }
    return 0;
}

// ---- 3. classify and measure -----------------------------------------------------------
using Line = br::Line<kMaxSlots>;   // what k_al_classify leaves of a line

__device__ __forceinline__ void sam_line(const uint8_t* __restrict__ s, uint32_t n, const Rec& r, Line& ln)
{
    uint32_t nf = 1, p = 0;
    for (; p < n && nf < 6; ++p)   // stops at the start of CIGAR
        if (s[p] == '\t') ln.fo[nf++ - 1] = p + 1;
    if (nf < 6) { ln.kind = K_FEW6; return; }
    const uint32_t qname = ln.fo[0] - 1, flag_len = ln.fo[1] - 1 - ln.fo[0], mapq = ln.fo[4] - 1 - ln.fo[3], c0 = ln.fo[4];
    uint32_t rname = ln.fo[2] - 1 - ln.fo[1];
    uint64_t flag = 0;
    if (bt::parse_coord<K_FLAG, K_FLAG, K_FLAG>(s, ln.fo[0], ln.fo[1] - 1, &flag) || flag > 65535) { ln.kind = K_FLAG; return; }
    ln.fo[O_FLAG] = (uint32_t)flag;
    uint64_t start = 0, stop = 1, digits = 0;
    uint32_t cnt = 1, cls = C_REC;
    if (flag & 4) {
        if (!r.all_reads) { ln.cls = C_DROPPED; return; }
        cls = C_UNMAPPED;
        rname = 9;   // _unmapped
    } else {
        if (rname == 0 || (rname == 1 && s[ln.fo[1]] == '*')) { ln.kind = K_RNAME; return; }
        uint64_t pos = 0;
        if ((ln.kind = parse_coord(s, ln.fo[2], ln.fo[3] - 1, &pos))) return;
        if (pos < 1) { ln.kind = K_ZERO; return; }
        start = pos - 1;
        uint32_t runs = 0;
        uint64_t end = start;   // the position after the last reference base
        if (c0 == n || s[c0] == '\t') { ln.kind = K_CIGAR; return; }
        if (!(s[c0] == '*' && (c0 + 1 == n || s[c0 + 1] == '\t'))) {
            CigarWalk w{c0, start, 0};
            uint64_t ra = 0, rb = 0;
            while (sam_next_run(s, n, w, r.split_deletions != 0, &ra, &rb)) {
                ++runs;
                digits += dec_digits(ra) + dec_digits(rb);
            }
            if (w.bad) { ln.kind = K_CIGAR; return; }
            end = w.at;
        }
        stop = end > start ? end : start + 1;
        if (stop > kLimit) { ln.kind = K_OVER; return; }
        if (r.split && runs) {
            cls = C_SPLIT;
            cnt = runs;
        }
    }
    if (cls != C_SPLIT) digits = dec_digits(start) + dec_digits(stop);
    // RNAME start stop QNAME FLAG strand [MAPQ CIGAR...]: five TABs, the strand, and '\n' or TAB MAPQ TAB tail '\n'
    const uint64_t fixed = (uint64_t)rname + qname + flag_len + 6 + (r.reduced ? 1ull : (uint64_t)mapq + 3 + (n - c0));
    ln.cls = cls;
    ln.a = start;
    ln.b = stop;
    ln.cnt = cnt;
    ln.ob = cnt * fixed + digits;
}

__device__ __forceinline__ void psl_line(const uint8_t* __restrict__ s, uint32_t n, const Rec& r, Line& ln)
{
    uint32_t nf = 1;
    for (uint32_t p = 0; p < n; ++p)
        if (s[p] == '\t') {
            if (nf == P_FIELDS) { ln.kind = K_MANY21; return; }
            ln.fo[nf++ - 1] = p + 1;
        }
    if (nf < P_FIELDS) { ln.kind = K_FEW21; return; }
    // field k is s[fb(k), fe(k))
    auto fb = [&](uint32_t k) { return k ? ln.fo[k - 1] : 0u; };
    auto fe = [&](uint32_t k) { return k + 1 < P_FIELDS ? ln.fo[k] - 1 : n; };
    for (uint32_t k = 0; k < P_FIELDS; ++k)
        if (fb(k) == fe(k)) { ln.kind = K_FIELD; return; }
    uint64_t tstart = 0, tend = 0, tsize = 0, blocks = 0;
    if ((ln.kind = parse_coord(s, fb(P_TSIZE), fe(P_TSIZE), &tsize))) return;
    if ((ln.kind = parse_coord(s, fb(P_TSTART), fe(P_TSTART), &tstart))) return;
    if ((ln.kind = parse_coord(s, fb(P_TEND), fe(P_TEND), &tend))) return;
    if ((ln.kind = parse_coord(s, fb(P_BLOCKS), fe(P_BLOCKS), &blocks))) return;
    const uint32_t s0 = fb(P_STRAND), sl = fe(P_STRAND) - s0;
    bool sok = sl == 1 || sl == 2;
    for (uint32_t k = 0; sok && k < sl; ++k) sok = s[s0 + k] == '+' || s[s0 + k] == '-';
    if (!sok) { ln.kind = K_STRAND; return; }
    if (tstart >= tend) { ln.kind = K_STOP; return; }
    // all of the line with tStart and tEnd written anew, and '\n'
    const uint64_t fixed = (uint64_t)n + 1 - (fe(P_TSTART) - fb(P_TSTART)) - (fe(P_TEND) - fb(P_TEND));
    ln.cls = C_REC;
    ln.a = tstart;
    ln.b = tend;
    ln.cnt = 1;
    ln.ob = fixed + dec_digits(tstart) + dec_digits(tend);
    if (!r.split) return;
    const bool reverse = sl == 2 && s[s0 + 1] == '-';
    uint32_t p1 = fb(P_SIZES), p2 = fb(P_TSTARTS);
    const uint32_t e1 = fe(P_SIZES), e2 = n;
    uint64_t digits = 0, size = 0, t = 0, ba = 0, bb = 0;
    for (uint64_t k = 0; k < blocks; ++k) {
        if (list_next(s, e1, p1, &size) || list_next(s, e2, p2, &t)) { ln.kind = K_LIST; return; }
        if ((ln.kind = psl_block(size, t, reverse, tsize, &ba, &bb))) return;
        digits += dec_digits(ba) + dec_digits(bb);
    }
    if (list_next(s, e1, p1, &size) != 1 || list_next(s, e2, p2, &t) != 1) { ln.kind = K_LIST; return; }
    ln.a = tsize;
    ln.cnt = (uint32_t)blocks;   // at least two bytes of the line each
    ln.ob = blocks * fixed + digits;
}

__device__ __forceinline__ void rmsk_line(const uint8_t* __restrict__ s, uint32_t n, Line& ln)
{
    uint32_t ts[16], te[16];
    const uint32_t nt = tokens(s, n, ts, te);   // 17: more than 16
    if (nt == 0 || token_is(s, ts[0], te[0], "SW", 2) || token_is(s, ts[0], te[0], "score", 5)) { ln.cls = C_HEADER; return; }
    if (!(nt == 15 || (nt == 16 && token_is(s, ts[15], te[15], "*", 1)))) { ln.kind = K_TOKENS; return; }
    if (!(te[8] - ts[8] == 1 && (s[ts[8]] == '+' || s[ts[8]] == 'C'))) { ln.kind = K_RSTRAND; return; }
    uint64_t begin = 0, end = 0;
    if ((ln.kind = parse_coord(s, ts[5], te[5], &begin))) return;
    if ((ln.kind = parse_coord(s, ts[6], te[6], &end))) return;
    if (begin < 1) { ln.kind = K_ZERO; return; }
    if (end < begin) { ln.kind = K_END; return; }
    uint64_t bytes = nt;   // nt - 1 TABs and '\n'
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k)
        if (k != 5 && k != 6) bytes += te[k] - ts[k];
    ln.cls = C_REC;
    ln.a = begin - 1;
    ln.b = end;
    ln.cnt = 1;
    ln.ob = bytes + dec_digits(ln.a) + dec_digits(ln.b);
}

// PSL: whether line 1 begins with psLayout, and the first line that begins with -----
__global__ void __launch_bounds__(kThreads) k_al_psl_head(const Rec r)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= r.L) return;
    const uint64_t b = line_beg(r.line_end, i), n = r.line_end[i] - 1 - b;
    const uint8_t* s = r.in + b;
    if (i == 0 && n >= 8 && is_word(s, "psLayout", 8)) r.scal[S_PSL] = 1;
    if (n >= 5 && is_word(s, "-----", 5)) atomicMin(&r.scal[S_DASH], (unsigned long long)i);
}

template <int kFormat>
__global__ void __launch_bounds__(kThreads) k_al_classify(const Rec r)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= r.L) return;
    const uint64_t b = line_beg(r.line_end, i), e = r.line_end[i] - 1;
    const uint8_t* s = r.in + b;
    Line ln;
    if (e - b >= 0xffffffffull) ln.kind = K_LONG;
    else if (kFormat == STARCH_ALIGN_SAM) {
        if (e == b || s[0] == '@') ln.cls = C_HEADER;
        else sam_line(s, (uint32_t)(e - b), r, ln);
    } else if (kFormat == STARCH_ALIGN_PSL) {
        const unsigned long long dash = r.scal[S_DASH];
        if (r.scal[S_PSL] && i <= dash) {
            ln.cls = C_HEADER;
            if (i == 0 && dash == ~0ull) ln.kind = K_NODASH;
        }
        else if (e == b) ln.cls = C_HEADER;
        else psl_line(s, (uint32_t)(e - b), r, ln);
    } else {
        rmsk_line(s, (uint32_t)(e - b), ln);
    }
    drop_bad(r, i, ln);   // (two calls on purpose: merged into one function the kernel is other code, bed_records.hpp)
    store_line<slots_of(kFormat)>(r, i, ln);
}

// ---- 4. output ---------------------------------------------------------------------------
// A thread writes the output lines of its input line, one per round; a tail of
// kWaveCopyBytes or more is left to the whole wave, line after line.
template <int kFormat>
__global__ void __launch_bounds__(kThreads)
k_al_write(const Rec r, const uint64_t* __restrict__ hord, const uint64_t* __restrict__ off, uint64_t out_bytes,
           uint8_t* __restrict__ out)
{
    constexpr uint32_t kSlots = slots_of(kFormat);
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < r.L;
    uint32_t nout = valid ? r.cnt[i] : 0u;
    if (nout && off[i] + r.ob[i] > out_bytes) nout = 0;
    const uint64_t b = valid ? line_beg(r.line_end, i) : 0;
    const uint8_t* s = r.in + b;
    const uint32_t n = valid ? (uint32_t)(r.line_end[i] - 1 - b) : 0u;
    const uint32_t cls = nout ? r.cls[i] : (uint32_t)C_BAD;
    uint32_t f[kSlots + 1];   // f[k]: where field k starts (SAM, PSL); SAM: f[O_FLAG + 1] is FLAG
    f[0] = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSlots; ++k) f[k + 1] = nout ? r.fo[(uint64_t)k * r.L + i] : 0u;
    uint64_t start = nout ? r.a[i] : 0, stop = nout ? r.b[i] : 0;
    Writer<> w{out, nout ? off[i] : 0};
    // where the walks of a split record stand
    CigarWalk cw{0, start, 0};
    const bool psl_split = kFormat == STARCH_ALIGN_PSL && r.split && cls == C_REC;
    const uint64_t tsize = start;   // of a split PSL record
    uint32_t p1 = 0, p2 = 0;
    bool reverse = false;
    uint32_t ts[16] = {}, te[16] = {};   // RepeatMasker: the tokens
    uint32_t nt = 0;
    if constexpr (kFormat == STARCH_ALIGN_SAM) cw.p = f[5];
    if constexpr (kFormat == STARCH_ALIGN_PSL) {
        p1 = f[P_SIZES];
        p2 = f[P_TSTARTS];
        reverse = psl_split && f[P_QNAME] - 1 - f[P_STRAND] == 2 && s[f[P_STRAND] + 1] == '-';
    }
    if constexpr (kFormat == STARCH_ALIGN_RMSK) {
        if (cls == C_REC) nt = tokens(s, n, ts, te);
    }
    for (uint32_t round = 0; __ballot(round < nout) != 0; ++round) {
        w.big_len[0] = 0;
        if (round < nout) {
            if (cls == C_HEADER) {
                header_line(w, hord[i], s, n);
            } else if constexpr (kFormat == STARCH_ALIGN_SAM) {
                if (cls == C_SPLIT) (void)sam_next_run(s, n, cw, r.split_deletions != 0, &start, &stop);
                if (cls == C_UNMAPPED) w.bytes(reinterpret_cast<const uint8_t*>("_unmapped"), 9);
                else w.bytes(s + f[2], f[3] - 1 - f[2]);
                w.tab();
                w.dec(start);
                w.tab();
                w.dec(stop);
                w.tab();
                w.bytes(s, f[2]);   // QNAME, FLAG and their TABs
                w.out[w.o++] = (f[O_FLAG + 1] & 16) ? '-' : '+';
                if (r.reduced) w.out[w.o++] = '\n';
                else {
                    w.tab();
                    w.bytes(s + f[4], f[5] - f[4]);   // MAPQ and its TAB
                    w.tail(s + f[5], n - f[5]);       // CIGAR and every column after it
                }
            } else if constexpr (kFormat == STARCH_ALIGN_PSL) {
                if (psl_split) {   // the lists were checked when they were measured
                    uint64_t size = 0, t = 0;
                    (void)list_next(s, f[P_QSTARTS] - 1, p1, &size);
                    (void)list_next(s, n, p2, &t);
                    (void)psl_block(size, t, reverse, tsize, &start, &stop);
                }
                w.bytes(s + f[P_TNAME], f[P_TSIZE] - f[P_TNAME]);       // tName and its TAB
                w.dec(start);
                w.tab();
                w.dec(stop);
                w.tab();
                w.bytes(s + f[P_QNAME], f[P_QSIZE] - f[P_QNAME]);       // qName
                w.bytes(s, f[1]);                                       // matches
                w.bytes(s + f[P_STRAND], f[P_QNAME] - f[P_STRAND]);     // strand
                w.bytes(s + f[P_QSIZE], f[P_QSTART] - f[P_QSIZE]);      // qSize
                w.bytes(s + f[1], f[P_STRAND] - f[1]);                  // misMatches to tBaseInsert
                w.bytes(s + f[P_QSTART], f[P_TNAME] - f[P_QSTART]);     // qStart, qEnd
                w.bytes(s + f[P_TSIZE], f[P_TSTART] - f[P_TSIZE]);      // tSize
                w.tail(s + f[P_BLOCKS], n - f[P_BLOCKS]);               // blockCount and the three lists
            } else {
                auto tok = [&](uint32_t k) { w.bytes(s + ts[k], te[k] - ts[k]); w.tab(); };
                tok(4);       // query
                w.dec(start);
                w.tab();
                w.dec(stop);
                w.tab();
                tok(9);       // repeat
                tok(0);       // score
                w.out[w.o++] = s[ts[8]] == 'C' ? '-' : '+';
                w.tab();
                tok(1);
                tok(2);
                tok(3);
                tok(7);       // (left)
                tok(10);      // class/family
                tok(11);
                tok(12);
                tok(13);
                if (nt == 16) { tok(14); w.tail(s + ts[15], te[15] - ts[15]); }
                else w.tail(s + ts[14], te[14] - ts[14]);
            }
        }
        bt::wave_copy_tails(w, out, lane);
    }
}

template <int kFormat>
void launch_format(const Rec& r, const uint64_t* hord, const uint64_t* off, uint64_t bytes, uint8_t* o, bool write, hipStream_t st)
{
    const dim3 grid(blocks_for(r.L, kThreads)), block(kThreads);
    if (write) hipLaunchKernelGGL(k_al_write<kFormat>, grid, block, 0, st, r, hord, off, bytes, o);
    else hipLaunchKernelGGL(k_al_classify<kFormat>, grid, block, 0, st, r);
}

void launch(uint32_t format, const Rec& r, const uint64_t* hord, const uint64_t* off, uint64_t bytes, uint8_t* o, bool write,
            hipStream_t st)
{
    switch (format) {
        case STARCH_ALIGN_SAM: launch_format<STARCH_ALIGN_SAM>(r, hord, off, bytes, o, write, st); break;
        case STARCH_ALIGN_PSL: launch_format<STARCH_ALIGN_PSL>(r, hord, off, bytes, o, write, st); break;
        default: launch_format<STARCH_ALIGN_RMSK>(r, hord, off, bytes, o, write, st); break;
    }
    HIP_CHECK(hipGetLastError());
}

const char* bad_text(uint32_t k)
{
    switch (k) {
        case K_FEW6: return "fewer than six tab-separated fields";
        case K_FLAG: return "FLAG is not a decimal number from 0 to 65535";
        case K_RNAME: return "mapped record without a reference name";
        case K_CIGAR: return "CIGAR is not * or pieces of a count of 1 to 9 digits and one of MIDNSHP=X";
        case K_NODASH: return "psLayout header without a line of dashes";
        case K_FEW21: return "fewer than 21 tab-separated fields";
        case K_MANY21: return "more than 21 tab-separated fields";
        case K_FIELD: return "empty field";
        case K_STRAND: return "strand is not +, - or two of them";
        case K_LIST: return "blockSizes and tStarts do not hold blockCount comma-terminated numbers";
        case K_BLOCK0: return "block of size 0";
        case K_UNDER: return "block start and size exceed tSize on the reverse strand";
        case K_TOKENS: return "a record has 15 tokens, or 16 with a last *";
        case K_RSTRAND: return "strand is not + or C";
        default: return br::bad_text(k);
    }
}

}  // namespace

const char* command_of(uint32_t format)
{
    return format == STARCH_ALIGN_SAM ? "sam2bed" : (format == STARCH_ALIGN_PSL ? "psl2bed" : "rmsk2bed");
}

void AlignWorkspace::run(sb::SortWorkspace& sorter, const AlignOptions& opt, const uint8_t* d_in, uint64_t n, hipStream_t st,
                         DevBuf& out, AlignResult& res)
{
    res = AlignResult{};
    (void)out.as<uint8_t>(64);
    timer.start(st);
    auto finish = [&](int from) { timer.finish(from, st, {&res.ms_frame, &res.ms_parse, &res.ms_write}); };
    if (n == 0) return finish(1);

    // 1. framing
    const uint64_t L = sorter.stage_frame(d_in, n, st);
    res.n_lines = L;
    timer.mark(1, st);

    // 2, 3. the PSL header's end; classify and measure
    const char* command = command_of(opt.format);
    Rec r{};
    reset_and_bind(rb, r, d_in, sorter.ln.line_end, L, slots_of((int)opt.format), st);
    r.split = opt.split;
    r.split_deletions = opt.split_deletions;
    r.all_reads = opt.all_reads;
    r.reduced = opt.reduced;
    r.keep_header = opt.keep_header;
    if (opt.format == STARCH_ALIGN_PSL) {
        hipLaunchKernelGGL(k_al_psl_head, dim3(blocks_for(L, kThreads)), dim3(kThreads), 0, st, r);
        HIP_CHECK(hipGetLastError());
    }
    launch(opt.format, r, nullptr, nullptr, 0, nullptr, false, st);
    const First first = first_of(rb, st);
    if (first.bad != ~0ull) throw_bad(command, first.bad, bad_text);

    // 4. header ordinals, counts, places
    const Placed p = place<Tally>(rb, r, L, command, st);
    res.header_lines = p.tot[S_HDR];
    res.records = p.tot[S_REC];
    res.unmapped_dropped = p.tot[S_DROPPED];
    timer.mark(2, st);
    const uint64_t bytes = p.tot[S_BYTES];
    if (bytes) {
        uint8_t* o = out.as<uint8_t>(bytes + 64);
        launch(opt.format, r, p.hord, p.off, bytes, o, true, st);
    }
    res.lines_out = p.tot[S_LINES];
    res.out_bytes = bytes;
    finish(3);
}

}  // namespace al
