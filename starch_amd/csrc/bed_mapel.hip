// starch_amd/csrc/bed_mapel.hip -- bedmap-elements on MI355X: for every line of
// a sorted reference, the list of the lines of a sorted map that satisfy an
// overlap criterion, and the columns written from it (include/starch_amd.h has
// the definition).
//
// Both inputs lie back to back in one buffer; the reference is input 0.  Stages:
//   1. bed_setops.hip's stage_lines over the whole buffer: framing, parse,
//      global chromosome ranks, stop > start and the per-input order.
//   2. map arrays.  A, S: the map starts and stops in map order; rank r's lines
//      are [mlo[r], mlo[r + 1]).  M: the largest stop from the chromosome's
//      first line to each line (stage_merge's running maximum).  The hierarchy
//      of maxima over S (bed_hier.hpp).
//   3. k_me_find, one thread per reference line with window [s', e'), run
//      twice: first to count the hits, then -- after a 64-bit exclusive sum of
//      the counts -- to write them.  The candidates are
//        the span set: map lines with a < s' and b > s'.  They lie in
//            [pf, j0), j0 = #{a < s'}, pf the first line with M > t.  From
//            p = pf on, next_above finds the first j >= p with S[j] > t through
//            the hierarchy: up from p while no item exceeds t, then down into
//            the item that does, kFanout items per level at most each way, so
//            the cost of a candidate does not depend on the lines it skips.
//            t = s', or s' + n - 1 under BP_OVR n (a line that spans s' has
//            ov >= n exactly when b reaches s' + n, given a window of n bases).
//        the run: map lines with a in [s', e'), [j0, j1), all candidates.  Below
//            kHeavy lines the thread tests them one by one; from kHeavy on the
//            whole wave does, 64 contiguous lines at a time, and places the
//            hits by ballot.
//      Hits come out in map order: the span set lies before the run.  The fill
//      pass also leaves the reference line of every hit and the largest stop
//      among a line's hits.
//   4. format.  k_me_hit_len: per hit and list column a byte length, and the
//      lowest hit that lacks a column it is asked for.  One exclusive sum per
//      list column over all hits (a line's part is the difference of two
//      entries).  k_me_len and the exclusive sum over the lines give the line
//      offsets; k_me_write_line writes the per-line columns and delimiters and
//      leaves where each list column begins; k_me_write_hit, one thread per
//      hit, writes its pieces.  The writer and its wave copy are bed_text.hpp's,
//      the host steps from the line lengths to the sized output format_tail's
//      (common.hpp); both are shared with every BED command.
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/starch_amd.h"
#include "bed_hier.hpp"
#include "bed_mapel.hpp"
#include "bed_search.hpp"
#include "bed_text.hpp"

namespace me {
namespace {

using bc::Hier;
using bc::kFanout;
using bc::kFanShift;

constexpr int kThreads = 256;
constexpr uint64_t kNone = ~0ull;
enum : int { S_BYTES = 0, S_KEPT, S_HEAVY, S_STEPS, S_BAD, S_COUNT = 8 };   // device scalars (u64)
enum : int { L_MAP = 0, L_ID, L_SCORE, L_SIZE, L_OVR };                      // list slots: code - STARCH_MAPEL_ECHO_MAP

using bt::dec_digits;
using bt::line_beg;

// ---- 3. hits --------------------------------------------------------------------------
struct Crit {
    uint32_t code;
    uint64_t n, range, num, den;
};

// x * y >= u * v in 128 bits
__device__ __forceinline__ bool prod_ge(uint64_t x, uint64_t y, uint64_t u, uint64_t v)
{
    const uint64_t h1 = __umul64hi(x, y), l1 = x * y, h2 = __umul64hi(u, v), l2 = u * v;
    return h1 > h2 || (h1 == h2 && l1 >= l2);
}

// the candidate (a, b) of the reference line (s, e) with window [sp, ep): a < ep and b > sp hold
__device__ __forceinline__ bool is_hit(const Crit& c, uint64_t a, uint64_t b, uint64_t s, uint64_t e, uint64_t sp, uint64_t ep)
{
    const uint64_t ov = (b < ep ? b : ep) - (a > sp ? a : sp);
    switch (c.code) {
        case STARCH_MAPEL_CRIT_BP_OVR: return ov >= c.n;
        case STARCH_MAPEL_CRIT_RANGE: return true;
        case STARCH_MAPEL_CRIT_EXACT: return a == s && b == e;
        case STARCH_MAPEL_CRIT_FRACTION_REF: return prod_ge(ov, c.den, c.num, e - s);
        case STARCH_MAPEL_CRIT_FRACTION_MAP: return prod_ge(ov, c.den, c.num, b - a);
        case STARCH_MAPEL_CRIT_FRACTION_BOTH: return prod_ge(ov, c.den, c.num, e - s) && prod_ge(ov, c.den, c.num, b - a);
        default: return prod_ge(ov, c.den, c.num, e - s) || prod_ge(ov, c.den, c.num, b - a);   // FRACTION_EITHER
    }
}

// bm::lower and bm::upper with their probes counted
__device__ __forceinline__ uint64_t lower_c(const uint64_t* __restrict__ v, uint64_t lo, uint64_t hi, uint64_t x, uint64_t& steps)
{
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        ++steps;
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t upper_c(const uint64_t* __restrict__ v, uint64_t lo, uint64_t hi, uint64_t x, uint64_t& steps)
{
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        ++steps;
        if (v[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The first j >= p with S[j] > t, over the whole of S (kNone: there is none);
// p < cnt[0].  Item i of level k covers the stops [i << (k * kFanShift),
// (i + 1) << (k * kFanShift)).  Up: at every level the items from `cur` to the
// end of its group, left to right -- everything left of them has been ruled
// out, so the first item that exceeds t holds the answer.  Down: the first
// child that exceeds t.  Each loop runs kFanout times at most.  The caller
// compares the answer with the end of its range: the items may reach past it.
__device__ __forceinline__ uint64_t next_above(const Hier& h, uint64_t p, uint64_t t, uint64_t& steps)
{
    uint64_t cur = p, hit = kNone;
    int lv = 0;
    for (;;) {
        const uint64_t* __restrict__ v = h.lev[lv];
        const uint64_t ge = (cur | (uint64_t)(kFanout - 1)) + 1;
        const uint64_t ce = ge < h.cnt[lv] ? ge : h.cnt[lv];
        for (uint64_t i = cur; i < ce; ++i) {
            ++steps;
            if (v[i] > t) { hit = i; break; }
        }
        if (hit != kNone) break;
        if (lv + 1 >= h.nlev) return kNone;
        cur = (cur >> kFanShift) + 1;
        ++lv;
        if (cur >= h.cnt[lv]) return kNone;
    }
    while (lv > 0) {
        --lv;
        const uint64_t* __restrict__ v = h.lev[lv];
        const uint64_t cs = hit << kFanShift;
        const uint64_t ce = cs + kFanout < h.cnt[lv] ? cs + kFanout : h.cnt[lv];
        hit = cs;   // not kept: the parent's maximum is one of these
        for (uint64_t i = cs; i < ce; ++i) {
            ++steps;
            if (v[i] > t) { hit = i; break; }
        }
    }
    return hit;
}

struct Find {
    const uint32_t* rank;                 // of the reference lines (input 0: lines [0, Lr))
    const uint64_t *start, *stop;
    uint64_t Lr, Lm;
    const uint64_t *mlo, *A, *S, *M;
    Hier h;
    Crit crit;
    uint64_t* cnt;                        // count pass: hits per reference line
    const uint64_t* hoff;                 // fill pass: where a line's hits begin
    uint64_t T;                           // fill pass: the hits in all
    uint32_t *H, *R;                      // fill pass: per hit the map line and the reference line
    uint64_t* rmax;                       // fill pass: per reference line the largest stop of its hits
    unsigned long long* scal;             // count pass: S_HEAVY and S_STEPS are counted up
};

template <bool FILL>
__global__ void __launch_bounds__(kTileRefs)
k_me_find(const Find f)
{
    const int lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * kTileRefs + threadIdx.x;
    const bool valid = i < f.Lr;
    uint64_t s = 0, e = 0, sp = 0, ep = 0, j0 = 0, j1 = 0, n = 0, mx = 0;
    const uint64_t base = FILL && valid ? f.hoff[i] : 0;
    uint64_t steps = 0;
    bool heavy = false;
    auto take = [&](uint64_t j, uint64_t b) {
        if (FILL && base + n < f.T) { f.H[base + n] = (uint32_t)j; f.R[base + n] = (uint32_t)i; }
        mx = b > mx ? b : mx;
        ++n;
    };
    if (valid) {
        const uint32_t rk = f.rank[i];
        s = f.start[i];
        e = f.stop[i];
        sp = s > f.crit.range ? s - f.crit.range : 0;
        ep = e + f.crit.range < e ? ~0ull : e + f.crit.range;
        const uint64_t lo = f.mlo[rk], hi = f.mlo[rk + 1];
        const bool bp = f.crit.code == STARCH_MAPEL_CRIT_BP_OVR;
        if (lo < hi && !(bp && f.crit.n > ep - sp)) {
            j0 = lower_c(f.A, lo, hi, sp, steps);
            j1 = lower_c(f.A, j0, hi, ep, steps);
            if (f.crit.code != STARCH_MAPEL_CRIT_EXACT && j0 > lo) {   // the span set
                const uint64_t t = bp ? sp + (f.crit.n - 1) : sp;
                uint64_t p = upper_c(f.M, lo, j0, t, steps);
                while (p < j0) {
                    p = next_above(f.h, p, t, steps);
                    if (p >= j0) break;
                    const uint64_t b = f.S[p];
                    if (is_hit(f.crit, f.A[p], b, s, e, sp, ep)) take(p, b);
                    ++p;
                }
            }
            heavy = j1 - j0 >= kHeavy;
            if (!heavy)
                for (uint64_t j = j0; j < j1; ++j) {
                    const uint64_t b = f.S[j];
                    if (is_hit(f.crit, f.A[j], b, s, e, sp, ep)) take(j, b);
                }
        }
    }
    // the runs of kHeavy lines or more, one after the other, by the whole wave
    const unsigned long long hm = __ballot(heavy);
    unsigned long long m = hm;
    while (m) {
        const int l = __ffsll(m) - 1;
        m &= m - 1;
        const uint64_t ws = __shfl(s, l, 64), we = __shfl(e, l, 64), wsp = __shfl(sp, l, 64), wep = __shfl(ep, l, 64);
        const uint64_t w0 = __shfl(j0, l, 64), w1 = __shfl(j1, l, 64), wb = __shfl(base + n, l, 64), wi = __shfl(i, l, 64);
        uint64_t got = 0, lmx = 0;
        for (uint64_t jb = w0; jb < w1; jb += 64) {
            const uint64_t j = jb + lane;
            bool hit = false;
            if (j < w1) {
                const uint64_t b = f.S[j];
                hit = is_hit(f.crit, f.A[j], b, ws, we, wsp, wep);
                if (hit) lmx = b > lmx ? b : lmx;
            }
            const unsigned long long bm = __ballot(hit);
            if (FILL && hit) {
                const uint64_t pos = wb + got + __popcll(bm & ((1ull << lane) - 1));
                if (pos < f.T) { f.H[pos] = (uint32_t)j; f.R[pos] = (uint32_t)wi; }
            }
            got += __popcll(bm);
        }
        for (int d = 32; d > 0; d >>= 1) {
            const uint64_t o = __shfl_xor(lmx, d, 64);
            lmx = o > lmx ? o : lmx;
        }
        if (lane == l) { n += got; mx = lmx > mx ? lmx : mx; }
    }
    if (FILL) {
        if (valid && n) f.rmax[i] = mx;
        return;
    }
    if (valid) f.cnt[i] = n;
    uint64_t ws = steps;
    for (int d = 32; d > 0; d >>= 1) ws += __shfl_xor(ws, d, 64);
    if (lane == 0) {
        if (ws) atomicAdd(f.scal + S_STEPS, (unsigned long long)ws);
        if (hm) atomicAdd(f.scal + S_HEAVY, (unsigned long long)__popcll(hm));
    }
}

// ---- 4. format ------------------------------------------------------------------------
struct Format {
    const uint8_t* bed;
    const uint64_t *line_end, *start, *stop;   // of every line of the buffer; map line j is line m0 + j
    const uint32_t* chr_len;
    const uint64_t *cnt, *hoff;                // hoff: Lr + 1 entries
    const uint32_t *H, *R;
    const uint64_t* rmax;
    uint32_t* lens[kListCols];                 // per hit, of the list columns asked for
    uint64_t* P[kListCols];                    // their exclusive sums over all hits, T + 1 entries
    uint64_t* cs[kListCols];                   // per reference line: where the list column begins in the output
    uint64_t Lr, m0, T, range;
    MapelOptions opt;
    uint32_t slots;                            // bit k: list slot k is asked for
    unsigned long long* scal;
};

// field k (from 0) of the line bed[lb, le): false when the line has k fields or fewer
__device__ __forceinline__ bool field(const uint8_t* __restrict__ bed, uint64_t lb, uint64_t le, int k, uint64_t* fb, uint64_t* fe)
{
    uint64_t p = lb;
    for (int c = 0; c < k; ++c) {
        while (p < le && bed[p] != '\t') ++p;
        if (p == le) return false;
        ++p;
    }
    *fb = p;
    while (p < le && bed[p] != '\t') ++p;
    *fe = p;
    return true;
}

// the bytes that list slot k copies for map line g (length 0 when the column is missing), or the number it prints
__device__ __forceinline__ bool piece(const Format& f, int k, uint64_t i, uint64_t g, uint64_t* src, uint64_t* len, uint64_t* num)
{
    const uint64_t lb = line_beg(f.line_end, g), le = f.line_end[g] - 1;
    *src = lb;
    *len = 0;
    *num = 0;
    if (k == L_MAP) { *len = le - lb; return true; }
    if (k == L_ID || k == L_SCORE) {
        uint64_t fb = 0, fe = 0;
        if (!field(f.bed, lb, le, k == L_ID ? 3 : 4, &fb, &fe)) return false;
        *src = fb;
        *len = fe - fb;
        return true;
    }
    const uint64_t a = f.start[g], b = f.stop[g];
    if (k == L_SIZE) *num = b - a;
    else {
        const uint64_t s = f.start[i], e = f.stop[i];
        const uint64_t sp = s > f.range ? s - f.range : 0, ep = e + f.range < e ? ~0ull : e + f.range;
        *num = (b < ep ? b : ep) - (a > sp ? a : sp);
    }
    *len = dec_digits(*num);
    return true;
}

__global__ void __launch_bounds__(kThreads)
k_me_hit_len(const Format f)
{
    const uint64_t h = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (h >= f.T) return;
    const uint64_t i = f.R[h], j = f.H[h];
    for (int k = 0; k < kListCols; ++k) {
        if (!((f.slots >> k) & 1)) continue;
        uint64_t src, len, num;
        if (!piece(f, k, i, f.m0 + j, &src, &len, &num)) atomicMin(f.scal + S_BAD, (unsigned long long)j);
        f.lens[k][h] = (uint32_t)len;
    }
}

// the bytes of "chrom:start-stop" or "chrom\tstart\tstop" of a line with chr bytes of name
__device__ __forceinline__ uint64_t bed3_len(uint32_t chr, uint64_t a, uint64_t b) { return (uint64_t)chr + 2 + dec_digits(a) + dec_digits(b); }

// len: bytes of output line i with its '\n' (0: left out); keep (may be NULL): 1 when it is written
__global__ void __launch_bounds__(kThreads)
k_me_len(const Format f, uint64_t* __restrict__ len, uint32_t* __restrict__ keep)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= f.Lr) return;
    const uint64_t c = f.cnt[i];
    uint64_t n = 0;
    if (!(f.opt.skip_unmapped && c == 0)) {
        n = (uint64_t)f.opt.delim_len * (f.opt.ncols - 1) + 1;
        for (uint32_t k = 0; k < f.opt.ncols; ++k) {
            const uint32_t col = f.opt.cols[k];
            switch (col) {
                case STARCH_MAPEL_ECHO: n += f.line_end[i] - 1 - line_beg(f.line_end, i); break;
                case STARCH_MAPEL_COUNT: n += dec_digits(c); break;
                case STARCH_MAPEL_INDICATOR: n += 1; break;
                case STARCH_MAPEL_ECHO_REF_SIZE: n += dec_digits(f.stop[i] - f.start[i]); break;
                case STARCH_MAPEL_ECHO_REF_NAME: n += bed3_len(f.chr_len[i], f.start[i], f.stop[i]); break;
                case STARCH_MAPEL_ECHO_REF_ROW_ID: n += 3 + dec_digits(i + 1); break;
                case STARCH_MAPEL_ECHO_MAP_RANGE:
                    if (c) n += bed3_len(f.chr_len[i], f.start[f.m0 + f.H[f.hoff[i]]], f.rmax[i]);
                    break;
                default:   // a list column
                    if (c) {
                        const uint64_t* P = f.P[col - STARCH_MAPEL_ECHO_MAP];
                        n += P[f.hoff[i + 1]] - P[f.hoff[i]] + (c - 1) * f.opt.multi_len;
                    }
            }
        }
    }
    len[i] = n;
    if (keep) keep[i] = n ? 1u : 0u;
}

// A thread writes the per-line columns and the delimiters of its line and
// leaves in cs where every list column begins; an echo of kWaveCopyBytes or
// more is left to the whole wave, line after line.
__global__ void __launch_bounds__(kThreads)
k_me_write_line(const Format f, const uint64_t* __restrict__ len, const uint64_t* __restrict__ off, uint64_t out_bytes,
                uint8_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bt::Writer<> w{out, 0};
    if (i < f.Lr && len[i] && off[i] + len[i] <= out_bytes) {
        const uint64_t c = f.cnt[i];
        w.o = off[i];
        auto chrom = [&] { w.bytes(f.bed + line_beg(f.line_end, i), f.chr_len[i]); };
        for (uint32_t k = 0; k < f.opt.ncols; ++k) {
            const uint32_t col = f.opt.cols[k];
            if (k) w.delim(f.opt.delim, f.opt.delim_len);
            switch (col) {
                case STARCH_MAPEL_ECHO: {
                    const uint64_t b = line_beg(f.line_end, i);
                    w.copy(0, f.bed + b, f.line_end[i] - 1 - b);
                    break;
                }
                case STARCH_MAPEL_COUNT: w.dec(c); break;
                case STARCH_MAPEL_INDICATOR: out[w.o++] = c ? '1' : '0'; break;
                case STARCH_MAPEL_ECHO_REF_SIZE: w.dec(f.stop[i] - f.start[i]); break;
                case STARCH_MAPEL_ECHO_REF_NAME:
                    chrom();
                    out[w.o++] = ':';
                    w.dec(f.start[i]);
                    out[w.o++] = '-';
                    w.dec(f.stop[i]);
                    break;
                case STARCH_MAPEL_ECHO_REF_ROW_ID:
                    w.bytes(reinterpret_cast<const uint8_t*>("id-"), 3);
                    w.dec(i + 1);
                    break;
                case STARCH_MAPEL_ECHO_MAP_RANGE:
                    if (c) {
                        chrom();
                        w.tab();
                        w.dec(f.start[f.m0 + f.H[f.hoff[i]]]);
                        w.tab();
                        w.dec(f.rmax[i]);
                    }
                    break;
                default: {   // a list column: its hits write it
                    const uint32_t slot = col - STARCH_MAPEL_ECHO_MAP;
                    f.cs[slot][i] = w.o;
                    if (c) w.o += f.P[slot][f.hoff[i + 1]] - f.P[slot][f.hoff[i]] + (c - 1) * f.opt.multi_len;
                }
            }
        }
        out[w.o] = '\n';
    }
    bt::wave_copy_tails(w, out, lane);
}

// A thread writes the pieces of its hit, each after its multi-delimiter unless
// it is the line's first; a copied piece of kWaveCopyBytes or more is left to
// the whole wave, one after another.
__global__ void __launch_bounds__(kThreads)
k_me_write_hit(const Format f, uint64_t out_bytes, uint8_t* __restrict__ out)
{
    const uint64_t h = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bt::Writer<3> w{out, 0};   // the cursor is set for every piece
    if (h < f.T) {
        const uint64_t i = f.R[h], g = f.m0 + f.H[h], h0 = f.hoff[i], r = h - h0;
        for (int k = 0; k < kListCols; ++k) {
            if (!((f.slots >> k) & 1)) continue;
            uint64_t src, n, num;
            (void)piece(f, k, i, g, &src, &n, &num);
            const uint64_t o = f.cs[k][i] + (f.P[k][h] - f.P[k][h0]) + r * f.opt.multi_len;
            if (o + n > out_bytes || o < r * f.opt.multi_len) continue;
            if (r) {
                w.o = o - f.opt.multi_len;
                w.delim(f.opt.multi, f.opt.multi_len);
            }
            w.o = o;
            if (k >= L_SIZE) w.dec(num, (uint32_t)n);
            else w.copy(k, f.bed + src, n);
        }
    }
    bt::wave_copy_tails(w, out, lane);
}

}  // namespace

int MapelWorkspace::hits(sb::SortWorkspace& sorter, so::SetopWorkspace& lines, const char* name, const MapelOptions& opt,
                         const uint8_t* d_cat, uint64_t n, const std::vector<uint64_t>& in_end, hipStream_t st, StageMarks tm,
                         HitList& hl)
{
    hl = HitList{};
    const uint64_t N = in_end.size();
    if (n == 0) return 0;   // both inputs are empty

    // 1. parse, ranks, checks; the reference is lines [0, Lr), the map [m0, m0 + Lm)
    std::vector<uint64_t> first;
    const uint64_t L = lines.stage_lines(sorter, name, d_cat, n, in_end, st, first);
    const uint64_t Lr = first[1], m0 = N == 2 ? Lr : 0, Lm = N == 2 ? L - Lr : L;
    if (Lr + Lm >= (1ull << 32))
        throw StarchError(STARCH_ERR_ARG, std::string(name) + ": 2^32 lines or more over reference and map");
    hl.Lr = Lr;
    hl.Lm = Lm;
    hl.m0 = m0;
    hl.n_chromosomes = sorter.n_chromosomes;
    tm.mark(0, st);
    if (Lr == 0) return 1;

    const uint64_t C = sorter.n_chromosomes;
    const uint32_t* rank = sorter.ln.rank;
    const uint64_t* start = sorter.ln.start;
    const uint64_t* stop = sorter.ln.stop;
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    HIP_CHECK(hipMemsetAsync(scal, 0, S_COUNT * sizeof(uint64_t), st));
    HIP_CHECK(hipMemsetAsync(scal + S_BAD, 0xff, sizeof(uint64_t), st));

    // 2. map arrays
    Find q{};
    q.rank = rank;
    q.start = start;
    q.stop = stop;
    q.Lr = Lr;
    q.Lm = Lm;
    q.A = start + m0;
    q.S = stop + m0;
    q.crit = Crit{opt.criterion, opt.n, opt.range, opt.frac_num, opt.frac_den};
    q.scal = reinterpret_cast<unsigned long long*>(scal);
    uint64_t* mlo = b_mlo.as<uint64_t>(C + 1);
    hipLaunchKernelGGL(bm::k_bm_bounds, dim3(blocks_for(C + 1, bm::kBoundsThreads)), dim3(bm::kBoundsThreads), 0, st, rank + m0,
                       Lm, C, mlo);
    HIP_CHECK(hipGetLastError());
    q.mlo = mlo;
    if (Lm) {
        (void)lines.stage_merge(start + m0, stop + m0, lines.head + m0, Lm, st);
        q.M = lines.incl;
        bc::build_hier(q.S, Lm, b_hier, st, name, &q.h);
    }
    tm.mark(1, st);

    // 3. count, scan, fill
    const unsigned qblocks = blocks_for(Lr, kTileRefs);
    uint64_t* cnt = b_cnt.as<uint64_t>(Lr);
    uint64_t* hoff = b_hoff.as<uint64_t>(Lr + 1);
    q.cnt = cnt;
    hipLaunchKernelGGL(k_me_find<false>, dim3(qblocks), dim3(kTileRefs), 0, st, q);
    HIP_CHECK(hipGetLastError());
    scan::excl_sum_u64(cnt, hoff, Lr, hoff + Lr, b_tmp, st);
    uint64_t T = 0, counted[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(&T, hoff + Lr, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(counted, scal + S_HEAVY, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    // (a line has fewer than 2^32 hits and there are fewer than 2^32 lines: the sum cannot wrap)
    if (T >= (1ull << 32)) throw StarchError(STARCH_ERR_ARG, std::string(name) + ": result too large (2^32 hits or more)");
    hl.T = T;
    hl.heavy_lines = counted[0];
    hl.walk_steps = counted[1];
    uint32_t* H = b_H.as<uint32_t>(T);
    uint32_t* R = b_R.as<uint32_t>(T);
    uint64_t* rmax = b_rmax.as<uint64_t>(Lr);
    if (T) {
        q.hoff = hoff;
        q.T = T;
        q.H = H;
        q.R = R;
        q.rmax = rmax;
        hipLaunchKernelGGL(k_me_find<true>, dim3(qblocks), dim3(kTileRefs), 0, st, q);
        HIP_CHECK(hipGetLastError());
    }
    tm.mark(2, st);
    hl.cnt = cnt;
    hl.hoff = hoff;
    hl.H = H;
    hl.R = R;
    hl.rmax = rmax;
    return 3;
}

void MapelWorkspace::run(sb::SortWorkspace& sorter, so::SetopWorkspace& lines, const MapelOptions& opt, const uint8_t* d_cat,
                         uint64_t n, const std::vector<uint64_t>& in_end, hipStream_t st, DevBuf& out, MapelResult& res)
{
    res = MapelResult{};
    const uint64_t N = in_end.size();
    (void)out.as<uint8_t>(64);
    timer.start(st);
    auto finish = [&](int from) { timer.finish(from, st, {&res.ms_parse, &res.ms_build, &res.ms_query, &res.ms_format}); };

    // 1 to 3. the hit list
    HitList hl;
    const int done = hits(sorter, lines, "bedmap-elements", opt, d_cat, n, in_end, st, timer.marks_from(1), hl);
    res.n_ref = hl.Lr;
    res.n_map = hl.Lm;
    res.n_chromosomes = hl.n_chromosomes;
    res.hits = hl.T;
    res.heavy_lines = hl.heavy_lines;
    res.walk_steps = hl.walk_steps;
    if (done < 3) return finish(done + 1);
    const uint64_t Lr = hl.Lr, m0 = hl.m0, T = hl.T;
    const uint64_t *start = sorter.ln.start, *stop = sorter.ln.stop, *cnt = hl.cnt, *hoff = hl.hoff, *rmax = hl.rmax;
    const uint32_t *H = hl.H, *R = hl.R;
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);

    // 4. format
    Format f{};
    f.bed = d_cat;
    f.line_end = sorter.ln.line_end;
    f.start = start;
    f.stop = stop;
    f.chr_len = sorter.ln.chr_len;
    f.cnt = cnt;
    f.hoff = hoff;
    f.H = H;
    f.R = R;
    f.rmax = rmax;
    f.Lr = Lr;
    f.m0 = m0;
    f.T = T;
    f.range = opt.range;
    f.opt = opt;
    f.scal = reinterpret_cast<unsigned long long*>(scal);
    for (uint32_t k = 0; k < opt.ncols; ++k)
        if (opt.cols[k] >= STARCH_MAPEL_ECHO_MAP && opt.cols[k] <= STARCH_MAPEL_ECHO_OVERLAP_SIZE)
            f.slots |= 1u << (opt.cols[k] - STARCH_MAPEL_ECHO_MAP);
    for (int k = 0; k < kListCols; ++k) {
        if (!((f.slots >> k) & 1)) continue;
        f.lens[k] = b_lens[k].as<uint32_t>(T);
        f.P[k] = b_P[k].as<uint64_t>(T + 1);
        f.cs[k] = b_cs[k].as<uint64_t>(Lr);
    }
    if (T && f.slots) {
        hipLaunchKernelGGL(k_me_hit_len, dim3(blocks_for(T, kThreads)), dim3(kThreads), 0, st, f);
        HIP_CHECK(hipGetLastError());
        for (int k = 0; k < kListCols; ++k)
            if ((f.slots >> k) & 1) scan::excl_sum_u32_to_u64(f.lens[k], f.P[k], T, f.P[k] + T, b_tmp, st);
        if (f.slots & ((1u << L_ID) | (1u << L_SCORE))) {
            uint64_t bad = kNone;
            HIP_CHECK(hipMemcpyAsync(&bad, scal + S_BAD, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (bad != kNone)
                throw StarchError(STARCH_ERR_DATA, "bedmap-elements: input " + std::to_string(N == 2 ? 1 : 0) + ", line " +
                                                       std::to_string(bad + 1) +
                                                       ": the line is a hit and lacks a column that --echo-map-id (4) or "
                                                       "--echo-map-score (5) asks for");
        }
    }
    const unsigned rblocks = blocks_for(Lr, kThreads);
    uint64_t* len = b_len.as<uint64_t>(Lr);
    uint64_t* off = b_off.as<uint64_t>(Lr);
    uint32_t* keep = opt.skip_unmapped ? b_keep.as<uint32_t>(Lr) : nullptr;
    hipLaunchKernelGGL(k_me_len, dim3(rblocks), dim3(kThreads), 0, st, f, len, keep);
    HIP_CHECK(hipGetLastError());
    uint64_t tot[2] = {0, 0};
    const FormatTail ft = format_tail(Lr, len, off, keep, keep ? b_kpos.as<uint64_t>(Lr) : nullptr, scal + S_BYTES, tot,
                                      keep ? 2 : 1, b_tmp, out, st, "bedmap-elements", true);
    uint8_t* o = static_cast<uint8_t*>(out.p);
    hipLaunchKernelGGL(k_me_write_line, dim3(rblocks), dim3(kThreads), 0, st, f, len, off, ft.bytes, o);
    if (T && f.slots) hipLaunchKernelGGL(k_me_write_hit, dim3(blocks_for(T, kThreads)), dim3(kThreads), 0, st, f, ft.bytes, o);
    HIP_CHECK(hipGetLastError());
    res.out_bytes = ft.bytes;
    res.lines_out = ft.lines_kept;
    finish(4);
}

}  // namespace me
