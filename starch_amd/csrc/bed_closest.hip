// starch_amd/csrc/bed_closest.hip -- closest-features on MI355X: for every line
// of a sorted reference, the nearest line of a sorted query to its left and to
// its right (include/starch_amd.h has the definition).
//
// Both inputs lie back to back in one buffer; the reference is input 0.  Stages:
//   1. bed_setops.hip's stage_lines over the whole buffer: framing, parse,
//      global chromosome ranks, stop > start and the per-input order.
//   2. query arrays.  A, S: the query starts and stops in query order, which is
//      (rank, start, stop) order; rank r's lines are [mlo[r], mlo[r + 1]).
//      M: the largest stop from the chromosome's first line to each line
//      (stage_merge's running maximum).  H: a hierarchy of maxima over S --
//      level k holds the maximum of every aligned group of kFanout^k stops,
//      up to the level with one item.  With no_overlaps also B, the stops in
//      (rank, stop) order, and the query line each came from: S itself when no
//      query line is nested in another (the sort's order check finds no
//      descent), else through the sort's stable radix stage.
//   3. k_bc_query, one thread per reference line (c, s, e), lo = mlo[c],
//      hi = mlo[c + 1]:
//        p      = lo + #{query lines on c with (a, b) < (s, e)}: a search on A,
//                 then on S inside the run of starts equal to s.
//        right  = p (default: a does not decrease from p on, so neither does
//                 dist), or the first line with a >= e (no_overlaps).
//        left   = default: with m = M[p - 1], the last j in [lo, p) with
//                 S[j] >= (m > s ? s + 1 : m) -- the last line that overlaps,
//                 or if none does the last with the largest stop.  last_at_least
//                 walks H: up from p while no item reaches the threshold, then
//                 down into the item that does, kFanout items per level at most.
//                 no_overlaps: the line of the entry before upper(B, s).
//      closest drops the farther of the two (a tie drops the right one).
//   4. format: k_bc_len, an exclusive sum, k_bc_write (the writer and its wave
//      copy: bed_text.hpp; the host steps between the two kernels: format_tail
//      in common.hpp; both shared with every BED command).
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/starch_amd.h"
#include "bed_closest.hpp"
#include "bed_hier.hpp"
#include "bed_search.hpp"
#include "bed_text.hpp"

namespace bc {
namespace {

using bm::lower;
using bm::upper;

constexpr int kThreads = 256;
constexpr uint32_t kNA = ~0u;
enum : int { S_BYTES = 0, S_LEFT_NA, S_RIGHT_NA, S_COUNT = 4 };   // device scalars (u64)

using bt::dec_digits;
using bt::line_beg;

// ---- 2. query arrays (the hierarchy's level kernel and builder: bed_hier.hpp) ----------
__global__ void __launch_bounds__(kThreads)
k_bc_gather(const uint32_t* __restrict__ idx, const uint64_t* __restrict__ v, uint64_t n, uint64_t* __restrict__ out)
{
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j < n) out[j] = v[idx[j]];
}

// ---- 3. query -------------------------------------------------------------------------
// The last j in [lo, p) with S[j] >= t, where lo < p and such a j exists.  Item
// i of level k covers the stops [i << (k * kFanShift), (i + 1) << (k * kFanShift)).
// Up: at every level the items below `end` that their parent does not cover
// whole, from the right.  Down: the children of the item found, from the
// right.  The item that holds lo is taken whatever its maximum (it may come
// from the chromosome before): everything right of it has been ruled out, so
// the j that exists is inside it.  Each loop runs kFanout times at most.
__device__ __forceinline__ uint64_t last_at_least(const Hier& h, uint64_t lo, uint64_t p, uint64_t t)
{
    uint64_t end = p, hit = ~0ull;
    int lv = 0;
    for (; lv < h.nlev; ++lv) {
        const uint64_t* __restrict__ v = h.lev[lv];
        const uint64_t lol = lo >> (kFanShift * lv);
        const uint64_t gs = end & ~(uint64_t)(kFanout - 1);
        for (uint64_t i = end; i-- > gs;)
            if (i == lol || v[i] >= t) { hit = i; break; }
        if (hit != ~0ull) break;
        end >>= kFanShift;
        if (end == 0) break;
    }
    if (hit == ~0ull) return p - 1;   // not reached: the item of lo ends every walk
    while (lv > 0) {
        --lv;
        const uint64_t* __restrict__ v = h.lev[lv];
        const uint64_t lol = lo >> (kFanShift * lv);
        const uint64_t cs = hit << kFanShift;
        const uint64_t ce = cs + kFanout < h.cnt[lv] ? cs + kFanout : h.cnt[lv];
        hit = cs;
        for (uint64_t i = ce; i-- > cs;)
            if (i == lol || v[i] >= t) { hit = i; break; }
    }
    return hit;
}

struct Query {
    const uint32_t* rank;                 // of the reference lines (input 0: lines [0, Lr))
    const uint64_t *start, *stop;
    uint64_t Lr;
    const uint64_t *mlo, *A, *S, *M, *B;  // B, bidx: with no_overlaps alone
    const uint32_t* bidx;                 // the query line of B's entries (NULL: B is S)
    Hier h;
    uint32_t no_overlaps, closest;
    uint32_t *left, *right;               // per reference line: a query line, or kNA
    unsigned long long* na;               // S_LEFT_NA, S_RIGHT_NA are counted up
};

__global__ void __launch_bounds__(kTileRefs)
k_bc_query(const Query q)
{
    const uint64_t i = (uint64_t)blockIdx.x * kTileRefs + threadIdx.x;
    const bool valid = i < q.Lr;
    uint32_t L = kNA, R = kNA;
    uint64_t s = 0, e = 0;
    if (valid) {
        const uint32_t rk = q.rank[i];
        s = q.start[i];
        e = q.stop[i];
        const uint64_t lo = q.mlo[rk], hi = q.mlo[rk + 1];
        if (lo < hi) {
            if (q.no_overlaps) {
                const uint64_t r = lower(q.A, lo, hi, e);
                if (r < hi) R = (uint32_t)r;
                const uint64_t k = upper(q.B, lo, hi, s);
                if (k > lo) L = q.bidx ? q.bidx[k - 1] : (uint32_t)(k - 1);
            } else {
                const uint64_t j0 = lower(q.A, lo, hi, s), j1 = upper(q.A, j0, hi, s);
                const uint64_t p = lower(q.S, j0, j1, e);
                if (p < hi) R = (uint32_t)p;
                if (p > lo) {
                    const uint64_t m = q.M[p - 1];
                    L = (uint32_t)last_at_least(q.h, lo, p, m > s ? s + 1 : m);
                }
            }
        }
    }
    const unsigned long long nl = __ballot(valid && L == kNA), nr = __ballot(valid && R == kNA);
    if ((threadIdx.x & 63) == 0) {
        if (nl) atomicAdd(q.na + S_LEFT_NA, (unsigned long long)__popcll(nl));
        if (nr) atomicAdd(q.na + S_RIGHT_NA, (unsigned long long)__popcll(nr));
    }
    if (!valid) return;
    if (q.closest && L != kNA && R != kNA) {
        const uint64_t b = q.S[L], a = q.A[R];
        const uint64_t dl = b > s ? 0 : s - b + 1, dr = a < e ? 0 : a - e + 1;
        if (dr < dl) L = kNA;
        else R = kNA;
    }
    q.left[i] = L;
    q.right[i] = R;
}

// ---- 4. format ------------------------------------------------------------------------
struct Format {
    const uint64_t *line_end, *start, *stop;   // of every line of the buffer; query line j is line m0 + j
    const uint32_t *left, *right;
    uint64_t Lr, m0;
    ClosestOptions opt;
};

// the element fields of reference line i: one with closest (the side that was kept), else left and right
__device__ __forceinline__ uint32_t elements(const Format& f, uint64_t i, uint32_t el[2])
{
    const uint32_t L = f.left[i], R = f.right[i];
    if (f.opt.closest) { el[0] = L != kNA ? L : R; return 1; }
    el[0] = L;
    el[1] = R;
    return 2;
}

// the distance of query line j from reference line i: its magnitude, and whether it is negative
__device__ __forceinline__ uint64_t distance(const Format& f, uint64_t i, uint32_t j, bool* neg)
{
    const uint64_t s = f.start[i], e = f.stop[i], a = f.start[f.m0 + j], b = f.stop[f.m0 + j];
    *neg = b <= s;
    return b <= s ? s - b + 1 : (a >= e ? a - e + 1 : 0);
}

// len: bytes of output line i with its '\n'
__global__ void __launch_bounds__(kThreads)
k_bc_len(const Format f, uint64_t* __restrict__ len)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= f.Lr) return;
    uint32_t el[2];
    const uint32_t ne = elements(f, i, el);
    const uint32_t fields = (f.opt.no_ref ? 0 : 1) + ne * (f.opt.dist ? 2 : 1);
    uint64_t n = (uint64_t)f.opt.delim_len * (fields - 1) + 1;
    if (!f.opt.no_ref) n += f.line_end[i] - 1 - line_beg(f.line_end, i);
    for (uint32_t k = 0; k < ne; ++k) {
        if (el[k] == kNA) { n += f.opt.dist ? 4 : 2; continue; }
        const uint64_t g = f.m0 + el[k];
        n += f.line_end[g] - 1 - line_beg(f.line_end, g);
        if (f.opt.dist) {
            bool neg;
            const uint64_t d = distance(f, i, el[k], &neg);
            n += dec_digits(d) + (neg ? 1 : 0);
        }
    }
    len[i] = n;
}

// A thread writes its line; a copied line of kWaveCopyBytes or more (the
// reference line, either element) is left to the whole wave, one after another.
__global__ void __launch_bounds__(kThreads)
k_bc_write(const uint8_t* __restrict__ bed, const Format f, const uint64_t* __restrict__ len, const uint64_t* __restrict__ off,
           uint64_t out_bytes, uint8_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bt::Writer<3> w{out, 0};   // slots: the reference line, the first element, the second
    if (i < f.Lr && off[i] + len[i] <= out_bytes) {
        w.o = off[i];
        bool first = true;
        auto delim = [&] {
            if (!first) w.delim(f.opt.delim, f.opt.delim_len);
            first = false;
        };
        auto copy_line = [&](uint64_t g, int slot) {
            const uint64_t b = line_beg(f.line_end, g);
            w.copy(slot, bed + b, f.line_end[g] - 1 - b);
        };
        auto na_text = [&] { w.bytes(reinterpret_cast<const uint8_t*>("NA"), 2); };
        if (!f.opt.no_ref) { delim(); copy_line(i, 0); }
        uint32_t el[2];
        const uint32_t ne = elements(f, i, el);
#pragma unroll
        for (uint32_t k = 0; k < 2; ++k) {
            if (k >= ne) break;
            const bool na = el[k] == kNA;
            delim();
            if (na) na_text();
            else copy_line(f.m0 + el[k], 1 + (int)k);
            if (f.opt.dist) {
                delim();
                if (na) na_text();
                else {
                    bool neg;
                    const uint64_t d = distance(f, i, el[k], &neg);
                    if (neg) out[w.o++] = '-';
                    w.dec(d);
                }
            }
        }
        out[w.o] = '\n';
    }
    bt::wave_copy_tails(w, out, lane);
}

}  // namespace

void ClosestWorkspace::run(sb::SortWorkspace& sorter, so::SetopWorkspace& lines, const ClosestOptions& opt, const uint8_t* d_cat,
                           uint64_t n, const std::vector<uint64_t>& in_end, hipStream_t st, DevBuf& out, ClosestResult& res)
{
    res = ClosestResult{};
    if (in_end.size() != 2) throw StarchError(STARCH_ERR_INTERNAL, "closest-features: two inputs are needed");
    (void)out.as<uint8_t>(64);
    timer.start(st);
    auto finish = [&](int from) { timer.finish(from, st, {&res.ms_parse, &res.ms_build, &res.ms_query, &res.ms_format}); };
    if (n == 0) return finish(1);   // both inputs are empty

    // 1. parse, ranks, checks; the reference is lines [0, Lr), the query [Lr, Lr + Lq)
    std::vector<uint64_t> first;
    const uint64_t L = lines.stage_lines(sorter, "closest-features", d_cat, n, in_end, st, first);
    const uint64_t Lr = first[1], m0 = Lr, Lq = L - Lr;
    if (L >= (1ull << 32)) throw StarchError(STARCH_ERR_ARG, "closest-features: 2^32 lines or more over both inputs");
    res.n_ref = Lr;
    res.n_query = Lq;
    res.n_chromosomes = sorter.n_chromosomes;
    timer.mark(1, st);
    if (Lr == 0) return finish(2);

    const uint64_t C = sorter.n_chromosomes;
    const uint32_t* rank = sorter.ln.rank;
    const uint64_t* start = sorter.ln.start;
    const uint64_t* stop = sorter.ln.stop;
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    HIP_CHECK(hipMemsetAsync(scal, 0, S_COUNT * sizeof(uint64_t), st));

    // 2. query arrays
    Query q{};
    q.rank = rank;
    q.start = start;
    q.stop = stop;
    q.Lr = Lr;
    q.no_overlaps = opt.no_overlaps;
    q.closest = opt.closest;
    q.A = start + m0;
    q.S = stop + m0;
    q.B = q.S;
    uint64_t* mlo = b_mlo.as<uint64_t>(C + 1);
    hipLaunchKernelGGL(bm::k_bm_bounds, dim3(blocks_for(C + 1, bm::kBoundsThreads)), dim3(bm::kBoundsThreads), 0, st, rank + m0,
                       Lq, C, mlo);
    HIP_CHECK(hipGetLastError());
    q.mlo = mlo;
    if (Lq) {
        (void)lines.stage_merge(start + m0, stop + m0, lines.head + m0, Lq, st);
        q.M = lines.incl;
        // the levels above the stops, one after the other in b_hier
        build_hier(q.S, Lq, b_hier, st, "closest-features", &q.h);
        const sb::KeyBits kb = sorter.stage_check(rank + m0, stop + m0, stop + m0, Lq, st);
        if (kb.desc != ~0ull) {   // a query line ends below the one before it: it is nested
            res.stops_sorted = 1;
            if (opt.no_overlaps) {
                uint32_t passes = 0;
                const uint32_t* idx = sorter.stage_radix(rank + m0, stop + m0, nullptr, Lq, kb, st, &passes);
                if (!idx) throw StarchError(STARCH_ERR_INTERNAL, "closest-features: no order for the query stops");
                uint64_t* B = b_B.as<uint64_t>(Lq);
                hipLaunchKernelGGL(k_bc_gather, dim3(blocks_for(Lq, kThreads)), dim3(kThreads), 0, st, idx, stop + m0, Lq, B);
                HIP_CHECK(hipGetLastError());
                q.B = B;
                q.bidx = idx;   // the sorter is not used again before the query has run
            }
        }
    }
    q.left = b_left.as<uint32_t>(Lr);
    q.right = b_right.as<uint32_t>(Lr);
    q.na = reinterpret_cast<unsigned long long*>(scal);
    timer.mark(2, st);

    // 3. query
    hipLaunchKernelGGL(k_bc_query, dim3(blocks_for(Lr, kTileRefs)), dim3(kTileRefs), 0, st, q);
    HIP_CHECK(hipGetLastError());
    timer.mark(3, st);

    // 4. format
    Format f{sorter.ln.line_end, start, stop, q.left, q.right, Lr, m0, opt};
    const unsigned rblocks = blocks_for(Lr, kThreads);
    uint64_t* len = b_len.as<uint64_t>(Lr);
    uint64_t* off = b_off.as<uint64_t>(Lr);
    hipLaunchKernelGGL(k_bc_len, dim3(rblocks), dim3(kThreads), 0, st, f, len);
    HIP_CHECK(hipGetLastError());
    uint64_t tot[3] = {0, 0, 0};   // the bytes, and with them the two NA counts of the query
    const FormatTail ft = format_tail(Lr, len, off, nullptr, nullptr, scal + S_BYTES, tot, 3, b_tmp, out, st,
                                      "closest-features", false);
    hipLaunchKernelGGL(k_bc_write, dim3(rblocks), dim3(kThreads), 0, st, d_cat, f, len, off, ft.bytes,
                       static_cast<uint8_t*>(out.p));
    HIP_CHECK(hipGetLastError());
    res.out_bytes = ft.bytes;
    res.lines_out = ft.lines_kept;
    res.left_na = tot[S_LEFT_NA];
    res.right_na = tot[S_RIGHT_NA];
    finish(4);
}

}  // namespace bc
