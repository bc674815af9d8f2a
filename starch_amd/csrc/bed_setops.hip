// starch_amd/csrc/bed_setops.hip -- bedops --merge / --intersect / --difference /
// --symmdiff / --complement on MI355X: the number of inputs that cover each
// base, from a sweep over sorted interval ends.
//
// The inputs lie back to back in one buffer.  Stages (struct-of-arrays, one
// thread per element; nothing is sized by the number of inputs):
//   1. sort_bed.hip's framing, parse and chromosome ranks over the whole
//      buffer (ranks are global across inputs); k_so_first_line finds each
//      input's first line by a search of line_end for the input's byte end.
//   2. k_so_check: stop <= start and the per-input order check (first offender
//      by atomicMin), and the segment heads: a line that is the first of its
//      input or whose rank differs from its predecessor's.
//   3. per-input merge: a segmented inclusive max-scan of stop over the lines
//      (k_so_reduce, k_so_parts, k_so_down: the operator works on (max, head
//      flag), the carry crosses tiles).  A line opens a run when it is a head
//      or starts above the maximum before it; k_so_ends writes every run's two
//      ends (rank, position, +-weight).
//   4. the ends ordered by (rank, position) with the sort's radix stage.
//   5. sweep: inclusive sum of the weights in sorted order, one group per
//      distinct (rank, position) with the sum at its last end as depth
//      (k_so_gather, k_so_groups); k_so_flags marks where an output interval
//      starts and where it ends, k_so_emit compacts both.
//   6. format: k_so_len, an exclusive sum, k_so_write (on bed_text.hpp's writer).
//
// Weights are 64-bit: input 0 counts 2^32, every other input 1, so one running
// sum holds "input 0 covers this base" in its high half and the number of
// other inputs that cover it in its low half.
//
// run_bedops adds --element-of / --not-element-of (7: the other inputs merged
// together, a range maximum of run lengths, one thread per line of input 0),
// --partition (8: the sweep over the raw lines' ends), --chop (9: piece counts
// per merged run, one thread per piece) and --everything (the sort's radix
// order and line gather); DESIGN.md section 13.
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/starch_amd.h"
#include "bed_setops.hpp"
#include "bed_text.hpp"
#include "seg_max.hpp"

namespace so {
namespace {

constexpr int kThreads = 256;
enum : int { S_BAD = 0, S_RUNS, S_GROUPS, S_OUT, S_OUT_END, S_BYTES, S_COUNT = 8 };   // device scalars (u64)

// ---- 1. first line of every input ----------------------------------------------
// first[k + 1] = lines that end at or before in_end[k] (every input ends in '\n',
// so line_end holds in_end[k] itself when input k is not empty)
__global__ void __launch_bounds__(kThreads)
k_so_first_line(const uint64_t* __restrict__ line_end, uint64_t L, const uint64_t* __restrict__ in_end, uint64_t N,
                uint64_t* __restrict__ first)
{
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= N) return;
    const uint64_t e = in_end[k];
    uint64_t lo = 0, hi = L;   // first index with line_end > e
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (line_end[mid] <= e) lo = mid + 1;
        else hi = mid;
    }
    first[k + 1] = lo;
    if (k == 0) first[0] = 0;
}

// head (zeroed): 2 at the first line of every input that has lines
__global__ void __launch_bounds__(kThreads)
k_so_mark(const uint64_t* __restrict__ first, uint64_t N, uint64_t L, uint8_t* __restrict__ head)
{
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= N) return;
    const uint64_t a = first[k], b = first[k + 1];
    if (a < b && a < L) head[a] = 2;
}

// ---- 2. order check and segment heads --------------------------------------------
// bad: min of (line << 1) | what (0: stop <= start, 1: key below the previous
// line of the same input).  head: bit 1 in, bit 0 (segment head) added.
__global__ void __launch_bounds__(kThreads)
k_so_check(const uint32_t* __restrict__ rank, const uint64_t* __restrict__ start, const uint64_t* __restrict__ stop,
           uint64_t L, uint8_t* __restrict__ head, unsigned long long* __restrict__ bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= L) return;
    const bool inp = i == 0 || (head[i] & 2);
    const uint32_t r = rank[i];
    const uint64_t s = start[i], t = stop[i];
    bool hd = inp;
    bool desc = false;
    if (!inp) {
        const uint32_t pr = rank[i - 1];
        const uint64_t ps = start[i - 1], pt = stop[i - 1];
        hd = pr != r;
        desc = r < pr || (r == pr && (s < ps || (s == ps && t < pt)));
    }
    head[i] = (uint8_t)((inp ? 2 : 0) | (hd ? 1 : 0));
    if (t <= s) atomicMin(bad, (unsigned long long)(i << 1));
    else if (desc) atomicMin(bad, (unsigned long long)((i << 1) | 1));
}

// ---- 3. segmented max-scan and the runs' ends -------------------------------------
__global__ void __launch_bounds__(kScanThreads)
k_so_reduce(const uint64_t* __restrict__ stop, const uint8_t* __restrict__ head, uint64_t L, uint64_t* __restrict__ part_m,
            uint32_t* __restrict__ part_f)
{
    __shared__ uint64_t sh_m[kScanThreads / 64];
    __shared__ uint32_t sh_f[kScanThreads / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    MF acc{0, 0};
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const uint64_t i = base + k;
        if (i < L) acc = comb(acc, MF{stop[i], (uint32_t)(head[i] & 1)});
    }
    MF tot;
    (void)block_excl_mf(acc, sh_m, sh_f, &tot);
    if (threadIdx.x == 0) { part_m[blockIdx.x] = tot.m; part_f[blockIdx.x] = tot.f; }
}

// single workgroup: exclusive scan of the tile aggregates in place
__global__ void __launch_bounds__(1024)
k_so_parts(uint64_t* __restrict__ part_m, uint32_t* __restrict__ part_f, uint64_t nb)
{
    __shared__ uint64_t sh_m[1024 / 64];
    __shared__ uint32_t sh_f[1024 / 64];
    MF carry{0, 0};
    for (uint64_t b = 0; b < nb; b += 1024) {
        const uint64_t i = b + threadIdx.x;
        const MF v = i < nb ? MF{part_m[i], part_f[i]} : MF{0, 0};
        MF tot;
        const MF e = block_excl_mf(v, sh_m, sh_f, &tot);
        if (i < nb) {
            const MF o = comb(carry, e);
            part_m[i] = o.m;
            part_f[i] = o.f;
        }
        carry = comb(carry, tot);
    }
}

// incl[i]: the largest stop from i's segment head to i; open[i]: i opens a merged run
__global__ void __launch_bounds__(kScanThreads)
k_so_down(const uint64_t* __restrict__ start, const uint64_t* __restrict__ stop, const uint8_t* __restrict__ head, uint64_t L,
          const uint64_t* __restrict__ part_m, const uint32_t* __restrict__ part_f, uint64_t* __restrict__ incl,
          uint32_t* __restrict__ open)
{
    __shared__ uint64_t sh_m[kScanThreads / 64];
    __shared__ uint32_t sh_f[kScanThreads / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    MF v[kScanItems];
    MF acc{0, 0};
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const uint64_t i = base + k;
        v[k] = i < L ? MF{stop[i], (uint32_t)(head[i] & 1)} : MF{0, 0};
        acc = comb(acc, v[k]);
    }
    const MF pre = block_excl_mf(acc, sh_m, sh_f, (MF*)nullptr);
    MF run = comb(MF{part_m[blockIdx.x], part_f[blockIdx.x]}, pre);
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const uint64_t i = base + k;
        if (i < L) {
            const bool o = v[k].f || start[i] > run.m;   // equality joins
            run = comb(run, v[k]);
            incl[i] = run.m;
            open[i] = o ? 1u : 0u;
        }
    }
}

// run r of line i: pos[i] + open[i] - 1.  Its opener writes (rank, start, +w),
// its last line (rank, largest stop, -w); w = 2^32 for input 0's lines, else 1.
__global__ void __launch_bounds__(kThreads)
k_so_ends(const uint32_t* __restrict__ rank, const uint64_t* __restrict__ start, const uint64_t* __restrict__ incl,
          const uint32_t* __restrict__ open, const uint64_t* __restrict__ pos, uint64_t L, uint64_t first1,
          uint32_t* __restrict__ e_rank, uint64_t* __restrict__ e_pos, uint64_t* __restrict__ e_w)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= L) return;
    const uint32_t o = open[i];
    const uint64_t r = pos[i] + o - 1;
    const uint64_t w = i < first1 ? (1ull << 32) : 1ull;
    const uint32_t rk = rank[i];
    if (o) {
        e_rank[2 * r] = rk;
        e_pos[2 * r] = start[i];
        e_w[2 * r] = w;
    }
    if (i + 1 == L || open[i + 1]) {
        e_rank[2 * r + 1] = rk;
        e_pos[2 * r + 1] = incl[i];
        e_w[2 * r + 1] = 0 - w;
    }
}

// ---- 5. sweep -------------------------------------------------------------------------
// weights in sorted order, and the last end of every (rank, position) group
__global__ void __launch_bounds__(kThreads)
k_so_gather(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ e_rank, const uint64_t* __restrict__ e_pos,
            const uint64_t* __restrict__ e_w, uint64_t E, uint64_t* __restrict__ g_w, uint32_t* __restrict__ g_last)
{
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= E) return;
    const uint64_t i = idx ? idx[j] : j;
    g_w[j] = e_w[i];
    bool last = j + 1 == E;
    if (!last) {
        const uint64_t n = idx ? idx[j + 1] : j + 1;
        last = e_rank[n] != e_rank[i] || e_pos[n] != e_pos[i];
    }
    g_last[j] = last ? 1u : 0u;
}

__global__ void __launch_bounds__(kThreads)
k_so_groups(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ e_rank, const uint64_t* __restrict__ e_pos,
            const uint64_t* __restrict__ g_w, const uint64_t* __restrict__ g_sum, const uint32_t* __restrict__ g_last,
            const uint64_t* __restrict__ g_pos, uint64_t E, uint32_t* __restrict__ grp_rank, uint64_t* __restrict__ grp_pos,
            uint64_t* __restrict__ grp_depth)
{
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= E || !g_last[j]) return;
    const uint64_t i = idx ? idx[j] : j;
    const uint64_t g = g_pos[j];
    grp_rank[g] = e_rank[i];
    grp_pos[g] = e_pos[i];
    grp_depth[g] = g_sum[j] + g_w[j];   // inclusive sum at the group's last end
}

__device__ __forceinline__ bool holds(int op, uint64_t depth, uint64_t N)
{
    const uint64_t hi = depth >> 32, lo = depth & 0xffffffffull;
    switch (op) {
        case STARCH_SETOP_MERGE: return hi + lo >= 1;
        case STARCH_SETOP_INTERSECT: return hi + lo == N;
        case STARCH_SETOP_DIFFERENCE: return hi == 1 && lo == 0;
        case STARCH_SETOP_SYMMDIFF: return hi + lo == 1;
        default: return hi + lo == 0;   // complement
    }
}

// group g is on when the bases from it to the next group (same rank) are in the
// result; an output interval starts at an on group after one that is not, and
// ends at the first group after it that is not on
__global__ void __launch_bounds__(kThreads)
k_so_flags(const uint32_t* __restrict__ grp_rank, const uint64_t* __restrict__ grp_depth, uint64_t G, int op, uint64_t N,
           uint32_t* __restrict__ f_start, uint32_t* __restrict__ f_end)
{
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= G) return;
    const uint32_t r = grp_rank[g];
    const bool cur = g + 1 < G && grp_rank[g + 1] == r && holds(op, grp_depth[g], N);
    const bool prev = g > 0 && grp_rank[g - 1] == r && holds(op, grp_depth[g - 1], N);
    f_start[g] = cur && !prev ? 1u : 0u;
    f_end[g] = prev && !cur ? 1u : 0u;
}

__global__ void __launch_bounds__(kThreads)
k_so_emit(const uint32_t* __restrict__ grp_rank, const uint64_t* __restrict__ grp_pos, const uint32_t* __restrict__ f_start,
          const uint32_t* __restrict__ f_end, const uint64_t* __restrict__ p_start, const uint64_t* __restrict__ p_end,
          uint64_t G, uint64_t K, uint32_t* __restrict__ o_rank, uint64_t* __restrict__ o_start, uint64_t* __restrict__ o_stop)
{
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= G) return;
    if (f_start[g]) {
        const uint64_t k = p_start[g];
        if (k < K) { o_rank[k] = grp_rank[g]; o_start[k] = grp_pos[g]; }
    }
    if (f_end[g]) {
        const uint64_t k = p_end[g];
        if (k < K) o_stop[k] = grp_pos[g];
    }
}

// ---- 6. format ------------------------------------------------------------------------
using bt::dec_digits;

__global__ void __launch_bounds__(kThreads)
k_so_len(const uint32_t* __restrict__ o_rank, const uint64_t* __restrict__ o_start, const uint64_t* __restrict__ o_stop,
         const uint32_t* __restrict__ name_len, uint64_t K, uint32_t* __restrict__ o_len)
{
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k < K) o_len[k] = name_len[o_rank[k]] + dec_digits(o_start[k]) + dec_digits(o_stop[k]) + 3;
}

__global__ void __launch_bounds__(kThreads)
k_so_write(const uint8_t* __restrict__ bed, const uint32_t* __restrict__ o_rank, const uint64_t* __restrict__ o_start,
           const uint64_t* __restrict__ o_stop, const uint64_t* __restrict__ name_off, const uint32_t* __restrict__ name_len,
           const uint64_t* __restrict__ o_off, uint64_t K, uint64_t out_bytes, uint8_t* __restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= K) return;
    const uint32_t r = o_rank[k], nl = name_len[r];
    const uint64_t s = o_start[k], t = o_stop[k];
    const uint32_t ds = dec_digits(s), dt = dec_digits(t);
    const uint64_t off = o_off[k];
    if (off + nl + ds + dt + 3 > out_bytes) return;
    bt::Writer<> w{out, off};
    w.bytes(bed + name_off[r], nl);
    w.tab();
    w.dec(s, ds);
    w.tab();
    w.dec(t, dt);
    out[w.o] = '\n';
}

// ---- 7. element-of: the largest overlap of a line with one run ---------------------
// first index in [lo, hi) with v[index] >= x (hi: none)
__device__ __forceinline__ uint64_t lower(const uint64_t* v, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// first index in [lo, hi) with v[index] > x
__device__ __forceinline__ uint64_t upper(const uint64_t* v, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// first of n ordered ranks that is >= c
__device__ __forceinline__ uint64_t lower_rank(const uint32_t* __restrict__ rank, uint64_t n, uint64_t c)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (rank[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kThreads)
k_eo_gather(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ rank, const uint64_t* __restrict__ start,
            const uint64_t* __restrict__ stop, uint64_t n, uint32_t* __restrict__ s_rank, uint64_t* __restrict__ s_start,
            uint64_t* __restrict__ s_stop)
{
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const uint64_t i = idx[j];
    s_rank[j] = rank[i];
    s_start[j] = start[i];
    s_stop[j] = stop[i];
}

// head[i] = 1 at the first of the ordered lines of every chromosome
__global__ void __launch_bounds__(kThreads)
k_eo_heads(const uint32_t* __restrict__ rank, uint64_t n, uint8_t* __restrict__ head)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) head[i] = i == 0 || rank[i - 1] != rank[i] ? 1 : 0;
}

// run r of line i: pos[i] + open[i] - 1; its opener has its rank and start, its last line its stop
__global__ void __launch_bounds__(kThreads)
k_eo_runs(const uint32_t* __restrict__ rank, const uint64_t* __restrict__ start, const uint64_t* __restrict__ incl,
          const uint32_t* __restrict__ open, const uint64_t* __restrict__ pos, uint64_t L, uint64_t R,
          uint32_t* __restrict__ u_rank, uint64_t* __restrict__ u_start, uint64_t* __restrict__ u_stop)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= L) return;
    const uint32_t o = open[i];
    const uint64_t r = pos[i] + o - 1;
    if (r >= R) return;
    if (o) { u_rank[r] = rank[i]; u_start[r] = start[i]; }
    if (i + 1 == L || open[i + 1]) u_stop[r] = incl[i];
}

// a wave per tile of kRmqTile runs: the largest run length (whatever the runs' chromosomes)
static_assert(kRmqTile == 64, "k_eo_tile_max gives one lane to each run of a tile");
__global__ void __launch_bounds__(kThreads)
k_eo_tile_max(const uint64_t* __restrict__ u_start, const uint64_t* __restrict__ u_stop, uint64_t R, uint64_t NT,
              uint64_t* __restrict__ tmax)
{
    const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x, tile = r >> 6;
    uint64_t v = r < R ? u_stop[r] - u_start[r] : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0 && tile < NT) tmax[tile] = v;
}

// next[i] = max(prev[i], prev[i + half]): the largest over 2 * half tiles from tile i on
__global__ void __launch_bounds__(kThreads)
k_eo_level(const uint64_t* __restrict__ prev, uint64_t* __restrict__ next, uint64_t cnt, uint64_t half)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= cnt) return;
    const uint64_t a = prev[i], b = prev[i + half];
    next[i] = a > b ? a : b;
}

struct ElemQuery {
    const uint32_t* rank;                  // of input 0's lines: [0, Lr)
    const uint64_t *start, *stop;
    uint64_t Lr;
    const uint32_t* u_rank;                // the R runs of the other inputs' union, by (rank, start)
    const uint64_t *u_start, *u_stop;
    uint64_t R;
    const uint64_t* sp;                    // sp[k * NT + i]: the largest run length in tiles [i, i + 2^k)
    uint64_t NT;
    uint64_t threshold;
    uint32_t percent, invert;
    uint32_t* keep;
};

// the largest length of the runs [x, y), x < y: the two ragged tiles run by run, the whole tiles between in two probes
__device__ __forceinline__ uint64_t range_max(const ElemQuery& q, uint64_t x, uint64_t y)
{
    const uint64_t tx = x / kRmqTile, ty = (y - 1) / kRmqTile;
    uint64_t m = 0;
    const uint64_t head_end = tx == ty ? y : (tx + 1) * kRmqTile;
    for (uint64_t r = x; r < head_end; ++r) {
        const uint64_t l = q.u_stop[r] - q.u_start[r];
        m = l > m ? l : m;
    }
    if (tx == ty) return m;
    for (uint64_t r = ty * kRmqTile; r < y; ++r) {
        const uint64_t l = q.u_stop[r] - q.u_start[r];
        m = l > m ? l : m;
    }
    const uint64_t a = tx + 1, b = ty;   // whole tiles [a, b)
    if (a < b) {
        const uint32_t k = 63 - (uint32_t)__clzll((unsigned long long)(b - a));
        const uint64_t v0 = q.sp[k * q.NT + a], v1 = q.sp[k * q.NT + b - (1ull << k)];
        m = v0 > m ? v0 : m;
        m = v1 > m ? v1 : m;
    }
    return m;
}

// One thread per line of input 0.  A workgroup's lines are cut into chromosome
// segments; a segment's last thread finds the chromosome's slice of the runs and
// leaves it in LDS under the segment's head, every thread searches inside it.
__global__ void __launch_bounds__(kThreads)
k_eo_query(const ElemQuery q)
{
    __shared__ int sh_head[kThreads / 64];           // the last segment head of every wave (-1: none)
    __shared__ uint32_t sh_lo[kThreads], sh_hi[kThreads];
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + t;
    const bool valid = i < q.Lr;
    const uint32_t rk = valid ? q.rank[i] : 0u;
    const bool hd = t == 0 || !valid || q.rank[i - 1] != rk;
    const bool last = valid && (t == kThreads - 1 || i + 1 == q.Lr || q.rank[i + 1] != rk);
    const unsigned long long hm = __ballot(hd);
    const unsigned long long below = hm & ((2ull << lane) - 1);
    int head = below ? wid * 64 + 63 - __clzll(below) : -1;
    if (lane == 63) sh_head[wid] = hm ? wid * 64 + 63 - __clzll(hm) : -1;
    __syncthreads();
    for (int w = wid - 1; head < 0 && w >= 0; --w) head = sh_head[w];   // thread 0 is a head
    if (last) {
        sh_lo[head] = (uint32_t)lower_rank(q.u_rank, q.R, rk);            // R is below 2^31
        sh_hi[head] = (uint32_t)lower_rank(q.u_rank, q.R, (uint64_t)rk + 1);
    }
    __syncthreads();
    if (!valid) return;
    const uint64_t lo = sh_lo[head], hi = sh_hi[head];
    const uint64_t s = q.start[i], e = q.stop[i];
    // starts and stops both increase inside the slice
    const uint64_t f = upper(q.u_stop, lo, hi, s);    // the first run that ends above s
    const uint64_t l = lower(q.u_start, f, hi, e);    // one past the last run that starts below e
    uint64_t ov = 0;
    if (f < l) {
        const uint64_t a0 = q.u_start[f], b0 = q.u_stop[f];
        ov = (b0 < e ? b0 : e) - (a0 > s ? a0 : s);
        if (l - f > 1) {
            const uint64_t a1 = q.u_start[l - 1], b1 = q.u_stop[l - 1];
            const uint64_t o1 = (b1 < e ? b1 : e) - (a1 > s ? a1 : s);
            ov = o1 > ov ? o1 : ov;
        }
        if (l - f > 2) {   // the runs between the two lie wholly inside the line
            const uint64_t m = range_max(q, f + 1, l - 1);
            ov = m > ov ? m : ov;
        }
    }
    bool sel;
    if (q.percent) {   // ov * 100 >= p * (e - s), in 128 bits
        const uint64_t len = e - s;
        const uint64_t ah = __umul64hi(ov, 100ull), al = ov * 100ull;
        const uint64_t bh = __umul64hi(len, q.threshold), bl = len * q.threshold;
        sel = ah > bh || (ah == bh && al >= bl);
    } else {
        sel = ov >= q.threshold;
    }
    q.keep[i] = sel != (q.invert != 0) ? 1u : 0u;
}

__global__ void __launch_bounds__(kThreads)
k_eo_compact(const uint32_t* __restrict__ keep, const uint64_t* __restrict__ kpos, uint64_t Lr, uint64_t K,
             uint32_t* __restrict__ order)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= Lr || !keep[i]) return;
    const uint64_t k = kpos[i];
    if (k < K) order[k] = (uint32_t)i;
}

// ---- 8. partition ---------------------------------------------------------------------
// both ends of every line as they stand, weights +1 and -1
__global__ void __launch_bounds__(kThreads)
k_pt_ends(const uint32_t* __restrict__ rank, const uint64_t* __restrict__ start, const uint64_t* __restrict__ stop, uint64_t L,
          uint32_t* __restrict__ e_rank, uint64_t* __restrict__ e_pos, uint64_t* __restrict__ e_w)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= L) return;
    const uint32_t rk = rank[i];
    e_rank[2 * i] = rk;
    e_pos[2 * i] = start[i];
    e_w[2 * i] = 1;
    e_rank[2 * i + 1] = rk;
    e_pos[2 * i + 1] = stop[i];
    e_w[2 * i + 1] = 0 - 1ull;
}

// group g gives a piece when a line covers the bases from it to the next group of its chromosome
__global__ void __launch_bounds__(kThreads)
k_pt_flags(const uint32_t* __restrict__ grp_rank, const uint64_t* __restrict__ grp_depth, uint64_t G, uint32_t* __restrict__ f)
{
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= G) return;
    f[g] = g + 1 < G && grp_rank[g + 1] == grp_rank[g] && grp_depth[g] != 0 ? 1u : 0u;
}

__global__ void __launch_bounds__(kThreads)
k_pt_emit(const uint32_t* __restrict__ grp_rank, const uint64_t* __restrict__ grp_pos, const uint32_t* __restrict__ f,
          const uint64_t* __restrict__ p, uint64_t G, uint64_t K, uint32_t* __restrict__ o_rank, uint64_t* __restrict__ o_start,
          uint64_t* __restrict__ o_stop)
{
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= G || !f[g]) return;   // a flagged group has a successor
    const uint64_t k = p[g];
    if (k >= K) return;
    o_rank[k] = grp_rank[g];
    o_start[k] = grp_pos[g];
    o_stop[k] = grp_pos[g + 1];
}

// ---- 9. chop ----------------------------------------------------------------------------
// pieces of run [a, b): k = 0, 1, ... while a + k * g < b, that is ceil((b - a) / g);
// without the short ones, those with b - (a + k * g) >= w, a prefix of them.
// Capped at 2^32, from where the result is refused anyway.
__global__ void __launch_bounds__(kThreads)
k_ch_count(const uint64_t* __restrict__ o_start, const uint64_t* __restrict__ o_stop, uint64_t K, uint64_t w, uint64_t g,
           uint32_t exclude_short, uint64_t* __restrict__ cnt)
{
    const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= K) return;
    const uint64_t len = o_stop[r] - o_start[r];   // above 0
    uint64_t c;
    if (exclude_short) c = len < w ? 0 : (len - w) / g + 1;
    else c = (len - 1) / g + 1;
    cnt[r] = c < (1ull << 32) ? c : (1ull << 32);
}

// One thread per piece.  A workgroup finds the runs its pieces come from with two
// searches of the scanned counts, stages their offsets in LDS when there are at
// most kExpandTile of them, and every thread finds its run and its k there.
static_assert(kExpandTile >= 64 && kExpandTile % 64 == 0, "k_ch_expand: whole waves; the two searches go to lane 0 of the first and last");
__global__ void __launch_bounds__(kExpandTile)
k_ch_expand(const uint32_t* __restrict__ o_rank, const uint64_t* __restrict__ o_start, const uint64_t* __restrict__ o_stop,
            const uint64_t* __restrict__ coff, uint64_t K, uint64_t T, uint64_t w, uint64_t g, uint32_t* __restrict__ c_rank,
            uint64_t* __restrict__ c_start, uint64_t* __restrict__ c_stop)
{
    __shared__ uint64_t sh_off[kExpandTile];
    __shared__ uint64_t sh_win[2];
    const int t = threadIdx.x;
    const uint64_t j0 = (uint64_t)blockIdx.x * kExpandTile, j = j0 + t;
    const uint64_t jl = (j0 + kExpandTile < T ? j0 + kExpandTile : T) - 1;   // j0 < T
    // the last run whose offset is at or below j holds piece j (runs without pieces share their successor's offset)
    if (t == 0) sh_win[0] = upper(coff, 0, K, j0) - 1;
    if (t == kExpandTile - 64) sh_win[1] = upper(coff, 0, K, jl) - 1;   // lane 0 of the last wave
    __syncthreads();
    const uint64_t r0 = sh_win[0], r1 = sh_win[1], W = r1 - r0 + 1;
    const bool staged = W <= (uint64_t)kExpandTile;
    if (staged) {
        if ((uint64_t)t < W) sh_off[t] = coff[r0 + t];
        __syncthreads();
    }
    if (j >= T) return;
    uint64_t r, k;
    if (staged) {   // searched in the __shared__ array itself, so that the reads are LDS reads
        uint32_t lo = 0, hi = (uint32_t)W;   // first entry above j
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (sh_off[mid] <= j) lo = mid + 1;
            else hi = mid;
        }
        r = r0 + lo - 1;
        k = j - sh_off[lo - 1];
    } else {
        r = upper(coff, r0, r1 + 1, j) - 1;
        k = j - coff[r];
    }
    const uint64_t a = o_start[r], b = o_stop[r];
    const uint64_t s = a + k * g;          // below b: nothing wraps
    const uint64_t rem = b - s;
    c_rank[j] = o_rank[r];
    c_start[j] = s;
    c_stop[j] = rem > w ? s + w : b;       // s + w < b
}

}  // namespace

uint64_t SetopWorkspace::stage_lines(sb::SortWorkspace& sorter, const char* tool, const uint8_t* d_cat, uint64_t n,
                                     const std::vector<uint64_t>& in_end, hipStream_t st, std::vector<uint64_t>& first)
{
    const uint64_t N = in_end.size();
    const std::string name(tool);
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    unsigned long long* uscal = reinterpret_cast<unsigned long long*>(scal);
    HIP_CHECK(hipMemsetAsync(scal, 0, S_COUNT * sizeof(uint64_t), st));
    HIP_CHECK(hipMemsetAsync(scal + S_BAD, 0xff, sizeof(uint64_t), st));

    // 1. framing, parse, first lines, ranks
    uint64_t bad = 0;
    const uint64_t L = sorter.stage_parse(d_cat, n, st, &bad);
    const uint64_t* line_end = sorter.ln.line_end;
    uint64_t* d_in_end = b_in_end.as<uint64_t>(N);
    uint64_t* d_first = b_first.as<uint64_t>(N + 1);
    HIP_CHECK(hipMemcpyAsync(d_in_end, in_end.data(), N * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_so_first_line, dim3(blocks_for(N, kThreads)), dim3(kThreads), 0, st, line_end, L, d_in_end, N,
                       d_first);
    HIP_CHECK(hipGetLastError());
    first.assign(N + 1, 0);
    HIP_CHECK(hipMemcpyAsync(first.data(), d_first, (N + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    // "input K, line M" of line i of the whole buffer
    auto where = [&](uint64_t i) {
        const uint64_t k = (uint64_t)(std::upper_bound(first.begin() + 1, first.end(), i) - (first.begin() + 1));
        return name + ": input " + std::to_string(k) + ", line " + std::to_string(i - first[k] + 1) + ": ";
    };
    if (bad != ~0ull) throw StarchError(STARCH_ERR_DATA, where(bad >> 8) + sb::bad_text((uint32_t)(bad & 255)));
    sorter.stage_rank(d_cat, st);

    // 2. order check, segment heads
    head = b_head.as<uint8_t>(L);
    HIP_CHECK(hipMemsetAsync(head, 0, L, st));
    hipLaunchKernelGGL(k_so_mark, dim3(blocks_for(N, kThreads)), dim3(kThreads), 0, st, d_first, N, L, head);
    hipLaunchKernelGGL(k_so_check, dim3(blocks_for(L, kThreads)), dim3(kThreads), 0, st, sorter.ln.rank, sorter.ln.start,
                       sorter.ln.stop, L, head, uscal + S_BAD);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(&bad, scal + S_BAD, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (bad != ~0ull)
        throw StarchError(STARCH_ERR_DATA,
                          where(bad >> 1) + ((bad & 1) ? "the line sorts below the line before it; sort the input with sort-bed"
                                                       : "stop is not above start; " + name + " needs stop > start in every line of "
                                                         "an input sorted with sort-bed"));
    return L;
}

uint64_t SetopWorkspace::stage_merge(const uint64_t* start, const uint64_t* stop, const uint8_t* hd, uint64_t L, hipStream_t st)
{
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    const uint64_t nb = ceil_div(L, kScanTile);
    uint64_t* part_m = b_part_m.as<uint64_t>(nb);
    uint32_t* part_f = b_part_f.as<uint32_t>(nb);
    incl = b_incl.as<uint64_t>(L);
    open = b_open.as<uint32_t>(L);
    pos = b_pos.as<uint64_t>(L);
    hipLaunchKernelGGL(k_so_reduce, dim3((unsigned)nb), dim3(kScanThreads), 0, st, stop, hd, L, part_m, part_f);
    hipLaunchKernelGGL(k_so_parts, dim3(1), dim3(1024), 0, st, part_m, part_f, nb);
    hipLaunchKernelGGL(k_so_down, dim3((unsigned)nb), dim3(kScanThreads), 0, st, start, stop, hd, L, part_m, part_f, incl,
                       open);
    HIP_CHECK(hipGetLastError());
    scan::excl_sum_u32_to_u64(open, pos, L, scal + S_RUNS, b_tmp, st);
    uint64_t R = 0;
    HIP_CHECK(hipMemcpyAsync(&R, scal + S_RUNS, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return R;
}

// records the timer's events from `from` on, waits for the stream and fills the stage times
void SetopWorkspace::finish(hipStream_t st, SetopResult& res, int from)
{
    timer.finish(from, st, {&res.ms_parse, &res.ms_merge, &res.ms_sort, &res.ms_sweep, &res.ms_format});
}

void SetopWorkspace::run(sb::SortWorkspace& sorter, int op, const uint8_t* d_cat, uint64_t n,
                         const std::vector<uint64_t>& in_end, hipStream_t st, DevBuf& out, SetopResult& res)
{
    res = SetopResult{};
    (void)out.as<uint8_t>(64);
    timer.start(st);
    if (n == 0) return finish(st, res, 1);   // every input is empty: nothing is covered
    const uint64_t K = stage_intervals(sorter, op, d_cat, n, in_end, st, res);
    res.lines_out = K;
    if (K == 0) return finish(st, res, 4);
    timer.mark(4, st);
    res.out_bytes = stage_format(sorter, d_cat, b_o_rank.as<uint32_t>(K), b_o_start.as<uint64_t>(K), b_o_stop.as<uint64_t>(K), K,
                                 0, st, out);
    finish(st, res, 5);
}

uint64_t SetopWorkspace::stage_sweep(sb::SortWorkspace& sorter, const uint32_t* e_rank, const uint64_t* e_pos,
                                     const uint64_t* e_w, uint64_t E, hipStream_t st, SetopResult& res)
{
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    // 4. the ends by (rank, position)
    const sb::KeyBits kb = sorter.stage_check(e_rank, e_pos, e_pos, E, st);
    const uint32_t* idx = kb.desc == ~0ull ? nullptr : sorter.stage_radix(e_rank, e_pos, nullptr, E, kb, st, &res.radix_passes);
    timer.mark(3, st);

    // 5. sweep
    const unsigned eblocks = blocks_for(E, kThreads);
    uint64_t* g_w = b_g_w.as<uint64_t>(E);
    uint64_t* g_sum = b_g_sum.as<uint64_t>(E);
    uint32_t* g_last = b_g_last.as<uint32_t>(E);
    uint64_t* g_pos = b_g_pos.as<uint64_t>(E);
    hipLaunchKernelGGL(k_so_gather, dim3(eblocks), dim3(kThreads), 0, st, idx, e_rank, e_pos, e_w, E, g_w, g_last);
    HIP_CHECK(hipGetLastError());
    scan::excl_sum_u64(g_w, g_sum, E, (uint64_t*)nullptr, b_tmp, st);
    scan::excl_sum_u32_to_u64(g_last, g_pos, E, scal + S_GROUPS, b_tmp, st);
    uint64_t G = 0;
    HIP_CHECK(hipMemcpyAsync(&G, scal + S_GROUPS, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (G == 0 || G > E) throw StarchError(STARCH_ERR_INTERNAL, "bedops: the group count is out of range");
    res.groups = G;
    grp_rank = b_grp_rank.as<uint32_t>(G);
    grp_pos = b_grp_pos.as<uint64_t>(G);
    grp_depth = b_grp_depth.as<uint64_t>(G);
    hipLaunchKernelGGL(k_so_groups, dim3(eblocks), dim3(kThreads), 0, st, idx, e_rank, e_pos, g_w, g_sum, g_last, g_pos, E,
                       grp_rank, grp_pos, grp_depth);
    HIP_CHECK(hipGetLastError());
    return G;
}

uint64_t SetopWorkspace::stage_intervals(sb::SortWorkspace& sorter, int op, const uint8_t* d_cat, uint64_t n,
                                         const std::vector<uint64_t>& in_end, hipStream_t st, SetopResult& res)
{
    const uint64_t N = in_end.size();
    // 1, 2. parse, ranks, order check, segment heads
    std::vector<uint64_t> first;
    const uint64_t L = stage_lines(sorter, "bedops", d_cat, n, in_end, st, first);
    res.n_lines = L;
    res.n_chromosomes = sorter.n_chromosomes;
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    const uint64_t* start = sorter.ln.start;
    const uint64_t* stop = sorter.ln.stop;
    const uint32_t* rank = sorter.ln.rank;
    const unsigned lblocks = blocks_for(L, kThreads);
    if (L >= (1ull << 31))
        throw StarchError(STARCH_ERR_ARG, "bedops: 2^31 lines or more over all inputs (the interval ends are indexed with 32 bits)");
    timer.mark(1, st);

    // 3. per-input merge
    const uint64_t R = stage_merge(start, stop, head, L, st);
    if (R == 0 || R > L) throw StarchError(STARCH_ERR_INTERNAL, "bedops: the run count is out of range");
    res.runs_merged = R;
    const uint64_t E = 2 * R;   // below 2^32
    uint32_t* e_rank = b_e_rank.as<uint32_t>(E);
    uint64_t* e_pos = b_e_pos.as<uint64_t>(E);
    uint64_t* e_w = b_e_w.as<uint64_t>(E);
    hipLaunchKernelGGL(k_so_ends, dim3(lblocks), dim3(kThreads), 0, st, rank, start, incl, open, pos, L, first[1], e_rank,
                       e_pos, e_w);
    HIP_CHECK(hipGetLastError());
    timer.mark(2, st);

    // 4, 5. the ends by (rank, position), and their groups
    const uint64_t G = stage_sweep(sorter, e_rank, e_pos, e_w, E, st, res);
    const unsigned gblocks = blocks_for(G, kThreads);
    uint32_t* f_start = b_f_start.as<uint32_t>(G);
    uint32_t* f_end = b_f_end.as<uint32_t>(G);
    uint64_t* p_start = b_p_start.as<uint64_t>(G);
    uint64_t* p_end = b_p_end.as<uint64_t>(G);
    hipLaunchKernelGGL(k_so_flags, dim3(gblocks), dim3(kThreads), 0, st, grp_rank, grp_depth, G, op, N, f_start, f_end);
    HIP_CHECK(hipGetLastError());
    scan::excl_sum_u32_to_u64(f_start, p_start, G, scal + S_OUT, b_tmp, st);
    scan::excl_sum_u32_to_u64(f_end, p_end, G, scal + S_OUT_END, b_tmp, st);
    uint64_t KK[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(KK, scal + S_OUT, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (KK[0] != KK[1] || KK[0] > G) throw StarchError(STARCH_ERR_INTERNAL, "bedops: interval starts and ends do not pair");
    const uint64_t K = KK[0];
    if (K) {
        uint32_t* o_rank = b_o_rank.as<uint32_t>(K);
        uint64_t* o_start = b_o_start.as<uint64_t>(K);
        uint64_t* o_stop = b_o_stop.as<uint64_t>(K);
        hipLaunchKernelGGL(k_so_emit, dim3(gblocks), dim3(kThreads), 0, st, grp_rank, grp_pos, f_start, f_end, p_start, p_end,
                           G, K, o_rank, o_start, o_stop);
        HIP_CHECK(hipGetLastError());
    }
    return K;
}

uint64_t SetopWorkspace::stage_format(sb::SortWorkspace& sorter, const uint8_t* d_cat, const uint32_t* o_rank,
                                      const uint64_t* o_start, const uint64_t* o_stop, uint64_t K, uint64_t limit,
                                      hipStream_t st, DevBuf& out)
{
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    const uint64_t C = sorter.n_chromosomes;
    uint64_t* name_off = b_name_off.as<uint64_t>(C);
    uint32_t* name_len = b_name_len.as<uint32_t>(C);
    HIP_CHECK(hipMemcpyAsync(name_off, sorter.chrom_off.data(), C * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(name_len, sorter.chrom_len.data(), C * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    const unsigned kblocks = blocks_for(K, kThreads);
    uint32_t* o_len = b_o_len.as<uint32_t>(K);
    uint64_t* o_off = b_o_off.as<uint64_t>(K);
    hipLaunchKernelGGL(k_so_len, dim3(kblocks), dim3(kThreads), 0, st, o_rank, o_start, o_stop, name_len, K, o_len);
    HIP_CHECK(hipGetLastError());
    scan::excl_sum_u32_to_u64(o_len, o_off, K, scal + S_BYTES, b_tmp, st);
    uint64_t B = 0;
    HIP_CHECK(hipMemcpyAsync(&B, scal + S_BYTES, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (limit && B >= limit) throw StarchError(STARCH_ERR_ARG, "bedops: result too large (2^40 bytes or more)");
    uint8_t* o = out.as<uint8_t>(B + 64);
    hipLaunchKernelGGL(k_so_write, dim3(kblocks), dim3(kThreads), 0, st, d_cat, o_rank, o_start, o_stop, name_off, name_len,
                       o_off, K, B, o);
    HIP_CHECK(hipGetLastError());
    return B;
}

// ---- element-of, not-element-of ---------------------------------------------------------
void SetopWorkspace::element_of(sb::SortWorkspace& sorter, const BedopsOptions& opt, const uint8_t* d_cat, uint64_t L,
                                uint64_t Lr, hipStream_t st, DevBuf& out, SetopResult& res)
{
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    const uint64_t Lq = L - Lr;   // lines of inputs 1 .. N-1: [Lr, L)
    if (Lr == 0) return finish(st, res, 2);
    ElemQuery q{};
    q.rank = sorter.ln.rank;
    q.start = sorter.ln.start;
    q.stop = sorter.ln.stop;
    q.Lr = Lr;
    q.threshold = opt.threshold;
    q.percent = opt.percent ? 1u : 0u;
    q.invert = opt.op == STARCH_SETOP_NOT_ELEMENT_OF ? 1u : 0u;
    if (Lq) {
        // the other inputs' lines in (rank, start) order, merged together
        const uint32_t* q_rank = sorter.ln.rank + Lr;
        const uint64_t* q_start = sorter.ln.start + Lr;
        const uint64_t* q_stop = sorter.ln.stop + Lr;
        const unsigned qblocks = blocks_for(Lq, kThreads);
        const sb::KeyBits kb = sorter.stage_check(q_rank, q_start, q_start, Lq, st);
        if (kb.desc != ~0ull) {
            const uint32_t* idx = sorter.stage_radix(q_rank, q_start, nullptr, Lq, kb, st, &res.radix_passes);
            if (!idx) throw StarchError(STARCH_ERR_INTERNAL, "bedops: no order for the lines to merge");
            uint32_t* s_rank = b_q_rank.as<uint32_t>(Lq);
            uint64_t* s_start = b_q_start.as<uint64_t>(Lq);
            uint64_t* s_stop = b_q_stop.as<uint64_t>(Lq);
            hipLaunchKernelGGL(k_eo_gather, dim3(qblocks), dim3(kThreads), 0, st, idx, q_rank, q_start, q_stop, Lq, s_rank,
                               s_start, s_stop);
            HIP_CHECK(hipGetLastError());
            q_rank = s_rank;
            q_start = s_start;
            q_stop = s_stop;
        }
        uint8_t* q_head = b_q_head.as<uint8_t>(Lq);
        hipLaunchKernelGGL(k_eo_heads, dim3(qblocks), dim3(kThreads), 0, st, q_rank, Lq, q_head);
        HIP_CHECK(hipGetLastError());
        timer.mark(2, st);
        const uint64_t R = stage_merge(q_start, q_stop, q_head, Lq, st);
        if (R == 0 || R > Lq) throw StarchError(STARCH_ERR_INTERNAL, "bedops: the run count is out of range");
        res.runs_merged = R;
        uint32_t* u_rank = b_u_rank.as<uint32_t>(R);
        uint64_t* u_start = b_u_start.as<uint64_t>(R);
        uint64_t* u_stop = b_u_stop.as<uint64_t>(R);
        hipLaunchKernelGGL(k_eo_runs, dim3(qblocks), dim3(kThreads), 0, st, q_rank, q_start, incl, open, pos, Lq, R, u_rank,
                           u_start, u_stop);
        HIP_CHECK(hipGetLastError());
        // largest run length per tile of kRmqTile runs, then per 2^k tiles from every tile on
        const uint64_t NT = ceil_div(R, kRmqTile);
        uint32_t levels = 1;
        while ((2ull << (levels - 1)) <= NT) ++levels;
        uint64_t* sp = b_rmq.as<uint64_t>(NT * levels);
        hipLaunchKernelGGL(k_eo_tile_max, dim3(blocks_for(NT * 64, kThreads)), dim3(kThreads), 0, st, u_start, u_stop, R, NT, sp);
        for (uint32_t k = 1; k < levels; ++k) {
            const uint64_t half = 1ull << (k - 1), cnt = NT - 2 * half + 1;
            hipLaunchKernelGGL(k_eo_level, dim3(blocks_for(cnt, kThreads)), dim3(kThreads), 0, st, sp + (k - 1) * NT,
                               sp + k * NT, cnt, half);
        }
        HIP_CHECK(hipGetLastError());
        q.u_rank = u_rank;
        q.u_start = u_start;
        q.u_stop = u_stop;
        q.R = R;
        q.sp = sp;
        q.NT = NT;
    } else {
        timer.mark(2, st);
    }
    timer.mark(3, st);

    // overlap with one run, flags, and the lines that stay
    const unsigned rblocks = blocks_for(Lr, kThreads);
    uint32_t* keep = b_keep.as<uint32_t>(Lr);
    uint64_t* kpos = b_kpos.as<uint64_t>(Lr);
    q.keep = keep;
    hipLaunchKernelGGL(k_eo_query, dim3(rblocks), dim3(kThreads), 0, st, q);
    HIP_CHECK(hipGetLastError());
    scan::excl_sum_u32_to_u64(keep, kpos, Lr, scal + S_OUT, b_tmp, st);
    uint64_t K = 0;
    HIP_CHECK(hipMemcpyAsync(&K, scal + S_OUT, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (K > Lr) throw StarchError(STARCH_ERR_INTERNAL, "bedops: more lines kept than there are");
    res.lines_out = K;
    timer.mark(4, st);
    if (K) {
        uint32_t* order = b_order.as<uint32_t>(K);
        hipLaunchKernelGGL(k_eo_compact, dim3(rblocks), dim3(kThreads), 0, st, keep, kpos, Lr, K, order);
        HIP_CHECK(hipGetLastError());
        res.out_bytes = sorter.stage_gather(d_cat, order, K, ~0ull, nullptr, st, out);
    }
    finish(st, res, 5);
}

// ---- partition ----------------------------------------------------------------------------
void SetopWorkspace::partition(sb::SortWorkspace& sorter, const uint8_t* d_cat, uint64_t L, hipStream_t st, DevBuf& out,
                               SetopResult& res)
{
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    const uint64_t E = 2 * L;   // below 2^32
    uint32_t* e_rank = b_e_rank.as<uint32_t>(E);
    uint64_t* e_pos = b_e_pos.as<uint64_t>(E);
    uint64_t* e_w = b_e_w.as<uint64_t>(E);
    hipLaunchKernelGGL(k_pt_ends, dim3(blocks_for(L, kThreads)), dim3(kThreads), 0, st, sorter.ln.rank, sorter.ln.start,
                       sorter.ln.stop, L, e_rank, e_pos, e_w);
    HIP_CHECK(hipGetLastError());
    timer.mark(2, st);
    const uint64_t G = stage_sweep(sorter, e_rank, e_pos, e_w, E, st, res);
    const unsigned gblocks = blocks_for(G, kThreads);
    uint32_t* f_start = b_f_start.as<uint32_t>(G);
    uint64_t* p_start = b_p_start.as<uint64_t>(G);
    hipLaunchKernelGGL(k_pt_flags, dim3(gblocks), dim3(kThreads), 0, st, grp_rank, grp_depth, G, f_start);
    HIP_CHECK(hipGetLastError());
    scan::excl_sum_u32_to_u64(f_start, p_start, G, scal + S_OUT, b_tmp, st);
    uint64_t K = 0;
    HIP_CHECK(hipMemcpyAsync(&K, scal + S_OUT, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (K == 0 || K >= G) throw StarchError(STARCH_ERR_INTERNAL, "bedops: the piece count is out of range");
    res.lines_out = K;
    uint32_t* o_rank = b_o_rank.as<uint32_t>(K);
    uint64_t* o_start = b_o_start.as<uint64_t>(K);
    uint64_t* o_stop = b_o_stop.as<uint64_t>(K);
    hipLaunchKernelGGL(k_pt_emit, dim3(gblocks), dim3(kThreads), 0, st, grp_rank, grp_pos, f_start, p_start, G, K, o_rank,
                       o_start, o_stop);
    HIP_CHECK(hipGetLastError());
    timer.mark(4, st);
    res.out_bytes = stage_format(sorter, d_cat, o_rank, o_start, o_stop, K, 0, st, out);
    finish(st, res, 5);
}

// ---- chop -----------------------------------------------------------------------------------
// K > 0 merged runs lie in o_rank / o_start / o_stop
void SetopWorkspace::chop(sb::SortWorkspace& sorter, const BedopsOptions& opt, const uint8_t* d_cat, uint64_t K, hipStream_t st,
                          DevBuf& out, SetopResult& res)
{
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);
    const uint32_t* o_rank = b_o_rank.as<uint32_t>(K);
    const uint64_t* o_start = b_o_start.as<uint64_t>(K);
    const uint64_t* o_stop = b_o_stop.as<uint64_t>(K);
    uint64_t* cnt = b_cnt.as<uint64_t>(K);
    uint64_t* coff = b_coff.as<uint64_t>(K);
    hipLaunchKernelGGL(k_ch_count, dim3(blocks_for(K, kThreads)), dim3(kThreads), 0, st, o_start, o_stop, K, opt.chop,
                       opt.stagger, opt.exclude_short ? 1u : 0u, cnt);
    HIP_CHECK(hipGetLastError());
    scan::excl_sum_u64(cnt, coff, K, scal + S_OUT, b_tmp, st);
    uint64_t T = 0;
    HIP_CHECK(hipMemcpyAsync(&T, scal + S_OUT, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    // (a run's count is capped at 2^32 and there are fewer than 2^31 runs: the sum cannot wrap)
    if (T >= (1ull << 32)) throw StarchError(STARCH_ERR_ARG, "bedops: result too large (2^32 pieces or more)");
    res.lines_out = T;
    if (T == 0) return finish(st, res, 4);
    uint32_t* c_rank = b_c_rank.as<uint32_t>(T);
    uint64_t* c_start = b_c_start.as<uint64_t>(T);
    uint64_t* c_stop = b_c_stop.as<uint64_t>(T);
    hipLaunchKernelGGL(k_ch_expand, dim3(blocks_for(T, kExpandTile)), dim3(kExpandTile), 0, st, o_rank, o_start, o_stop, coff, K,
                       T, opt.chop, opt.stagger, c_rank, c_start, c_stop);
    HIP_CHECK(hipGetLastError());
    timer.mark(4, st);
    res.out_bytes = stage_format(sorter, d_cat, c_rank, c_start, c_stop, T, 1ull << 40, st, out);
    finish(st, res, 5);
}

// ---- everything -------------------------------------------------------------------------------
void SetopWorkspace::everything(sb::SortWorkspace& sorter, const uint8_t* d_cat, uint64_t n, uint64_t L, hipStream_t st,
                                DevBuf& out, SetopResult& res)
{
    timer.mark(2, st);
    const sb::KeyBits kb = sorter.stage_check(sorter.ln.rank, sorter.ln.start, sorter.ln.stop, L, st);
    const uint32_t* order = kb.desc == ~0ull ? nullptr
                                             : sorter.stage_radix(sorter.ln.rank, sorter.ln.start, sorter.ln.stop, L, kb, st,
                                                                  &res.radix_passes);
    timer.mark(3, st);
    timer.mark(4, st);
    res.lines_out = L;
    if (!order) {   // the inputs one after the other are in order as they stand
        const bool open_end = sorter.ln.open_end;
        res.out_bytes = n + (open_end ? 1 : 0);
        uint8_t* o = out.as<uint8_t>(res.out_bytes + 64);
        HIP_CHECK(hipMemcpyAsync(o, d_cat, n, hipMemcpyDeviceToDevice, st));
        if (open_end) HIP_CHECK(hipMemsetAsync(o + n, '\n', 1, st));
    } else {
        res.out_bytes = sorter.stage_gather(d_cat, order, L, n + (sorter.ln.open_end ? 1 : 0), nullptr, st, out);
    }
    finish(st, res, 5);
}

void SetopWorkspace::run_bedops(sb::SortWorkspace& sorter, const BedopsOptions& opt, const uint8_t* d_cat, uint64_t n,
                                const std::vector<uint64_t>& in_end, hipStream_t st, DevBuf& out, SetopResult& res)
{
    if (opt.op <= STARCH_SETOP_COMPLEMENT) return run(sorter, opt.op, d_cat, n, in_end, st, out, res);
    res = SetopResult{};
    (void)out.as<uint8_t>(64);
    timer.start(st);
    if (n == 0) return finish(st, res, 1);   // every input is empty
    if (opt.op == STARCH_SETOP_CHOP) {
        const uint64_t K = stage_intervals(sorter, STARCH_SETOP_MERGE, d_cat, n, in_end, st, res);
        if (K == 0) throw StarchError(STARCH_ERR_INTERNAL, "bedops: lines but no merged run");
        return chop(sorter, opt, d_cat, K, st, out, res);
    }
    std::vector<uint64_t> first;
    const uint64_t L = stage_lines(sorter, "bedops", d_cat, n, in_end, st, first);
    res.n_lines = L;
    res.n_chromosomes = sorter.n_chromosomes;
    if (L >= (1ull << 31))
        throw StarchError(STARCH_ERR_ARG, "bedops: 2^31 lines or more over all inputs (the interval ends are indexed with 32 bits)");
    timer.mark(1, st);
    if (opt.op == STARCH_SETOP_PARTITION) return partition(sorter, d_cat, L, st, out, res);
    if (opt.op == STARCH_SETOP_EVERYTHING) return everything(sorter, d_cat, n, L, st, out, res);
    element_of(sorter, opt, d_cat, L, first[1], st, out, res);
}

}  // namespace so
