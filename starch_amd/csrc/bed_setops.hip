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
//   6. format: k_so_len, an exclusive sum, k_so_write.
//
// Weights are 64-bit: input 0 counts 2^32, every other input 1, so one running
// sum holds "input 0 covers this base" in its high half and the number of
// other inputs that cover it in its low half.
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/starch_amd.h"
#include "bed_setops.hpp"
#include "seg_max.hpp"

namespace so {
namespace {

constexpr int kThreads = 256;
enum : int { S_BAD = 0, S_RUNS, S_GROUPS, S_OUT, S_OUT_END, S_BYTES, S_COUNT = 8 };   // device scalars (u64)

inline unsigned blocks_for(uint64_t items, uint64_t per_block) { return (unsigned)ceil_div(items, per_block); }

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
__device__ __forceinline__ uint32_t dec_digits(uint64_t v)
{
    uint32_t d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}

__device__ __forceinline__ void put_dec(uint8_t* o, uint64_t v, uint32_t d)
{
    for (uint32_t k = d; k-- > 0;) { o[k] = (uint8_t)('0' + v % 10); v /= 10; }
}

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
    uint8_t* o = out + off;
    const uint8_t* nm = bed + name_off[r];
    for (uint32_t q = 0; q < nl; ++q) o[q] = nm[q];
    o += nl;
    *o++ = '\t';
    put_dec(o, s, ds);
    o += ds;
    *o++ = '\t';
    put_dec(o, t, dt);
    o += dt;
    *o = '\n';
}

}  // namespace

SetopWorkspace::~SetopWorkspace()
{
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
}

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

void SetopWorkspace::run(sb::SortWorkspace& sorter, int op, const uint8_t* d_cat, uint64_t n,
                         const std::vector<uint64_t>& in_end, hipStream_t st, DevBuf& out, SetopResult& res)
{
    res = SetopResult{};
    const uint64_t N = in_end.size();
    for (auto& e : ev)
        if (!e && hipEventCreate(&e) != hipSuccess) { e = nullptr; throw StarchError(STARCH_ERR_DEVICE, "hipEventCreate"); }
    (void)out.as<uint8_t>(64);
    HIP_CHECK(hipEventRecord(ev[0], st));
    if (n == 0) {   // every input is empty: nothing is covered
        for (int k = 1; k < 6; ++k) HIP_CHECK(hipEventRecord(ev[k], st));
        HIP_CHECK(hipStreamSynchronize(st));
        return;
    }

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
    HIP_CHECK(hipEventRecord(ev[1], st));

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
    HIP_CHECK(hipEventRecord(ev[2], st));

    // 4. the ends by (rank, position)
    const sb::KeyBits kb = sorter.stage_check(e_rank, e_pos, e_pos, E, st);
    const uint32_t* idx = kb.desc == ~0ull ? nullptr : sorter.stage_radix(e_rank, e_pos, nullptr, E, kb, st, &res.radix_passes);
    HIP_CHECK(hipEventRecord(ev[3], st));

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
    uint32_t* grp_rank = b_grp_rank.as<uint32_t>(G);
    uint64_t* grp_pos = b_grp_pos.as<uint64_t>(G);
    uint64_t* grp_depth = b_grp_depth.as<uint64_t>(G);
    hipLaunchKernelGGL(k_so_groups, dim3(eblocks), dim3(kThreads), 0, st, idx, e_rank, e_pos, g_w, g_sum, g_last, g_pos, E,
                       grp_rank, grp_pos, grp_depth);
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
    res.lines_out = K;
    if (K == 0) {
        for (int k = 4; k < 6; ++k) HIP_CHECK(hipEventRecord(ev[k], st));
    } else {
        uint32_t* o_rank = b_o_rank.as<uint32_t>(K);
        uint64_t* o_start = b_o_start.as<uint64_t>(K);
        uint64_t* o_stop = b_o_stop.as<uint64_t>(K);
        hipLaunchKernelGGL(k_so_emit, dim3(gblocks), dim3(kThreads), 0, st, grp_rank, grp_pos, f_start, f_end, p_start, p_end,
                           G, K, o_rank, o_start, o_stop);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ev[4], st));

        // 6. format
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
        uint8_t* o = out.as<uint8_t>(B + 64);
        hipLaunchKernelGGL(k_so_write, dim3(kblocks), dim3(kThreads), 0, st, d_cat, o_rank, o_start, o_stop, name_off, name_len,
                           o_off, K, B, o);
        HIP_CHECK(hipGetLastError());
        res.out_bytes = B;
        HIP_CHECK(hipEventRecord(ev[5], st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipEventElapsedTime(&res.ms_parse, ev[0], ev[1]));
    HIP_CHECK(hipEventElapsedTime(&res.ms_merge, ev[1], ev[2]));
    HIP_CHECK(hipEventElapsedTime(&res.ms_sort, ev[2], ev[3]));
    HIP_CHECK(hipEventElapsedTime(&res.ms_sweep, ev[3], ev[4]));
    HIP_CHECK(hipEventElapsedTime(&res.ms_format, ev[4], ev[5]));
}

}  // namespace so
