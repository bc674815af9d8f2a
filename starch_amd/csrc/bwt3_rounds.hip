// starch_amd/csrc/bwt3_rounds.hip -- block sort: what runs between the sorts
// of consecutive rounds.  Text rounds: the tie groups classified for their
// next sort (k3_classify_text).  Doubling: dense ranks (k3_rk_*), the keys of
// a round gathered (k3_gather, k3_gather_big), a round's verdict per block
// (k3_round_end) and the batch's (k3_finish); periodic blocks found up front
// (k3_period); counters cleared (k3_zero).  Overview: bz2_bwt3.hip.
#include "bwt3_int.hpp"

namespace bz {
namespace bwt3 {
namespace {

// ---------------------------------------------------------------------------
// text rounds: classify the tie groups (keys come from the PSS at an offset)
// ---------------------------------------------------------------------------
constexpr uint32_t CT_IPT = 16;       // tie groups per thread in k3_classify_text

// tie groups -> size-class lists for the next text round (as wg_classify, CT_IPT
// groups per thread: one LDS atomic per thread and class, one global atomic
// per workgroup and class, the groups held in registers between the passes)
__global__ void __launch_bounds__(256) k3_classify_text(Ctx c, const uint64_t* __restrict__ items, uint32_t nitems)
{
    __shared__ uint32_t cls_cnt[8], cls_base[8];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    if (tid < 8) cls_cnt[tid] = 0;
    __syncthreads();
    const uint64_t i0 = (uint64_t)blockIdx.x * 256u * CT_IPT + tid;
    uint64_t it[CT_IPT];
    uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tied = 0;
#pragma unroll
    for (uint32_t k = 0; k < CT_IPT; ++k) {
        const uint64_t i = i0 + (uint64_t)k * 256u;
        it[k] = i < nitems ? items[i] : 0ull;
        if (i < nitems) {
            const uint32_t m = it_size(it[k]);
            ++cnt[size_class(m)];
            tied += m;
        }
    }
    uint32_t off[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) off[q] = cnt[q] ? atomicAdd(&cls_cnt[q], cnt[q]) : 0u;
    __syncthreads();
    if (tid < 8 && cls_cnt[tid]) cls_base[tid] = atomicAdd(class_ctr(c, (int)tid), cls_cnt[tid]);
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < CT_IPT; ++k) {
        const uint64_t i = i0 + (uint64_t)k * 256u;
        if (i < nitems) {
            const uint32_t slot = it_slot(it[k]), m = it_size(it[k]);
            const int cls = size_class(m);
            uint32_t o = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) if (q == cls) o = off[q]++;
            const Geo g = c.L.geo[slot];
            class_list(c, cls)[cls_base[cls] + o] = mk_item(slot, it_start(it[k]), m, g.Dp * g.B, 0);
            if (cls == 6 && m > HG_MIN_PUSH) atomicMax(&c.L.ctr[C_LM0 + c.lsel], m);
        }
    }
    tied = wave_reduce_add<uint32_t>(tied);
    if (lane == 0 && tied) atomicAdd(&c.L.ctr[C_TIE_ELEMS], tied);
}

// ---------------------------------------------------------------------------
// doubling round: gather keys of tied rotations, classify their groups
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k3_gather(Ctx c, const uint64_t* __restrict__ items, uint32_t nitems,
                                                  uint32_t round, uint32_t rtext)
{
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    bool active = i < nitems;
    uint64_t item = active ? items[i] : 0;
    uint32_t slot = it_slot(item), s = it_start(item), m = it_size(item);
    uint32_t n = 1;
    uint32_t hm = 0;
    if (active) {
        active = c.L.periodic[slot] == 0;
        n = c.blocks[c.b0 + slot].n;
        const Geo g = c.L.geo[slot];
        const uint64_t h = ((uint64_t)g.D + (uint64_t)rtext * g.Dp) << (round - 1);
        if (active && h >= n) {   // sorted on >= n symbols: remaining ties are equal rotations
            c.L.periodic[slot] = 1;
            active = false;
        }
        hm = (uint32_t)(h % n);
    }
    const uint64_t so = (uint64_t)slot * c.scr.stride;
    if (active && m <= 64) {
        for (uint32_t q = s; q < s + m; ++q) {
            uint32_t t = c.scr.SA[so + q] + hm;
            if (t >= n) t -= n;
            c.scr.K2[so + q] = c.scr.RK[so + t];
        }
    }
    // groups above GB_MIN: gathered by the whole grid (k3_gather_big) -- one
    // wave walking a group of 450k tied rotations took most of a round
    bool taken = false;
    {
        const bool huge = active && m > GB_MIN;
        const uint64_t hb = __ballot(huge);
        if (hb) {
            const int lead = __ffsll((unsigned long long)hb) - 1;
            uint32_t b0 = 0;
            if (lane == lead) b0 = atomicAdd(&c.L.ctr[C_GB], (uint32_t)__popcll(hb));
            b0 = (uint32_t)__shfl((int)b0, lead, 64);
            const uint32_t o = b0 + (uint32_t)__popcll(hb & lanemask_lt());
            taken = huge && o < GB_MAXN;
            if (taken) {
                c.L.gb[o] = mk_item(slot, s, m, 0, 0);
                c.L.gb_h[o] = hm;
            }
        }
    }
    uint64_t bigm = __ballot(active && m > 64 && !taken);
    while (bigm) {
        const int l = __ffsll((unsigned long long)bigm) - 1;
        bigm &= bigm - 1;
        const uint32_t ls = __shfl(s, l, 64), lm = __shfl(m, l, 64), lslot = __shfl(slot, l, 64);
        const uint32_t ln = __shfl(n, l, 64), lh = __shfl(hm, l, 64);
        const uint64_t lso = (uint64_t)lslot * c.scr.stride;
        for (uint32_t q = ls + lane; q < ls + lm; q += 64) {
            uint32_t t = c.scr.SA[lso + q] + lh;
            if (t >= ln) t -= ln;
            c.scr.K2[lso + q] = c.scr.RK[lso + t];
        }
    }
    __shared__ uint32_t cls_sh[16];
    wg_classify(c, cls_sh, active, slot, s, m, RBITS, 0);
    wave_add_slot(c.L.gin, active, slot, 1u);
    const uint32_t tied = wave_reduce_add<uint32_t>(active ? m : 0u);
    if (lane == 0 && tied) atomicAdd(&c.L.ctr[C_TIE_ELEMS], tied);
}

__global__ void __launch_bounds__(256) k3_gather_big(Ctx c)
{
    const uint32_t ng = min(c.L.ctr[C_GB], GB_MAXN);
    const GridSplit gs = grid_split(ng);
    if (gs.idle) return;
    const uint32_t step = gs.per * 256u;
    for (uint32_t q = gs.q0; q < ng; q += gs.gstride) {
        const uint64_t item = c.L.gb[q];
        const uint32_t slot = it_slot(item), s = it_start(item), m = it_size(item), hm = c.L.gb_h[q];
        const uint32_t n = c.blocks[c.b0 + slot].n;
        const uint64_t so = (uint64_t)slot * c.scr.stride;
        for (uint32_t i = gs.slice * 256u + threadIdx.x; i < m; i += step) {
            uint32_t t = c.scr.SA[so + s + i] + hm;
            if (t >= n) t -= n;
            c.scr.K2[so + s + i] = c.scr.RK[so + t];
        }
    }
}

// ---- switch to doubling: dense ranks for the blocks that are still tied ----
__global__ void k3_mark_tied(Ctx c, const uint64_t* __restrict__ items, uint32_t nitems)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nitems) c.L.tied[it_slot(items[i])] = 1;
}

__global__ void __launch_bounds__(256) k3_rk_dense(Ctx c)
{
    const uint32_t slot = blockIdx.y;
    if (!c.L.tied[slot]) return;
    const uint32_t n = c.blocks[c.b0 + slot].n;
    const uint64_t so = (uint64_t)slot * c.scr.stride;
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) c.scr.RK[so + c.scr.SA[so + j]] = j;
}

__global__ void __launch_bounds__(256) k3_rk_groups(Ctx c, const uint64_t* __restrict__ items, uint32_t nitems)
{
    // one wave per group
    const int lane = threadIdx.x & 63;
    const uint32_t gi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gi >= nitems) return;
    const uint64_t item = items[gi];
    const uint32_t slot = it_slot(item), s = it_start(item), m = it_size(item);
    const uint64_t so = (uint64_t)slot * c.scr.stride;
    if (m > GB_MIN) {                     // the whole grid takes it (k3_rk_big) unless the list is full
        uint32_t o = 0;
        if (lane == 0) o = atomicAdd(&c.L.ctr[C_GB], 1u);
        o = (uint32_t)__shfl((int)o, 0, 64);
        if (o < GB_MAXN) {
            if (lane == 0) c.L.gb[o] = item;
            return;
        }
    }
    for (uint32_t q = s + lane; q < s + m; q += 64) c.scr.RK[so + c.scr.SA[so + q]] = s;
}

__global__ void __launch_bounds__(256) k3_rk_big(Ctx c)
{
    const uint32_t ng = min(c.L.ctr[C_GB], GB_MAXN);
    const GridSplit gs = grid_split(ng);
    if (gs.idle) return;
    const uint32_t step = gs.per * 256u;
    for (uint32_t q = gs.q0; q < ng; q += gs.gstride) {
        const uint64_t item = c.L.gb[q];
        const uint32_t slot = it_slot(item), s = it_start(item), m = it_size(item);
        const uint64_t so = (uint64_t)slot * c.scr.stride;
        for (uint32_t i = gs.slice * 256u + threadIdx.x; i < m; i += step) c.scr.RK[so + c.scr.SA[so + s + i]] = s;
    }
}

__global__ void k3_round_end(Ctx c, uint32_t nb)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= nb) return;
    const uint32_t g = c.L.gin[slot];
    if (g) {
        c.L.rounds[slot] += 1;
        if (c.L.runs[slot] == g) c.L.periodic[slot] = 1;   // no group split: equal rotations
    }
    c.L.gin[slot] = 0;
    c.L.runs[slot] = 0;
}

__global__ void k3_finish(Ctx c, uint32_t nb, unsigned long long* stats)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= nb) return;
    const uint32_t p = c.L.periodic[slot];
    c.blocks[c.b0 + slot].flags = p ? 1u : 0u;
    atomicAdd(stats, (unsigned long long)c.L.rounds[slot]);
    if (p) atomicAdd(stats + 1, 1ull);
    if (slot == 0) atomicAdd(stats + 2, (unsigned long long)c.L.ctr[C_TIE_ELEMS]);
}

// Periodic blocks up front: a cyclic block has equal rotations iff its minimal
// period divides n and is < n, iff block[i] == block[i + n/q] (i < n - n/q)
// for a prime q of n.  Flagged blocks take no doubling round (k3_gather drops
// their groups); the flag is the one the rounds would reach.  One workgroup per
// block, 4 KiB steps, so a non-periodic block stops after its first step.
__global__ void __launch_bounds__(256) k3_period(Ctx c)
{
    __shared__ uint32_t q_sh[16];
    __shared__ uint32_t nq_sh;
    __shared__ uint32_t dv[32];                    // divisors d <= sqrt(n) < 1024, as bits
    const uint32_t slot = blockIdx.x, b = c.b0 + slot;
    const uint32_t n = c.blocks[b].n;
    if (n < 2) return;
    // prime factors of n: the workgroup marks every divisor <= sqrt(n) (a few
    // trial divisions per thread: there is no integer divide, and one thread
    // walking all ~950 candidates took ~70 us), then one thread divides out the
    // marked ones in increasing order (composites no longer divide by then)
    if (threadIdx.x < 32) dv[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t d = 2 + threadIdx.x; d * d <= n; d += 256)
        if (n % d == 0) atomicOr(&dv[d >> 5], 1u << (d & 31));
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t m = n, k = 0;
        for (uint32_t w = 0; w < 32; ++w)
            for (uint32_t bits = dv[w]; bits; bits &= bits - 1) {
                const uint32_t d = 32 * w + (uint32_t)__builtin_ctz(bits);
                if (m % d == 0) {
                    q_sh[k++] = d;
                    while (m % d == 0) m /= d;
                }
            }
        if (m > 1) q_sh[k++] = m;
        nq_sh = k;
    }
    __syncthreads();
    const uint8_t* blk = c.blkbytes + (uint64_t)b * c.stride;
    const uint32_t nq = nq_sh;
    for (uint32_t j = 0; j < nq; ++j) {
        const uint32_t p = n / q_sh[j], e = n - p;
        int bad = 0;
        for (uint32_t a = 0; a < e && !bad; a += 4096) {
            const uint32_t z = a + 4096 < e ? a + 4096 : e;
            int mis = 0;
            for (uint32_t i = a + threadIdx.x; i < z; i += 256) mis |= blk[i] != blk[i + p];
            bad = __syncthreads_or(mis);
        }
        if (!bad) {
            if (threadIdx.x == 0) c.L.periodic[slot] = 1;
            return;
        }
    }
}

// zero the counters whose bits are set (one launch instead of a memset each)
__global__ void k3_zero(uint32_t* __restrict__ ctr, uint64_t mask)
{
    const uint32_t i = threadIdx.x;
    if (i < 64 && ((mask >> i) & 1ull)) ctr[i] = 0;
}

}  // namespace

void launch_zero(uint32_t* ctr, uint64_t mask, hipStream_t st)
{
    static_assert(C_N <= 64, "k3_zero masks");
    hipLaunchKernelGGL(k3_zero, dim3(1), dim3(64), 0, st, ctr, mask);
}

void launch_period(const Ctx& c, hipStream_t st)
{
    hipLaunchKernelGGL(k3_period, dim3(c.nb), dim3(256), 0, st, c);
}

void launch_classify_text(const Ctx& c, const uint64_t* items, uint32_t nitems, hipStream_t st)
{
    hipLaunchKernelGGL(k3_classify_text, dim3((nitems + 256 * CT_IPT - 1) / (256 * CT_IPT)), dim3(256), 0, st, c,
                       items, nitems);
    HIP_CHECK(hipGetLastError());
}

void launch_rk_init(const Ctx& c, const uint64_t* items, uint32_t nitems, int ncu, hipStream_t st)
{
    hipLaunchKernelGGL(k3_mark_tied, dim3((nitems + 255) / 256), dim3(256), 0, st, c, items, nitems);
    hipLaunchKernelGGL(k3_rk_dense, dim3(64, c.nb), dim3(256), 0, st, c);
    launch_zero(c.L.ctr, 1ull << C_GB, st);
    hipLaunchKernelGGL(k3_rk_groups, dim3((nitems + 3) / 4), dim3(256), 0, st, c, items, nitems);
    hipLaunchKernelGGL(k3_rk_big, dim3(ncu * 4), dim3(256), 0, st, c);
    HIP_CHECK(hipGetLastError());
}

void launch_gather(const Ctx& c, const uint64_t* items, uint32_t nitems, uint32_t round, uint32_t rtext, int ncu,
                   hipStream_t st)
{
    hipLaunchKernelGGL(k3_gather, dim3((nitems + 255) / 256), dim3(256), 0, st, c, items, nitems, round, rtext);
    hipLaunchKernelGGL(k3_gather_big, dim3(ncu * 4), dim3(256), 0, st, c);
    HIP_CHECK(hipGetLastError());
}

void launch_round_end(const Ctx& c, hipStream_t st)
{
    hipLaunchKernelGGL(k3_round_end, dim3((c.nb + 255) / 256), dim3(256), 0, st, c, c.nb);
}

void launch_finish(const Ctx& c, unsigned long long* stats, hipStream_t st)
{
    hipLaunchKernelGGL(k3_finish, dim3((c.nb + 255) / 256), dim3(256), 0, st, c, c.nb, stats);
    HIP_CHECK(hipGetLastError());
}

}  // namespace bwt3
}  // namespace bz

