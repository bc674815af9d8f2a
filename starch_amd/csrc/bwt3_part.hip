// starch_amd/csrc/bwt3_part.hip -- block sort: the work lists binned by block
// into per-XCD segments (k3_bin_*), and the groups too large for a leaf sort
// partitioned on their next key bits, by one workgroup each (k3_part_l) or,
// above HG_MIN, by the whole grid (k3_hg_*).  Overview: bz2_bwt3.hip.
#include "bwt3_int.hpp"

#include <algorithm>

namespace bz {
namespace bwt3 {
namespace {

// ---------------------------------------------------------------------------
// binning of a work list by block into per-XCD segments (blocks x, x+8, ...).
// A batch of few blocks (nb < 64) bins by (block, 64-item run mod 8) instead
// (vs = 3), so its groups spread over all XCDs: one block's PSS fits every
// L2, and binning by block alone would leave 7 of 8 XCDs idle.  Lists come
// out of the sorts mostly grouped by block: a wave whose 64 items share a bin
// counts / places them with one LDS atomic (one atomic per item serialised
// the wave on one address).
// ---------------------------------------------------------------------------
constexpr uint32_t BIN_CH = 4096;     // items per binning workgroup (at least)

__device__ __forceinline__ uint32_t bin_of(uint64_t it, uint32_t i, uint32_t vs)
{
    return (it_slot(it) << vs) | ((i >> 6) & ((1u << vs) - 1u));
}

// chunks are multiples of 64 items, so every wave's 64 items share i >> 6
__global__ void __launch_bounds__(256) k3_bin_hist(const uint64_t* __restrict__ in, uint32_t n, uint32_t nb,
                                                    uint32_t ch, uint32_t* __restrict__ hist,
                                                    uint32_t* __restrict__ colsum, uint32_t vs)
{
    __shared__ uint32_t h[4096];
    for (uint32_t i = threadIdx.x; i < nb; i += 256) h[i] = 0;
    __syncthreads();
    const uint32_t a = blockIdx.x * ch, e = a + ch < n ? a + ch : n;
    for (uint32_t i0 = a; i0 < e; i0 += 256) {     // wave-uniform trip count
        const uint32_t i = i0 + threadIdx.x;
        const bool ok = i < e;
        const uint32_t b = ok ? bin_of(in[i], i, vs) : 0u;
        const uint64_t act = __ballot(ok);
        if (!act) continue;
        const int lead = __ffsll((unsigned long long)act) - 1;
        const uint32_t b0 = (uint32_t)__shfl((int)b, lead, 64);
        if (__ballot(ok && b == b0) == act) {
            if ((int)(threadIdx.x & 63) == lead) atomicAdd(&h[b0], (uint32_t)__popcll(act));
        } else if (ok) {
            atomicAdd(&h[b], 1u);
        }
    }
    __syncthreads();
    // this chunk's place inside each bin: one global atomic per non-empty bin
    // (chunks take their places in any order; a bin's items are independent)
    for (uint32_t i = threadIdx.x; i < nb; i += 256) {
        const uint32_t x = h[i];
        hist[(uint64_t)blockIdx.x * nb + i] = x ? atomicAdd(&colsum[i], x) : 0u;
    }
}

// one workgroup: the bins' totals (k3_bin_hist's atomics), reset for the
// next binning, and their XCD-ordered exclusive scan -> each bin's start;
// seg[x] = start of XCD x's segment.  (Per-(chunk, bin) offsets used to be
// scanned here row by row: a dependent walk over up to 128 rows per bin.)
__global__ void __launch_bounds__(1024) k3_bin_scan(uint32_t* __restrict__ colsum, uint32_t* __restrict__ bstart,
                                                     uint32_t nb, uint32_t* __restrict__ seg)
{
    __shared__ uint32_t scan_sh[1024 / 64 + 1];
    const int tid = threadIdx.x;
    const uint32_t NS = (nb + 7) / 8;               // blocks per XCD segment (upper bound)
    // XCD-ordered sequence j -> block s = (j / NS) + 8 * (j % NS); 4 entries per thread
    uint32_t v[4], sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t j = tid * 4 + q;
        const uint32_t s = (j / NS) + 8u * (j % NS);
        v[q] = 0u;
        if (j < 8 * NS && s < nb) {
            v[q] = colsum[s];
            colsum[s] = 0u;
        }
        sum += v[q];
    }
    uint32_t total = 0;
    uint32_t run = block_excl_scan_add<uint32_t>(sum, scan_sh, &total);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t j = tid * 4 + q;
        const uint32_t s = (j / NS) + 8u * (j % NS);
        if (j < 8 * NS && (j % NS) == 0) seg[j / NS] = run;
        if (j < 8 * NS && s < nb) bstart[s] = run;
        run += v[q];
    }
    if (tid == 0) seg[8] = total;
}

__global__ void __launch_bounds__(256) k3_bin_scatter(const uint64_t* __restrict__ in, uint32_t n, uint32_t nb,
                                                       uint32_t ch, const uint32_t* __restrict__ hist,
                                                       const uint32_t* __restrict__ bstart,
                                                       uint64_t* __restrict__ out, uint32_t vs)
{
    __shared__ uint32_t cur[4096];
    for (uint32_t i = threadIdx.x; i < nb; i += 256) cur[i] = bstart[i] + hist[(uint64_t)blockIdx.x * nb + i];
    __syncthreads();
    const uint32_t a = blockIdx.x * ch, e = a + ch < n ? a + ch : n;
    for (uint32_t i0 = a; i0 < e; i0 += 256) {     // wave-uniform trip count
        const uint32_t i = i0 + threadIdx.x;
        const bool ok = i < e;
        const uint64_t it = ok ? in[i] : 0ull;
        const uint32_t b = ok ? bin_of(it, i, vs) : 0u;
        const uint64_t act = __ballot(ok);
        if (!act) continue;
        const int lane = (int)(threadIdx.x & 63), lead = __ffsll((unsigned long long)act) - 1;
        const uint32_t b0 = (uint32_t)__shfl((int)b, lead, 64);
        uint32_t pos;
        if (__ballot(ok && b == b0) == act) {          // one bin: one atomic, items in lane order
            uint32_t base = 0;
            if (lane == lead) base = atomicAdd(&cur[b0], (uint32_t)__popcll(act));
            base = (uint32_t)__shfl((int)base, lead, 64);
            pos = base + (uint32_t)__popcll(act & ((1ull << lane) - 1ull));
        } else {
            pos = ok ? atomicAdd(&cur[b], 1u) : 0u;
        }
        if (ok) out[pos] = it;
    }
}

// ---------------------------------------------------------------------------
// k3_part_l: MSD partition of one large group on its next <= 8 key bits
// (persistent over a binned list; values ping-pong SA <-> V, and in doubling
// mode the K2 <-> K keys with them)
// ---------------------------------------------------------------------------
constexpr int LT = 512;
constexpr int LW = LT / 64;
// round 0 / text rounds: the first pass keeps every element's digit in LDS,
// so the scatter pass re-reads only the (coalesced) rotations, not their
// PSS keys (random 8-byte loads); groups above PL_CAP recompute the keys
constexpr uint32_t PL_CAP = 40960;
constexpr uint32_t PL_STG = STARCH_PL_STG;

template <bool DBL>
__global__ void __launch_bounds__(LT) k3_part_l(Ctx c, const uint64_t* __restrict__ items)
{
    __shared__ uint32_t wh[LW][256];
    __shared__ uint32_t st[256], cur[256], cntd[256];
    __shared__ uint32_t scan_sh[LW + 1];
    __shared__ uint32_t big[257];
    __shared__ uint32_t qs[8];
    __shared__ uint32_t job_sh;
    __shared__ uint32_t cls_sh[16];
    __shared__ uint8_t dcache[DBL ? 4 : PL_CAP];
    // round 0 / text rounds: the partitioned rotations of a group up to
    // PL_STG are assembled here and stored in one coalesced pass (the scatter
    // into 256 sub-buckets wrote one lone 4-byte word per rotation)
    __shared__ uint32_t stg[DBL ? 1 : PL_STG];
    const int tid = threadIdx.x, wid = tid >> 6;
    const uint32_t x = xcc_id();
    load_qsizes_binned(c, qs);
    for (;;) {
        const uint32_t job = wg_pop(c, qs, &job_sh, x);
        if (job == 0xFFFFFFFFu) break;
        const uint64_t item = items[c.qseg[job >> 28] + (job & 0x0FFFFFFFu)];
        const uint32_t slot = it_slot(item), s = it_start(item), m = it_size(item), shift = it_shift(item),
                       par = it_par(item);
        if (m == 0) continue;                          // taken by the grid-wide path (k3_hg_pick); uniform
        const uint32_t b = c.b0 + slot;
        const uint64_t so = (uint64_t)slot * c.scr.stride;
        const uint64_t base = so + s;
        const KeySrc ks = key_src(c, slot, par);
        const uint32_t* sv = (par ? c.scr.V : c.scr.SA) + base;
        uint32_t* dv = (par ? c.scr.SA : c.scr.V) + base;
        uint64_t* dk = (par ? c.kA : c.kB) + base;              // keys by position (keysrc 1) only
        uint32_t* SA = c.scr.SA + base;
        uint32_t* RK = c.scr.RK + so;
        const uint32_t db = shift < 8 ? shift : 8;
        const uint32_t sh2 = shift - db;
        const uint64_t dmask = (1ull << db) - 1ull;
        // a top-level L bucket of round 0: the scatter left each rotation's
        // digit (its key bits [SH, SH + 8)) in LL next to it
        const uint8_t* sdig = nullptr;
        if (!DBL && c.sdig && c.rtext == 0 && !c.mode && par == 0 && db == 8) {
            const Geo g = c.L.geo[slot];
            if (shift == g.KB - g.SH) sdig = c.scr.LL + base;
        }
        for (int i = tid; i < LW * 256; i += LT) (&wh[0][0])[i] = 0;
        if (tid == 0) big[256] = 0;
        __syncthreads();
        constexpr int PU = STARCH_PART_PU;             // elements in flight per thread
        // (each pass issues all PU loads of a step before using any: a load
        // chosen per element inside the unrolled loop was waited on one by one)
        for (uint32_t i0 = 0; i0 < m; i0 += PU * LT) {
            uint32_t d[PU];
            if (sdig) {
#pragma unroll
                for (int u = 0; u < PU; ++u) {
                    const uint32_t i = i0 + u * LT + tid;
                    d[u] = sdig[i < m ? i : 0u];
                }
            } else {
                uint32_t vv[PU];
#pragma unroll
                for (int u = 0; u < PU; ++u) {
                    const uint32_t i = i0 + u * LT + tid;
                    vv[u] = sv[i < m ? i : 0u];
                }
#pragma unroll
                for (int u = 0; u < PU; ++u) {
                    const uint32_t i = i0 + u * LT + tid;
                    d[u] = (uint32_t)((elem_key<DBL>(ks, s + (i < m ? i : 0u), vv[u]) >> sh2) & dmask);
                }
            }
#pragma unroll
            for (int u = 0; u < PU; ++u) {
                const uint32_t i = i0 + u * LT + tid;
                if (!DBL && m <= PL_CAP && i < m) dcache[i] = (uint8_t)d[u];
            }
#pragma unroll
            for (int u = 0; u < PU; ++u)
                if (i0 + u * LT + tid < m) atomicAdd(&wh[wid][d[u]], 1u);
        }
        __syncthreads();
        uint32_t tcount = 0;
        if (tid < 256) for (int w = 0; w < LW; ++w) tcount += wh[w][tid];
        const uint32_t pre = block_excl_scan_add<uint32_t>(tid < 256 ? tcount : 0u, scan_sh, (uint32_t*)nullptr);
        if (tid < 256) { st[tid] = pre; cur[tid] = pre; cntd[tid] = tcount; }
        __syncthreads();
        const bool staged = !DBL && m <= PL_STG && !(STARCH_PL_STG == 0);
        for (uint32_t i0 = 0; i0 < m; i0 += PU * LT) {
            uint32_t v[PU];
            uint64_t k[PU];
#pragma unroll
            for (int u = 0; u < PU; ++u) {
                const uint32_t i = i0 + u * LT + tid;
                v[u] = sv[i < m ? i : 0u];
            }
            if (!DBL && m <= PL_CAP) {                 // only the digit is used below
#pragma unroll
                for (int u = 0; u < PU; ++u) {
                    const uint32_t i = i0 + u * LT + tid;
                    k[u] = (uint64_t)dcache[i < m ? i : 0u] << sh2;
                }
            } else if (sdig) {
#pragma unroll
                for (int u = 0; u < PU; ++u) {
                    const uint32_t i = i0 + u * LT + tid;
                    k[u] = (uint64_t)sdig[i < m ? i : 0u] << sh2;
                }
            } else {
#pragma unroll
                for (int u = 0; u < PU; ++u) {
                    const uint32_t i = i0 + u * LT + tid;
                    k[u] = elem_key<DBL>(ks, s + (i < m ? i : 0u), v[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < PU; ++u) {
                if (i0 + u * LT + tid < m) {
                    const uint32_t p = atomicAdd(&cur[(uint32_t)((k[u] >> sh2) & dmask)], 1u);
                    if (!DBL && staged) stg[p] = v[u];
                    else dv[p] = v[u];
                    if constexpr (DBL) dk[p] = k[u];
                }
            }
        }
        __syncthreads();
        if (!DBL && staged) {
            for (uint32_t i = tid; i < m; i += LT) dv[i] = stg[i];
            __syncthreads();
        }
        uint32_t nruns = 0;
        if (tid < 256) {
            const uint32_t cc = cntd[tid], ss = st[tid];
            if (cc == 1) {
                const uint32_t v = dv[ss];
                if (!par) SA[ss] = v;
                c.scr.LL[base + ss] = last_sym(c, slot, v);
                if (c.mode) RK[v] = s + ss;
                if (v == 0) c.blocks[b].orig_ptr = s + ss;
                nruns = 1;
            } else if (size_class(cc) == 6 && sh2 == 0) {
                big[atomicAdd(&big[256], 1u)] = tid;   // all keys equal: one group
                nruns = 1;
            }
        }
        {
            const uint32_t cc = tid < 256 ? cntd[tid] : 0u;
            const bool push = tid < 256 && cc >= 2 && !(size_class(cc) == 6 && sh2 == 0);
            wg_classify(c, cls_sh, push, slot, s + (tid < 256 ? st[tid] : 0u), cc, sh2, par ^ 1u);
        }
        if (tid < 256) {
            const uint32_t r = wave_reduce_add(nruns);
            if (c.mode && (tid & 63) == 0 && r) atomicAdd(&c.L.runs[slot], r);
        }
        __syncthreads();
        const uint32_t nbig = big[256];
        for (uint32_t q = 0; q < nbig; ++q) {
            const uint32_t d = big[q];
            const uint32_t ss = st[d], cc = cntd[d];
            for (uint32_t i = tid; i < cc; i += LT) {
                const uint32_t v = dv[ss + i];
                if (!par) SA[ss + i] = v;
                c.scr.LL[base + ss + i] = last_sym(c, slot, v);
                if (c.mode) RK[v] = s + ss;
                if (v == 0) c.blocks[b].orig_ptr = s + ss + i;
            }
            if (tid == 0) {
                const uint32_t o = atomicAdd(c.L.ctr + C_T0 + c.tsel, 1u);
                c.L.t[c.tsel][o] = mk_item(slot, s + ss, cc, 0, 0);
                atomicAdd(c.L.ctr + C_TS0 + c.tsel, cc);
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Huge groups (> HG_MIN rotations): k3_part_l's MSD partition step spread over
// the whole grid.  One k3_part_l workgroup per group left a group of
// hundreds of thousands of tied rotations -- every doubling round of a
// near-periodic block (per-position BED: "0\n" repeated, broken once) -- to
// one CU for the whole round.  Here a group is cut into HG_CH-element chunks:
// per-chunk digit histograms (k3_hg_hist), one workgroup per group scans them
// into per-chunk cursors and classifies the sub-buckets exactly as k3_part_l
// does (k3_hg_scan), every chunk scatters its elements (k3_hg_scatter), and
// sub-buckets that are final (singletons, or all-equal keys with no key bits
// left) are written out by k3_hg_final -- after the scatter, so no chunk's
// source reads race the final SA writes.
// ---------------------------------------------------------------------------
constexpr uint32_t HG_CH = 1024;        // elements per chunk: 4 per thread, every chunk in flight at once
constexpr uint32_t HG_MAXCH = 1u << 22; // chunks per level (the pick's budget: any batch)
constexpr uint32_t HG_FINAL = 1u << 31;
// k3_hg_scan's verdict on a group whose digit window holds no varying key bit
// (hg_vary): HG_SKIP_ALL -- every remaining key bit is equal: the whole group
// is one final tie group, written out from where it is; HG_SKIP_RELABEL -- it
// goes back to the L list with its shift lowered to its highest varying bit.
// Either way no element moves at this level.  (Near-periodic blocks -- a
// per-position BED's "0\n" repeated -- send groups of ~450k rotations whose
// 52-64 key bits are all equal through here: seven 8-bit levels each, per
// round, before this.)
constexpr uint32_t HG_SKIP_ALL = 1, HG_SKIP_RELABEL = 2;
// ... and when more than half the group's keys equal its first element's key
// over every remaining bit -- a doubling round's unresolved rotations, all
// ranked at the same tie group -- the level is a three-way split instead of a
// digit: below / equal / above that key.  The equal part is final at once (a
// tie group for the next round); the other two keep the shift.  One pass per
// round instead of a digit level per 8 key bits, each moving the whole group.
constexpr uint32_t HG_THREE = 3;
// The three-way split in place (par 0): only the
// elements outside their part's range move (each into a hole of its part,
// through short lists), and the equal part -- most of the group -- stays where
// it is.  Its rank (RK) is any position inside its range (ranks only have to
// order the groups' disjoint ranges), so the previous round's rank is kept
// when it still lies inside: a doubling round of a near-periodic block then
// writes neither SA nor RK for its unresolved rotations.
constexpr uint32_t HG_THREE_IP = 4;
constexpr uint32_t HG_KEEP = 0xFFFFFFFFu;

// L-list items above HG_MIN whose chunks fit go to the huge list; their
// L-list entry gets size 0 (k3_part_l skips it)
__global__ void k3_hg_pick(Ctx c, uint64_t* __restrict__ list, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t item = list[i];
    const uint32_t m = it_size(item);
    if (m <= HG_MIN) return;
    const uint32_t nch = (m + HG_CH - 1) / HG_CH;
    const uint32_t k = atomicAdd(&c.L.ctr[C_HG], 1u);
    if (k >= HG_MAXN) return;
    const uint32_t base = atomicAdd(&c.L.ctr[C_HGC], nch);
    if (base + nch > HG_MAXCH) {            // over budget: k3_part_l keeps it
        c.L.hg[k] = 0;
        return;
    }
    c.L.hg[k] = item;
    list[i] = mk_item(it_slot(item), it_start(item), 0, it_shift(item), it_par(item));
}

struct HgGroup {
    uint32_t slot, s, m, shift, par, db, sh2, nch;
    uint64_t dmask;
};
__device__ __forceinline__ HgGroup hg_group(uint64_t item)
{
    HgGroup g;
    g.slot = it_slot(item);
    g.s = it_start(item);
    g.m = it_size(item);
    g.shift = it_shift(item);
    g.par = it_par(item);
    g.db = g.shift < 8 ? g.shift : 8;
    g.sh2 = g.shift - g.db;
    g.dmask = (1ull << g.db) - 1ull;
    g.nch = (g.m + HG_CH - 1) / HG_CH;
    return g;
}

// count[d] += 1 for a wave's lanes (one LDS atomic when they share a digit:
// a skewed group sends most elements to one bin); returns the lane's slot
__device__ __forceinline__ uint32_t wave_bin_add(uint32_t* cnt, bool act, uint32_t d)
{
    const uint64_t a = __ballot(act);
    if (!a) return 0;
    const int lead = __ffsll((unsigned long long)a) - 1;
    const uint32_t d0 = (uint32_t)__shfl((int)d, lead, 64);
    const int lane = threadIdx.x & 63;
    if (__ballot(act && d == d0) == a) {
        uint32_t b = 0;
        if (lane == lead) b = atomicAdd(&cnt[d0], (uint32_t)__popcll(a));
        b = (uint32_t)__shfl((int)b, lead, 64);
        return b + (uint32_t)__popcll(a & lanemask_lt());
    }
    return act ? atomicAdd(&cnt[d], 1u) : 0u;
}

// the chunks of every huge group as one flat index space: chunk j of the
// launch -> (group q, chunk in group), from the groups' chunk-count prefix
// (k3_hg_prefix, global: thousands of groups per level)
__device__ __forceinline__ uint32_t hg_count(const Ctx& c) { return min(c.L.ctr[C_HG], HG_MAXN); }
__device__ __forceinline__ uint32_t hg_group_of(const uint32_t* __restrict__ pre, uint32_t nh, uint32_t j)
{
    uint32_t lo = 0, hi = nh - 1;
    while (lo < hi) {                      // last q with pre[q] <= j (empty groups share a start)
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= j) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one workgroup: the huge groups' chunk counts, prefix-summed (0 for a group
// left to k3_part_l)
__global__ void __launch_bounds__(1024) k3_hg_prefix(Ctx c)
{
    __shared__ uint32_t scan_sh[17];
    const uint32_t nh = hg_count(c), tid = threadIdx.x;
    uint32_t run = 0;
    for (uint32_t q0 = 0; q0 < nh; q0 += 1024) {
        const uint32_t q = q0 + tid;
        const uint32_t k = q < nh ? hg_group(c.L.hg[q]).nch : 0u;
        uint32_t tot = 0;
        const uint32_t p = block_excl_scan_add<uint32_t>(k, scan_sh, &tot);
        if (q < nh) c.L.hg_pre[q] = run + p;
        run += tot;
        __syncthreads();
    }
    if (tid == 0) c.L.hg_pre[nh] = run;
}

// per-chunk digit counts, added into the group's 256 bin totals; and the key
// bits that vary inside the group (OR of key ^ the group's first key)
template <bool DBL>
__global__ void __launch_bounds__(256) k3_hg_hist(Ctx c)
{
    __shared__ uint32_t h[256];
    __shared__ uint64_t vx[4];
    __shared__ uint32_t ve[4], vl[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t nh = hg_count(c);
    if (nh == 0) return;
    const uint32_t total = c.L.hg_pre[nh];
    for (uint32_t j = blockIdx.x; j < total; j += gridDim.x) {
        const uint32_t q = hg_group_of(c.L.hg_pre, nh, j), ch = j - c.L.hg_pre[q];
        const HgGroup g = hg_group(c.L.hg[q]);
        const KeySrc ks = key_src(c, g.slot, g.par);
        const uint32_t* sv = (g.par ? c.scr.V : c.scr.SA) + (uint64_t)g.slot * c.scr.stride + g.s;
        h[tid] = 0;
        __syncthreads();
        const uint32_t a = ch * HG_CH, e = min(g.m, a + HG_CH);
        const uint64_t ref = elem_key<DBL>(ks, g.s, sv[0]);
        uint32_t d[HG_CH / 256];
        uint64_t vary = 0;
        uint32_t neq = 0, nlt = 0;
#pragma unroll
        for (uint32_t u = 0; u < HG_CH / 256; ++u) {   // all loads issued first
            const uint32_t i = a + u * 256 + tid, ic = i < e ? i : a;
            const uint64_t k = elem_key<DBL>(ks, g.s + ic, sv[ic]);
            d[u] = (uint32_t)((k >> g.sh2) & g.dmask);
            vary |= k ^ ref;
            neq += (i < e && k == ref) ? 1u : 0u;
            nlt += (i < e && k < ref) ? 1u : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < HG_CH / 256; ++u) (void)wave_bin_add(h, a + u * 256 + tid < e, d[u]);
        vary = wave_reduce_or64(vary);
        neq = wave_reduce_add<uint32_t>(neq);
        nlt = wave_reduce_add<uint32_t>(nlt);
        if ((tid & 63) == 0) { vx[tid >> 6] = vary; ve[tid >> 6] = neq; vl[tid >> 6] = nlt; }
        __syncthreads();
        if (h[tid]) atomicAdd(&c.L.hg_info[(uint64_t)q * 512 + 256 + tid], h[tid]);   // bin totals
        if (tid == 0) {
            const uint64_t v = vx[0] | vx[1] | vx[2] | vx[3];
            if (v) atomicOr(reinterpret_cast<unsigned long long*>(&c.L.hg_vary[q]), (unsigned long long)v);
            const uint32_t te = ve[0] + ve[1] + ve[2] + ve[3], tl = vl[0] + vl[1] + vl[2] + vl[3];
            if (te) atomicAdd(&c.L.hg_eqlt[2 * q], te);
            if (tl) atomicAdd(&c.L.hg_eqlt[2 * q + 1], tl);
        }
        __syncthreads();
    }
}

// one workgroup per huge group: bin starts -> the group's global cursors,
// sub-bucket classes (k3_part_l's rules), final-bin flags; or, when the digit
// window holds no varying key bit, one of the two skips (HG_SKIP_*)
__global__ void __launch_bounds__(256) k3_hg_scan(Ctx c)
{
    __shared__ uint32_t scan_sh[5];
    __shared__ uint32_t cls_sh[16];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    if (q >= hg_count(c)) return;
    const uint64_t item = c.L.hg[q];
    if (it_size(item) == 0) return;                   // uniform
    const HgGroup g = hg_group(item);
    const uint64_t vary = c.L.hg_vary[q] & (g.shift >= 64 ? ~0ull : ((1ull << g.shift) - 1ull));
    const int hb = vary ? 63 - __clzll((long long)vary) : -1;   // highest unsorted bit that varies
    if (hb < (int)g.sh2) {                            // uniform: no element moves at this level
        if (hb < 0) {                                 // every remaining key bit equal: one final tie group
            if (tid == 0) {
                c.L.hg_flag[q] = HG_SKIP_ALL;
                const uint32_t o = atomicAdd(c.L.ctr + C_T0 + c.tsel, 1u);
                c.L.t[c.tsel][o] = mk_item(g.slot, g.s, g.m, 0, 0);
                atomicAdd(c.L.ctr + C_TS0 + c.tsel, g.m);
                if (c.mode) atomicAdd(&c.L.runs[g.slot], 1u);
            }
            wg_classify(c, cls_sh, false, 0, 0, 0, 0, 0);
        } else {                                      // back to the L list at its highest varying bit
            if (tid == 0) c.L.hg_flag[q] = HG_SKIP_RELABEL;
            wg_classify(c, cls_sh, tid == 0, g.slot, g.s, g.m, (uint32_t)hb + 1u, g.par);
        }
        return;
    }
    uint32_t* info = c.L.hg_info + (uint64_t)q * 512;   // [0,256) start | flags, [256,512) totals -> cursors
    const uint32_t neq = c.L.hg_eqlt[2 * q], nlt = c.L.hg_eqlt[2 * q + 1];
    static_assert(L_MIN < HG_MIN, "three-way parts above L_MIN stay L items");
    if (2 * neq > g.m) {                              // uniform: three-way split around the first key
        const uint32_t ngt = g.m - neq - nlt;
        const uint32_t st3[3] = {0u, nlt, nlt + neq}, n3[3] = {nlt, neq, ngt};
        const bool ip = g.par == 0;
        if (tid == 0) {
            c.L.hg_flag[q] = ip ? HG_THREE_IP : HG_THREE;
            if (ip) {
                uint32_t rk = g.s + nlt + neq / 2;
                if (c.mode) {                         // keep the previous rank if it lies in the equal part
                    const uint64_t so = (uint64_t)g.slot * c.scr.stride;
                    const uint32_t r0 = c.scr.RK[so + c.scr.SA[so + g.s]];
                    if (r0 >= g.s + nlt && r0 < g.s + nlt + neq) rk = HG_KEEP;
                }
                c.L.hg_rank[q] = rk;
            }
        }
        if (tid < 3) {
            const bool f = tid == 1 || n3[tid] == 1;
            info[tid] = st3[tid] | (f ? HG_FINAL : 0u);
            info[256 + tid] = st3[tid];
        } else {
            info[tid] = g.m;                          // empty bins after the three
            info[256 + tid] = g.m;
        }
        if (tid == 1 && neq >= 2) {                   // the equal part: a final tie group
            const uint32_t o = atomicAdd(c.L.ctr + C_T0 + c.tsel, 1u);
            c.L.t[c.tsel][o] = mk_item(g.slot, g.s + nlt, neq, 0, 0);
            atomicAdd(c.L.ctr + C_TS0 + c.tsel, neq);
        }
        const uint32_t t3 = tid == 2 ? 2u : 0u;      // the two parts that are sorted further
        const bool push = (tid == 0 || tid == 2) && n3[t3] >= 2;
        wg_classify(c, cls_sh, push, g.slot, g.s + st3[t3], n3[t3], g.shift, ip ? g.par : g.par ^ 1u);   // in place: same buffer
        if (tid == 0 && c.mode) atomicAdd(&c.L.runs[g.slot], 1u + (nlt == 1 ? 1u : 0u) + (ngt == 1 ? 1u : 0u));
        return;
    }
    const uint32_t cc = info[256 + tid];
    const uint32_t ss = block_excl_scan_add<uint32_t>(cc, scan_sh, (uint32_t*)nullptr);
    info[256 + tid] = ss;                             // scatter cursor
    const bool alleq = cc >= 2 && size_class(cc) == 6 && g.sh2 == 0;   // one tie group
    const bool fin = cc == 1 || alleq;
    info[tid] = ss | (fin ? HG_FINAL : 0u);
    if (alleq) {
        const uint32_t o = atomicAdd(c.L.ctr + C_T0 + c.tsel, 1u);
        c.L.t[c.tsel][o] = mk_item(g.slot, g.s + ss, cc, 0, 0);
        atomicAdd(c.L.ctr + C_TS0 + c.tsel, cc);
    }
    wg_classify(c, cls_sh, cc >= 2 && !alleq, g.slot, g.s + ss, cc, g.sh2, g.par ^ 1u);
    const uint32_t r = wave_reduce_add<uint32_t>(fin ? 1u : 0u);
    if (c.mode && (tid & 63) == 0 && r) atomicAdd(&c.L.runs[g.slot], r);
}

// In-place three-way lists of a group (parts L = [0, nlt), E, G = [nlt + neq,
// m) of its range): an element outside its part's range is a mover (its
// value -- and, doubling, its key -- goes to its part's list in the
// other-parity buffers, free for this group) and its position a hole of the
// part it sits in.  Lists: movers to L / G / E at offsets 0 / nlt / nlt + ngt
// of dv (and keys of dk; at most nlt / ngt / nlt + ngt of them); holes
// likewise in RK's range (round 0: RK unused)
// or, doubling, in dk after the keys (nlt + ngt < m / 2: everything fits).
__device__ __forceinline__ uint32_t* hg_hole_list(const Ctx& c, const HgGroup& g, uint64_t* dk, uint32_t nlt,
                                                  uint32_t ngt)
{
    if (c.mode) return reinterpret_cast<uint32_t*>(dk + nlt + ngt);
    return c.scr.RK + (uint64_t)g.slot * c.scr.stride + g.s;
}

template <bool DBL>
__device__ __forceinline__ void hg_inplace_lists(const Ctx& c, uint32_t q, const HgGroup& g, const KeySrc& ks,
                                                 const uint32_t* sv, uint32_t* dv, uint64_t* dk, uint32_t a,
                                                 uint32_t e, uint32_t* cnt)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t neq = c.L.hg_eqlt[2 * q], nlt = c.L.hg_eqlt[2 * q + 1], ngt = g.m - neq - nlt;
    const uint32_t lo[3] = {0u, nlt + ngt, nlt};      // list offsets of the parts L, E, G (sizes <= nlt, nlt + ngt, ngt)
    uint32_t* hl = hg_hole_list(c, g, dk, nlt, ngt);
    const uint64_t ref = elem_key<DBL>(ks, g.s, sv[0]);
    constexpr uint32_t U = HG_CH / 256;
    uint32_t v[U], cl[U], rg[U], rm[U], rh[U];
    uint64_t k[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t i = a + u * 256 + tid, ic = i < e ? i : a;
        v[u] = sv[ic];
        k[u] = elem_key<DBL>(ks, g.s + ic, v[u]);
        cl[u] = k[u] < ref ? 0u : k[u] == ref ? 1u : 2u;
        rg[u] = ic < nlt ? 0u : ic < nlt + neq ? 1u : 2u;
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const bool mis = a + u * 256 + tid < e && cl[u] != rg[u];
        rm[u] = wave_bin_add(cnt, mis, cl[u]);
        rh[u] = wave_bin_add(cnt + 3, mis, rg[u]);
    }
    __syncthreads();
    if (tid < 6) {
        const uint32_t x = cnt[tid];
        cnt[8 + tid] = x ? atomicAdd(&c.L.hg_mc[6 * q + tid], x) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
        const uint32_t i = a + u * 256 + tid;
        if (i < e && cl[u] != rg[u]) {
            const uint32_t km = lo[cl[u]] + cnt[8 + cl[u]] + rm[u];
            dv[km] = v[u];
            if constexpr (DBL) if (cl[u] != 1) dk[km] = k[u];
            hl[lo[rg[u]] + cnt[11 + rg[u]] + rh[u]] = i;
        }
    }
    __syncthreads();
}

// in-place three-way groups: every mover into a hole of its part (the k-th
// mover of a part fills its k-th hole); keys move with the values while
// doubling (the parts L and G are sorted further by them)
template <bool DBL>
__global__ void __launch_bounds__(256) k3_hg_move(Ctx c)
{
    const uint32_t nh = hg_count(c);
    const GridSplit gs = grid_split(nh);
    if (gs.idle) return;
    for (uint32_t q = gs.q0; q < nh; q += gs.gstride) {
        if (c.L.hg_flag[q] != HG_THREE_IP) continue;
        const HgGroup g = hg_group(c.L.hg[q]);
        const KeySrc ks = key_src(c, g.slot, g.par);
        const uint64_t base = (uint64_t)g.slot * c.scr.stride + g.s;
        uint32_t* sv = c.scr.SA + base;               // par 0
        const uint32_t* dv = c.scr.V + base;
        uint64_t* dk = c.kB + base;
        uint64_t* sk = c.kA + base;
        const uint32_t neq = c.L.hg_eqlt[2 * q], nlt = c.L.hg_eqlt[2 * q + 1], ngt = g.m - neq - nlt;
        const uint32_t* hl = hg_hole_list(c, g, dk, nlt, ngt);
        const uint32_t n0 = c.L.hg_mc[6 * q], n1 = c.L.hg_mc[6 * q + 1], n2 = c.L.hg_mc[6 * q + 2];
        const uint32_t lo[3] = {0u, nlt + ngt, nlt};   // as in hg_inplace_lists
        (void)ks;
        for (uint32_t x = gs.slice * 256u + threadIdx.x; x < n0 + n1 + n2; x += gs.per * 256u) {
            const uint32_t part = x < n0 ? 0u : x < n0 + n2 ? 2u : 1u;   // L, G, then E
            const uint32_t kk = part == 0 ? x : part == 2 ? x - n0 : x - n0 - n2;
            const uint32_t j = lo[part] + kk;
            const uint32_t pos = hl[j];
            sv[pos] = dv[j];
            if constexpr (DBL) if (part != 1) sk[pos] = dk[j];
        }
    }
}

// every chunk: its elements to their bins (one global reservation per bin
// and chunk, then LDS cursors)
template <bool DBL>
__global__ void __launch_bounds__(256) k3_hg_scatter(Ctx c)
{
    __shared__ uint32_t cnt[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t nh = hg_count(c);
    if (nh == 0) return;
    const uint32_t total = c.L.hg_pre[nh];
    constexpr uint32_t U = HG_CH / 256;
    for (uint32_t j = blockIdx.x; j < total; j += gridDim.x) {
        const uint32_t q = hg_group_of(c.L.hg_pre, nh, j), ch = j - c.L.hg_pre[q];
        const uint32_t flag = c.L.hg_flag[q];
        if (flag && flag != HG_THREE && flag != HG_THREE_IP) continue;   // uniform: skipped at this level
        const HgGroup g = hg_group(c.L.hg[q]);
        const KeySrc ks = key_src(c, g.slot, g.par);
        const uint64_t base = (uint64_t)g.slot * c.scr.stride + g.s;
        const uint32_t* sv = (g.par ? c.scr.V : c.scr.SA) + base;
        uint32_t* dv = (g.par ? c.scr.SA : c.scr.V) + base;
        uint64_t* dk = (g.par ? c.kA : c.kB) + base;
        uint32_t* cur = c.L.hg_info + (uint64_t)q * 512 + 256;
        cnt[tid] = 0;
        __syncthreads();
        const uint32_t a = ch * HG_CH, e = min(g.m, a + HG_CH);
        if (flag == HG_THREE_IP) {                    // uniform
            hg_inplace_lists<DBL>(c, q, g, ks, sv, dv, dk, a, e, cnt);
            continue;
        }
        uint32_t v[U], d[U], r[U];
        uint64_t k[U];
        const uint64_t ref = flag == HG_THREE ? elem_key<DBL>(ks, g.s, sv[0]) : 0ull;
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t i = a + u * 256 + tid, ic = i < e ? i : a;
            v[u] = sv[ic];
            k[u] = elem_key<DBL>(ks, g.s + ic, v[u]);
            d[u] = flag == HG_THREE ? (k[u] < ref ? 0u : k[u] == ref ? 1u : 2u) : (uint32_t)((k[u] >> g.sh2) & g.dmask);
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) r[u] = wave_bin_add(cnt, a + u * 256 + tid < e, d[u]);
        __syncthreads();
        const uint32_t mine = cnt[tid];
        __syncthreads();
        if (mine) cnt[tid] = atomicAdd(&cur[tid], mine);   // this chunk's range of bin tid
        __syncthreads();
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t i = a + u * 256 + tid;
            if (i < e) {
                const uint32_t p = cnt[d[u]] + r[u];
                dv[p] = v[u];
                if constexpr (DBL) dk[p] = k[u];
            }
        }
        __syncthreads();
    }
}

// final sub-buckets of every huge group: SA, last column, RK, origPtr.  The
// grid's workgroups split over the groups (several per group when there are
// fewer groups than workgroups); a group skipped whole (HG_SKIP_ALL) is
// written from where its elements are, as one run headed at its start.
__global__ void __launch_bounds__(256) k3_hg_final(Ctx c)
{
    __shared__ uint32_t fin_pre[257];
    __shared__ uint32_t scan_sh[5];
    const uint32_t tid = threadIdx.x;
    const uint32_t nh = hg_count(c), G = gridDim.x;
    if (nh == 0) return;
    const uint32_t per = nh >= G ? 1u : G / nh;      // workgroups per group
    const uint32_t gstride = G / per;                 // groups in progress at once
    if (blockIdx.x >= per * gstride) return;
    const uint32_t slice = blockIdx.x % per;
    for (uint32_t q = blockIdx.x / per; q < nh; q += gstride) {
        const uint64_t item = c.L.hg[q];
        if (it_size(item) == 0) continue;
        const HgGroup g = hg_group(item);
        const uint32_t flag = c.L.hg_flag[q];
        if (flag == HG_SKIP_RELABEL) continue;
        const uint64_t so = (uint64_t)g.slot * c.scr.stride, base = so + g.s;
        if (flag == HG_THREE_IP) {                    // uniform: in SA already (par 0)
            const uint32_t neq = c.L.hg_eqlt[2 * q], nlt = c.L.hg_eqlt[2 * q + 1], ngt = g.m - neq - nlt;
            const uint32_t rk = c.L.hg_rank[q];
            const uint32_t* sa = c.scr.SA + base;
            if (c.mode && rk != HG_KEEP)
                for (uint32_t p = nlt + slice * 256u + tid; p < nlt + neq; p += per * 256u) c.scr.RK[so + sa[p]] = rk;
            if (slice == 0 && tid < 2) {              // a part of one rotation is final
                const bool one = tid == 0 ? nlt == 1 : ngt == 1;
                if (one) {
                    const uint32_t p = tid == 0 ? 0u : g.m - 1u;
                    const uint32_t v = sa[p];
                    c.scr.LL[base + p] = last_sym(c, g.slot, v);
                    if (c.mode) c.scr.RK[so + v] = g.s + p;
                    if (v == 0) c.blocks[c.b0 + g.slot].orig_ptr = g.s + p;
                }
            }
            continue;
        }
        if (flag == HG_SKIP_ALL) {                    // uniform
            const uint32_t* sv = (g.par ? c.scr.V : c.scr.SA) + base;
            // (a tie group: its last column is written once it resolves --
            // every tie is re-sorted later, or its block is periodic and
            // k_fallback_exact rebuilds that block's last column)
            for (uint32_t p = slice * 256u + tid; p < g.m; p += per * 256u) {
                const uint32_t v = sv[p];
                if (g.par) c.scr.SA[base + p] = v;
                if (c.mode) c.scr.RK[so + v] = g.s;
                if (v == 0) c.blocks[c.b0 + g.slot].orig_ptr = g.s + p;
            }
            continue;
        }
        const uint32_t* dv = (g.par ? c.scr.SA : c.scr.V) + base;
        const uint32_t* info = c.L.hg_info + (uint64_t)q * 512;
        // final bins' sizes (bin end = next bin's start; the last ends at m)
        const uint32_t st = info[tid] & ~HG_FINAL;
        const uint32_t en = tid < 255 ? (info[tid + 1] & ~HG_FINAL) : g.m;
        const uint32_t fsz = (info[tid] & HG_FINAL) ? en - st : 0u;
        uint32_t ftot = 0;
        const uint32_t fp = block_excl_scan_add<uint32_t>(fsz, scan_sh, &ftot);
        fin_pre[tid] = fp;
        if (tid == 255) fin_pre[256] = ftot;
        __syncthreads();
        for (uint32_t x = slice * 256u + tid; x < ftot; x += per * 256u) {
            uint32_t lo = 0, hi = 255;                 // the final bin holding flat index x
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (fin_pre[mid] <= x) lo = mid; else hi = mid - 1;
            }
            const uint32_t b0 = info[lo] & ~HG_FINAL;
            const uint32_t p = b0 + (x - fin_pre[lo]);
            const uint32_t v = dv[p];
            if (!g.par) c.scr.SA[base + p] = v;
            const uint32_t be = lo < 255 ? (info[lo + 1] & ~HG_FINAL) : g.m;
            if (be - b0 == 1) c.scr.LL[base + p] = last_sym(c, g.slot, v);   // ties: once resolved
            if (c.mode) c.scr.RK[so + v] = g.s + b0;
            if (v == 0) c.blocks[c.b0 + g.slot].orig_ptr = g.s + p;
        }
        __syncthreads();
    }
}

}  // namespace

void launch_bin(const uint64_t* list, uint32_t n, uint32_t nbv, uint32_t vs, uint32_t* binh, uint32_t* bincol,
                uint32_t* binst, uint32_t* seg, uint64_t* out, hipStream_t st)
{
    uint32_t nwg = (n + BIN_CH - 1) / BIN_CH;
    if (nwg > BIN_MAXWG) nwg = BIN_MAXWG;
    const uint32_t ch = ((n + nwg - 1) / nwg + 63) & ~63u;   // whole waves of items
    hipLaunchKernelGGL(k3_bin_hist, dim3(nwg), dim3(256), 0, st, list, n, nbv, ch, binh, bincol, vs);
    hipLaunchKernelGGL(k3_bin_scan, dim3(1), dim3(1024), 0, st, bincol, binst, nbv, seg);
    hipLaunchKernelGGL(k3_bin_scatter, dim3(nwg), dim3(256), 0, st, list, n, nbv, ch, binh, binst, out, vs);
    HIP_CHECK(hipGetLastError());
}

void launch_hg_pick(const Ctx& c, uint64_t* list, uint32_t nl, hipStream_t st)
{
    launch_zero(c.L.ctr, (1ull << C_HG) | (1ull << C_HGC), st);
    const uint64_t nhm = std::min<uint64_t>(nl, HG_MAXN);   // huge groups: at most this many
    HIP_CHECK(hipMemsetAsync(c.L.hg_info, 0, nhm * 512 * sizeof(uint32_t), st));
    HIP_CHECK(hipMemsetAsync(c.L.hg_vary, 0, nhm * sizeof(uint64_t), st));
    HIP_CHECK(hipMemsetAsync(c.L.hg_flag, 0, nhm * sizeof(uint32_t), st));
    HIP_CHECK(hipMemsetAsync(c.L.hg_eqlt, 0, 2 * nhm * sizeof(uint32_t), st));
    HIP_CHECK(hipMemsetAsync(c.L.hg_mc, 0, 6 * nhm * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k3_hg_pick, dim3((nl + 255) / 256), dim3(256), 0, st, c, list, nl);
    hipLaunchKernelGGL(k3_hg_prefix, dim3(1), dim3(1024), 0, st, c);
}

void launch_hg_level(const Ctx& c, uint32_t nl, int ncu, hipStream_t st)
{
    const dim3 gh(ncu * 4);
    dbl(c.keysrc, [&](auto d) {
        constexpr bool D = decltype(d)::value;
        hipLaunchKernelGGL(k3_hg_hist<D>, gh, dim3(256), 0, st, c);
        hipLaunchKernelGGL(k3_hg_scan, dim3((uint32_t)std::min<uint64_t>(nl, HG_MAXN)), dim3(256), 0, st, c);
        hipLaunchKernelGGL(k3_hg_scatter<D>, gh, dim3(256), 0, st, c);
        hipLaunchKernelGGL(k3_hg_move<D>, gh, dim3(256), 0, st, c);
        hipLaunchKernelGGL(k3_hg_final, gh, dim3(256), 0, st, c);
    });
    HIP_CHECK(hipGetLastError());
}

void launch_part_l(const Ctx& c, const uint64_t* items, int ncu, hipStream_t st)
{
    dbl(c.keysrc, [&](auto d) {
        hipLaunchKernelGGL(k3_part_l<decltype(d)::value>, dim3(ncu * STARCH_PL_WG), dim3(LT), 0, st, c, items);
    });
    HIP_CHECK(hipGetLastError());
}

}  // namespace bwt3
}  // namespace bz
