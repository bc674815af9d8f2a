// starch_amd/csrc/bwt3_round0.hip -- block sort, round 0: the packed symbol
// stream with the per-tile histograms of the top-level digit (k3_pss_hist),
// bucket starts, tile cursors and class lists (k3_scan), and the rotations
// scattered into bucket order (k3_scatter_lds).  Overview: bz2_bwt3.hip.
#include "bwt3_int.hpp"

namespace bz {
namespace bwt3 {
namespace {

constexpr int PT = 256;                 // hist threads

// top-level bucket of a rotation from its 64-bit key window (MSB first)
__device__ __forceinline__ uint32_t top_digit(uint64_t v, const Geo& g)
{
    if (!g.D1) return (uint32_t)(v >> (64 - PDIG));
    const uint32_t mask = (1u << g.B) - 1u;
    const uint32_t s0 = (uint32_t)(v >> (64 - g.B)) & mask;
    const uint32_t s1 = (uint32_t)(v >> (64 - 2 * g.B)) & mask;
    const uint32_t s2 = (uint32_t)(v >> (64 - 3 * g.B)) & mask;
    return (s0 * g.nin + s1) * g.nin + s2;
}

__device__ __forceinline__ int bits_for3(uint32_t x) { return x ? 32 - __clz(x) : 0; }

// symbol map of a block (rank among used byte values), >= 256 threads
__device__ __forceinline__ void load_sym(const BlockDesc& bd, uint8_t* sym, uint32_t* nin_out)
{
    const int tid = threadIdx.x;
    if (tid < 256) {
        uint32_t c = tid, below = 0;
        for (uint32_t j = 0; j < (c >> 5); ++j) below += __popc(bd.in_use[j]);
        below += __popc(bd.in_use[c >> 5] & ((1u << (c & 31)) - 1u));
        sym[c] = (uint8_t)below;
    }
    uint32_t nin = 0;
    for (int j = 0; j < 8; ++j) nin += __popc(bd.in_use[j]);
    *nin_out = nin;
}

// tile cursors / totals live in K after the PSS
__device__ __forceinline__ uint32_t* tile_hist(const Ctx& c, uint32_t slot)
{
    return reinterpret_cast<uint32_t*>(c.scr.K + (uint64_t)slot * c.scr.stride + pss_words(c.scr.stride));
}

// ---------------------------------------------------------------------------
// k3_pss_hist: the packed symbol stream and the per-tile bucket histogram
// (-> thist[slot][tile][NB]) in one pass over the block bytes; also the
// block's key geometry and nInUse (tile 0).
//
// The unit of work is a group of 64 consecutive rotations: their symbols are
// exactly B PSS words (so a tile, PTILE / 64 groups, owns whole words), built
// in registers, stored, and funnel-shifted for the 64 top-level digits without
// reading the PSS back.  The digits of a group's last rotations reach up to 15
// bits into the next group, so a group also packs the first ceil(16 / B)
// symbols after it.  A group whose 80 bytes lie inside the block takes five
// 16-byte loads; the block's last groups read byte by byte, wrapped mod n.
// The workgroup of a block's last tile also writes the wrapped tail of the
// PSS ((n + 128) * B bits plus one word, which the key loads of the last
// rotations read).  B is a template parameter of the group code: every shift
// and word index below is a constant.
// ---------------------------------------------------------------------------
constexpr uint32_t PGRP = 64;           // rotations per group
static_assert(PTILE % PGRP == 0, "tiles own whole groups, groups own whole PSS words");

template <int B>
__device__ __forceinline__ void pss_hist_group(const uint8_t* __restrict__ blk, const uint8_t* sym, uint32_t n,
                                               uint32_t g, uint32_t nw, uint64_t* __restrict__ pss, uint32_t* cnt,
                                               Geo geo)
{
    constexpr int NTAIL = (16 + B - 1) / B;         // symbols after the group a digit can reach
    constexpr int NRAW = (int)(PGRP + 16) / 4;      // the group's bytes and the 16 after it, as u32
    static_assert(NTAIL <= 16, "the tail symbols come from one more 16-byte load");
    const uint32_t j0 = g * PGRP;
    uint32_t raw[NRAW];
    if (j0 + PGRP + 16 <= n) {
        const uint4* q = reinterpret_cast<const uint4*>(blk + j0);
        const uint4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3], v4 = q[4];
        raw[0] = v0.x; raw[1] = v0.y; raw[2] = v0.z; raw[3] = v0.w;
        raw[4] = v1.x; raw[5] = v1.y; raw[6] = v1.z; raw[7] = v1.w;
        raw[8] = v2.x; raw[9] = v2.y; raw[10] = v2.z; raw[11] = v2.w;
        raw[12] = v3.x; raw[13] = v3.y; raw[14] = v3.z; raw[15] = v3.w;
        raw[16] = v4.x; raw[17] = v4.y; raw[18] = v4.z; raw[19] = v4.w;
    } else {                                        // positions at or past n wrap
        uint32_t jj = j0 < n ? j0 : j0 % n;
#pragma unroll
        for (int i = 0; i < NRAW; ++i) {
            uint32_t x = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (4 * i + t < (int)PGRP + NTAIL) {
                    x |= (uint32_t)blk[jj] << (8 * t);
                    jj = jj + 1 == n ? 0u : jj + 1;
                }
            }
            raw[i] = x;
        }
    }
    uint64_t w[B + 1];
#pragma unroll
    for (int i = 0; i <= B; ++i) w[i] = 0;
#pragma unroll
    for (int k = 0; k < (int)PGRP + NTAIL; ++k) {    // symbol k at bits [k * B, k * B + B), MSB first
        const uint64_t sy = sym[(raw[k >> 2] >> (8 * (k & 3))) & 0xffu];
        const int bit = k * B, ix = bit >> 6, sh = 64 - B - (bit & 63);
        if (sh >= 0) {
            w[ix] |= sy << sh;
        } else {
            w[ix] |= sy >> (-sh);
            if (ix < B) w[ix + 1] |= sy << (64 + sh);
        }
    }
    const uint32_t w0 = g * B;
    if (w0 + B <= nw) {
#pragma unroll
        for (int i = 0; i < B; ++i) pss[w0 + i] = w[i];
    } else {
#pragma unroll
        for (int i = 0; i < B; ++i)
            if (w0 + i < nw) pss[w0 + i] = w[i];
    }
    if (j0 >= n) return;                            // the wrapped tail holds no rotations
    geo.B = B;
#pragma unroll
    for (int k = 0; k < (int)PGRP; ++k) {
        const int bit = k * B, ix = bit >> 6, p = bit & 63;
        const uint64_t v = (w[ix] << p) | ((w[ix + 1] >> 1) >> (63 - p));
        if (j0 + k < n) atomicAdd(&cnt[top_digit(v, geo)], 1u);
    }
}

template <int NB>
__global__ void __launch_bounds__(PT) k3_pss_hist(Ctx c)
{
    __shared__ uint32_t cnt[NB];
    __shared__ uint8_t sym[256];
    const uint32_t slot = blockIdx.y, b = c.b0 + slot, tile = blockIdx.x;
    const uint32_t n = c.blocks[b].n;
    // every workgroup derives the block's geometry itself (it waits on no
    // other); tile 0 publishes it for k3_scan and everything after
    uint32_t nin;
    load_sym(c.blocks[b], sym, &nin);
    Geo geo;
    geo.B = nin > 1 ? (uint32_t)bits_for3(nin - 1) : 1u;
    geo.D = 64 / geo.B;
    geo.KB = geo.D * geo.B;
    geo.Dp = (64 - PDIG) / geo.B;
    geo.nin = nin;
    geo.D1 = (c.nbins == PNB_WIDE && geo.B == 5 && nin <= 20) ? 3u : 0u;
    geo.SH = geo.D1 ? 3 * geo.B : PDIG;
    geo.pad = 0;
    if (tile == 0 && threadIdx.x == 0) {
        c.L.geo[slot] = geo;
        c.blocks[b].n_in_use = nin;
    }
    const uint32_t t0 = tile * PTILE;
    if (t0 >= n) return;
    for (int i = threadIdx.x; i < NB; i += PT) cnt[i] = 0;
    __syncthreads();
    const uint32_t B = geo.B;
    const uint32_t nw = (uint32_t)(((uint64_t)(n + 128) * B + 63) / 64 + 1);
    const uint32_t g0 = tile * (PTILE / PGRP);
    const uint32_t g1 = n - t0 <= (uint32_t)PTILE ? (nw + B - 1) / B : g0 + PTILE / PGRP;
    const uint8_t* blk = c.blkbytes + (uint64_t)b * c.stride;
    uint64_t* pss = c.scr.K + (uint64_t)slot * c.scr.stride;
    auto run = [&](auto bc) {
        for (uint32_t g = g0 + threadIdx.x; g < g1; g += PT)
            pss_hist_group<decltype(bc)::value>(blk, sym, n, g, nw, pss, cnt, geo);
    };
    switch (B) {
    case 1: run(std::integral_constant<int, 1>{}); break;
    case 2: run(std::integral_constant<int, 2>{}); break;
    case 3: run(std::integral_constant<int, 3>{}); break;
    case 4: run(std::integral_constant<int, 4>{}); break;
    case 5: run(std::integral_constant<int, 5>{}); break;
    case 6: run(std::integral_constant<int, 6>{}); break;
    case 7: run(std::integral_constant<int, 7>{}); break;
    default: run(std::integral_constant<int, 8>{}); break;
    }
    __syncthreads();
    uint32_t* th = tile_hist(c, slot) + (uint64_t)tile * NB;
    for (int i = threadIdx.x; i < NB; i += PT) th[i] = cnt[i];
}

// ---------------------------------------------------------------------------
// k3_scan: per block -- totals, bucket starts, per-tile cursors, class lists
// ---------------------------------------------------------------------------
constexpr int ST = 1024;              // k3_scan threads: NB/1024 consecutive buckets each

template <int NB>
__global__ void __launch_bounds__(ST) k3_scan(Ctx c)
{
    constexpr int Q = NB / (4 * ST);      // uint4 per thread
    __shared__ uint32_t scan_sh[ST / 64 + 1];
    __shared__ uint32_t cls_sh[16];
    const int tid = threadIdx.x;
    const uint32_t slot = blockIdx.x, b = c.b0 + slot;
    const uint32_t n = c.blocks[b].n;
    const uint32_t ntile = (n + PTILE - 1) / PTILE;
    uint4* th = reinterpret_cast<uint4*>(tile_hist(c, slot));   // [tile][NB/4]
    uint4* tot = th + (uint64_t)MAXT * (NB / 4);
    uint4 a[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) a[j] = make_uint4(0, 0, 0, 0);
#pragma unroll 4
    for (uint32_t k = 0; k < ntile; ++k) {
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            const uint4 x = th[(uint64_t)k * (NB / 4) + tid * Q + j];
            a[j].x += x.x; a[j].y += x.y; a[j].z += x.z; a[j].w += x.w;
        }
    }
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < Q; ++j) { tot[tid * Q + j] = a[j]; sum += a[j].x + a[j].y + a[j].z + a[j].w; }
    const uint32_t pre = block_excl_scan_add<uint32_t>(sum, scan_sh, (uint32_t*)nullptr);
    uint4 run[Q];
    {
        uint32_t r = pre;
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            run[j] = make_uint4(r, r + a[j].x, r + a[j].x + a[j].y, r + a[j].x + a[j].y + a[j].z);
            r += a[j].x + a[j].y + a[j].z + a[j].w;
        }
    }
#pragma unroll 4
    for (uint32_t k = 0; k < ntile; ++k) {
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            uint4& x = th[(uint64_t)k * (NB / 4) + tid * Q + j];
            const uint4 v = x;
            x = run[j];
            run[j].x += v.x; run[j].y += v.y; run[j].z += v.z; run[j].w += v.w;
        }
    }
    const Geo geo = c.L.geo[slot];
    const uint32_t shift = geo.KB - geo.SH;
    uint32_t st = pre;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        const uint32_t cnt4[4] = {a[j].x, a[j].y, a[j].z, a[j].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            wg_classify(c, cls_sh, cnt4[q] >= 2, slot, st, cnt4[q], shift, 0);
            st += cnt4[q];
        }
    }
}

// ---------------------------------------------------------------------------
// k3_scatter_lds: rotations -> bucket order in SA (persistent, per-XCD block
// streams: queue x holds the tiles of blocks x, x+8, ... in order), with the
// writes staged in LDS.  Each 32 K
// tile is handled in two 16 K halves: the half's rotations are counting-
// sorted by bucket inside LDS (entry = digit << 15 | rotation in the tile), then written
// out in local order, so consecutive threads store consecutive SA positions
// of a bucket's run instead of one scattered 4-byte store per rotation (a
// direct scatter's writes cost ~2.5-3.5x their bytes in HBM traffic).
//
// Thread t owns bins [t * BPT, (t + 1) * BPT): it scans their local counts and
// keeps their SA cursors in registers.  The scan leaves one word per bin for
// the write-out, (cursor - local start) mod 2^RBITS | flags, so a staged entry
// j of bin d goes to SA position (ent[d] + j) mod 2^RBITS and the write-out
// reads two LDS words per rotation.  The last stage of a job pops the next
// job and loads its cursor row and first PSS words while it writes out.
// ---------------------------------------------------------------------------
constexpr int SCT = 1024;

template <int NB>
__global__ void __launch_bounds__(SCT) k3_scatter_lds(Ctx c)
{
    // rotations staged at a time: half a tile (4096 bins), a quarter (8192 bins: LDS)
    constexpr uint32_t SH_HALF = NB == PNB ? PTILE / 2 : PTILE / 4;
    constexpr int SU = (int)(SH_HALF / SCT);       // consecutive rotations per thread
    constexpr int BPT = NB / SCT;                  // bins per thread in the local scan
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    constexpr uint32_t PMASK = (1u << RBITS) - 1u;
    constexpr uint32_t F_ONE = 1u << 30, F_L = 1u << 31;   // ent flags: singleton bucket, L-class bucket
    static_assert(BPT % 4 == 0 && BPT * 2 <= 32, "cursor rows load as uint4; two flag bits per owned bin");
    __shared__ uint32_t lst[NB];                   // local counts, then local bucket starts
    __shared__ uint32_t ent[NB];
    __shared__ uint32_t stage[SH_HALF];
    // the next 8 key bits below the top-level digit of every staged rotation,
    // by rotation: written next to the SA entries of the heavy (L-class)
    // buckets, where k3_part_l's first partition reads them instead of
    // gathering each rotation's key again
    __shared__ __attribute__((aligned(16))) uint8_t stage8[SH_HALF];
    __shared__ uint32_t scan_sh[SCT / 64];
    __shared__ uint32_t qs[8];
    __shared__ uint32_t job_sh;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t x = xcc_id();
    if (tid < 8) qs[tid] = ((uint32_t)tid < c.nb ? (c.nb - tid + 7) / 8 : 0u) * MAXT;
    for (int i = tid; i < NB; i += SCT) lst[i] = 0;   // (every stage leaves the counts cleared)
    __syncthreads();
    uint32_t job = wg_pop(c, qs, &job_sh, x);
    uint32_t curv[BPT];                            // SA cursors of this thread's bins
    uint64_t w0[4];                                // the first stage's PSS words
    bool pre = false;                              // curv / w0 hold this job's (loaded by the job before)
    uint32_t flv = 0, fslot = NONE;                // flag bits of this thread's bins, and the slot they belong to
    auto load_row = [&](const uint32_t* th, uint32_t tile) {
        const uint4* row = reinterpret_cast<const uint4*>(th + (uint64_t)tile * NB + tid * BPT);
#pragma unroll
        for (int q = 0; q < BPT / 4; ++q) {
            const uint4 v = row[q];
            curv[4 * q] = v.x; curv[4 * q + 1] = v.y; curv[4 * q + 2] = v.z; curv[4 * q + 3] = v.w;
        }
    };
    auto load_w0 = [&](const uint64_t* pss, uint32_t t0, uint32_t B) {
        const uint64_t qw = ((uint64_t)(t0 + tid * SU) * B) >> 6;
#pragma unroll
        for (int q = 0; q < 4; ++q) w0[q] = pss[qw + q];
    };
    while (job != NONE) {
        const uint32_t y = job >> 28, k = job & 0x0FFFFFFFu;
        const uint32_t slot = y + 8u * (k / MAXT), tile = k % MAXT;
        const uint32_t b = c.b0 + slot;
        const uint32_t n = c.blocks[b].n;
        const uint32_t t0 = tile * PTILE;
        if (t0 >= n) {                               // uniform
            job = wg_pop(c, qs, &job_sh, x);
            pre = false;
            continue;
        }
        const uint64_t so = (uint64_t)slot * c.scr.stride;
        const uint32_t* th = tile_hist(c, slot);
        const Geo geo = c.L.geo[slot];
        const uint32_t B = geo.B;
        const uint64_t* pss = c.scr.K + so;
        uint32_t* SA = c.scr.SA + so;
        uint8_t* LL = c.scr.LL + so;
        if (!pre) {
            load_row(th, tile);
            load_w0(pss, t0, B);
        }
        if (slot != fslot) {                         // bucket totals are per block: their flags once per slot
            const uint32_t* tot = th + (uint64_t)MAXT * NB + tid * BPT;
            flv = 0;
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                const uint32_t t = tot[q];
                flv |= (t == 1u ? 1u : t > L_MIN ? 2u : 0u) << (2 * q);
            }
            fslot = slot;
        }
        const uint32_t e = n - t0 < (uint32_t)PTILE ? n - t0 : (uint32_t)PTILE;
        uint32_t njob = NONE;
        pre = false;
        for (uint32_t h0 = 0; h0 < e; h0 += SH_HALF) {
            const uint32_t he = e - h0 < SH_HALF ? e - h0 : SH_HALF;
            const bool last = h0 + SH_HALF >= e;
            // the next job's number travels through job_sh behind this stage's barriers
            if (last && tid == 0) job_sh = xq_pop(c.qhead, qs, x);
            // digits of SU consecutive rotations from four PSS words; local counts
            const uint32_t q0 = tid * SU;                // SCT * SU == SH_HALF
            uint32_t d[SU], p[SU];
            {
                const uint64_t bit0 = (uint64_t)(t0 + h0 + q0) * B;
                const uint64_t qw = bit0 >> 6;
                const uint32_t p0 = (uint32_t)(bit0 & 63u);
                if (h0 != 0) {                           // (the first stage's words are loaded already)
#pragma unroll
                    for (int q = 0; q < 4; ++q) w0[q] = pss[qw + q];
                }
                const uint32_t sds = 64u - geo.SH - 8u;       // (the key window's bits [SH, SH + 8))
                uint32_t sdw[SU / 4] = {};
#pragma unroll
                for (int u = 0; u < SU; ++u) {
                    const uint32_t bit = p0 + (uint32_t)u * B;
                    const uint32_t ix = bit >> 6, pb = bit & 63u;
                    const uint64_t a = ix == 0 ? w0[0] : ix == 1 ? w0[1] : w0[2];
                    const uint64_t nx = ix == 0 ? w0[1] : ix == 1 ? w0[2] : w0[3];
                    const uint64_t v = (a << pb) | ((nx >> 1) >> (63u - pb));
                    d[u] = top_digit(v, geo);
                    sdw[u / 4] |= ((uint32_t)(v >> sds) & 0xFFu) << (8 * (u % 4));
                }
                uint32_t* s8 = reinterpret_cast<uint32_t*>(stage8 + q0);   // SU bytes per thread, in rotation order
#pragma unroll
                for (int q = 0; q < SU / 4; ++q) s8[q] = sdw[q];
            }
#pragma unroll
            for (int u = 0; u < SU; ++u) p[u] = (q0 + u < he) ? atomicAdd(&lst[d[u]], 1u) : 0u;
            __syncthreads();
            if (last) njob = job_sh;
            // local bucket starts (exclusive scan, BPT bins per thread), the
            // write-out words, and the cursors moved past this stage
            {
                uint32_t v[BPT], sum = 0;
#pragma unroll
                for (int q = 0; q < BPT; ++q) { v[q] = lst[tid * BPT + q]; sum += v[q]; }
                const uint32_t inc = wave_incl_scan_add(sum);
                if (lane == 63) scan_sh[wid] = inc;
                __syncthreads();
                uint32_t run = wave_reduce_add<uint32_t>(lane < wid ? scan_sh[lane] : 0u) + inc - sum;
#pragma unroll
                for (int q = 0; q < BPT; ++q) {
                    lst[tid * BPT + q] = run;
                    ent[tid * BPT + q] = ((curv[q] - run) & PMASK) | (((flv >> (2 * q)) & 3u) << 30);
                    curv[q] += v[q];
                    run += v[q];
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < SU; ++u)
                if (q0 + u < he) {
                    const uint32_t j = lst[d[u]] + p[u];
                    stage[j] = (d[u] << 15) | (h0 + q0 + u);   // 13 + 15 bits
                }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < BPT; ++q) lst[tid * BPT + q] = 0;
            // the next job's cursor row and first PSS words load while this stage writes out
            if (njob != NONE) {                          // uniform
                const uint32_t nk = njob & 0x0FFFFFFFu;
                const uint32_t nslot = (njob >> 28) + 8u * (nk / MAXT), ntile = nk % MAXT;
                if (ntile * (uint32_t)PTILE < c.blocks[c.b0 + nslot].n) {
                    load_row(tile_hist(c, nslot), ntile);
                    load_w0(c.scr.K + (uint64_t)nslot * c.scr.stride, ntile * (uint32_t)PTILE, c.L.geo[nslot].B);
                    pre = true;
                }
            }
            // write out in local (bucket) order: runs of a bucket land on consecutive SA slots
            // (four entries' LDS reads in flight per step)
            for (int u0 = 0; u0 < SU && (uint32_t)tid + (uint32_t)u0 * SCT < he; u0 += 4) {
                uint32_t sv[4], se[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t j = (uint32_t)tid + (uint32_t)(u0 + i) * SCT;
                    sv[i] = stage[j < he ? j : (uint32_t)tid];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) se[i] = ent[sv[i] >> 15];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                const uint32_t j = (uint32_t)tid + (uint32_t)(u0 + i) * SCT;
                if (j >= he) break;
                const uint32_t v = sv[i];
                const uint32_t r = t0 + (v & 0x7FFFu);
                const uint32_t en = se[i];
                const uint32_t pos = (en + j) & PMASK;
                SA[pos] = r;
                if (en & F_ONE) {                      // singleton bucket: final
                    LL[pos] = (uint8_t)pss_bits(pss, (uint64_t)(r ? r - 1u : n - 1u) * B, B);
                    if (r == 0) c.blocks[b].orig_ptr = pos;
                } else if (en & F_L) {                 // L class: its first partition digit (LL is free there until then)
                    LL[pos] = stage8[(v & 0x7FFFu) - h0];
                }
                }
            }
            __syncthreads();
        }
        job = njob;
    }
}

}  // namespace

void launch_round0(const Ctx& c, bool wide, int ncu, hipStream_t st)
{
    // the scatter: about one block in flight per XCD: one 1024-thread workgroup
    // per CU, a block's MAXT tiles spread over its XCD's CUs
    const dim3 gsc((ncu + 7) / 8 * 8);
    auto run = [&](auto bins) {
        constexpr int NB = decltype(bins)::value;
        hipLaunchKernelGGL(k3_pss_hist<NB>, dim3(MAXT, c.nb), dim3(PT), 0, st, c);
        hipLaunchKernelGGL(k3_scan<NB>, dim3(c.nb), dim3(ST), 0, st, c);
        hipLaunchKernelGGL(k3_scatter_lds<NB>, gsc, dim3(SCT), 0, st, c);
    };
    if (wide) run(std::integral_constant<int, PNB_WIDE>{});
    else run(std::integral_constant<int, PNB>{});
    HIP_CHECK(hipGetLastError());
}

}  // namespace bwt3
}  // namespace bz
