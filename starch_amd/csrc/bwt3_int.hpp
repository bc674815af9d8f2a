// starch_amd/csrc/bwt3_int.hpp -- what the units of the default block sort
// share (overview: bz2_bwt3.hip): its compile-time tuning, constants, work
// items, the launch context, the device helpers more than one unit uses, and
// the host launchers each unit exports.
//
//   bwt3_round0.hip  k3_pss_hist, k3_scan, k3_scatter_lds
//   bwt3_part.hip    k3_bin_*, k3_part_l, k3_hg_*
//   bwt3_leaf.hip    k3_sort_w, k3_sort_lds, k3_sort_grp
//   bwt3_rounds.hip  k3_classify_text, k3_gather*, k3_rk_*, k3_period, ...
//   bz2_bwt3.hip     launch_bwt3: the metadata arena and the control flow
#pragma once
#include "bz2_int.hpp"
#include "bz2_bwt.hpp"

#include <type_traits>

// ---------------------------------------------------------------------------
// Tuning: every compile-time knob of the block sort, with what it sizes and
// what was measured (block-sort ms per step on one MI355X; cfg2 = BED3,
// cfg4 = narrowPeak; DESIGN.md sections 4, 5 and 8 have the full record).
// tools/sweep_build.sh overrides them with EXTRA=-DSTARCH_...=n.
// ---------------------------------------------------------------------------
#ifndef STARCH_L_MIN
#define STARCH_L_MIN 4096   // groups above it are MSD-partitioned (k3_part_l), not sorted whole (2048/1024/512/256: cfg2 22.5/24.9/25.9/26.0 vs 22.6, cfg4 112/132/180/282 vs 107)
#endif
#ifndef STARCH_PL_WG
#define STARCH_PL_WG 2   // k3_part_l workgroups per CU (1/3/4: cfg2 21.1-21.3 in every arm)
#endif
#ifndef STARCH_PL_STG
#define STARCH_PL_STG 24576   // k3_part_l, PSS keys: largest group whose partitioned rotations are assembled in LDS and stored coalesced
#endif
#ifndef STARCH_PART_PU
#define STARCH_PART_PU 24   // k3_part_l: elements per thread and step, loads batched (cfg2 block sort: 4 -> 16 -> 24 -> 32: 21.3, 20.6, 20.4, 20.7 ms)
#endif
#ifndef STARCH_RANK_UNROLL
#define STARCH_RANK_UNROLL 4   // rank_in: keys in flight per step: 4 (cfg2 sort 22.8 -> 21.5-21.9 ms, cfg4 107.6 -> 104.1-104.4); 8 no better; 0 one at a time
#endif
// register budget (waves per SIMD) of the sort kernels: keeps a few groups
// resident per CU while their loads are in flight (sort_wpe, bwt3_leaf.hip)
#ifndef STARCH_WPE_GRP
#define STARCH_WPE_GRP 1   // the one-wave sorts: k3_sort_grp and k3_sort_lds<1, 4> (1/2: noise, profiles/r01_v22_sweep_hardq_wpe.json)
#endif
#ifndef STARCH_WPE_S
#define STARCH_WPE_S STARCH_WPE_GRP   // the S class (one wave, E = 2)
#endif
#ifndef STARCH_WPE_M1
#define STARCH_WPE_M1 1   // M1 (513..1024): k3_sort_lds<4, 4>
#endif
#ifndef STARCH_WPE_M0
#define STARCH_WPE_M0 6   // M0 (257..512): 6 waves per SIMD (cfg2 sort -0.5 ms, cfg4 -3 ms; profiles/r03_v5/sweep_*_m0w6.json)
#endif
#ifndef STARCH_M2_DB
#define STARCH_M2_DB 11   // k3_sort_lds: MSD digit bits of the M2 class (a 10-bit digit with 4 waves per SIMD: no gain)
#endif
#ifndef STARCH_LIM_NUM
#define STARCH_LIM_NUM 256   // k3_sort_lds: largest sub-bucket ranked by comparison, times E (64/128/512: within +-0.5 ms on cfg2, worse on cfg4)
#endif
#ifndef STARCH_LIM2_NUM
#define STARCH_LIM2_NUM 512   // ... and largest second-level sub-bucket, times E (256: as above)
#endif
#ifndef STARCH_W2_MAX
#define STARCH_W2_MAX 6   // k3_sort_lds: the second digit gives each large sub-bucket at most 2^W2_MAX bins
#endif
#ifndef STARCH_HARD_Q
#define STARCH_HARD_Q 32   // k3_sort_grp leaves a group to k3_sort_lds when its sub-bucket sizes z have sum z^2 > HARD_Q * m (24/48/64: noise; 16: -7 %, profiles/r01_v22_sweep_hardq_wpe.json)
#endif
#ifndef STARCH_GRP_CHUNK
#define STARCH_GRP_CHUNK 8   // k3_sort_grp: groups per queue pop, S class (measured table in the kernel)
#endif
#ifndef STARCH_GRP_CHUNK_S2
#define STARCH_GRP_CHUNK_S2 8    // ... S2 class (at 16 and 32 the groups in flight span more blocks per XCD than its L2 holds)
#endif

namespace bz {
namespace bwt3 {

constexpr int PTILE = 32768;            // rotations per partition tile
constexpr int PDIG = 12;
constexpr int PNB = 1 << PDIG;          // 4096 top-level buckets per block (binary digit)
// Blocks of 17..20 symbols (B = 5: narrowPeak / BED6+ text) take a mixed-radix
// top-level digit instead: their first 3 symbols, s0*nin^2 + s1*nin + s2 <
// 8000, so every bucket shares 15 key bits (the binary digit covers 2.4
// symbols there and leaves buckets ~6x larger).  Batches holding such blocks
// run the top-level kernels with 8192 bins.
constexpr int PNB_WIDE = 8192;
static_assert(PTILE <= 32768 && PNB_WIDE <= 8192, "k3_scatter_lds packs (digit << 15) | rotation-in-tile");
constexpr int MAXT = (900064 + PTILE - 1) / PTILE;   // tiles per block (bs <= 9)
// size classes: W rank-by-compare (one wave), S wave-private LDS sort,
// M1..M3 workgroup LDS sort, L MSD partition
constexpr uint32_t W_MAX = 64, S1_MAX = 128, S_MAX = 256, M0_MAX = 512, M1_MAX = 1024, M2_MAX = 2048, M3_MAX = 4096;
// groups above L_MIN are MSD-partitioned (k3_part_l) instead of sorted whole
constexpr uint32_t L_MIN = STARCH_L_MIN;
constexpr uint32_t GB_MIN = 16384;      // doubling: tie groups above this are gathered by the whole grid
constexpr uint32_t GB_MAXN = 8192;      // (two per block of a 2,048-block batch of near-periodic blocks, and spare)
constexpr uint32_t HG_MIN_PUSH = 32768;  // (= HG_MIN) L groups above it are partitioned by the whole grid
constexpr uint32_t HG_MIN = HG_MIN_PUSH;
constexpr uint32_t HG_MAXN = 8192;      // huge groups per level (two per near-periodic block of a full batch)
constexpr uint32_t BIN_MAXWG = 128;     // binning workgroups per list, at most (k3_bin_*)
constexpr uint32_t RBITS = 20;          // rank bits (n <= 899,985 < 2^20)
constexpr uint32_t TEXT_ROUNDS = 4;     // max text-extension rounds before doubling

// counters (u32) in the meta buffer
enum { C_W = 0, C_S, C_S2, C_M1, C_M2, C_M3, C_L0, C_L1, C_T0, C_T1, C_TIE_ELEMS, C_ERR, C_TS0, C_TS1, C_H, C_M0,
       C_HG, C_HGC, C_GB, C_LM0, C_LM1, C_N };

// item = slot[63:52] | start[51:32] | size[31:12] | parity[7] | shift[6:0]
__device__ __forceinline__ uint64_t mk_item(uint32_t slot, uint32_t s, uint32_t m, uint32_t shift, uint32_t par)
{
    return ((uint64_t)slot << 52) | ((uint64_t)s << 32) | ((uint64_t)m << 12) | ((uint64_t)par << 7) | shift;
}
__device__ __forceinline__ uint32_t it_slot(uint64_t x) { return (uint32_t)(x >> 52); }
__device__ __forceinline__ uint32_t it_start(uint64_t x) { return (uint32_t)(x >> 32) & 0xFFFFFu; }
__device__ __forceinline__ uint32_t it_size(uint64_t x) { return (uint32_t)(x >> 12) & 0xFFFFFu; }
__device__ __forceinline__ uint32_t it_par(uint64_t x) { return (uint32_t)(x >> 7) & 1u; }
__device__ __forceinline__ uint32_t it_shift(uint64_t x) { return (uint32_t)x & 127u; }

struct Geo {                   // per block key geometry
    uint32_t B;                // bits per symbol
    uint32_t D;                // symbols per round-0 key (KB = D*B bits)
    uint32_t Dp;               // symbols per text-round key (52/B)
    uint32_t KB;
    uint32_t nin;              // symbols in use
    uint32_t D1;               // top-level digit: 3 = mixed radix over 3 symbols, 0 = top PDIG key bits
    uint32_t SH;               // key bits every top-level bucket shares (3*B or PDIG)
    uint32_t pad;
};

__host__ __device__ constexpr uint64_t pss_words(uint64_t stride) { return stride / 8 + 64; }

struct Lists {
    uint32_t* ctr;          // C_N counters
    uint64_t* w;            // m <= 64
    uint64_t* s;            // m <= 128
    uint64_t* s2;           // m <= 256
    uint64_t* m0;           // m <= 512
    uint64_t* m1;           // m <= 1024
    uint64_t* m2;           // m <= 2048
    uint64_t* m3;           // m <= 4096
    uint64_t* l[2];         // m > 4096 (MSD partition), ping-pong by level
    uint64_t* t[2];         // tie groups, ping-pong by round
    Geo* geo;               // per slot
    uint32_t* gin;          // per slot: groups entering this round
    uint32_t* runs;         // per slot: runs produced this round
    uint32_t* periodic;     // per slot
    uint32_t* rounds;       // per slot: doubling rounds with work
    uint32_t* tied;         // per slot: still tied when doubling starts
    uint64_t* hg;           // huge groups of the current partition level (k3_hg_*), HG_MAXN
    uint32_t* hg_info;      // [HG_MAXN][512]: bin start | final flag; bin totals -> scatter cursors
    uint32_t* hg_pre;       // [HG_MAXN + 1]: chunk prefix of the huge groups (k3_hg_prefix)
    uint64_t* hg_vary;      // [HG_MAXN]: key bits that differ inside the group (OR of key ^ first key)
    uint32_t* hg_flag;      // [HG_MAXN]: HG_SKIP_* / HG_THREE (k3_hg_scan)
    uint32_t* hg_eqlt;      // [HG_MAXN][2]: elements equal to / below the group's first key
    uint32_t* hg_mc;        // [HG_MAXN][6]: in-place three-way: movers to / holes in each part
    uint32_t* hg_rank;      // [HG_MAXN]: in-place three-way: the equal part's rank (HG_KEEP: as it is)
    uint64_t* gb;           // doubling: tie groups gathered by the whole grid (k3_gather_big), GB_MAXN
    uint32_t* gb_h;         // ... their key offset h mod n
};

struct Ctx {
    BlockDesc* blocks;
    uint32_t b0;
    const uint8_t* blkbytes;
    uint64_t stride;        // block byte stride
    BwtScratch scr;
    Lists L;
    uint32_t nb;
    uint32_t lsel;          // L list that part/classify pushes into
    uint32_t tsel;          // tie list the sorts push into
    uint32_t mode;          // 0: SA only (round 0, text rounds); 1: doubling (RK, runs)
    uint32_t keysrc;        // 0: PSS at the text-round offset; 1 (doubling): keys by group position (kA/kB)
    uint64_t* kA;           // keysrc 1: keys of parity-0 items (K2) ...
    uint64_t* kB;           // ... and of parity-1 items (K)
    uint32_t rtext;         // text round (0: round 0)
    uint32_t* qhead;        // 8 queue heads of the current persistent launch
    const uint32_t* qseg;   // 9 per-XCD segment offsets of the current binned list
    uint32_t nbins;         // top-level bins of this batch (PNB or PNB_WIDE)
    uint32_t sdig;          // round 0, first L level: the scatter wrote the L buckets' first digits into LL
};

__device__ __forceinline__ uint64_t lanemask_lt()
{
    const int lane = threadIdx.x & 63;
    return lane ? (~0ull >> (64 - lane)) : 0ull;
}

// push a group [s, s+m) of slot with key bits [0, shift) still unsorted to its
// size class list (W, S, S2, M1, M2, M3, L).
// Pushes reserve their slots with LDS atomics and
// the workgroup takes ONE global atomic per class (the class counters are
// shared by every workgroup of the launch; per-wave global atomics on them
// serialise).  Every thread of the workgroup must call it; sh: 16 u32 of LDS.
__device__ __forceinline__ int size_class(uint32_t m)
{
    return m <= W_MAX ? 0 : m <= S1_MAX ? 1 : m <= S_MAX ? 2 : m > L_MIN ? 6 : m <= M0_MAX ? 7 : m <= M1_MAX ? 3 : m <= M2_MAX ? 4
         : m <= M3_MAX ? 5 : 6;
}
// class k's list and counter (0 W, 1 S, 2 S2, 3 M1, 4 M2, 5 M3, 6 L, 7 M0)
__device__ __forceinline__ uint64_t* class_list(const Ctx& c, int cls)
{
    return cls == 0 ? c.L.w : cls == 1 ? c.L.s : cls == 2 ? c.L.s2 : cls == 3 ? c.L.m1 : cls == 4 ? c.L.m2
         : cls == 5 ? c.L.m3 : cls == 7 ? c.L.m0 : c.L.l[c.lsel];
}
__device__ __forceinline__ uint32_t* class_ctr(const Ctx& c, int cls)
{
    return c.L.ctr + (cls == 0 ? C_W : cls == 1 ? C_S : cls == 2 ? C_S2 : cls == 3 ? C_M1 : cls == 4 ? C_M2
                      : cls == 5 ? C_M3 : cls == 7 ? C_M0 : C_L0 + c.lsel);
}

__device__ __forceinline__ void wg_classify(const Ctx& c, uint32_t* sh, bool pred, uint32_t slot, uint32_t s,
                                            uint32_t m, uint32_t shift, uint32_t par)
{
    const int cls = pred ? size_class(m) : -1;
    if (threadIdx.x < 8) sh[threadIdx.x] = 0;
    __syncthreads();
    uint32_t loff = 0;
    if (cls >= 0) loff = atomicAdd(&sh[cls], 1u);
    __syncthreads();
    if (threadIdx.x < 8 && sh[threadIdx.x]) sh[8 + threadIdx.x] = atomicAdd(class_ctr(c, (int)threadIdx.x), sh[threadIdx.x]);
    __syncthreads();
    if (cls >= 0) class_list(c, cls)[sh[8 + cls] + loff] = mk_item(slot, s, m, shift, par);
    if (cls == 6 && m > HG_MIN_PUSH) atomicMax(&c.L.ctr[C_LM0 + c.lsel], m);   // the host launches k3_hg_* only then
    __syncthreads();
}

// bits [bit, bit+nbits) of a packed symbol stream, right-aligned (1 <= nbits <= 64)
__device__ __forceinline__ uint64_t pss_bits(const uint64_t* __restrict__ w, uint64_t bit, uint32_t nbits)
{
    const uint64_t q = bit >> 6;
    const uint32_t p = (uint32_t)(bit & 63u);
    const uint64_t a = w[q];
    const uint64_t v = p ? ((a << p) | (w[q + 1] >> (64u - p))) : a;
    return v >> (64u - nbits);
}

// Key of a group element: rotation r (PSS modes) or group position q (K2/K).
struct KeySrc {
    const uint64_t* pss;
    const uint64_t* k;      // keys by position of this group's buffer (kA or kB by parity), slot base
    uint32_t B, kbits, n, off, usek;
    __device__ __forceinline__ uint64_t operator()(uint64_t q, uint32_t r) const
    {
        if (usek) return k[q];
        uint32_t rr = r + off;
        if (rr >= n) rr -= n;
        return pss_bits(pss, (uint64_t)rr * B, kbits);
    }
    // PSS key of rotation r, branch-free (two word loads, a funnel shift)
    __device__ __forceinline__ uint64_t key_pss(uint32_t r) const
    {
        uint32_t rr = r + off;
        rr = rr >= n ? rr - n : rr;
        const uint64_t bit = (uint64_t)rr * B;
        const uint64_t q = bit >> 6;
        const uint32_t p = (uint32_t)(bit & 63u);
        const uint64_t v = (pss[q] << p) | ((pss[q + 1] >> 1) >> (63u - p));
        return v >> (64u - kbits);
    }
    // ... and the last-column symbol of r (the symbol before it): its B bits sit
    // right before the key window, so three consecutive words cover both
    // (rotation 0 wraps: its symbol is the block's last)
    __device__ __forceinline__ uint64_t key_pss(uint32_t r, uint32_t& ls) const
    {
        const uint32_t pr = r ? r - 1u : n - 1u;
        uint32_t rr = r + off;
        rr = rr >= n ? rr - n : rr;
        if (off == 0 && r != 0) {
            const uint64_t bit0 = (uint64_t)pr * B;
            const uint64_t q0 = bit0 >> 6;
            const uint32_t p0 = (uint32_t)(bit0 & 63u);
            const uint64_t w0 = pss[q0], w1 = pss[q0 + 1], w2 = pss[q0 + 2];
            ls = (uint32_t)(((w0 << p0) | ((w1 >> 1) >> (63u - p0))) >> (64u - B));
            const uint32_t ps = p0 + B;                      // key start, relative to word q0
            const uint64_t a = ps >= 64 ? w1 : w0, b = ps >= 64 ? w2 : w1;
            const uint32_t p = ps & 63u;
            const uint64_t v = (a << p) | ((b >> 1) >> (63u - p));
            return v >> (64u - kbits);
        }
        const uint64_t pbit = (uint64_t)pr * B;
        const uint64_t pq = pbit >> 6;
        const uint32_t pp = (uint32_t)(pbit & 63u);
        const uint64_t pv = (pss[pq] << pp) | ((pss[pq + 1] >> 1) >> (63u - pp));
        ls = (uint32_t)(pv >> (64u - B));
        return key_pss(r);
    }
};

__device__ __forceinline__ KeySrc key_src(const Ctx& c, uint32_t slot, uint32_t par)
{
    KeySrc k;
    const uint64_t so = (uint64_t)slot * c.scr.stride;
    const Geo g = c.L.geo[slot];
    k.n = c.blocks[c.b0 + slot].n;
    k.B = g.B;
    k.usek = c.keysrc;
    k.pss = c.scr.K + so;
    k.k = (par ? c.kB : c.kA) + so;
    if (c.rtext == 0) {
        k.kbits = g.KB;
        k.off = 0;
    } else {
        k.kbits = g.Dp * g.B;
        k.off = (uint32_t)(((uint64_t)g.D + (uint64_t)(c.rtext - 1) * g.Dp) % k.n);
    }
    return k;
}

// Last-column symbol of rotation v: the rank (among the block's used byte
// values) of block[(v - 1) mod n] -- what the MTF consumes.  Rounds 0 and text
// rounds read it from the PSS; doubling rounds (PSS overwritten by keys) from
// the block text.  Written next to every final SA entry, so no separate
// gather pass over the block is needed.
__device__ __forceinline__ uint8_t last_sym(const Ctx& c, uint32_t slot, uint32_t v)
{
    const uint32_t b = c.b0 + slot;
    const uint32_t n = c.blocks[b].n;
    const uint32_t p = v ? v - 1u : n - 1u;
    if (!c.keysrc) {
        const uint32_t B = c.L.geo[slot].B;
        return (uint8_t)pss_bits(c.scr.K + (uint64_t)slot * c.scr.stride, (uint64_t)p * B, B);
    }
    const uint32_t byte = c.blkbytes[(uint64_t)b * c.stride + p];
    uint32_t r = __popc(c.blocks[b].in_use[byte >> 5] & ((1u << (byte & 31u)) - 1u));
    for (uint32_t j = 0; j < (byte >> 5); ++j) r += __popc(c.blocks[b].in_use[j]);
    return (uint8_t)r;
}

// key of the group element at position q holding rotation v: doubling keys
// (DBL) or the PSS; ls = its last-column symbol
template <bool DBL>
__device__ __forceinline__ uint64_t elem_key(const Ctx& c, const KeySrc& ks, uint32_t slot, uint64_t q, uint32_t v,
                                             uint32_t& ls)
{
    if constexpr (DBL) {
        ls = last_sym(c, slot, v);
        return ks.k[q];
    } else {
        return ks.key_pss(v, ls);
    }
}
template <bool DBL>
__device__ __forceinline__ uint64_t elem_key(const KeySrc& ks, uint64_t q, uint32_t v)
{
    if constexpr (DBL) return ks.k[q];
    else return ks.key_pss(v);
}

// persistent-kernel job fetch: one lane pops, the value is broadcast
__device__ __forceinline__ uint32_t wg_pop(const Ctx& c, const uint32_t* qs, uint32_t* job_sh, uint32_t x)
{
    if (threadIdx.x == 0) *job_sh = xq_pop(c.qhead, qs, x);
    __syncthreads();
    const uint32_t j = *job_sh;
    __syncthreads();
    return j;
}

// queue sizes of a binned list (LDS), before the first pop
__device__ __forceinline__ void load_qsizes_binned(const Ctx& c, uint32_t* qs)
{
    if (threadIdx.x < 8) qs[threadIdx.x] = c.qseg[threadIdx.x + 1] - c.qseg[threadIdx.x];
    __syncthreads();
}

// the grid split over ng groups: several workgroups per group when there are
// fewer groups than workgroups, else one (every workgroup looping over all
// groups cost thousands of empty iterations per workgroup with 4k groups)
struct GridSplit {
    uint32_t per, gstride, q0, slice;
    bool idle;
};
__device__ __forceinline__ GridSplit grid_split(uint32_t ng)
{
    GridSplit s;
    const uint32_t G = gridDim.x;
    s.per = ng >= G ? 1u : G / (ng ? ng : 1u);
    s.gstride = G / s.per;
    s.idle = blockIdx.x >= s.per * s.gstride;
    s.q0 = blockIdx.x / s.per;
    s.slice = blockIdx.x % s.per;
    return s;
}

// arr[slot] += v over the wave's active lanes, one atomic per distinct slot
// (per-group atomics on one block's counter serialise: a block of 450k tied
// pairs spent ~5 ms per doubling round in them).  Wave-uniform call.
__device__ __forceinline__ void wave_add_slot(uint32_t* arr, bool act, uint32_t slot, uint32_t v)
{
    const uint32_t lane = threadIdx.x & 63;
    uint64_t pend = __ballot(act);
    while (pend) {
        const int l = __ffsll((unsigned long long)pend) - 1;
        const uint32_t s0 = (uint32_t)__shfl((int)slot, l, 64);
        const bool mine = act && slot == s0;
        const uint32_t tot = wave_reduce_add<uint32_t>(mine ? v : 0u);
        if (lane == (uint32_t)l && tot) atomicAdd(&arr[s0], tot);
        pend &= ~__ballot(mine);
    }
}

// ---------------------------------------------------------------------------
// Host side.  Every launcher only enqueues on st, in the order it names its
// kernels; ncu = the device's compute units.
// ---------------------------------------------------------------------------
// f(std::true_type) in doubling rounds (keys by position in kA / kB), else
// f(std::false_type) (keys from the PSS): picks a kernel's DBL instantiation
template <class F>
inline void dbl(uint32_t keysrc, F&& f)
{
    if (keysrc) f(std::true_type{});
    else f(std::false_type{});
}

// bwt3_round0.hip: k3_pss_hist, k3_scan, k3_scatter_lds (c.qhead: a zeroed queue set)
void launch_round0(const Ctx& c, bool wide, int ncu, hipStream_t st);

// bwt3_part.hip
// k3_bin_hist, k3_bin_scan, k3_bin_scatter: list[0, n) -> out, binned into nbv
// bins (see bin_of); seg: the 9 segment offsets the next launch reads as c.qseg
void launch_bin(const uint64_t* list, uint32_t n, uint32_t nbv, uint32_t vs, uint32_t* binh, uint32_t* bincol,
                uint32_t* binst, uint32_t* seg, uint64_t* out, hipStream_t st);
// a partition level with groups above HG_MIN: the hg_* arrays cleared,
// k3_hg_pick, k3_hg_prefix (before the L list is binned) ...
void launch_hg_pick(const Ctx& c, uint64_t* list, uint32_t nl, hipStream_t st);
// ... and k3_hg_hist, k3_hg_scan, k3_hg_scatter, k3_hg_move, k3_hg_final (after)
void launch_hg_level(const Ctx& c, uint32_t nl, int ncu, hipStream_t st);
void launch_part_l(const Ctx& c, const uint64_t* items, int ncu, hipStream_t st);

// bwt3_leaf.hip: the sort of one size class over its binned list; the S
// classes clear C_H, run k3_sort_grp and then k3_sort_lds over the groups it
// listed as hard in `list` (the class list it consumed)
enum LeafClass { LEAF_W, LEAF_S, LEAF_S2, LEAF_M0, LEAF_M1, LEAF_M2, LEAF_M3 };
void launch_leaf(const Ctx& c, LeafClass k, const uint64_t* binned, uint64_t* list, int ncu, hipStream_t st);

// bwt3_rounds.hip
void launch_zero(uint32_t* ctr, uint64_t mask, hipStream_t st);    // k3_zero: the counters whose bits are set
void launch_period(const Ctx& c, hipStream_t st);
void launch_classify_text(const Ctx& c, const uint64_t* items, uint32_t nitems, hipStream_t st);
// k3_mark_tied, k3_rk_dense, C_GB cleared, k3_rk_groups, k3_rk_big
void launch_rk_init(const Ctx& c, const uint64_t* items, uint32_t nitems, int ncu, hipStream_t st);
// k3_gather, k3_gather_big
void launch_gather(const Ctx& c, const uint64_t* items, uint32_t nitems, uint32_t round, uint32_t rtext, int ncu,
                   hipStream_t st);
void launch_round_end(const Ctx& c, hipStream_t st);
void launch_finish(const Ctx& c, unsigned long long* stats, hipStream_t st);

}  // namespace bwt3
}  // namespace bz

