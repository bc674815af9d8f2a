// starch_amd/csrc/bwt3_leaf.hip -- block sort: the leaf sorts of the size
// classes.  k3_sort_w (W: groups <= 64, packed over a wave's lanes),
// k3_sort_grp (S, S2: one wave per group) and k3_sort_lds (M0..M3: one
// workgroup per group; and the groups k3_sort_grp lists as hard).  Every sort
// writes SA and the last column and lists the runs of equal keys.  Overview:
// bz2_bwt3.hip.
#include "bwt3_int.hpp"

namespace bz {
namespace bwt3 {
namespace {

__device__ __forceinline__ void wave_sync_lds3()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Append `item` for every lane with pred to list/ctr; one atomic per wave.
// Must be reached by all 64 lanes of the wave.
__device__ __forceinline__ void wave_push(uint32_t* ctr, uint64_t* list, bool pred, uint64_t item)
{
    const uint64_t m = __ballot(pred);
    if (!m) return;
    const int leader = __ffsll((unsigned long long)m) - 1;
    const int lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(ctr, (uint32_t)__popcll(m));
    base = __shfl(base, leader, 64);
    if (pred) list[base + __popcll(m & lanemask_lt())] = item;
}

// Finish a sorted group: SA, RK, origPtr, tie groups, run count.
// Called by every thread of a wave with (j = sorted position in the group,
// v = rotation, valid, hp = head position of j's run, end = j ends its run,
// lsym = last-column symbol of v).
__device__ __forceinline__ void emit_sorted(const Ctx& c, uint32_t slot, uint32_t s, uint32_t j, uint32_t v,
                                            bool valid, uint32_t hp, bool end, uint32_t& runs_acc, uint32_t lsym)
{
    const uint64_t so = (uint64_t)slot * c.scr.stride;
    if (valid) {
        c.scr.SA[so + s + j] = v;
        c.scr.LL[so + s + j] = (uint8_t)lsym;
        if (c.mode) c.scr.RK[so + v] = s + hp;
        if (v == 0) c.blocks[c.b0 + slot].orig_ptr = s + j;
    }
    const bool tie = valid && end && j > hp;
    const uint64_t tb = __ballot(tie);
    if (tb) {
        wave_push(c.L.ctr + C_T0 + c.tsel, c.L.t[c.tsel], tie, mk_item(slot, s + hp, j - hp + 1, 0, 0));
        const uint32_t te = wave_reduce_add<uint32_t>(tie ? j - hp + 1 : 0u);
        if ((threadIdx.x & 63) == 0) atomicAdd(c.L.ctr + C_TS0 + c.tsel, te);
    }
    runs_acc += (uint32_t)__popcll(__ballot(valid && end));
}

// The values half of emit_sorted, for the kernels that reserve their tie-list
// slots once per group (tie_reserve) instead of once per wave and row
__device__ __forceinline__ void emit_vals(const Ctx& c, uint32_t slot, uint32_t s, uint32_t j, uint32_t v, bool valid,
                                          uint32_t hp, uint32_t lsym)
{
    if (valid) {
        const uint64_t so = (uint64_t)slot * c.scr.stride;
        c.scr.SA[so + s + j] = v;
        c.scr.LL[so + s + j] = (uint8_t)lsym;
        if (c.mode) c.scr.RK[so + v] = s + hp;
        if (v == 0) c.blocks[c.b0 + slot].orig_ptr = s + j;
    }
}

// First tie-list slot for a group's tcnt tie runs (tcnt: this wave's count,
// uniform per wave): one global atomic per group.  The tie-list counter is
// one address shared by every wave of the launch; a returning atomic per wave
// and row serialised there (text with many short repeats -- narrowPeak --
// pushes millions of tie runs per batch).  NW > 1: every wave of the
// workgroup (one group) calls it; tc/tb: NW + 1 words of LDS.
template <int NW>
__device__ __forceinline__ uint32_t tie_reserve(const Ctx& c, uint32_t tcnt, uint32_t* tc, int wid, int lane)
{
    uint32_t* ctr = c.L.ctr + C_T0 + c.tsel;
    if constexpr (NW == 1) {
        uint32_t base = 0;
        if (lane == 0 && tcnt) base = atomicAdd(ctr, tcnt);
        return (uint32_t)__shfl((int)base, 0, 64);
    } else {
        if (lane == 0) tc[wid] = tcnt;
        __syncthreads();
        if (wid == 0 && lane == 0) {
            uint32_t t = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += tc[w];
            tc[NW] = t ? atomicAdd(ctr, t) : 0u;
        }
        __syncthreads();
        uint32_t base = tc[NW];
        for (int w = 0; w < wid; ++w) base += tc[w];
        return base;
    }
}

// ---------------------------------------------------------------------------
// k3_sort_w: groups of <= 64, packed several to a wave.  Each wave takes
// chunks of 64 consecutive items of its XCD's segment (one item per lane,
// one coalesced load); groups are laid out back to back over the 64 lanes as
// far as they fit, so one round of loads (rotations, then keys) serves them
// all -- text-round tie groups are mostly pairs, one group per wave left 60
// lanes idle and paid a full load round trip per pair.  Every element ranks
// itself among its group's members (keys by lane shuffle), then sorted order
// goes through LDS; heads, ends and tie runs are per group.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, 64);
    return ((uint64_t)hi << 32) | lo;
}

template <bool DBL>
__global__ void __launch_bounds__(256) k3_sort_w(Ctx c, const uint64_t* __restrict__ items)
{
    __shared__ uint64_t skey[4][W_MAX + 1];
    __shared__ uint32_t sval[4][W_MAX];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    // static assignment: workgroup L works segment L mod 8 (the XCD it runs on);
    // its waves take 64-item chunks of that segment in turn
    // (chunks shrink when the segment has fewer than 64 items per wave, so a
    // small batch spreads over all waves instead of queueing on a few)
    const uint32_t xs8 = blockIdx.x & 7u, wseg = (gridDim.x >> 3) * 4u, w_in = (blockIdx.x >> 3) * 4u + wid;
    const uint32_t seg0 = c.qseg[xs8], seg1 = c.qseg[xs8 + 1];
    const uint32_t per_w = (seg1 - seg0 + wseg - 1) / wseg;
    const uint32_t ch = per_w >= 64u ? 64u : (per_w ? per_w : 1u);
    for (uint32_t cb = seg0 + w_in * ch; cb < seg1; cb += wseg * ch) {
        const uint32_t cnt = seg1 - cb < ch ? seg1 - cb : ch;
        const uint64_t myitem = lane < cnt ? items[cb + lane] : 0ull;
        const uint32_t msz = lane < cnt ? it_size(myitem) : 0u;
        for (uint32_t done = 0; done < cnt;) {
            // the groups done.. whose sizes sum to <= 64 (the first always fits)
            const uint32_t sz = (lane >= done && lane < cnt) ? msz : 0u;
            const uint32_t incl = wave_incl_scan_add(sz);
            const bool take = lane >= done && lane < cnt && incl <= 64u;
            const uint32_t ng = (uint32_t)__popcll(__ballot(take));
            const uint32_t off = incl - sz;
            const uint32_t total = (uint32_t)__shfl((int)incl, (int)(done + ng - 1), 64);
            const uint64_t smask = wave_reduce_or64(take ? (1ull << off) : 0ull);
            const bool valid = lane < total;
            const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
            const uint32_t gi = valid ? done + (uint32_t)__popcll(smask & upto) - 1u : done;
            const uint64_t item = shfl64(myitem, gi);
            const uint32_t goff = (uint32_t)__shfl((int)off, (int)gi, 64);   // every lane: gi may be past `total`
            const uint32_t gstart = valid ? goff : 0u;
            const uint32_t slot = it_slot(item), s = it_start(item), m = it_size(item), par = it_par(item);
            const uint32_t j = valid ? lane - gstart : 0u;
            const uint32_t* sv = (par ? c.scr.V : c.scr.SA) + (uint64_t)slot * c.scr.stride + s;
            const KeySrc ks = key_src(c, slot, par);
            const uint32_t v = sv[j];
            uint32_t ls;
            uint64_t k = elem_key<DBL>(c, ks, slot, s + j, v, ls);
            if (!valid) k = ~0ull;
            // rank among the group's members (lanes gstart .. gstart + m - 1):
            // scalar broadcasts when the pass holds one group, lane shuffles otherwise
            uint32_t r = 0;
            if (ng == 1) {
                for (uint32_t q = 0; q < total; ++q) {
                    const uint64_t kq = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(k >> 32), (int)q) << 32) |
                                        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)k, (int)q);
                    r += (kq < k || (kq == k && q < j)) ? 1u : 0u;
                }
            } else {
                const uint32_t maxm = wave_reduce_max(valid ? m : 0u);
                for (uint32_t q = 0; q < maxm; ++q) {
                    const bool in = valid && q < m;
                    const uint64_t kq = shfl64(k, in ? gstart + q : lane);
                    r += (in && (kq < k || (kq == k && q < j))) ? 1u : 0u;
                }
            }
            wave_sync_lds3();                            // the previous pass's reads are done
            if (valid) { skey[wid][gstart + r] = k; sval[wid][gstart + r] = v | (ls << 24); }
            wave_sync_lds3();
            const uint64_t key = valid ? skey[wid][lane] : 0;
            const uint32_t val = valid ? sval[wid][lane] : 0;
            const bool head = valid && (j == 0 || skey[wid][lane - 1] != key);
            const bool end = valid && (j + 1 == m || skey[wid][lane + 1] != key);
            const uint32_t hp = wave_incl_scan_max<uint32_t>(head ? lane : 0u) - gstart;   // a group start is a head
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // SA reads done before the writes
            uint32_t runs = 0;
            emit_sorted(c, slot, s, j, val & 0xFFFFFFu, valid, hp, end, runs, val >> 24);
            if (c.mode) {                                // runs per group, by its first lane
                const uint64_t em = __ballot(end);
                const uint64_t gm = (m >= 64 ? ~0ull : ((1ull << m) - 1ull)) << gstart;
                wave_add_slot(c.L.runs, valid && j == 0, slot, (uint32_t)__popcll(em & gm));
            }
            done += ng;
        }
    }
}

// ---------------------------------------------------------------------------
// k3_sort_lds<NW, E>: groups of <= NW*64*E rotations sorted by NW waves
// (NW = 1: four independent wave-private sorts per workgroup, no workgroup
// barrier; NW = 4: one group per workgroup).  Persistent over a binned list.
// Every group's keys share at least their top 12 bits (the bucket digit, the
// partition digits, or unused high bits); dropping them leaves room for the
// group-local index below the key: (key << IDXB) | index is unique and
// ordered like the key, so each exchange moves one u64 per element through
// LDS and ranking is one 64-bit compare per pair.
// Primary path: one MSD digit (the DB bits below the highest varying bit),
// then every element ranks itself inside its sub-bucket by comparison; a
// second digit for sub-buckets above LIMIT.  Otherwise: stable LSD radix over
// the varying 8-bit digits (8 ballots find a lane's digit peers; one lane per
// peer set adds the set's size to the wave's counter with a returning LDS
// atomic).
// ---------------------------------------------------------------------------
// rank of key kj among positions [rs, re) of xk.  Keys are (key << IDXB) |
// group index: unique, so one 64-bit compare orders them (ties of the key
// broken by index)
__device__ __forceinline__ uint32_t rank_in(const uint64_t* xk, uint32_t rs, uint32_t re, uint64_t kj)
{
    uint32_t r = 0;
    uint32_t q = rs;
    if constexpr (STARCH_RANK_UNROLL >= 8) {
        for (; q + 8 <= re; q += 8) {
            uint64_t x[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = xk[q + i];
#pragma unroll
            for (int i = 0; i < 8; ++i) r += x[i] < kj ? 1u : 0u;
        }
    }
    if constexpr (STARCH_RANK_UNROLL != 0) {
        for (; q + 4 <= re; q += 4) {
            const uint64_t a = xk[q], b = xk[q + 1], c2 = xk[q + 2], d = xk[q + 3];
            r += (a < kj ? 1u : 0u) + (b < kj ? 1u : 0u) + (c2 < kj ? 1u : 0u) + (d < kj ? 1u : 0u);
        }
    }
    for (; q < re; ++q) r += xk[q] < kj ? 1u : 0u;
    return r;
}

template <int NW>
__device__ __forceinline__ void gsync()
{
    if constexpr (NW == 1) wave_sync_lds3();
    else __syncthreads();
}

template <int E>
struct GrpIn {                 // one group's inputs, as loaded
    uint64_t item;
    KeySrc ks;
    uint32_t v[E];
    uint32_t v0;
    uint64_t kx[E];            // keys (PSS rounds: the first raw key word until grp_finish_keys)
    uint32_t ls[E];            // last-column symbols (PSS rounds: the first raw 32-bit window word)
    uint64_t k0;
    uint64_t kb[E];            // PSS rounds: the second raw key word
    uint32_t lb[E];            // ... and the second raw window word of the last-column symbol
    uint64_t k0b;
    bool one;                  // PSS round 0, B in {1,2,4,5,6,8}: kx/kb = ONE 16-B load holding the symbol and the key
};

// loads of a group that does not exist (ok false) go to element 0 of slot 0's
// SA, which always exists; their results are never used
template <int NW, int E>
__device__ __forceinline__ void grp_load_vals(const Ctx& c, GrpIn<E>& x, bool ok, int wid, int lane)
{
    if (!ok) x.item = mk_item(0, 0, 1, 0, 0);
    const uint32_t slot = it_slot(x.item), s = it_start(x.item), m = it_size(x.item), par = it_par(x.item);
    const uint32_t* sv = (par ? c.scr.V : c.scr.SA) + (uint64_t)slot * c.scr.stride + s;
    x.ks = key_src(c, slot, par);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t i = (uint32_t)(wid * 64 * E + e * 64 + lane);
        x.v[e] = sv[i < m ? i : 0u];
    }
    x.v0 = sv[0];
}

// PSS rounds: the key of rotation r is stream bits [(r + off) * B, + kbits) and its
// last-column symbol bits [(r - 1) * B, + B) (mod n).  grp_load_keys only issues
// the loads (two u64 words for the key, two 32-bit words for the symbol, in the
// stream's MSB-first order: the 32-bit word j of the stream sits at u32 index
// j ^ 1 of the little-endian u64 words); grp_finish_keys combines them one group
// later, so the random PSS reads overlap the current group's sort instead of
// being waited on where they are issued.
__device__ __forceinline__ uint32_t pss_rr(const KeySrc& ks, uint32_t r)
{
    const uint32_t rr = r + ks.off;
    return rr >= ks.n ? rr - ks.n : rr;
}
__device__ __forceinline__ uint32_t pss_pr(const KeySrc& ks, uint32_t r) { return r ? r - 1u : ks.n - 1u; }

// deferred key combination: the one-wave sorts of the PSS rounds only (measured best)
template <int NW, bool DBL>
constexpr bool defer_keys() { return !DBL && NW == 1; }

template <int NW, int E, bool DBL>
__device__ __forceinline__ void grp_load_keys(const Ctx& c, GrpIn<E>& x, int wid, int lane)
{
    const uint32_t s = it_start(x.item), m = it_size(x.item), slot = it_slot(x.item);
    if constexpr (!defer_keys<NW, DBL>()) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t i = (uint32_t)(wid * 64 * E + e * 64 + lane);
            x.kx[e] = elem_key<DBL>(c, x.ks, slot, s + (i < m ? i : 0u), x.v[e], x.ls[e]);
        }
        x.k0 = elem_key<DBL>(x.ks, s, x.v0);
    } else {
        const uint64_t* __restrict__ w = x.ks.pss;
        const uint32_t* __restrict__ w32 = reinterpret_cast<const uint32_t*>(w);
        const uint32_t B = x.ks.B;
        // round 0: the last-column symbol's B bits sit right before the key's KB
        // bits, and for these B the B + KB bits after the symbol's bit offset
        // within its word (a multiple of B <= 64 - B ... 63) never pass the
        // next word: one 16-byte load per element instead of four
        x.one = x.ks.off == 0 && (B == 1 || B == 2 || B == 4 || B == 5 || B == 6 || B == 8);
        if (x.one) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint32_t r = x.v[e];
                const uint64_t q = ((uint64_t)(r ? r - 1u : 0u) * B) >> 6;
                const uint4 kv = *reinterpret_cast<const uint4*>(w + q);
                x.kx[e] = ((uint64_t)kv.y << 32) | kv.x;
                x.kb[e] = ((uint64_t)kv.w << 32) | kv.z;
                if (r == 0) {                      // rotation 0: its symbol is the block's last
                    const uint64_t j = ((uint64_t)(x.ks.n - 1u) * B) >> 5;
                    x.ls[e] = w32[j ^ 1u];
                    x.lb[e] = w32[(j + 1u) ^ 1u];
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint64_t q = ((uint64_t)pss_rr(x.ks, x.v[e]) * B) >> 6;
                x.kx[e] = w[q];
                x.kb[e] = w[q + 1];
                const uint64_t j = ((uint64_t)pss_pr(x.ks, x.v[e]) * B) >> 5;
                x.ls[e] = w32[j ^ 1u];
                x.lb[e] = w32[(j + 1u) ^ 1u];
            }
        }
        const uint64_t q0 = ((uint64_t)pss_rr(x.ks, x.v0) * x.ks.B) >> 6;
        x.k0 = w[q0];
        x.k0b = w[q0 + 1];
    }
}

template <int NW, int E, bool DBL>
__device__ __forceinline__ void grp_finish_keys(GrpIn<E>& x)
{
    if constexpr (defer_keys<NW, DBL>()) {
        const KeySrc& ks = x.ks;
        if (x.one) {
            const uint32_t B = ks.B;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint32_t r = x.v[e];
                const uint64_t A = x.kx[e], W = x.kb[e];
                if (r) {
                    const uint32_t p0 = (uint32_t)(((uint64_t)(r - 1u) * B) & 63u), pk = p0 + B;
                    x.ls[e] = (uint32_t)(((A << p0) | ((W >> 1) >> (63u - p0))) >> (64u - B));
                    const uint64_t win = pk >= 64u ? (W << (pk - 64u)) : ((A << pk) | ((W >> 1) >> (63u - pk)));
                    x.kx[e] = win >> (64u - ks.kbits);
                } else {
                    x.kx[e] = A >> (64u - ks.kbits);
                    const uint32_t pl = (uint32_t)(((uint64_t)(ks.n - 1u) * B) & 31u);
                    const uint64_t lw = ((uint64_t)x.ls[e] << 32) | x.lb[e];
                    x.ls[e] = (uint32_t)((lw << pl) >> (64u - B));
                }
            }
        } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t p = (uint32_t)(((uint64_t)pss_rr(ks, x.v[e]) * ks.B) & 63u);
            const uint64_t v = (x.kx[e] << p) | ((x.kb[e] >> 1) >> (63u - p));
            x.kx[e] = v >> (64u - ks.kbits);
            const uint32_t pl = (uint32_t)(((uint64_t)pss_pr(ks, x.v[e]) * ks.B) & 31u);
            const uint64_t lw = ((uint64_t)x.ls[e] << 32) | x.lb[e];
            x.ls[e] = (uint32_t)((lw << pl) >> (64u - ks.B));
        }
        }
        const uint32_t p0 = (uint32_t)(((uint64_t)pss_rr(ks, x.v0) * ks.B) & 63u);
        const uint64_t v0 = (x.k0 << p0) | ((x.k0b >> 1) >> (63u - p0));
        x.k0 = v0 >> (64u - ks.kbits);
    }
}

// register budget (waves per SIMD) of the sort kernels: keeps a few groups
// resident per CU while their loads are in flight.  The instantiations are
// <4, 4> M1, <4, 2> M0, <1, 2> S, <1, 4> S2, and <8, 4> M2 / <16, 4> M3 (whole
// workgroups of 8 / 16 waves: no budget to set)
constexpr int sort_wpe(int NW, int E)
{
    return NW >= 8   ? 1
           : NW == 4 ? (E == 4 ? STARCH_WPE_M1 : STARCH_WPE_M0)
                     : (E == 2 ? STARCH_WPE_S : STARCH_WPE_GRP);
}

template <int NW, int E, bool DBL>
__global__ void __launch_bounds__(NW > 4 ? 64 * NW : 256) __attribute__((amdgpu_waves_per_eu(sort_wpe(NW, E))))
k3_sort_lds(Ctx c, const uint64_t* __restrict__ items,
                                                    const uint32_t* __restrict__ hard_n)
{
    constexpr int IPW = NW >= 4 ? 1 : 4 / NW;      // groups per workgroup
    constexpr int NWV = IPW * NW;                  // waves per workgroup
    constexpr int CAP = NW * 64 * E;
    constexpr int IDXB = CAP <= 256 ? 8 : 12;      // packed local index bits
    constexpr int KEYB = 64 - IDXB;
    constexpr uint64_t KMASK = (1ull << KEYB) - 1ull;
    constexpr int DPT = NW >= 4 ? 1 : 256 / (64 * NW);   // digits per thread in the offset scan (NW > 4: threads 0..255)
    static_assert(CAP <= (1 << IDXB), "index does not fit");
    constexpr int DB = CAP <= 128 ? 7 : (CAP <= 256 ? 8 : (CAP <= 1024 ? 10 : (CAP == 2048 ? STARCH_M2_DB : 11)));   // MSD digit bits
    constexpr int NBIN = 1 << DB;
    constexpr int T = NW * 64;
    constexpr int BPT = NBIN / T;                  // bins per thread
    constexpr uint32_t LIMIT = STARCH_LIM_NUM / E; // largest sub-bucket ranked by comparison
    __shared__ uint64_t xk_all[IPW][CAP];
    __shared__ uint32_t vb_all[IPW][CAP];          // rotations by group index
    // LDS is what caps residency here: sub-bucket starts as u16 (positions <=
    // CAP), and the scatter cursors share their words with the LSD path's
    // per-wave digit counters (the LSD path runs only after the MSD attempt)
    __shared__ uint16_t bst_all[IPW][NBIN + 2];   // sub-bucket starts
    constexpr int UR = NBIN > 256 * NW ? NBIN : 256 * NW;
    __shared__ uint32_t ur_all[IPW][UR];          // scatter cursors | LSD digit counters
    __shared__ uint32_t sc_all[IPW][NW + 1];
    constexpr int NB2 = NW == 1 ? 256 : 1024;      // second-digit bins
    constexpr uint32_t LIMIT2 = STARCH_LIM2_NUM / E;   // largest second-level sub-bucket ranked by comparison
    __shared__ uint32_t c2_all[IPW][NB2 + 1];
    __shared__ uint32_t sc2_all[IPW][NW + 1];
    __shared__ uint64_t red_all[NWV];
    __shared__ uint32_t wmax_all[NWV];
    __shared__ uint32_t flag_all[NWV];
    __shared__ uint32_t tc_all[NW + 1 > 5 ? NW + 1 : 5];
    uint32_t tacc = 0;                             // tied elements pushed (flushed at exit)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = wave / NW, wid = wave % NW, w0 = g * NW;
    uint64_t* xk = xk_all[g];
    uint32_t* wcnt = ur_all[g] + wid * 256;
    uint32_t* sc = sc_all[g];
    const uint64_t lt = lanemask_lt();
    // binned list: workgroup L walks the per-XCD segment L mod 8 with a fixed
    // stride (a workgroup per group for NW >= 4, a wave per group for NW = 1),
    // so an XCD's groups are worked in list order (neighbouring groups share
    // a block's PSS in its L2).
    // hard_n: an unbinned list of *hard_n groups, grid-strided.
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    const uint32_t nwk = gridDim.x * (uint32_t)IPW;
    const uint32_t e_end = hard_n ? *hard_n : 0u;
    uint32_t it_s = blockIdx.x * (uint32_t)IPW + (uint32_t)g;   // hard_n walk
    const uint32_t xs8 = blockIdx.x & 7u;                        // static: segment L mod 8
    const uint32_t s_end = hard_n ? e_end : c.qseg[xs8 + 1];
    const uint32_t s_nwk = hard_n ? nwk : (gridDim.x >> 3) * (uint32_t)IPW;
    if (!hard_n) it_s = c.qseg[xs8] + (blockIdx.x >> 3) * (uint32_t)IPW + (uint32_t)g;
    auto next_item = [&]() -> uint32_t {
        const uint32_t r = it_s < s_end ? it_s : NONE;
        it_s += s_nwk;
        return r;
    };
    // software pipeline (as k3_sort_grp): while a group sorts, the next
    // group's keys are in flight, and the rotations of the one after it
    uint32_t it = next_item();
    uint32_t it1 = it != NONE ? next_item() : NONE;
    GrpIn<E> cur, nxt;
    cur.item = it != NONE ? items[it] : 0ull;
    grp_load_vals<NW, E>(c, cur, it != NONE, wid, lane);
    grp_load_keys<NW, E, DBL>(c, cur, wid, lane);
    nxt.item = it1 != NONE ? items[it1] : 0ull;
    grp_load_vals<NW, E>(c, nxt, it1 != NONE, wid, lane);
    while (it != NONE) {
        const uint64_t item = cur.item;
        const uint32_t slot = it_slot(item), s = it_start(item), m = it_size(item);
        grp_finish_keys<NW, E, DBL>(cur);
        gsync<NW>();                                   // the previous group's LDS reads are done

        uint64_t k[E];
        uint64_t diff = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t i = (uint32_t)(wid * 64 * E + e * 64 + lane);
            if (i < m) {
                diff |= cur.kx[e] ^ cur.k0;
                k[e] = ((cur.kx[e] & KMASK) << IDXB) | i;
                vb_all[g][i] = cur.v[e] | (cur.ls[e] << 24);
            } else {
                k[e] = ~0ull;                              // pads: max key, last in stable order
            }
        }
        grp_load_keys<NW, E, DBL>(c, nxt, wid, lane);     // next group's keys (its rotations: one group ago)
        diff = wave_reduce_or64(diff);
        if constexpr (NW > 1) {
            if (lane == 0) red_all[wave] = diff;
            __syncthreads();
            diff = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) diff |= red_all[w0 + w];
        }
        if ((diff >> KEYB) && tid % (64 * NW) == 0) atomicOr(&c.L.ctr[C_ERR], 1u);   // top bits not shared

        bool moved = false;
        const uint64_t kdiff = diff & KMASK;
        if (kdiff) {
            uint16_t* bst = bst_all[g];
            uint32_t* bcur = ur_all[g];
            const int tg = wid * 64 + lane;
            const int hb = 63 - __clzll((long long)kdiff);
            const int lo = hb + 1 - DB > 0 ? hb + 1 - DB : 0;
            for (int q = tg; q < NBIN; q += T) bcur[q] = 0;
            gsync<NW>();
            uint32_t dg[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                dg[e] = (uint32_t)((k[e] >> (lo + IDXB)) & (uint64_t)(NBIN - 1));
                if ((uint32_t)(wid * 64 * E + e * 64 + lane) < m) atomicAdd(&bcur[dg[e]], 1u);
            }
            gsync<NW>();
            uint32_t loc[BPT], sum = 0, mx = 0;
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                loc[q] = bcur[tg * BPT + q];
                sum += loc[q];
                mx = loc[q] > mx ? loc[q] : mx;
            }
            const uint32_t incl = wave_incl_scan_add(sum);
            uint32_t run = incl - sum;
            mx = wave_reduce_max(mx);
            if constexpr (NW > 1) {
                if (lane == 63) sc[wid] = incl;
                if (lane == 0) wmax_all[wave] = mx;
                __syncthreads();
                for (int w = 0; w < wid; ++w) run += sc[w];
                mx = 0;
                for (int w = 0; w < NW; ++w) mx = wmax_all[w0 + w] > mx ? wmax_all[w0 + w] : mx;
            }
            // rank every element inside its final sub-bucket [rs, re) by comparison
            // (p = its scatter position: the tie-break), then move keys into place
            // rank in digit order: position j holds kj, whose final sub-bucket
            // [rs, re) range_of() recomputes from the key (lanes of a row mostly
            // share a sub-bucket: equal trip counts, broadcast LDS reads); then
            // move keys into place
            auto rank_place = [&](auto&& range_of) {
                uint32_t p[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const uint32_t j = (uint32_t)(wid * 64 * E + e * 64 + lane);
                    p[e] = j;                          // pads keep the tail
                    if (j < m) {
                        const uint64_t kj = xk[j];
                        uint32_t rs, re;
                        range_of(kj, rs, re);
                        p[e] = rs + rank_in(xk, rs, re, kj);
                        k[e] = kj;
                    }
                }
                gsync<NW>();
#pragma unroll
                for (int e = 0; e < E; ++e) xk[p[e]] = k[e];
                gsync<NW>();
#pragma unroll
                for (int e = 0; e < E; ++e) k[e] = xk[wid * 64 * E + e * 64 + lane];
            };
            if (mx <= LIMIT) {                         // uniform per group
#pragma unroll
                for (int q = 0; q < BPT; ++q) { bst[tg * BPT + q] = run; bcur[tg * BPT + q] = run; run += loc[q]; }
                if (tg == T - 1) bst[NBIN] = run;
                gsync<NW>();
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if ((uint32_t)(wid * 64 * E + e * 64 + lane) < m) xk[atomicAdd(&bcur[dg[e]], 1u)] = k[e];
                gsync<NW>();
                rank_place([&](uint64_t kj, uint32_t& rs, uint32_t& re) {
                    const uint32_t d = (uint32_t)((kj >> (lo + IDXB)) & (uint64_t)(NBIN - 1));
                    rs = bst[d];
                    re = bst[d + 1];
                });
                moved = true;
            } else if (lo > 0) {
                // Second MSD digit for the sub-buckets larger than LIMIT: the w2 bits
                // right below the first digit, counted per (big sub-bucket, digit)
                // bin; bins are numbered in key order, so one exclusive scan places
                // them all.  Sub-buckets <= LIMIT keep their first-digit place.
                uint32_t* c2 = c2_all[g];
                uint32_t* sc2 = sc2_all[g];
                uint32_t nbl = 0;
#pragma unroll
                for (int q = 0; q < BPT; ++q) nbl += loc[q] > LIMIT ? 1u : 0u;
                const uint32_t binc = wave_incl_scan_add(nbl);
                uint32_t bb = binc - nbl, nbig = 0;
                if constexpr (NW > 1) {
                    if (lane == 63) sc2[wid] = binc;
                    __syncthreads();
                    for (int w = 0; w < NW; ++w) { if (w < wid) bb += sc2[w]; nbig += sc2[w]; }
                } else {
                    nbig = (uint32_t)__builtin_amdgcn_readlane((int)binc, 63);
                }
                uint32_t w2 = 0;
                while (w2 < STARCH_W2_MAX && (nbig << (w2 + 1)) <= (uint32_t)NB2) ++w2;
                if (w2 > (uint32_t)lo) w2 = (uint32_t)lo;
                const int lo2 = lo - (int)w2;
                const uint32_t nb2 = nbig << w2;
#pragma unroll
                for (int q = 0; q < BPT; ++q) {
                    bst[tg * BPT + q] = run;
                    bcur[tg * BPT + q] = loc[q] > LIMIT ? (0x80000000u | ((bb++) << w2)) : run;
                    run += loc[q];
                }
                if (tg == T - 1) bst[NBIN] = run;
                for (uint32_t q = (uint32_t)tg; q < nb2; q += T) c2[q] = 0;
                gsync<NW>();
                uint32_t b2[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    b2[e] = ~0u;
                    if ((uint32_t)(wid * 64 * E + e * 64 + lane) < m) {
                        const uint32_t x = bcur[dg[e]];
                        if (x >> 31) {
                            b2[e] = (x & 0x7FFFFFFFu) + (uint32_t)((k[e] >> (lo2 + IDXB)) & ((1ull << w2) - 1ull));
                            atomicAdd(&c2[b2[e]], 1u);
                        }
                    }
                }
                gsync<NW>();
                constexpr int BPT2 = (NB2 + T - 1) / T;
                uint32_t l2[BPT2], s2 = 0, m2 = 0;
#pragma unroll
                for (int q = 0; q < BPT2; ++q) {
                    const uint32_t ix = (uint32_t)(tg * BPT2 + q);
                    l2[q] = ix < nb2 ? c2[ix] : 0u;
                    s2 += l2[q];
                    m2 = l2[q] > m2 ? l2[q] : m2;
                }
                const uint32_t inc2 = wave_incl_scan_add(s2);
                uint32_t r2 = inc2 - s2;
                m2 = wave_reduce_max(m2);
                if constexpr (NW > 1) {
                    __syncthreads();                   // sc2 reads (nbig) done
                    if (lane == 63) sc2[wid] = inc2;
                    if (lane == 0) wmax_all[wave] = m2;
                    __syncthreads();
                    for (int w = 0; w < wid; ++w) r2 += sc2[w];
                    for (int w = 0; w < NW; ++w) m2 = wmax_all[w0 + w] > m2 ? wmax_all[w0 + w] : m2;
                }
#pragma unroll
                for (int q = 0; q < BPT2; ++q) {
                    const uint32_t ix = (uint32_t)(tg * BPT2 + q);
                    if (ix < nb2) c2[ix] = r2;
                    r2 += l2[q];
                }
                gsync<NW>();
                if (m2 <= LIMIT2) {                    // uniform per group
                    // c2 = bin starts among the big sub-buckets' elements; an
                    // element's place: its sub-bucket's start + (bin cursor - the
                    // start of the sub-bucket's first bin)
                    uint32_t sb[E];
#pragma unroll
                    for (int e = 0; e < E; ++e) sb[e] = b2[e] != ~0u ? c2[bcur[dg[e]] & 0x7FFFFFFFu] : 0u;
                    gsync<NW>();
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        if ((uint32_t)(wid * 64 * E + e * 64 + lane) < m) {
                            const uint32_t p = b2[e] != ~0u ? bst[dg[e]] + atomicAdd(&c2[b2[e]], 1u) - sb[e]
                                                            : atomicAdd(&bcur[dg[e]], 1u);
                            xk[p] = k[e];
                        }
                    }
                    gsync<NW>();
                    // after the scatter c2[b] = end of bin b = start of bin b + 1;
                    // big sub-buckets still carry their tag in bcur
                    rank_place([&](uint64_t kj, uint32_t& rs, uint32_t& re) {
                        const uint32_t d = (uint32_t)((kj >> (lo + IDXB)) & (uint64_t)(NBIN - 1));
                        const uint32_t x = bcur[d];
                        if (x >> 31) {
                            const uint32_t base = x & 0x7FFFFFFFu;
                            const uint32_t b = base + (uint32_t)((kj >> (lo2 + IDXB)) & ((1ull << w2) - 1ull));
                            const uint32_t s0 = base ? c2[base - 1] : 0u;
                            rs = bst[d] + (b ? c2[b - 1] : 0u) - s0;
                            re = bst[d] + c2[b] - s0;
                        } else {
                            rs = bst[d];
                            re = bst[d + 1];
                        }
                    });
                    moved = true;
                }
            } else {
                gsync<NW>();                           // bcur/sc reads done before the LSD passes
            }
        }
        bool lsd_moved = false;
        for (int dbit = 0; dbit < KEYB && !moved; dbit += 8) {
            if ((kdiff >> dbit & 0xffull) == 0) continue;    // uniform per group
            for (int q = lane; q < 256; q += 64) wcnt[q] = 0;
            wave_sync_lds3();
            uint32_t dg[E], rk[E], ld[E], ret[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint32_t d = (uint32_t)((k[e] >> (dbit + IDXB)) & 255u);
                uint64_t peers = ~0ull;
#pragma unroll
                for (int bb = 0; bb < 8; ++bb) {
                    const uint64_t bal = __ballot((d >> bb) & 1u);
                    peers &= ((d >> bb) & 1u) ? bal : ~bal;
                }
                const uint32_t leader = (uint32_t)__ffsll((unsigned long long)peers) - 1u;
                dg[e] = d;
                ld[e] = leader;
                rk[e] = (uint32_t)__popcll(peers & lt);
                ret[e] = 0;
                if ((uint32_t)lane == leader) ret[e] = atomicAdd(&wcnt[d], (uint32_t)__popcll(peers));
            }
#pragma unroll
            for (int e = 0; e < E; ++e) rk[e] += (uint32_t)__shfl((int)ret[e], (int)ld[e], 64);
            gsync<NW>();
            {   // digit offsets: base(d) + counts of earlier waves, in place
                const int t = wid * 64 + lane;
                const bool has = t * DPT < 256;
                uint32_t loc[DPT], sum = 0;
#pragma unroll
                for (int q = 0; q < DPT; ++q) {
                    uint32_t a = 0;
#pragma unroll
                    for (int w = 0; w < NW; ++w) a += has ? ur_all[g][w * 256 + t * DPT + q] : 0u;
                    loc[q] = a;
                    sum += a;
                }
                const uint32_t incl = wave_incl_scan_add(sum);
                uint32_t run = incl - sum;
                if constexpr (NW > 1) {
                    if (lane == 63) sc[wid] = incl;
                    __syncthreads();
                    for (int w = 0; w < wid; ++w) run += sc[w];
                }
#pragma unroll
                for (int q = 0; q < DPT && has; ++q) {
                    uint32_t r = run;
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        const uint32_t xx = ur_all[g][w * 256 + t * DPT + q];
                        ur_all[g][w * 256 + t * DPT + q] = r;
                        r += xx;
                    }
                    run += loc[q];
                }
            }
            gsync<NW>();
#pragma unroll
            for (int e = 0; e < E; ++e) xk[rk[e] + wcnt[dg[e]]] = k[e];
            gsync<NW>();
#pragma unroll
            for (int e = 0; e < E; ++e) k[e] = xk[wid * 64 * E + e * 64 + lane];
            lsd_moved = true;
        }
        moved |= lsd_moved;
        if (!moved) {
#pragma unroll
            for (int e = 0; e < E; ++e) xk[wid * 64 * E + e * 64 + lane] = k[e];
        }
        gsync<NW>();
        // runs of equal keys in sorted order j = wid*64*E + e*64 + lane
        bool tie_here = false;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t j = (uint32_t)(wid * 64 * E + e * 64 + lane);
            if (j > 0 && j < m && ((xk[j - 1] ^ k[e]) >> IDXB) == 0) tie_here = true;
        }
        bool ties = __ballot(tie_here) != 0;
        if constexpr (NW > 1) {
            if (lane == 0) flag_all[wave] = ties ? 1u : 0u;
            __syncthreads();
            ties = false;
            for (int w = 0; w < NW; ++w) ties |= flag_all[w0 + w] != 0;
        }
        uint32_t hp[E];
        if (!ties) {
#pragma unroll
            for (int e = 0; e < E; ++e) hp[e] = (uint32_t)(wid * 64 * E + e * 64 + lane);
        } else {
            uint32_t carry = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint32_t j = (uint32_t)(wid * 64 * E + e * 64 + lane);
                const bool head = j < m && (j == 0 || ((xk[j - 1] ^ k[e]) >> IDXB) != 0);
                uint32_t xx = wave_incl_scan_max<uint32_t>(head ? j : 0u);
                xx = xx > carry ? xx : carry;
                hp[e] = xx;
                carry = (uint32_t)__builtin_amdgcn_readlane((int)xx, 63);
            }
            if constexpr (NW > 1) {
                if (lane == 0) wmax_all[wave] = carry;
                __syncthreads();
                uint32_t pre = 0;
                for (int w = 0; w < wid; ++w) pre = wmax_all[w0 + w] > pre ? wmax_all[w0 + w] : pre;
#pragma unroll
                for (int e = 0; e < E; ++e) hp[e] = hp[e] > pre ? hp[e] : pre;
            }
        }
        // the group's rotations and keys were consumed into registers/LDS (their
        // loads complete) before any write of its SA range; the loads in flight
        // now belong to other groups' disjoint ranges
        uint32_t runs = 0, tcnt = 0;
        uint64_t tm[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t j = (uint32_t)(wid * 64 * E + e * 64 + lane);
            const bool valid = j < m;
            const uint32_t vb = valid ? vb_all[g][(uint32_t)(k[e] & ((1u << IDXB) - 1u))] : 0u;
            const bool end = valid && (!ties || j + 1 == m || ((xk[j + 1] ^ k[e]) >> IDXB) != 0);
            emit_vals(c, slot, s, j, vb & 0xFFFFFFu, valid, hp[e], vb >> 24);
            const bool tie = end && j > hp[e];
            tm[e] = __ballot(tie);
            tcnt += (uint32_t)__popcll(tm[e]);
            tacc += tie ? j - hp[e] + 1u : 0u;
            runs += (uint32_t)__popcll(__ballot(end));
        }
        if (c.mode && lane == 0 && runs) atomicAdd(&c.L.runs[slot], runs);
        if (ties) {                                    // uniform per group
            uint32_t tb = tie_reserve<NW>(c, tcnt, tc_all, wid, lane);
            uint64_t* tl = c.L.t[c.tsel];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint32_t j = (uint32_t)(wid * 64 * E + e * 64 + lane);
                if ((tm[e] >> lane) & 1ull) tl[tb + (uint32_t)__popcll(tm[e] & lt)] = mk_item(slot, s + hp[e], j - hp[e] + 1u, 0, 0);
                tb += (uint32_t)__popcll(tm[e]);
            }
        }
        // rotate the pipeline
        const uint32_t it2 = it1 != NONE ? next_item() : NONE;
        cur = nxt;
        nxt.item = it2 != NONE ? items[it2] : 0ull;
        grp_load_vals<NW, E>(c, nxt, it2 != NONE, wid, lane);
        it = it1;
        it1 = it2;
    }
    tacc = wave_reduce_add<uint32_t>(tacc);
    if (lane == 0 && tacc) atomicAdd(c.L.ctr + C_TS0 + c.tsel, tacc);
}

// ---------------------------------------------------------------------------
// k3_sort_grp<NW, E>: the common case of k3_sort_lds without its LSD path.
// One MSD digit (the DB bits below the highest varying key bit) scatters the
// group in LDS; then every element ranks itself inside its sub-bucket by
// comparison, working in digit order so the lanes of a wave mostly share a
// sub-bucket.  Ranking costs about sum(z^2) comparisons over the sub-bucket
// sizes z: a group whose digit spreads it badly (sum z^2 > HARD_Q * m) is
// left untouched and listed for k3_sort_lds.  While a group is sorted, the
// next group's rotations and keys are already being loaded (software
// pipeline: item two ahead, rotations and keys one ahead).
// ---------------------------------------------------------------------------
constexpr uint32_t HARD_Q = STARCH_HARD_Q;

template <int NW, int E, bool DBL>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sort_wpe(NW, E))))
k3_sort_grp(Ctx c, const uint64_t* __restrict__ items,
                                                    uint64_t* __restrict__ hard)
{
    constexpr int IPW = 4 / NW;                    // groups per workgroup
    constexpr int CAP = NW * 64 * E;
    constexpr int IDXB = CAP <= 256 ? 8 : 12;      // packed local index bits
    constexpr int KEYB = 64 - IDXB;
    constexpr uint64_t KMASK = (1ull << KEYB) - 1ull;
    static_assert(CAP <= (1 << IDXB), "index does not fit");
    constexpr int DB = CAP <= 128 ? 7 : (CAP <= 256 ? 8 : (CAP <= 1024 ? 10 : 11));   // MSD digit bits
    constexpr int NBIN = 1 << DB;
    constexpr int T = NW * 64;
    constexpr int BPT = NBIN / T;                  // bins per thread
    __shared__ uint64_t xk_all[IPW][CAP];
    __shared__ uint32_t vb_all[IPW][CAP];          // rotations by group index
    __shared__ uint32_t bst_all[IPW][NBIN + 1];    // sub-bucket starts
    __shared__ uint32_t bcur_all[IPW][NBIN];       // scatter cursors
    __shared__ uint32_t sc_all[IPW][NW + 1];
    __shared__ uint64_t red_all[4];
    __shared__ uint32_t wsq_all[4];
    __shared__ uint32_t wmax_all[4];
    __shared__ uint32_t flag_all[4];
    __shared__ uint32_t tc_all[5];
    uint32_t tacc = 0;                             // tied elements pushed (flushed at exit)
    const uint64_t lt = lanemask_lt();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = wave / NW, wid = wave % NW, w0 = g * NW;
    uint64_t* xk = xk_all[g];
    uint32_t* sc = sc_all[g];
    uint32_t* bst = bst_all[g];
    uint32_t* bcur = bcur_all[g];
    const int tg = wid * 64 + lane;
    // groups per queue pop, S (E = 2) and S2 (E = 4).  With the pop waited for where it
    // was issued, small chunks lost to the atomic's latency (8 / 16 / 32 / 64 / 128 for
    // both: cfg2 block sort 25.0, 20.5, 19.7, 20.0, 21.8 ms) and the code sat at 32 / 16.
    // With the pop prefetched (WaveQueue), one-lane cfg2, both macros at the same value,
    // per step: kernel ms and fetched bytes of k3_sort_grp<1,2> | <1,4>, and ms_bwt
    //   (waited, 32 / 16)   4.03 ms 4.65 GB | 1.88 ms  6.61 GB | 17.86
    //   32                  3.68 ms 5.35 GB | 2.15 ms 14.56 GB | 17.83
    //   16                  3.59 ms 2.36 GB | 1.68 ms  6.54 GB | 17.05
    //    8                  3.62 ms 2.19 GB | 1.57 ms  1.64 GB | 17.21
    //    4                  3.70 ms 2.14 GB | 1.57 ms  1.26 GB | 16.76
    // (profiles/r07_queue/).  The bytes fall to a third; the time follows only a little
    // way: with their keys in L2 these sorts wait on LDS and issue, not on HBM.
    // dynamic assignment (NW == 1): each wave pops groups, STARCH_GRP_CHUNK at a time,
    // from its XCD's queue, so the XCD's waves stay on neighbouring groups (one block's
    // PSS in its L2) however uneven the groups' costs; static striding drifted
    // apart by many blocks over a launch (a third of the key loads missed L2)
    static_assert(NW == 1, "k3_sort_grp: one wave per group");
    __shared__ uint32_t qs[8];
    const uint32_t xs = xcc_id();
    load_qsizes_binned(c, qs);
    WaveQueue<E == 4 ? STARCH_GRP_CHUNK_S2 : STARCH_GRP_CHUNK> wq;
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    // software pipeline, two groups deep: while group n sorts, the keys of
    // n + 1 are issued (its rotations were issued an iteration ago) and the
    // items of n + 2 and n + 3 are fetched
    uint32_t it = wq.next(c.qhead, qs, c.qseg, xs);
    uint32_t it1 = it != NONE ? wq.next(c.qhead, qs, c.qseg, xs) : NONE;
    uint32_t it2 = it1 != NONE ? wq.next(c.qhead, qs, c.qseg, xs) : NONE;
    GrpIn<E> cur, nxt;
    cur.item = it != NONE ? items[it] : 0ull;
    nxt.item = it1 != NONE ? items[it1] : 0ull;
    grp_load_vals<NW, E>(c, cur, it != NONE, wid, lane);
    grp_load_keys<NW, E, DBL>(c, cur, wid, lane);
    grp_load_vals<NW, E>(c, nxt, it1 != NONE, wid, lane);
    uint64_t nitem2 = it2 != NONE ? items[it2] : 0ull;
    while (it != NONE) {
        const uint64_t item = cur.item;
        const uint32_t slot = it_slot(item), s = it_start(item), m = it_size(item);
        grp_finish_keys<NW, E, DBL>(cur);
        gsync<NW>();                                   // the previous group's LDS reads are done

        uint64_t k[E];
        uint64_t diff = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t i = (uint32_t)(wid * 64 * E + e * 64 + lane);
            if (i < m) {
                diff |= cur.kx[e] ^ cur.k0;
                k[e] = ((cur.kx[e] & KMASK) << IDXB) | i;
                vb_all[g][i] = cur.v[e] | (cur.ls[e] << 24);
            } else {
                k[e] = ~0ull;                              // pads: max key, last in order
            }
        }
        // the next group's key gathers go out now, so they are in flight during
        // this group's LDS-only sort phases (issued after the sort, the emit's
        // returning atomics and the queue pops waited for them at once: every
        // vmcnt wait is in issue order).  The pop of the next chunk of groups goes
        // out ahead of them for the same reason; next() reads it chunks later
        wq.prefetch(c.qhead, xs);
        grp_load_keys<NW, E, DBL>(c, nxt, wid, lane);
        diff = wave_reduce_or64(diff);
        if constexpr (NW > 1) {
            if (lane == 0) red_all[wave] = diff;
            __syncthreads();
            diff = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) diff |= red_all[w0 + w];
        }
        if ((diff >> KEYB) && tg == 0) atomicOr(&c.L.ctr[C_ERR], 1u);   // top bits not shared

        bool is_hard = false;
        const uint64_t kdiff = diff & KMASK;
        if (kdiff) {
            const int hb = 63 - __clzll((long long)kdiff);
            const int lo = hb + 1 - DB > 0 ? hb + 1 - DB : 0;
            for (int q = tg; q < NBIN; q += T) bcur[q] = 0;
            gsync<NW>();
            uint32_t dg[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                dg[e] = (uint32_t)((k[e] >> (lo + IDXB)) & (uint64_t)(NBIN - 1));
                if ((uint32_t)(wid * 64 * E + e * 64 + lane) < m) atomicAdd(&bcur[dg[e]], 1u);
            }
            gsync<NW>();
            uint32_t loc[BPT], sum = 0, sq = 0;
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                loc[q] = bcur[tg * BPT + q];
                sum += loc[q];
                sq += loc[q] * loc[q];
            }
            const uint32_t incl = wave_incl_scan_add(sum);
            uint32_t run = incl - sum;
            sq = wave_reduce_add(sq);
            if constexpr (NW > 1) {
                if (lane == 63) sc[wid] = incl;
                if (lane == 0) wsq_all[wave] = sq;
                __syncthreads();
                for (int w = 0; w < wid; ++w) run += sc[w];
                sq = 0;
                for (int w = 0; w < NW; ++w) sq += wsq_all[w0 + w];
            }
            is_hard = sq > HARD_Q * m;                 // uniform per group
            if (!is_hard) {
#pragma unroll
                for (int q = 0; q < BPT; ++q) { bst[tg * BPT + q] = run; bcur[tg * BPT + q] = run; run += loc[q]; }
                if (tg == T - 1) bst[NBIN] = run;
                gsync<NW>();
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if ((uint32_t)(wid * 64 * E + e * 64 + lane) < m) xk[atomicAdd(&bcur[dg[e]], 1u)] = k[e];
                gsync<NW>();
                // rank in digit order: position j holds kj; its final place is
                // bs + #{q in its sub-bucket: kq < kj, or kq == kj and q < j}
                uint32_t pos[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const uint32_t j = (uint32_t)(wid * 64 * E + e * 64 + lane);
                    pos[e] = j;
                    if (j < m) {
                        const uint64_t kj = xk[j];
                        const uint32_t d = (uint32_t)((kj >> (lo + IDXB)) & (uint64_t)(NBIN - 1));
                        const uint32_t bs = bst[d], be = bst[d + 1];
                        pos[e] = bs + rank_in(xk, bs, be, kj);
                        k[e] = kj;
                    }
                }
                gsync<NW>();
#pragma unroll
                for (int e = 0; e < E; ++e) xk[pos[e]] = k[e];
            } else {
                gsync<NW>();                           // bcur/sc reads done
                if (tg == 0) hard[atomicAdd(&c.L.ctr[C_H], 1u)] = item;
            }
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) xk[wid * 64 * E + e * 64 + lane] = k[e];
        }
        const uint32_t it3 = it2 != NONE ? wq.next(c.qhead, qs, c.qseg, xs) : NONE;
        const uint64_t nitem3 = it3 != NONE ? items[it3] : 0ull;
        if (!is_hard) {
            gsync<NW>();
#pragma unroll
            for (int e = 0; e < E; ++e) k[e] = xk[wid * 64 * E + e * 64 + lane];
            // runs of equal keys in sorted order j = wid*64*E + e*64 + lane
            bool tie_here = false;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint32_t j = (uint32_t)(wid * 64 * E + e * 64 + lane);
                if (j > 0 && j < m && ((xk[j - 1] ^ k[e]) >> IDXB) == 0) tie_here = true;
            }
            bool ties = __ballot(tie_here) != 0;
            if constexpr (NW > 1) {
                if (lane == 0) flag_all[wave] = ties ? 1u : 0u;
                __syncthreads();
                ties = false;
                for (int w = 0; w < NW; ++w) ties |= flag_all[w0 + w] != 0;
            }
            uint32_t hp[E];
            if (!ties) {
#pragma unroll
                for (int e = 0; e < E; ++e) hp[e] = (uint32_t)(wid * 64 * E + e * 64 + lane);
            } else {
                uint32_t carry = 0;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const uint32_t j = (uint32_t)(wid * 64 * E + e * 64 + lane);
                    const bool head = j < m && (j == 0 || ((xk[j - 1] ^ k[e]) >> IDXB) != 0);
                    uint32_t xx = wave_incl_scan_max<uint32_t>(head ? j : 0u);
                    xx = xx > carry ? xx : carry;
                    hp[e] = xx;
                    carry = (uint32_t)__builtin_amdgcn_readlane((int)xx, 63);
                }
                if constexpr (NW > 1) {
                    if (lane == 0) wmax_all[wave] = carry;
                    __syncthreads();
                    uint32_t pre = 0;
                    for (int w = 0; w < wid; ++w) pre = wmax_all[w0 + w] > pre ? wmax_all[w0 + w] : pre;
#pragma unroll
                    for (int e = 0; e < E; ++e) hp[e] = hp[e] > pre ? hp[e] : pre;
                }
            }
            // the group's SA range was read (values consumed above) before any write
            uint32_t runs = 0, tcnt = 0;
            uint64_t tm[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint32_t j = (uint32_t)(wid * 64 * E + e * 64 + lane);
                const bool valid = j < m;
                const uint32_t vb = valid ? vb_all[g][(uint32_t)(k[e] & ((1u << IDXB) - 1u))] : 0u;
                const bool end = valid && (!ties || j + 1 == m || ((xk[j + 1] ^ k[e]) >> IDXB) != 0);
                emit_vals(c, slot, s, j, vb & 0xFFFFFFu, valid, hp[e], vb >> 24);
                const bool tie = end && j > hp[e];
                tm[e] = __ballot(tie);
                tcnt += (uint32_t)__popcll(tm[e]);
                tacc += tie ? j - hp[e] + 1u : 0u;
                runs += (uint32_t)__popcll(__ballot(end));
            }
            if (c.mode && lane == 0 && runs) atomicAdd(&c.L.runs[slot], runs);
            if (ties) {                                    // uniform per group
                uint32_t tb = tie_reserve<NW>(c, tcnt, tc_all, wid, lane);
                uint64_t* tl = c.L.t[c.tsel];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const uint32_t j = (uint32_t)(wid * 64 * E + e * 64 + lane);
                    if ((tm[e] >> lane) & 1ull) tl[tb + (uint32_t)__popcll(tm[e] & lt)] = mk_item(slot, s + hp[e], j - hp[e] + 1u, 0, 0);
                    tb += (uint32_t)__popcll(tm[e]);
                }
            }
        }
        // rotate the pipeline
        cur = nxt;
        nxt.item = nitem2;
        nitem2 = nitem3;
        grp_load_vals<NW, E>(c, nxt, it2 != NONE, wid, lane);
        it = it1;
        it1 = it2;
        it2 = it3;
    }
    tacc = wave_reduce_add<uint32_t>(tacc);
    if (lane == 0 && tacc) atomicAdd(c.L.ctr + C_TS0 + c.tsel, tacc);
}

// grids: a multiple of 8 (static per-XCD segments).  Static assignment needs
// every workgroup resident at once: one wave of workgroups, sized by the
// kernel's occupancy
dim3 resident(const void* f, int threads, int ncu)
{
    int per_cu = 0;
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, threads, 0));
    return dim3(((uint32_t)ncu * (uint32_t)(per_cu > 0 ? per_cu : 1) + 7) / 8 * 8);
}

// One class: NW waves per group, E rotations per lane.  M classes:
// k3_sort_lds (MSD digit(s) + compare, LSD fallback).  S classes (NW == 1):
// k3_sort_grp, then the groups it listed as hard (k3_sort_lds) from the class
// list it consumed.  The grids are sized once per process and instantiation.
template <int NW, int E, bool D>
void run_class(const Ctx& c, const uint64_t* binned, uint64_t* list, int ncu, hipStream_t st)
{
    if constexpr (NW == 1) {
        static const dim3 g = resident(reinterpret_cast<const void*>(&k3_sort_grp<NW, E, D>), 256, ncu);
        launch_zero(c.L.ctr, 1ull << C_H, st);
        hipLaunchKernelGGL((k3_sort_grp<NW, E, D>), g, dim3(256), 0, st, c, binned, list);
        hipLaunchKernelGGL((k3_sort_lds<NW, E, D>), dim3(ncu / 2), dim3(256), 0, st, c, list, c.L.ctr + C_H);
    } else {
        constexpr int T = NW > 4 ? 64 * NW : 256;
        static const dim3 g = resident(reinterpret_cast<const void*>(&k3_sort_lds<NW, E, D>), T, ncu);
        hipLaunchKernelGGL((k3_sort_lds<NW, E, D>), g, dim3(T), 0, st, c, binned, nullptr);
    }
}

template <bool D>
void run_w(const Ctx& c, const uint64_t* binned, int ncu, hipStream_t st)
{
    static const dim3 g = resident(reinterpret_cast<const void*>(&k3_sort_w<D>), 256, ncu);
    hipLaunchKernelGGL(k3_sort_w<D>, g, dim3(256), 0, st, c, binned);
}

}  // namespace

void launch_leaf(const Ctx& c, LeafClass k, const uint64_t* binned, uint64_t* list, int ncu, hipStream_t st)
{
    dbl(c.keysrc, [&](auto d) {
        constexpr bool D = decltype(d)::value;
        switch (k) {
        // M2 / M3: 8 / 16 waves of 4 rotations per lane (the 4-wave, 8 / 16
        // per lane forms held 168 / 294 VGPRs: 3 / 1 waves per SIMD)
        case LEAF_M3: run_class<16, 4, D>(c, binned, list, ncu, st); break;
        case LEAF_M2: run_class<8, 4, D>(c, binned, list, ncu, st); break;
        case LEAF_M1: run_class<4, 4, D>(c, binned, list, ncu, st); break;
        case LEAF_M0: run_class<4, 2, D>(c, binned, list, ncu, st); break;
        case LEAF_S2: run_class<1, 4, D>(c, binned, list, ncu, st); break;
        case LEAF_S: run_class<1, 2, D>(c, binned, list, ncu, st); break;
        case LEAF_W: run_w<D>(c, binned, ncu, st); break;
        }
    });
}

}  // namespace bwt3
}  // namespace bz
