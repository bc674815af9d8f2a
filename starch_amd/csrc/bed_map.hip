// starch_amd/csrc/bed_map.hip -- bedmap on MI355X: for every line of a sorted
// reference, the number of lines of a sorted map that overlap it, the bases
// they cover, and the bases they cover counting each once.
//
// Both inputs lie back to back in one buffer; the reference is input 0.  Stages:
//   1. bed_setops.hip's stage_lines over the whole buffer: framing, parse,
//      chromosome ranks (global, so a reference line and a map line of one
//      chromosome carry one rank), stop > start and the per-input order.
//   2. map arrays.  A: the map starts, in (rank, start) order as they stand.
//      B: the map stops in (rank, stop) order -- the stops as they stand when
//      no map line is nested in another (the sort's order check finds no
//      descent), else through the sort's radix stage.  PA, PB: exclusive sums
//      of A and B (modulo 2^64).  Rank r's lines are [mlo[r], mlo[r + 1]) in
//      both.  For BASES_UNIQ the map is merged with itself by bed_setops.hip's
//      stage_merge into disjoint runs MS, ME with PL, the exclusive sum of
//      their lengths, and run bounds rlo per rank.
//   3. k_bm_query, one thread per reference line.  With the window
//      [s', e') = [max(0, start - range), stop + range) and
//      D(x) = sum over a < x of (x - a) - sum over b <= x of (x - b),
//      the map bases below x counted per line:
//        COUNT = #{a < e'} - #{b <= s'}   (b <= s' implies a < e')
//        BASES = D(e') - D(s')            from the four counts, PA and PB
//        BASES_UNIQ = U(e') - U(s'),      U(x) = PL[k - 1] + min(ME[k - 1], x) - MS[k - 1], k = #{MS < x}
//      A workgroup's 256 lines are cut into chromosome segments.  In a segment
//      s' does not decrease, so every answer lies between the count for the
//      segment's first s' and the count for its largest e' (a running maximum:
//      e' is not monotone).  The segment's last thread finds that window with
//      searches over the whole chromosome and leaves it in LDS; every thread
//      then searches inside the window alone.  When the tile is one segment
//      of 256 lines and its windows into A and B hold at most kLdsWindow
//      elements each, they are copied to LDS first and searched there
//      (measured: DESIGN.md section 12); the runs of BASES_UNIQ are always
//      searched in HBM.
//   4. format: k_bm_len, an exclusive sum, k_bm_write (the writer and its wave
//      copy: bed_text.hpp; the host steps between the two kernels: format_tail
//      in common.hpp; both shared with every BED command).
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/starch_amd.h"
#include "bed_map.hpp"
#include "bed_search.hpp"
#include "bed_text.hpp"
#include "seg_max.hpp"

namespace bm {
namespace {

constexpr int kThreads = kBoundsThreads;
enum : int { S_BYTES = 0, S_KEPT, S_COUNT = 4 };   // device scalars (u64)
enum : uint32_t { W_COUNT = 1, W_BASES = 2, W_UNIQ = 4 };

using bt::dec_digits;
using bt::line_beg;

// ---- 2. map arrays ------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
k_bm_gather(const uint32_t* __restrict__ idx, const uint64_t* __restrict__ v, uint64_t n, uint64_t* __restrict__ out)
{
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j < n) out[j] = v[idx[j]];
}

// run r of map line i: pos[i] + open[i] - 1; its opener has its rank and start, its last line its stop
__global__ void __launch_bounds__(kThreads)
k_bm_runs(const uint32_t* __restrict__ rank, const uint64_t* __restrict__ start, const uint64_t* __restrict__ incl,
          const uint32_t* __restrict__ open, const uint64_t* __restrict__ pos, uint64_t L, uint64_t R,
          uint32_t* __restrict__ m_rank, uint64_t* __restrict__ m_start, uint64_t* __restrict__ m_stop)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= L) return;
    const uint32_t o = open[i];
    const uint64_t r = pos[i] + o - 1;
    if (r >= R) return;
    if (o) { m_rank[r] = rank[i]; m_start[r] = start[i]; }
    if (i + 1 == L || open[i + 1]) m_stop[r] = incl[i];
}

__global__ void __launch_bounds__(kThreads)
k_bm_run_len(const uint64_t* __restrict__ m_start, const uint64_t* __restrict__ m_stop, uint64_t R, uint64_t* __restrict__ len)
{
    const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r < R) len[r] = m_stop[r] - m_start[r];
}

// ---- 3. query -------------------------------------------------------------------------
struct Query {
    const uint32_t* rank;                  // of the reference lines (input 0: lines [0, Lr))
    const uint64_t *start, *stop;
    uint64_t Lr, range;
    const uint64_t *mlo, *A, *B, *PA, *PB;   // PA, PB: one entry more than A, B
    const uint64_t *rlo, *MS, *ME, *PL;
    uint32_t want;                         // W_*
    uint64_t *cnt, *bases, *uniq;          // per reference line; those of want
};

__global__ void __launch_bounds__(kTileRefs)
k_bm_query(const Query q)
{
    __shared__ uint64_t sh_m[kTileRefs / 64];
    __shared__ uint32_t sh_f[kTileRefs / 64];
    __shared__ int sh_head[kTileRefs / 64];          // the last segment head of every wave (-1: none)
    __shared__ uint32_t sh_win[6][kTileRefs];        // by segment head: A, B and run windows (indices are below 2^32)
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kTileRefs, i = base + t;
    const bool valid = i < q.Lr;
    const uint32_t rk = valid ? q.rank[i] : 0u;
    uint64_t sp = 0, ep = 0;
    if (valid) {
        const uint64_t s = q.start[i], e = q.stop[i];
        sp = s > q.range ? s - q.range : 0;
        ep = e + q.range < e ? ~0ull : e + q.range;
    }
    const bool hd = t == 0 || !valid || q.rank[i - 1] != rk;
    const bool last = valid && (t == kTileRefs - 1 || i + 1 == q.Lr || q.rank[i + 1] != rk);

    // the segment's head and the largest e' from it to this line
    const so::MF own{ep, hd ? 1u : 0u};
    const uint64_t emax = so::comb(so::block_excl_mf(own, sh_m, sh_f, (so::MF*)nullptr), own).m;
    const unsigned long long hm = __ballot(hd);
    const unsigned long long below = hm & ((2ull << lane) - 1);
    int head = below ? wid * 64 + 63 - __clzll(below) : -1;
    if (lane == 63) sh_head[wid] = hm ? wid * 64 + 63 - __clzll(hm) : -1;
    __syncthreads();
    for (int w = wid - 1; head < 0 && w >= 0; --w) head = sh_head[w];   // thread 0 is a head

    const bool ab = (q.want & (W_COUNT | W_BASES)) != 0;
    if (last) {   // emax is the segment's largest e'
        const uint64_t s0 = q.start[base + head];
        const uint64_t sp0 = s0 > q.range ? s0 - q.range : 0;
        if (ab) {
            const uint64_t lo = q.mlo[rk], hi = q.mlo[rk + 1];
            const uint64_t a0 = lower(q.A, lo, hi, sp0), b0 = upper(q.B, lo, hi, sp0);
            sh_win[0][head] = (uint32_t)a0;
            sh_win[1][head] = (uint32_t)lower(q.A, a0, hi, emax);
            sh_win[2][head] = (uint32_t)b0;
            sh_win[3][head] = (uint32_t)upper(q.B, b0, hi, emax);
        }
        if (q.want & W_UNIQ) {
            const uint64_t lo = q.rlo[rk], hi = q.rlo[rk + 1];
            const uint64_t m0 = lower(q.MS, lo, hi, sp0);
            sh_win[4][head] = (uint32_t)m0;
            sh_win[5][head] = (uint32_t)lower(q.MS, m0, hi, emax);
        }
    }
    __syncthreads();

    if (ab) {
        __shared__ uint64_t sh_A[kLdsWindow], sh_B[kLdsWindow];
        const uint64_t a0 = sh_win[0][head], a1 = sh_win[1][head], b0 = sh_win[2][head], b1 = sh_win[3][head];
        // One chromosome, every line valid (so head is 0 for all) and small
        // windows: they are staged in LDS and searched there.
        const bool staged = __syncthreads_count(hd) == 1 && a1 - a0 <= kLdsWindow && b1 - b0 <= kLdsWindow;
        const uint64_t* A = q.A;
        const uint64_t* B = q.B;
        uint64_t ao = 0, bo = 0;   // the index of A[0] and B[0] in the map arrays
        if (staged) {
            for (uint64_t k = t; k < a1 - a0; k += kTileRefs) sh_A[k] = q.A[a0 + k];
            for (uint64_t k = t; k < b1 - b0; k += kTileRefs) sh_B[k] = q.B[b0 + k];
            __syncthreads();
            A = sh_A;
            B = sh_B;
            ao = a0;
            bo = b0;
        }
        if (valid) {
            const uint64_t ja_e = ao + lower(A, a0 - ao, a1 - ao, ep);     // lines with a < e' end here
            const uint64_t jb_s = bo + upper(B, b0 - bo, b1 - bo, sp);     // lines with b <= s'
            if (q.cnt) q.cnt[i] = ja_e - jb_s;
            if (q.want & W_BASES) {
                const uint64_t ja_s = ao + lower(A, a0 - ao, a1 - ao, sp);
                const uint64_t jb_e = bo + upper(B, b0 - bo, b1 - bo, ep);
                q.bases[i] = (ja_e - jb_e) * ep - (ja_s - jb_s) * sp - (q.PA[ja_e] - q.PA[ja_s]) + (q.PB[jb_e] - q.PB[jb_s]);
            }
        }
    }
    if (!valid) return;
    if (q.want & W_UNIQ) {
        const uint64_t lo = q.rlo[rk];
        const uint64_t m0 = sh_win[4][head], m1 = sh_win[5][head];
        const uint64_t ke = lower(q.MS, m0, m1, ep);      // runs that start below e'
        uint64_t u = 0;
        if (ke > lo) {
            const uint64_t ks = lower(q.MS, m0, m1, sp);
            const uint64_t te = q.ME[ke - 1];
            const uint64_t ue = q.PL[ke - 1] + (te < ep ? te : ep) - q.MS[ke - 1];
            uint64_t us = q.PL[lo];
            if (ks > lo) {
                const uint64_t ts = q.ME[ks - 1];
                us = q.PL[ks - 1] + (ts < sp ? ts : sp) - q.MS[ks - 1];
            }
            u = ue - us;
        }
        q.uniq[i] = u;
    }
}

// ---- 4. format ------------------------------------------------------------------------
struct Format {
    const uint64_t *line_end, *start, *stop, *cnt, *bases, *uniq;
    uint64_t Lr;
    MapOptions opt;
};

// the number column c of line i holds
__device__ __forceinline__ uint64_t col_value(const Format& f, uint32_t c, uint64_t i)
{
    switch (c) {
        case STARCH_MAP_COUNT: return f.cnt[i];
        case STARCH_MAP_BASES: return f.bases[i];
        case STARCH_MAP_BASES_UNIQ: return f.uniq[i];
        case STARCH_MAP_INDICATOR: return f.cnt[i] ? 1 : 0;
        default: return f.stop[i] - f.start[i];   // STARCH_MAP_ECHO_REF_SIZE
    }
}

// len: bytes of output line i with its '\n' (0: left out); keep (may be NULL): 1 when it is written
__global__ void __launch_bounds__(kThreads)
k_bm_len(const Format f, uint64_t* __restrict__ len, uint32_t* __restrict__ keep)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= f.Lr) return;
    uint64_t n = 0;
    if (!(f.opt.skip_unmapped && f.cnt[i] == 0)) {
        n = (uint64_t)f.opt.delim_len * (f.opt.ncols - 1) + 1;
        for (uint32_t k = 0; k < f.opt.ncols; ++k) {
            const uint32_t c = f.opt.cols[k];
            if (c == STARCH_MAP_ECHO) n += f.line_end[i] - 1 - line_beg(f.line_end, i);
            else n += dec_digits(col_value(f, c, i));
        }
    }
    len[i] = n;
    if (keep) keep[i] = n ? 1u : 0u;
}

// A thread writes its line; an echo of kWaveCopyBytes or more is left to the
// whole wave, line after line.
__global__ void __launch_bounds__(kThreads)
k_bm_write(const uint8_t* __restrict__ bed, const Format f, const uint64_t* __restrict__ len, const uint64_t* __restrict__ off,
           uint64_t out_bytes, uint8_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bt::Writer<> w{out, 0};
    if (i < f.Lr && len[i] && off[i] + len[i] <= out_bytes) {
        w.o = off[i];
        for (uint32_t k = 0; k < f.opt.ncols; ++k) {
            const uint32_t c = f.opt.cols[k];
            if (k) w.delim(f.opt.delim, f.opt.delim_len);
            if (c == STARCH_MAP_ECHO) {
                const uint64_t b = line_beg(f.line_end, i);
                w.copy(0, bed + b, f.line_end[i] - 1 - b);
            } else w.dec(col_value(f, c, i));
        }
        out[w.o] = '\n';
    }
    bt::wave_copy_tails(w, out, lane);
}

}  // namespace

void MapWorkspace::run(sb::SortWorkspace& sorter, so::SetopWorkspace& lines, const MapOptions& opt, const uint8_t* d_cat,
                       uint64_t n, const std::vector<uint64_t>& in_end, hipStream_t st, DevBuf& out, MapResult& res)
{
    res = MapResult{};
    const uint64_t N = in_end.size();
    (void)out.as<uint8_t>(64);
    timer.start(st);
    auto finish = [&](int from) { timer.finish(from, st, {&res.ms_parse, &res.ms_build, &res.ms_query, &res.ms_format}); };
    if (n == 0) return finish(1);   // both inputs are empty

    // 1. parse, ranks, checks; the reference is lines [0, Lr), the map [m0, m0 + Lm)
    std::vector<uint64_t> first;
    const uint64_t L = lines.stage_lines(sorter, "bedmap", d_cat, n, in_end, st, first);
    const uint64_t Lr = first[1], m0 = N == 2 ? Lr : 0, Lm = N == 2 ? L - Lr : L;
    if (Lr + Lm >= (1ull << 32)) throw StarchError(STARCH_ERR_ARG, "bedmap: 2^32 lines or more over reference and map");
    res.n_ref = Lr;
    res.n_map = Lm;
    res.n_chromosomes = sorter.n_chromosomes;
    timer.mark(1, st);
    if (Lr == 0) return finish(2);

    uint32_t want = 0;
    for (uint32_t k = 0; k < opt.ncols; ++k) {
        if (opt.cols[k] == STARCH_MAP_COUNT || opt.cols[k] == STARCH_MAP_INDICATOR) want |= W_COUNT;
        if (opt.cols[k] == STARCH_MAP_BASES) want |= W_BASES;
        if (opt.cols[k] == STARCH_MAP_BASES_UNIQ) want |= W_UNIQ;
    }
    if (opt.skip_unmapped) want |= W_COUNT;
    const uint64_t C = sorter.n_chromosomes;
    const uint32_t* rank = sorter.ln.rank;
    const uint64_t* start = sorter.ln.start;
    const uint64_t* stop = sorter.ln.stop;
    uint64_t* scal = b_scal.as<uint64_t>(S_COUNT);

    // 2. map arrays
    Query q{};
    q.rank = rank;
    q.start = start;
    q.stop = stop;
    q.Lr = Lr;
    q.range = opt.range;
    q.want = want;
    if (want & (W_COUNT | W_BASES)) {
        uint64_t* mlo = b_mlo.as<uint64_t>(C + 1);
        hipLaunchKernelGGL(k_bm_bounds, dim3(blocks_for(C + 1, kThreads)), dim3(kThreads), 0, st, rank + m0, Lm, C, mlo);
        HIP_CHECK(hipGetLastError());
        q.mlo = mlo;
        q.A = start + m0;
        q.B = stop + m0;
        if (Lm) {
            const sb::KeyBits kb = sorter.stage_check(rank + m0, stop + m0, stop + m0, Lm, st);
            if (kb.desc != ~0ull) {   // a map line ends below the one before it: it is nested
                uint32_t passes = 0;
                const uint32_t* idx = sorter.stage_radix(rank + m0, stop + m0, nullptr, Lm, kb, st, &passes);
                if (!idx) throw StarchError(STARCH_ERR_INTERNAL, "bedmap: no order for the map stops");
                uint64_t* B = b_B.as<uint64_t>(Lm);
                hipLaunchKernelGGL(k_bm_gather, dim3(blocks_for(Lm, kThreads)), dim3(kThreads), 0, st, idx, stop + m0, Lm, B);
                HIP_CHECK(hipGetLastError());
                q.B = B;
                res.stops_sorted = 1;
            }
        }
        if (want & W_BASES) {
            uint64_t* PA = b_PA.as<uint64_t>(Lm + 1);
            uint64_t* PB = b_PB.as<uint64_t>(Lm + 1);
            scan::excl_sum_u64(q.A, PA, Lm, PA + Lm, b_tmp, st);
            scan::excl_sum_u64(q.B, PB, Lm, PB + Lm, b_tmp, st);
            q.PA = PA;
            q.PB = PB;
        }
        if (want & W_COUNT) q.cnt = b_cnt.as<uint64_t>(Lr);
        if (want & W_BASES) q.bases = b_bases.as<uint64_t>(Lr);
    }
    if (want & W_UNIQ) {
        uint64_t R = 0;
        uint32_t* MR = nullptr;
        if (Lm) {
            R = lines.stage_merge(start + m0, stop + m0, lines.head + m0, Lm, st);
            if (R == 0 || R > Lm) throw StarchError(STARCH_ERR_INTERNAL, "bedmap: the run count is out of range");
            MR = b_MR.as<uint32_t>(R);
            uint64_t* MS = b_MS.as<uint64_t>(R);
            uint64_t* ME = b_ME.as<uint64_t>(R);
            uint64_t* ML = b_ML.as<uint64_t>(R);
            uint64_t* PL = b_PL.as<uint64_t>(R);
            hipLaunchKernelGGL(k_bm_runs, dim3(blocks_for(Lm, kThreads)), dim3(kThreads), 0, st, rank + m0, start + m0,
                               lines.incl, lines.open, lines.pos, Lm, R, MR, MS, ME);
            hipLaunchKernelGGL(k_bm_run_len, dim3(blocks_for(R, kThreads)), dim3(kThreads), 0, st, MS, ME, R, ML);
            HIP_CHECK(hipGetLastError());
            scan::excl_sum_u64(ML, PL, R, (uint64_t*)nullptr, b_tmp, st);
            q.MS = MS;
            q.ME = ME;
            q.PL = PL;
        }
        uint64_t* rlo = b_rlo.as<uint64_t>(C + 1);
        hipLaunchKernelGGL(k_bm_bounds, dim3(blocks_for(C + 1, kThreads)), dim3(kThreads), 0, st, MR, R, C, rlo);
        HIP_CHECK(hipGetLastError());
        q.rlo = rlo;
        q.uniq = b_uniq.as<uint64_t>(Lr);
        res.map_runs_merged = R;
    }
    timer.mark(2, st);

    // 3. query
    if (want) {
        hipLaunchKernelGGL(k_bm_query, dim3(blocks_for(Lr, kTileRefs)), dim3(kTileRefs), 0, st, q);
        HIP_CHECK(hipGetLastError());
    }
    timer.mark(3, st);

    // 4. format
    Format f{sorter.ln.line_end, start, stop, q.cnt, q.bases, q.uniq, Lr, opt};
    const unsigned rblocks = blocks_for(Lr, kThreads);
    uint64_t* len = b_len.as<uint64_t>(Lr);
    uint64_t* off = b_off.as<uint64_t>(Lr);
    uint32_t* keep = opt.skip_unmapped ? b_keep.as<uint32_t>(Lr) : nullptr;
    hipLaunchKernelGGL(k_bm_len, dim3(rblocks), dim3(kThreads), 0, st, f, len, keep);
    HIP_CHECK(hipGetLastError());
    uint64_t tot[2] = {0, 0};
    const FormatTail ft = format_tail(Lr, len, off, keep, keep ? b_kpos.as<uint64_t>(Lr) : nullptr, scal + S_BYTES, tot,
                                      keep ? 2 : 1, b_tmp, out, st, "bedmap", false);
    hipLaunchKernelGGL(k_bm_write, dim3(rblocks), dim3(kThreads), 0, st, d_cat, f, len, off, ft.bytes,
                       static_cast<uint8_t*>(out.p));
    HIP_CHECK(hipGetLastError());
    res.out_bytes = ft.bytes;
    res.lines_out = ft.lines_kept;
    finish(4);
}

}  // namespace bm
