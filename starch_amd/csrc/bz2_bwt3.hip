// starch_amd/csrc/bz2_bwt3.hip -- block sort v3 (the default): a batch-wide
// segmented sort of every rotation of every block, then refinement of the
// rotations whose packed prefix keys tie.
//
// Contract (same as k_bwt, bz2_bwt.hip): SA = the exact sorted order of the
// cyclic rotations of every non-periodic block (BZ2_blockSort's ptr[],
// bz:blocksort.c:1031-1089; unique because all rotations differ), origPtr =
// rank of rotation 0; periodic blocks are flagged (flags bit0) for
// k_fallback_exact, which reproduces fallbackSort's tie order.
//
// Why this shape: a 900 KB transformed-BED block almost never needs more than
// its packed D-symbol prefix (D = 64 / B symbols of B = ceil(log2 nInUse)
// bits in a u64 key; 16 for BED3 text): measured on cfg2 blocks, ~5 tied
// pairs per 900k rotations; cfg4 (narrowPeak) ~0.8 %.  So the work is a
// segmented sort of (block, 64-bit key) pairs, done for ALL blocks of a batch
// at once:
//
//   k3_pss_hist packed symbol stream (PSS) of every block: its symbols as
//               B-bit fields, MSB first, in u64 words, wrapped past the end;
//               the key of rotation r is bits [rB, rB+KB) -- two word loads
//               and a shift, so keys are never stored; and, from the same
//               registers, per 32k-rotation tile the 4096-bucket histogram
//               of the top 12 bits
//   k3_scan     per block: bucket starts, per-tile cursors, size-class lists
//   k3_scatter_lds  rotations -> bucket order in SA, staged in LDS.  Persistent,
//               per-XCD queues: each XCD streams ITS blocks one at a time, so
//               the writes of a block meet in that XCD's 4 MB L2
//   k3_bin_*    every work list is binned by block into 8 per-XCD segments
//               (blocks x, x+8, ... in order), so the persistent kernels below
//               touch ~one block's PSS per XCD at a time (L2-resident)
//   k3_part_l   buckets > 4096: MSD partition on the next 8 key bits, repeated
//   k3_sort_w   buckets <= 64: one wave, rank by comparison
//   k3_sort_lds buckets <= 256: one wave; <= 1024/2048/4096: one workgroup;
//               one MSD digit then ranking by comparison (LSD radix when a
//               sub-bucket is large), keys in registers, LDS exchange
//   -- every sort writes SA and lists the groups of equal keys --
//   text rounds a tied group is re-sorted by its NEXT D' = 52/B symbols, read
//               from the PSS at an offset (12 key bits stay free for the packed
//               group index); enough for BED text, where ties are short
//   k3_rk_*     blocks still tied after the text rounds (long repeats,
//               periodic blocks): dense RK = head position of every
//               rotation's group, then prefix doubling --
//   k3_gather   doubling round r: key(q) = RK[(SA[q] + h0*2^(r-1)) mod n] for
//               the tied rotations only (K2); the same kernels re-sort the
//               groups and update RK.  A round in which no group of a block
//               splits proves the block periodic.
//
// Scratch (BwtScratch, per batch slot, stride S elements): SA/V = rotations in
// bucket order (V: partition ping-pong); K = PSS + per-tile cursors (round 0,
// text rounds), key ping-pong while doubling; K2 = doubling keys; RK ranks;
// U = wave-class list; U2/V2 = tie-group lists of consecutive rounds (u64).
//
// This file is the host side: the metadata arena and the control flow of
// round 0, the text rounds and the doubling rounds.  The kernels live in
// bwt3_round0.hip, bwt3_part.hip, bwt3_leaf.hip and bwt3_rounds.hip, each
// behind the launchers that bwt3_int.hpp declares.
#include "bwt3_int.hpp"

namespace bz {
using namespace bwt3;

namespace {

// Bump carve of the metadata arena.  launch_bwt3 runs one sequence of take()
// calls twice, from address 0 to measure and from the buffer to assign, so the
// size and the layout cannot differ.  A region is aligned for its type.
struct Carve {
    uintptr_t p;
    template <class T>
    T* take(uint64_t count)
    {
        p = (p + alignof(T) - 1) & ~(uintptr_t)(alignof(T) - 1);
        T* r = reinterpret_cast<T*>(p);
        p += count * sizeof(T);
        return r;
    }
};

}  // namespace

// Host orchestration.  A handful of host round trips per batch (list sizes).
bool launch_bwt3(BlockDesc* blocks, uint32_t b0, uint32_t nb, const uint8_t* blkbytes, uint64_t stride,
                 const BwtScratch& scr, DevBuf& meta, uint32_t* hctr, unsigned long long* stats, hipStream_t st,
                 bool wide)
{
    if (nb == 0) return false;
    if (nb > 4095) throw StarchError(-2, "bwt3: batch too large");
    // The top-level tile, restated here and tied to the units' definition
    // (bwt3_int.hpp): this file is where the tile size has always been read
    // from, by the tests of every earlier revision among others.
    constexpr int PTILE = 32768;
    static_assert(PTILE == bwt3::PTILE && MAXT == (900064 + PTILE - 1) / PTILE, "one tile size");
    // the tile histograms live in K after the PSS: [MAXT + 1][bins] words (small
    // blocks, -1 .. -2, have room for the 4096-bin binary digit only)
    if (wide && pss_words(scr.stride) * 2 + (uint64_t)(MAXT + 1) * PNB_WIDE > 2 * scr.stride) wide = false;
    if (pss_words(scr.stride) * 2 + (uint64_t)(MAXT + 1) * PNB > 2 * scr.stride)
        throw StarchError(-2, "bwt3: block stride too small");
    const uint64_t N = (uint64_t)nb * scr.stride;
    const uint64_t cap_s = N / (W_MAX + 1) + 64, cap_s2 = N / (S1_MAX + 1) + 64, cap_m0 = N / (S_MAX + 1) + 64,
                   cap_m1 = N / (M0_MAX + 1) + 64,
                   cap_m2 = N / (M1_MAX + 1) + 64,
                   cap_m3 = N / (M2_MAX + 1) + 64, cap_l = N / ((L_MIN < M3_MAX ? L_MIN : M3_MAX) + 1) + 64;
    const uint64_t nb_bins = nb < 64 ? 8ull * nb : nb;     // bins of k3_bin_* (see bin_of)
    constexpr uint32_t QSETS = 64, QSET = 8 * XQ_STRIDE + 32;   // queue heads (a line each) + segments per launch
    Ctx c;
    c.blocks = blocks;
    c.b0 = b0;
    c.blkbytes = blkbytes;
    c.stride = stride;
    c.scr = scr;
    c.nb = nb;
    // The metadata arena, carved in this order.  qpool: the queue sets; bincol /
    // binst / binh: k3_bin_*'s per-bin running totals (reset by k3_bin_scan),
    // per-bin starts and per-chunk places; then the class lists, and what the
    // huge-group path (k3_hg_*, k3_gather_big) keeps per group.
    uint32_t *qpool, *bincol, *binst, *binh;
    auto carve = [&](Carve a) {
        c.L.ctr = a.take<uint32_t>(2 * C_N);
        c.L.gin = a.take<uint32_t>(nb);
        c.L.runs = a.take<uint32_t>(nb);
        c.L.periodic = a.take<uint32_t>(nb);
        c.L.rounds = a.take<uint32_t>(nb);
        c.L.tied = a.take<uint32_t>(nb);
        c.L.geo = a.take<Geo>(nb);
        qpool = a.take<uint32_t>(QSETS * QSET);
        bincol = a.take<uint32_t>(nb_bins);
        binst = a.take<uint32_t>(nb_bins);        // (everything before it is zeroed below)
        binh = a.take<uint32_t>(BIN_MAXWG * nb_bins);
        c.L.s = a.take<uint64_t>(cap_s);
        c.L.s2 = a.take<uint64_t>(cap_s2);
        c.L.m0 = a.take<uint64_t>(cap_m0);
        c.L.m1 = a.take<uint64_t>(cap_m1);
        c.L.m2 = a.take<uint64_t>(cap_m2);
        c.L.m3 = a.take<uint64_t>(cap_m3);
        c.L.l[0] = a.take<uint64_t>(cap_l);
        c.L.l[1] = a.take<uint64_t>(cap_l);
        c.L.hg = a.take<uint64_t>(HG_MAXN);
        c.L.gb = a.take<uint64_t>(GB_MAXN);
        c.L.gb_h = a.take<uint32_t>(GB_MAXN);
        c.L.hg_info = a.take<uint32_t>((uint64_t)HG_MAXN * 512);
        c.L.hg_vary = a.take<uint64_t>(HG_MAXN);
        c.L.hg_flag = a.take<uint32_t>(HG_MAXN);
        c.L.hg_pre = a.take<uint32_t>(HG_MAXN + 1);
        c.L.hg_eqlt = a.take<uint32_t>(2 * HG_MAXN);
        c.L.hg_mc = a.take<uint32_t>(6 * HG_MAXN);
        c.L.hg_rank = a.take<uint32_t>(HG_MAXN);
        return a.p;
    };
    uint8_t* mw = meta.as<uint8_t>(carve(Carve{0}));       // (a device allocation: aligned like address 0 for every region)
    carve(Carve{reinterpret_cast<uintptr_t>(mw)});
    c.L.w = reinterpret_cast<uint64_t*>(scr.U);
    c.L.t[0] = reinterpret_cast<uint64_t*>(scr.U2);
    c.L.t[1] = reinterpret_cast<uint64_t*>(scr.V2);
    c.lsel = 0;
    c.tsel = 0;
    c.mode = 0;
    c.keysrc = 0;
    c.kA = scr.K2;
    c.kB = scr.K;
    c.rtext = 0;
    c.qhead = nullptr;
    c.qseg = nullptr;
    c.nbins = wide ? PNB_WIDE : PNB;
    c.sdig = 0;
    // counters, per-block words, queue pool, bincol
    HIP_CHECK(hipMemsetAsync(mw, 0, reinterpret_cast<uint8_t*>(binst) - mw, st));
    launch_period(c, st);

    auto zero = [&](uint64_t mask) { launch_zero(c.L.ctr, mask, st); };
    auto bit = [](uint32_t i) { return 1ull << i; };
    uint32_t qnext = 0;
    auto next_q = [&](uint32_t*& head, uint32_t*& seg) {
        if (qnext == QSETS) {
            HIP_CHECK(hipMemsetAsync(qpool, 0, QSETS * QSET * sizeof(uint32_t), st));
            qnext = 0;
        }
        head = qpool + qnext * QSET;
        seg = head + 8 * XQ_STRIDE;
        ++qnext;
    };
    auto read_ctr = [&]() {
        HIP_CHECK(hipMemcpyAsync(hctr, c.L.ctr, C_N * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (hctr[C_ERR]) throw StarchError(-11, "bwt3: group keys do not share 12 top bits");
    };
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    static int ncu = 0;
    if (!ncu) {
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, dev));
        ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    // bin a list (n items, device) into `out`; sets c.qseg/c.qhead for the next launch
    auto bin = [&](const uint64_t* list, uint32_t n, uint64_t* out) {
        uint32_t* head;
        uint32_t* seg;
        next_q(head, seg);
        launch_bin(list, n, (uint32_t)nb_bins, nb_bins > nb ? 3u : 0u, binh, bincol, binst, seg, out, st);
        c.qhead = head;
        c.qseg = seg;
    };
    // partition large groups level by level, then run the leaf sorts.  Binned
    // copies go to K2 (free outside doubling) or, while doubling, to the tie
    // list the gather has just consumed (capacity N/2 items either way).
    auto sort_groups = [&]() {
        uint64_t* bout = c.keysrc ? c.L.t[c.tsel ^ 1u] : reinterpret_cast<uint64_t*>(scr.K2);
        uint32_t lsel = 0;
        for (int level = 0;; ++level) {
            read_ctr();
            const uint32_t nl = hctr[C_L0 + lsel];
            if (nl == 0) break;
            if (level > 64) throw StarchError(-10, "bwt3: partition did not converge");
            const bool huge = hctr[C_LM0 + lsel] > HG_MIN;
            if (huge) launch_hg_pick(c, c.L.l[lsel], nl, st);   // groups above HG_MIN: partitioned by the whole grid
            bin(c.L.l[lsel], nl, bout);
            c.lsel = lsel ^ 1u;
            zero(bit(C_L0 + (lsel ^ 1u)) | bit(C_LM0 + (lsel ^ 1u)));
            if (huge) launch_hg_level(c, nl, ncu, st);
            launch_part_l(c, bout, ncu, st);
            c.sdig = 0;                  // (deeper levels: the sub-buckets' digits are gathered)
            zero(bit(C_L0 + lsel) | bit(C_LM0 + lsel));
            lsel ^= 1u;
        }
        c.lsel = 0;
        // The leaf sorts, largest class first.  Every launch reads its own binned
        // copy; stream order lets them share one buffer.  Doubling rounds (keys
        // in K/K2) run their own instantiations.
        auto leaf = [&](LeafClass k, uint64_t* list, uint32_t n) {
            if (!n) return;
            bin(list, n, bout);
            launch_leaf(c, k, bout, list, ncu, st);
        };
        leaf(LEAF_M3, c.L.m3, hctr[C_M3]);
        leaf(LEAF_M2, c.L.m2, hctr[C_M2]);
        leaf(LEAF_M0, c.L.m0, hctr[C_M0]);
        leaf(LEAF_M1, c.L.m1, hctr[C_M1]);
        leaf(LEAF_S, c.L.s, hctr[C_S]);
        leaf(LEAF_S2, c.L.s2, hctr[C_S2]);
        leaf(LEAF_W, c.L.w, hctr[C_W]);
        HIP_CHECK(hipGetLastError());
        zero((0x3Full << C_W) | bit(C_M0));
    };

    // ---- round 0: packed prefix keys gathered from the PSS by every sort, as
    // the text rounds do ----
    {
        uint32_t* head;
        uint32_t* seg;
        next_q(head, seg);
        c.qhead = head;
        c.qseg = nullptr;
        c.sdig = 1;                      // (k3_scatter_lds leaves the L buckets' first partition digits in LL)
        launch_round0(c, wide, ncu, st);
    }
    sort_groups();
    c.sdig = 0;
    // ---- text rounds: extend the tied rotations' keys from the PSS ----
    uint32_t rtext = 0;
    uint64_t prev_tied = ~0ull;
    bool done = false;
    for (;;) {
        read_ctr();
        const uint32_t nt = hctr[C_T0 + c.tsel];
        const uint64_t tied = hctr[C_TS0 + c.tsel];
        if (nt == 0) { done = true; break; }
        if (rtext == TEXT_ROUNDS || (rtext > 0 && 2 * tied > prev_tied)) break;   // long repeats: double
        prev_tied = tied;
        ++rtext;
        c.rtext = rtext;
        const uint32_t cur = c.tsel;
        c.tsel ^= 1u;
        zero(bit(C_T0 + c.tsel) | bit(C_TS0 + c.tsel));
        launch_classify_text(c, c.L.t[cur], nt, st);
        zero(bit(C_T0 + cur));
        sort_groups();
    }
    // ---- prefix doubling on the blocks still tied ----
    if (!done) {
        const uint32_t nt = hctr[C_T0 + c.tsel];
        launch_rk_init(c, c.L.t[c.tsel], nt, ncu, st);
        c.mode = 1;
        c.keysrc = 1;
        for (uint32_t round = 1;; ++round) {
            if (round > 1) read_ctr();
            const uint32_t n2 = hctr[C_T0 + c.tsel];
            if (n2 == 0) break;
            if (round > 40) throw StarchError(-10, "bwt3: doubling did not converge");
            const uint32_t cur = c.tsel;
            c.tsel ^= 1u;
            zero(bit(C_T0 + c.tsel) | bit(C_TS0 + c.tsel) | bit(C_GB));
            launch_gather(c, c.L.t[cur], n2, round, rtext, ncu, st);
            zero(bit(C_T0 + cur));
            sort_groups();
            launch_round_end(c, st);
        }
    }
    launch_finish(c, stats, st);
    return !done;   // prefix doubling ran: some block may be periodic (flags bit 0)
}

}  // namespace bz
