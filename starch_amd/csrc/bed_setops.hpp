// starch_amd/csrc/bed_setops.hpp -- host interface of the BED set operations
// (bed_setops.hip): merge, intersect, difference, symmdiff, complement,
// element-of, not-element-of, partition, chop, everything.
#pragma once
#include <vector>

#include "common.hpp"
#include "sort_bed.hpp"

namespace so {

constexpr int kScanThreads = 256;
constexpr int kScanItems = 4;                            // lines per thread of a max-scan tile
constexpr int kScanTile = kScanThreads * kScanItems;     // lines per tile of the segmented max-scan
constexpr uint32_t kRmqTile = 64;                        // runs per tile of element-of's range maximum
constexpr int kExpandTile = 256;                         // pieces per workgroup of chop's expansion (and its LDS window, in runs)

struct SetopResult {
    uint64_t n_lines = 0, n_chromosomes = 0, runs_merged = 0, groups = 0, lines_out = 0, out_bytes = 0;
    uint32_t radix_passes = 0;
    float ms_parse = 0, ms_merge = 0, ms_sort = 0, ms_sweep = 0, ms_format = 0;
};

struct BedopsOptions {          // starch_bedops_options, checked
    int op = 0;
    uint64_t threshold = 100;   // element-of: bases, or percent (1 .. 100)
    bool percent = true;
    uint64_t chop = 1, stagger = 1;   // stagger: never 0 here
    bool exclude_short = false;
};

struct SetopWorkspace {
    DevBuf b_scal, b_tmp, b_in_end, b_first, b_head, b_open, b_incl, b_part_m, b_part_f, b_pos, b_e_rank, b_e_pos, b_e_w,
        b_g_w, b_g_sum, b_g_last, b_g_pos, b_grp_rank, b_grp_pos, b_grp_depth, b_f_start, b_f_end, b_p_start, b_p_end,
        b_o_rank, b_o_start, b_o_stop, b_o_len, b_o_off, b_name_off, b_name_len;
    // element-of: the other inputs' lines in order, their runs and the range maximum; chop: counts and pieces
    DevBuf b_q_rank, b_q_start, b_q_stop, b_q_head, b_u_rank, b_u_start, b_u_stop, b_rmq, b_keep, b_kpos, b_order, b_cnt,
        b_coff, b_c_rank, b_c_start, b_c_stop;
    StageTimer<6> timer;
    // The op (STARCH_SETOP_MERGE .. _COMPLEMENT) over the inputs that lie back to
    // back in d_cat[0, n): input k is d_cat[in_end[k-1], in_end[k]) (in_end[-1] = 0), and
    // every non-empty input ends in '\n'.  The BED3 result goes to out
    // (res.out_bytes of it).  sorter supplies framing, parse, ranks and the
    // radix order.  Throws StarchError as include/starch_amd.h describes.
    void run(sb::SortWorkspace& sorter, int op, const uint8_t* d_cat, uint64_t n, const std::vector<uint64_t>& in_end,
             hipStream_t st, DevBuf& out, SetopResult& res);
    // The same for every op of starch_bedops_host (opt is already checked); ops
    // 0 to 4 are run().
    void run_bedops(sb::SortWorkspace& sorter, const BedopsOptions& opt, const uint8_t* d_cat, uint64_t n,
                    const std::vector<uint64_t>& in_end, hipStream_t st, DevBuf& out, SetopResult& res);

    // The first stages of run(), for bed_map.hip.
    // 1, 2. framing, parse and ranks of d_cat[0, n), n > 0, through sorter (whose
    // ln then holds the per-line arrays), the first line of every input
    // (first: in_end.size() + 1 entries), stop > start and the per-input order;
    // errors are thrown with `tool` in front.  Returns the number of lines and
    // leaves head: bit 0 at the first line of every (input, chromosome) segment.
    uint64_t stage_lines(sb::SortWorkspace& sorter, const char* tool, const uint8_t* d_cat, uint64_t n,
                         const std::vector<uint64_t>& in_end, hipStream_t st, std::vector<uint64_t>& first);
    // 3. the segments of L > 0 checked lines merged with themselves: incl (the
    // largest stop from the segment's head to the line), open (1: the line opens
    // a merged run) and pos (open's exclusive sum).  Returns the number of runs.
    uint64_t stage_merge(const uint64_t* start, const uint64_t* stop, const uint8_t* hd, uint64_t L, hipStream_t st);
    uint8_t* head = nullptr;
    uint64_t *incl = nullptr, *pos = nullptr;
    uint32_t* open = nullptr;

private:
    // 4, 5a. E < 2^32 weighted ends ordered by (rank, position) and swept: one
    // group per distinct (rank, position) in grp_rank / grp_pos / grp_depth.
    // Records ev[3] of the timer after the order.  Returns the number of groups.
    uint64_t stage_sweep(sb::SortWorkspace& sorter, const uint32_t* e_rank, const uint64_t* e_pos, const uint64_t* e_w,
                         uint64_t E, hipStream_t st, SetopResult& res);
    // 1 to 5 of run(): the K result intervals in o_rank / o_start / o_stop.
    // Records ev[1] to ev[3] of the timer; first: as stage_lines leaves it.
    uint64_t stage_intervals(sb::SortWorkspace& sorter, int op, const uint8_t* d_cat, uint64_t n,
                             const std::vector<uint64_t>& in_end, hipStream_t st, SetopResult& res);
    // 6. K > 0 intervals as BED3 into out; returns the bytes.  limit: the result
    // is refused (STARCH_ERR_ARG) when it has that many bytes or more (0: none).
    uint64_t stage_format(sb::SortWorkspace& sorter, const uint8_t* d_cat, const uint32_t* o_rank, const uint64_t* o_start,
                          const uint64_t* o_stop, uint64_t K, uint64_t limit, hipStream_t st, DevBuf& out);
    void finish(hipStream_t st, SetopResult& res, int from);
    void element_of(sb::SortWorkspace& sorter, const BedopsOptions& opt, const uint8_t* d_cat, uint64_t L, uint64_t Lr,
                    hipStream_t st, DevBuf& out, SetopResult& res);
    void partition(sb::SortWorkspace& sorter, const uint8_t* d_cat, uint64_t L, hipStream_t st, DevBuf& out, SetopResult& res);
    void chop(sb::SortWorkspace& sorter, const BedopsOptions& opt, const uint8_t* d_cat, uint64_t K, hipStream_t st, DevBuf& out,
              SetopResult& res);
    void everything(sb::SortWorkspace& sorter, const uint8_t* d_cat, uint64_t n, uint64_t L, hipStream_t st, DevBuf& out,
                    SetopResult& res);
    uint32_t* grp_rank = nullptr;
    uint64_t *grp_pos = nullptr, *grp_depth = nullptr;
};

}  // namespace so
