// starch_amd/csrc/bed_setops.hpp -- host interface of the BED set operations
// (bed_setops.hip): merge, intersect, difference, symmdiff, complement.
#pragma once
#include <vector>

#include "common.hpp"
#include "sort_bed.hpp"

namespace so {

constexpr int kScanThreads = 256;
constexpr int kScanItems = 4;                            // lines per thread of a max-scan tile
constexpr int kScanTile = kScanThreads * kScanItems;     // lines per tile of the segmented max-scan

struct SetopResult {
    uint64_t n_lines = 0, n_chromosomes = 0, runs_merged = 0, groups = 0, lines_out = 0, out_bytes = 0;
    uint32_t radix_passes = 0;
    float ms_parse = 0, ms_merge = 0, ms_sort = 0, ms_sweep = 0, ms_format = 0;
};

struct SetopWorkspace {
    DevBuf b_scal, b_tmp, b_in_end, b_first, b_head, b_open, b_incl, b_part_m, b_part_f, b_pos, b_e_rank, b_e_pos, b_e_w,
        b_g_w, b_g_sum, b_g_last, b_g_pos, b_grp_rank, b_grp_pos, b_grp_depth, b_f_start, b_f_end, b_p_start, b_p_end,
        b_o_rank, b_o_start, b_o_stop, b_o_len, b_o_off, b_name_off, b_name_len;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // The op (STARCH_SETOP_*) over the inputs that lie back to back in
    // d_cat[0, n): input k is d_cat[in_end[k-1], in_end[k]) (in_end[-1] = 0), and
    // every non-empty input ends in '\n'.  The BED3 result goes to out
    // (res.out_bytes of it).  sorter supplies framing, parse, ranks and the
    // radix order.  Throws StarchError as include/starch_amd.h describes.
    void run(sb::SortWorkspace& sorter, int op, const uint8_t* d_cat, uint64_t n, const std::vector<uint64_t>& in_end,
             hipStream_t st, DevBuf& out, SetopResult& res);

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
    ~SetopWorkspace();
};

}  // namespace so
