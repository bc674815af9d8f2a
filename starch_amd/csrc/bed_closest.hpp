// starch_amd/csrc/bed_closest.hpp -- host interface of closest-features
// (bed_closest.hip): per reference line, the nearest query line to its left and
// to its right, and how far away each is.
#pragma once
#include <vector>

#include "bed_setops.hpp"
#include "common.hpp"
#include "sort_bed.hpp"

namespace bc {

constexpr int kTileRefs = 256;        // reference lines per query workgroup (one thread each)
constexpr uint32_t kFanShift = 4;
constexpr uint32_t kFanout = 1u << kFanShift;   // stops per tile of the hierarchy of maxima, and tiles per tile above
constexpr int kMaxLevels = 9;         // levels of 16^k stops, k = 0 .. 8: 2^32 lines end in one item

struct ClosestOptions {               // checked by the caller (api_bed.hip)
    uint32_t closest = 0, dist = 0, no_overlaps = 0, no_ref = 0;
    uint32_t delim_len = 0;
    uint8_t delim[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

struct ClosestResult {
    uint64_t n_ref = 0, n_query = 0, n_chromosomes = 0, stops_sorted = 0, left_na = 0, right_na = 0, lines_out = 0,
             out_bytes = 0;
    float ms_parse = 0, ms_build = 0, ms_query = 0, ms_format = 0;
};

struct ClosestWorkspace {
    DevBuf b_scal, b_tmp, b_mlo, b_B, b_hier, b_left, b_right, b_len, b_off;
    StageTimer<5> timer;
    // The inputs lie back to back in d_cat[0, n) as for bm::MapWorkspace::run:
    // in_end has two entries (reference, then query).  One line per reference
    // line goes to out (res.out_bytes of it).  sorter and lines supply parse,
    // ranks, checks, the running maximum of the query stops and the radix
    // order.  Throws StarchError as include/starch_amd.h describes.
    void run(sb::SortWorkspace& sorter, so::SetopWorkspace& lines, const ClosestOptions& opt, const uint8_t* d_cat, uint64_t n,
             const std::vector<uint64_t>& in_end, hipStream_t st, DevBuf& out, ClosestResult& res);
};

}  // namespace bc
