// starch_amd/csrc/bed_map.hpp -- host interface of bedmap (bed_map.hip): per
// reference line, the count and the bases of the map lines that overlap it.
#pragma once
#include <vector>

#include "bed_setops.hpp"
#include "common.hpp"
#include "sort_bed.hpp"

namespace bm {

constexpr int kTileRefs = 256;          // reference lines per query workgroup (one thread each)
constexpr uint32_t kLdsWindow = 1024;   // largest window into the map starts, and into the stops, staged in LDS

struct MapOptions {                     // checked by the caller (api_bed.hip)
    uint32_t ncols = 0;
    uint8_t cols[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // STARCH_MAP_*
    uint64_t range = 0;
    uint32_t skip_unmapped = 0;
    uint32_t delim_len = 0;
    uint8_t delim[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

struct MapResult {
    uint64_t n_ref = 0, n_map = 0, n_chromosomes = 0, map_runs_merged = 0, stops_sorted = 0, lines_out = 0, out_bytes = 0;
    float ms_parse = 0, ms_build = 0, ms_query = 0, ms_format = 0;
};

struct MapWorkspace {
    DevBuf b_scal, b_tmp, b_mlo, b_rlo, b_B, b_PA, b_PB, b_MR, b_MS, b_ME, b_ML, b_PL, b_cnt, b_bases, b_uniq, b_len, b_off,
        b_keep, b_kpos;
    StageTimer<5> timer;
    // The inputs lie back to back in d_cat[0, n) as for so::SetopWorkspace::run:
    // in_end has one entry (the reference is mapped onto itself) or two
    // (reference, then map).  The annotated reference lines go to out
    // (res.out_bytes of it).  sorter and lines supply parse, ranks, checks, the
    // radix order and the per-input merge.  Throws StarchError as
    // include/starch_amd.h describes.
    void run(sb::SortWorkspace& sorter, so::SetopWorkspace& lines, const MapOptions& opt, const uint8_t* d_cat, uint64_t n,
             const std::vector<uint64_t>& in_end, hipStream_t st, DevBuf& out, MapResult& res);
};

}  // namespace bm
