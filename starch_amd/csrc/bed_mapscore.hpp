// starch_amd/csrc/bed_mapscore.hpp -- host interface of bedmap-scores
// (bed_mapscore.hip): per reference line, exact statistics of column 5 of the
// map lines that satisfy the overlap criterion.  The hit list is
// bedmap-elements' (me::MapelWorkspace::hits).
#pragma once
#include <vector>

#include "bed_mapel.hpp"
#include "bed_setops.hpp"
#include "common.hpp"
#include "sort_bed.hpp"

namespace ms {

constexpr int kThreads = 256;
constexpr int kChunks = 8;                               // 64 contiguous hits at a time, this many times per wave
constexpr int kWaveHits = 64 * kChunks;                  // contiguous hits of one wave
constexpr int kTileHits = (kThreads / 64) * kWaveHits;   // contiguous hits of one workgroup of the reduction
constexpr int kMaxCols = 12;
constexpr int kCodes = 11;                               // STARCH_MAPSC_ECHO .. STARCH_MAPSC_MAX_ELEMENT

struct MapscOptions {                     // checked by the caller (api_bed.hip)
    uint32_t ncols = 0;
    uint8_t cols[kMaxCols] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // STARCH_MAPSC_*
    me::MapelOptions crit;                // criterion, n, range, frac_num, frac_den alone
    uint64_t kth_num = 0, kth_den = 1;    // KTH: f = kth_num / kth_den, kth_den = 10^digits
    uint32_t prec = 6;
    uint32_t skip_unmapped = 0;
    uint32_t delim_len = 0;
    uint8_t delim[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

struct MapscResult {
    uint64_t n_ref = 0, n_map = 0, n_chromosomes = 0, hits = 0, straddling = 0, sorted_hits = 0, radix_passes = 0, lines_out = 0,
             out_bytes = 0;
    float ms_parse = 0, ms_build = 0, ms_query = 0, ms_reduce = 0, ms_format = 0;
};

struct MapscWorkspace {
    DevBuf b_scal, b_tmp, b_V, b_ok, b_lo, b_hi, b_min, b_max, b_imin, b_imax, b_key, b_len, b_off, b_keep, b_kpos;
    StageTimer<6> timer;
    // The inputs lie back to back in d_cat[0, n) as for me::MapelWorkspace::run,
    // whose stages 1 to 3 (hitter.hits) find the hits.  One line per reference
    // line goes to out (res.out_bytes of it).  The sorter's radix stage orders
    // the hits for MEDIAN and KTH.  Throws StarchError as include/starch_amd.h
    // describes.
    void run(sb::SortWorkspace& sorter, so::SetopWorkspace& lines, me::MapelWorkspace& hitter, const MapscOptions& opt,
             const uint8_t* d_cat, uint64_t n, const std::vector<uint64_t>& in_end, hipStream_t st, DevBuf& out, MapscResult& res);
};

}  // namespace ms
