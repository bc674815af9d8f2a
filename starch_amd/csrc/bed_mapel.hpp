// starch_amd/csrc/bed_mapel.hpp -- host interface of bedmap-elements
// (bed_mapel.hip): per reference line, the list of the map lines that satisfy
// the overlap criterion, and the columns that are written from that list.
#pragma once
#include <vector>

#include "bed_closest.hpp"
#include "bed_setops.hpp"
#include "common.hpp"
#include "sort_bed.hpp"

namespace me {

constexpr int kTileRefs = 256;            // reference lines per workgroup of the count and fill passes (one thread each)
constexpr uint32_t kHeavy = 128;          // a run of this many candidates or more is tested by the whole wave, 64 at a time
constexpr int kMaxCols = 12;
constexpr int kListCols = 5;              // ECHO_MAP .. ECHO_OVERLAP_SIZE: one piece per hit
// Probes of the searches and of the hierarchy: at most this many per reference
// line (three binary searches over fewer than 2^32 lines and one walk that
// finds nothing) and per candidate found by a walk (kFanout items per level
// upwards and downwards).
constexpr uint32_t kStepsPerHit = 3 * 32 + bc::kFanout * (2 * bc::kMaxLevels - 1);

struct MapelOptions {                     // checked by the caller (api_bed.hip)
    uint32_t ncols = 0;
    uint8_t cols[kMaxCols] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // STARCH_MAPEL_*
    uint32_t criterion = 0;               // STARCH_MAPEL_CRIT_*
    uint64_t n = 1, range = 0;            // BP_OVR; RANGE
    uint64_t frac_num = 0, frac_den = 1;  // FRACTION_*: f = frac_num / frac_den, frac_den = 10^digits
    uint32_t skip_unmapped = 0;
    uint32_t delim_len = 0, multi_len = 0;
    uint8_t delim[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint8_t multi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

struct MapelResult {
    uint64_t n_ref = 0, n_map = 0, n_chromosomes = 0, hits = 0, heavy_lines = 0, walk_steps = 0, lines_out = 0, out_bytes = 0;
    float ms_parse = 0, ms_build = 0, ms_query = 0, ms_format = 0;
};

// The hit list that stages 1 to 3 leave in the workspace's buffers (and the
// parsed lines in the sorter's): reference line i has the cnt[i] hits
// [hoff[i], hoff[i + 1]) of the T in all; hit h is map line H[h] (line m0 + H[h]
// of the buffer) of reference line R[h], and R never decreases.
struct HitList {
    uint64_t Lr = 0, Lm = 0, m0 = 0, T = 0, n_chromosomes = 0, heavy_lines = 0, walk_steps = 0;
    const uint64_t *cnt = nullptr, *hoff = nullptr, *rmax = nullptr;   // hoff: Lr + 1 entries; rmax: the largest stop of a line's hits
    const uint32_t *H = nullptr, *R = nullptr;
};

struct MapelWorkspace {
    DevBuf b_scal, b_tmp, b_mlo, b_hier, b_cnt, b_hoff, b_H, b_R, b_rmax, b_lens[kListCols], b_P[kListCols], b_cs[kListCols],
        b_len, b_off, b_keep, b_kpos;
    StageTimer<5> timer;
    // Stages 1 to 3 for run() and for bedmap-scores (bed_mapscore.hip): parse
    // and checks, the map arrays, the count pass, the scan and the fill pass.
    // name begins the messages; of opt the criterion alone is read.  Marks 0,
    // 1 and 2 of tm are recorded after the parse, the map arrays and the fill
    // pass.  Returns how many of them were: 0 when both inputs are empty,
    // 1 when the reference has no line, else 3, and only then does hl hold the
    // arrays.
    int hits(sb::SortWorkspace& sorter, so::SetopWorkspace& lines, const char* name, const MapelOptions& opt,
             const uint8_t* d_cat, uint64_t n, const std::vector<uint64_t>& in_end, hipStream_t st, StageMarks tm, HitList& hl);
    // The inputs lie back to back in d_cat[0, n) as for bm::MapWorkspace::run:
    // in_end has one entry (the reference is its own map) or two (reference,
    // then map).  One line per reference line goes to out (res.out_bytes of
    // it).  sorter and lines supply parse, ranks, checks and the running
    // maximum of the map stops.  Throws StarchError as include/starch_amd.h
    // describes.
    void run(sb::SortWorkspace& sorter, so::SetopWorkspace& lines, const MapelOptions& opt, const uint8_t* d_cat, uint64_t n,
             const std::vector<uint64_t>& in_end, hipStream_t st, DevBuf& out, MapelResult& res);
};

}  // namespace me
