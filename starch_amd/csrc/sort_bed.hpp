// starch_amd/csrc/sort_bed.hpp -- host interface of the BED sort (sort_bed.hip).
#pragma once
#include <string>

#include "common.hpp"

namespace sb {

constexpr int kSortThreads = 256;
constexpr int kSortItems = 16;                           // keys per thread of a radix tile
constexpr int kSortTile = kSortThreads * kSortItems;     // lines per histogram / scatter tile
constexpr uint32_t kWaveCopyBytes = 256;                 // output lines (with '\n') this long or longer are copied by a whole wave

struct SortResult {
    uint64_t n_lines = 0, n_chromosomes = 0, out_bytes = 0;
    uint64_t first_unsorted_line = 0;   // 1-based; 0: the input is in order
    bool already_sorted = true;
    uint32_t radix_passes = 0;
    float ms_parse = 0, ms_rank = 0, ms_sort = 0, ms_gather = 0, ms_total = 0;
};

struct SortWorkspace {
    DevBuf b_tile_cnt, b_tile_off, b_scal, b_tmp, b_line_end, b_start, b_stop, b_chr_len, b_hash, b_rank, b_keys, b_rep,
        b_ent, b_names, b_name_dst, b_slot_rank, b_idx[2], b_digit, b_hist, b_hist_off, b_len, b_out_off;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // Sorts the BED bytes d_bed[0, n) into out (res.out_bytes of it); check_only
    // stops after the order check and leaves out alone.  Throws StarchError
    // (STARCH_ERR_DATA naming the first malformed line, STARCH_ERR_ARG for 2^32
    // lines or more).
    void run(const uint8_t* d_bed, uint64_t n, hipStream_t st, bool check_only, DevBuf& out, SortResult& res);
    ~SortWorkspace();
};

}  // namespace sb
