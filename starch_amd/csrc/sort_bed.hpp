// starch_amd/csrc/sort_bed.hpp -- host interface of the BED sort (sort_bed.hip).
#pragma once
#include <string>
#include <vector>

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

// OR and AND of every key word over the lines (a byte whose OR equals its AND
// is the same in every line), and the first line whose key is below its
// predecessor's (~0: none)
struct KeyBits {
    uint64_t or_rank = 0, and_rank = 0, or_start = 0, and_start = 0, or_stop = 0, and_stop = 0, desc = ~0ull;
};

// what is wrong with a malformed line: the low byte of stage_parse's *bad
const char* bad_text(uint32_t kind);

struct SortWorkspace {
    DevBuf b_tile_cnt, b_tile_off, b_scal, b_tmp, b_line_end, b_start, b_stop, b_chr_len, b_hash, b_rank, b_keys, b_rep,
        b_ent, b_names, b_name_dst, b_slot_rank, b_idx[2], b_digit, b_hist, b_hist_off, b_len, b_out_off;
    StageTimer<5> timer;
    // Sorts the BED bytes d_bed[0, n) into out (res.out_bytes of it); check_only
    // stops after the order check and leaves out alone.  Throws StarchError
    // (STARCH_ERR_DATA naming the first malformed line, STARCH_ERR_ARG for 2^32
    // lines or more).
    void run(const uint8_t* d_bed, uint64_t n, hipStream_t st, bool check_only, DevBuf& out, SortResult& res);

    // The stages of run(), for callers that put their own work between them
    // (bed_setops.hip).  Per-line arrays of the last stage_parse, in HBM:
    struct Lines {
        uint64_t L = 0;
        bool open_end = false;                          // the last line had no '\n'
        uint64_t *line_end = nullptr, *start = nullptr, *stop = nullptr;
        uint32_t *chr_len = nullptr, *rank = nullptr;   // rank: after stage_rank
    } ln;
    uint64_t n_chromosomes = 0;                // after stage_rank
    std::vector<uint64_t> chrom_off;           // by rank: the name's bytes in d_bed (its representative line's)
    std::vector<uint32_t> chrom_len;
    // 1a. line ends of d_bed[0, n), n > 0, cut at '\n': ln.L, ln.open_end and
    // ln.line_end alone (bed_convert.hip frames text that is not BED yet).
    // Returns the number of lines.
    uint64_t stage_frame(const uint8_t* d_bed, uint64_t n, hipStream_t st);
    // 1. stage_frame and the parse of every line.  Returns the number of
    // lines; *bad is ~0, or (line << 8) | kind of the first malformed line.
    uint64_t stage_parse(const uint8_t* d_bed, uint64_t n, hipStream_t st, uint64_t* bad);
    // 2. chromosome ranks of the parsed lines (none of them malformed)
    void stage_rank(const uint8_t* d_bed, hipStream_t st);
    // 3. key bits and first descent of any L keys (stop may equal start's array)
    KeyBits stage_check(const uint32_t* rank, const uint64_t* start, const uint64_t* stop, uint64_t L, hipStream_t st);
    // 4. stable radix order of L < 2^32 keys (rank, start, stop), skipping the
    // bytes kb says are constant; stop == nullptr: (rank, start) alone.  Returns
    // the permutation (position -> key index), or nullptr when no byte varies
    // and the order is the input's.
    const uint32_t* stage_radix(const uint32_t* rank, const uint64_t* start, const uint64_t* stop, uint64_t L,
                                const KeyBits& kb, hipStream_t st, uint32_t* passes);
    // 5. the K parsed lines order[0, K) (line indices of the last stage_parse),
    // whole and each ending in '\n', one after the other into out.  bytes: their
    // total when the caller knows it, ~0: it is read back from the scan of their
    // lengths.  long_list: K entries of scratch that are not order's (nullptr:
    // the workspace's own).  Returns the total.
    uint64_t stage_gather(const uint8_t* d_bed, const uint32_t* order, uint64_t K, uint64_t bytes, uint32_t* long_list,
                          hipStream_t st, DevBuf& out);
    DevBuf b_long;
};

}  // namespace sb
