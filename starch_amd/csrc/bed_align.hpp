// starch_amd/csrc/bed_align.hpp -- host interface of sam2bed, psl2bed and rmsk2bed
// (bed_align.hip): SAM, PSL and RepeatMasker .out text into BED lines, unsorted.
#pragma once
#include "bed_records.hpp"

namespace al {

constexpr int kThreads = br::kThreads;  // threads per block of the per-line kernels (one line each)
constexpr uint32_t kSlotsSam = 6;       // 32-bit values kept per SAM line: the starts of fields 2 to 6, FLAG
constexpr uint32_t kSlotsPsl = 20;      // per PSL line: the starts of fields 2 to 21 (a RepeatMasker line keeps none)

struct AlignOptions {                   // checked by the caller (api_bed.hip)
    uint32_t format = 0;                // STARCH_ALIGN_*
    uint32_t split = 0, split_deletions = 0, all_reads = 0, reduced = 0, keep_header = 0;
};

struct AlignResult {
    uint64_t n_lines = 0, header_lines = 0, records = 0, unmapped_dropped = 0, lines_out = 0, out_bytes = 0;
    float ms_frame = 0, ms_parse = 0, ms_write = 0;
};

// the command that converts a format ("sam2bed", ...): the prefix of its error texts
const char* command_of(uint32_t format);

struct AlignWorkspace {
    br::Buffers rb;
    StageTimer<4> timer;
    // The text d_in[0, n) in the format of opt, converted line by line as
    // include/starch_amd.h defines, into out (res.out_bytes of it, in input
    // order).  sorter supplies the framing (stage_frame) and is free again when
    // run returns.  Throws StarchError: STARCH_ERR_DATA naming the lowest line
    // that does not fit its format, STARCH_ERR_ARG for 2^32 lines or more.
    void run(sb::SortWorkspace& sorter, const AlignOptions& opt, const uint8_t* d_in, uint64_t n, hipStream_t st, DevBuf& out,
             AlignResult& res);
};

}  // namespace al
