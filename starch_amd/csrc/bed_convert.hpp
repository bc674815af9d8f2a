// starch_amd/csrc/bed_convert.hpp -- host interface of convert2bed
// (bed_convert.hip): GFF3, GTF, VCF and WIG text into BED lines, unsorted.
#pragma once
#include "bed_records.hpp"

namespace cv {

constexpr int kThreads = br::kThreads;  // threads per block of the per-line kernels (one line each)
constexpr uint32_t kSlots = 10;         // 32-bit offsets kept per line (field starts, the ID, a declaration's record)

struct ConvertOptions {                 // checked by the caller (api_bed.hip)
    uint32_t format = 0;                // STARCH_CONVERT_*
    uint32_t vcf_class = 0;             // STARCH_VCF_*
    uint32_t keep_header = 0;
};

struct ConvertResult {
    uint64_t n_lines = 0, header_lines = 0, data_lines = 0, declarations = 0, lines_out = 0, out_bytes = 0;
    float ms_frame = 0, ms_parse = 0, ms_write = 0;
};

struct ConvertWorkspace {
    br::Buffers rb;
    DevBuf b_aux, b_pk, b_dmax;         // WIG
    StageTimer<4> timer;
    // The text d_in[0, n) in the format of opt, converted line by line as
    // include/starch_amd.h defines, into out (res.out_bytes of it, in input
    // order).  sorter supplies the framing (stage_frame) and is free again when
    // run returns.  Throws StarchError: STARCH_ERR_DATA naming the lowest line
    // that does not fit its format, STARCH_ERR_ARG for 2^32 lines or more.
    void run(sb::SortWorkspace& sorter, const ConvertOptions& opt, const uint8_t* d_in, uint64_t n, hipStream_t st, DevBuf& out,
             ConvertResult& res);
};

}  // namespace cv
