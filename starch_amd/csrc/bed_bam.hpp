// starch_amd/csrc/bed_bam.hpp -- host interface of bam2bed (bed_bam.hip): inflated
// BAM in HBM into the BED lines that sam2bed writes for its SAM text, unsorted.
#pragma once
#include "bed_records.hpp"
#include "float_g.hpp"

namespace bam {

constexpr uint32_t kTileBytes = 16384;      // T: the framing's tile; tile t is the bytes [t * T, (t + 1) * T) of the inflated file
constexpr int kTableThreads = 1024;         // threads of the block that makes one tile's table
constexpr uint32_t kBatchTiles = 8192;      // tiles whose tables are in HBM at a time (2 * T bytes each: 256 MiB)
constexpr int kThreads = br::kThreads;      // threads per block of the per-record kernels (one record each)
constexpr uint32_t kWaveThreshold = 1024;   // W: an l_seq or a B count from which a record's text is left to a whole wave
constexpr uint32_t kMinRecord = 36;         // block_size (4 bytes) and the 32 fixed bytes it counts at least

struct BamOptions {                         // checked by the caller (api_bed.hip)
    uint32_t split = 0, split_deletions = 0, all_reads = 0, reduced = 0, keep_header = 0;
};

struct BamResult {
    uint64_t references = 0, header_lines = 0, records = 0, unmapped_dropped = 0, tiles = 0, wave_records = 0, lines_out = 0,
             out_bytes = 0;
    float ms_frame = 0, ms_parse = 0, ms_write = 0;
};

struct BamWorkspace {
    br::Buffers rb;
    DevBuf table, entry, count, base, rec_off, rest, names, header, fstate;
    StageTimer<4> timer;
    // The inflated BAM d_in[0, n), converted record by record as
    // include/starch_amd.h defines, into out (res.out_bytes of it: the kept header
    // lines, then the records in input order).  Throws StarchError:
    // STARCH_ERR_DATA for an input that is not BAM, a bad header, or naming the
    // lowest bad record; STARCH_ERR_ARG for 2^32 records or output lines or more.
    void run(const BamOptions& opt, const uint8_t* d_in, uint64_t n, hipStream_t st, DevBuf& out, BamResult& res);
};

using fg::float_g;   // float_g.hpp: the %g of a float32, exactly

}  // namespace bam
