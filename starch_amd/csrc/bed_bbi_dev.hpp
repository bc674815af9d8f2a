// starch_amd/csrc/bed_bbi_dev.hpp -- host interface of bigwig2bed / bigbed2bed
// (bed_bbi_dev.hip): the inflated blocks of a bigWig / bigBed file in HBM into
// BED lines, unsorted, in block order.
#pragma once
#include <string>
#include <vector>

#include "bed_bbi_rec.hpp"
#include "common.hpp"

namespace bbidev {

constexpr int kThreads = 256;               // threads per block of the per-record kernels (one record each)
constexpr uint32_t kWaveRest = 1024;        // bytes of a bigBed record's rest from which its whole wave checks and copies it
constexpr uint32_t kChainWindow = 1024;     // bytes a wave looks through per step of a bigBed block's chain (16 per lane)

struct Input {                              // the blocks to convert: block k is d[off[k], off[k] + len[k])
    uint32_t kind = 0;                      // bbi::KIND_BIGWIG or KIND_BIGBED
    const uint8_t* d = nullptr;
    std::vector<uint64_t> off, len;
    std::vector<uint64_t> index;            // block k's number in the file's table, for messages
    std::vector<std::string> chroms;        // names by chromId
    bbirec::Region rg{0, 0, 0, 0};
};

struct Result {
    uint64_t blocks = 0, records = 0, wave_records = 0, lines_out = 0, out_bytes = 0;
    float ms_frame = 0, ms_parse = 0, ms_write = 0;
};

struct Workspace {
    DevBuf boff, blen, cnt, base, scal, tmp, rec_off, rec_len, ob, off, names;
    StageTimer<4> timer;
    // in's blocks, checked and converted as include/starch_amd.h defines, into
    // out (res.out_bytes of it).  Throws StarchError: STARCH_ERR_DATA naming the
    // lowest bad block, with nothing written; STARCH_ERR_ARG for 2^32 records
    // or more.
    void run(const Input& in, hipStream_t st, DevBuf& out, Result& res);
};

}  // namespace bbidev
