// starch_amd/csrc/bed_bbi.hpp -- the host's reading of a bigWig / bigBed file
// (bed_bbi.hip): the header, the chromosome B+ tree, the R-tree's block table,
// and the blocks a region needs.  Host only; no device is touched.
#pragma once
#include <string>
#include <vector>

#include "common.hpp"

namespace bbi {

constexpr uint32_t kBigWigMagic = 0x888FFC26u, kBigBedMagic = 0x8789F2EBu;
constexpr uint32_t kChromTreeMagic = 0x78CA8C91u, kRTreeMagic = 0x2468ACE0u;

enum : uint32_t { KIND_AUTO = 0, KIND_BIGWIG = 1, KIND_BIGBED = 2 };

struct Chrom {
    std::string name;
    uint32_t size = 0;
};

struct Block {                 // a leaf item of the R-tree
    uint32_t start_chrom, start_base, end_chrom, end_base;
    uint64_t data_offset, data_size;
};

struct Info {                  // what the host reads of a file
    uint32_t kind = 0, version = 0, zoom_levels = 0, field_count = 0, defined_field_count = 0, uncompress_buf_size = 0;
    uint64_t chrom_tree_offset = 0, full_data_offset = 0, full_index_offset = 0;
    std::vector<Chrom> chroms;             // by chromId
    std::vector<Block> blocks;             // by data_offset
};

struct Region {                // none, a whole chromosome, or [start, end) of one
    bool any = false, whole = true;
    std::string chrom;
    uint64_t start = 0, end = 0;
};

// The header, the chromosome B+ tree and the R-tree of file[0, n), every
// offset and count checked against n before it is used.  Throws StarchError
// (STARCH_ERR_DATA) that names what is wrong.
void parse(const uint8_t* file, uint64_t n, Info& info);

// The indices into info.blocks of the blocks whose box meets the region, in
// order; all of them without a region, none for a chromosome the file lacks.
// *chrom_id: the region's chromosome, or -1.
std::vector<uint64_t> select(const Info& info, const Region& rg, int64_t* chrom_id);

}  // namespace bbi
