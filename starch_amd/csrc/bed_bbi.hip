// starch_amd/csrc/bed_bbi.hip -- the host's reading of a bigWig / bigBed file (the
// definition: include/starch_amd.h): the 64-byte header, the chromosome B+ tree
// and the R-tree are walked with explicit stacks, every offset and count checked
// against the file size; the R-tree's leaves are the block table, and a region
// chooses the blocks whose box meets it.  Host code only: nothing here launches
// a kernel.  The inputs are untrusted.
#include "bed_bbi.hpp"

#include <string.h>

#include <algorithm>
#include <unordered_set>
#include <utility>

#include "../../include/starch_amd.h"

namespace bbi {
namespace {

[[noreturn]] void bad_file(const std::string& why) { throw StarchError(STARCH_ERR_DATA, "bbi: " + why); }

struct Reader {
    const uint8_t* f;
    uint64_t n;
    void need(uint64_t off, uint64_t len, const char* what) const
    {
        if (off > n || len > n - off) bad_file(std::string(what) + " lies past the end of the file (offset " + std::to_string(off) + ")");
    }
    uint32_t u16(uint64_t o) const { return (uint32_t)f[o] | ((uint32_t)f[o + 1] << 8); }
    uint32_t u32(uint64_t o) const { return u16(o) | (u16(o + 2) << 16); }
    uint64_t u64(uint64_t o) const { return (uint64_t)u32(o) | ((uint64_t)u32(o + 4) << 32); }
};

uint32_t swap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// The nodes of a tree from root on, each once: leaf(off, count) or inner(off,
// count) is called with the offset of its first item; inner returns the child
// offsets through push.  The nodes of a tree are disjoint byte ranges of the
// file, so the bytes of the visited nodes (4 + count * item size each) are
// budgeted against the file size n, and a node that exceeds what is left ends
// the walk with an error before its children are pushed.  That bounds the walk
// whatever the offsets say: at most n / 4 nodes are visited, at most n / item
// size items are read, and the stack, which holds only items of visited inner
// nodes, never has more than n / inner_item entries.  A node reached twice (a
// child offset that points at itself or at an ancestor) is named as such.
template <class Leaf, class Inner>
void walk_tree(const Reader& rd, uint64_t root, uint64_t leaf_item, uint64_t inner_item, const char* what, Leaf leaf, Inner inner)
{
    std::vector<uint64_t> stack{root};
    std::unordered_set<uint64_t> seen;
    uint64_t budget = rd.n;
    while (!stack.empty()) {
        const uint64_t off = stack.back();
        stack.pop_back();
        if (!seen.insert(off).second) bad_file(std::string(what) + ": the node at offset " + std::to_string(off) + " is reached twice");
        rd.need(off, 4, what);
        const bool is_leaf = rd.f[off] != 0;
        const uint64_t count = rd.u16(off + 2);
        const uint64_t bytes = 4 + count * (is_leaf ? leaf_item : inner_item);   // (count < 2^16, an item is below 2^33: no overflow)
        rd.need(off, bytes, what);
        if (bytes > budget)
            bad_file(std::string(what) + ": its nodes overlap (together they claim more bytes than the file holds, at offset " +
                     std::to_string(off) + ")");
        budget -= bytes;
        if (is_leaf) leaf(off + 4, count);
        else {
            const size_t at = stack.size();
            inner(off + 4, count, stack);
            std::reverse(stack.begin() + at, stack.end());   // (the first child is visited first)
        }
    }
}

}  // namespace

void parse(const uint8_t* file, uint64_t n, Info& info)
{
    info = Info{};
    const Reader rd{file, n};
    if (n < 4) bad_file("the file is truncated (it has no magic)");
    const uint32_t magic = rd.u32(0);
    if (magic == kBigWigMagic) info.kind = KIND_BIGWIG;
    else if (magic == kBigBedMagic) info.kind = KIND_BIGBED;
    else if (swap32(magic) == kBigWigMagic || swap32(magic) == kBigBedMagic) bad_file("big-endian bigWig/bigBed is not supported");
    else bad_file("not a bigWig or bigBed file (bad magic)");
    if (n < 64) bad_file("the file is truncated (the header needs 64 bytes)");
    info.version = rd.u16(4);
    info.zoom_levels = rd.u16(6);
    info.chrom_tree_offset = rd.u64(8);
    info.full_data_offset = rd.u64(16);
    info.full_index_offset = rd.u64(24);
    info.field_count = rd.u16(32);
    info.defined_field_count = rd.u16(34);
    info.uncompress_buf_size = rd.u32(52);
    rd.need(64, 24ull * info.zoom_levels, "the zoom headers");
    rd.need(info.chrom_tree_offset, 32, "the chromosome tree (chromosomeTreeOffset)");
    rd.need(info.full_index_offset, 48, "the R-tree (fullIndexOffset)");
    if (info.full_data_offset > info.full_index_offset) bad_file("fullDataOffset lies past fullIndexOffset");

    // the chromosome B+ tree
    const uint64_t ct = info.chrom_tree_offset;
    if (rd.u32(ct) != kChromTreeMagic) bad_file("the chromosome tree has a bad magic");
    const uint64_t key_size = rd.u32(ct + 8), val_size = rd.u32(ct + 12), n_chrom = rd.u64(ct + 16);
    if (val_size != 8) bad_file("the chromosome tree's valSize is not 8");
    if (key_size == 0 || key_size > n) bad_file("the chromosome tree's keySize is 0 or exceeds the file");
    if (n_chrom > n / (key_size + 8)) bad_file("the chromosome tree's itemCount (" + std::to_string(n_chrom) + ") is more than the file can hold");
    // One byte per announced id here; the names are kept as they are found (the
    // walk's budget bounds them by the file's bytes) and placed by id afterwards.
    std::vector<uint8_t> have(n_chrom, 0);
    std::vector<std::pair<uint32_t, Chrom>> found;
    if (n_chrom)
        walk_tree(rd, ct + 32, key_size + 8, key_size + 8, "the chromosome tree",
                  [&](uint64_t at, uint64_t count) {
                      for (uint64_t k = 0; k < count; ++k, at += key_size + 8) {
                          const uint32_t id = rd.u32(at + key_size);
                          if (id >= n_chrom) bad_file("chromosome id " + std::to_string(id) + " is not below itemCount");
                          if (have[id]) bad_file("chromosome id " + std::to_string(id) + " appears twice");
                          have[id] = 1;
                          const void* z = memchr(file + at, 0, key_size);
                          const uint64_t len = z ? (uint64_t)(static_cast<const uint8_t*>(z) - (file + at)) : key_size;
                          if (len == 0) bad_file("chromosome id " + std::to_string(id) + " has an empty name");
                          if (memchr(file + at, '\t', len) || memchr(file + at, '\n', len))
                              bad_file("chromosome id " + std::to_string(id) + " has a TAB or a newline in its name");
                          found.emplace_back(id, Chrom{std::string(reinterpret_cast<const char*>(file + at), len), rd.u32(at + key_size + 4)});
                      }
                  },
                  [&](uint64_t at, uint64_t count, std::vector<uint64_t>& stack) {
                      for (uint64_t k = 0; k < count; ++k, at += key_size + 8) stack.push_back(rd.u64(at + key_size));
                  });
    for (uint64_t id = 0; id < n_chrom; ++id)
        if (!have[id]) bad_file("chromosome id " + std::to_string(id) + " is missing");
    info.chroms.resize(n_chrom);             // (every id was found once: as many names as the file holds)
    for (auto& f : found) info.chroms[f.first] = std::move(f.second);

    // the R-tree: its leaf items are the block table
    const uint64_t rt = info.full_index_offset;
    if (rd.u32(rt) != kRTreeMagic) bad_file("the R-tree has a bad magic");
    const uint64_t n_items = rd.u64(rt + 8);
    if (n_items > n / 32) bad_file("the R-tree's itemCount (" + std::to_string(n_items) + ") is more than the file can hold");
    if (n_items)
        walk_tree(rd, rt + 48, 32, 24, "the R-tree",
                  [&](uint64_t at, uint64_t count) {
                      for (uint64_t k = 0; k < count; ++k, at += 32) {
                          if (info.blocks.size() == n_items) bad_file("the R-tree holds more leaf items than its itemCount");
                          info.blocks.push_back(Block{rd.u32(at), rd.u32(at + 4), rd.u32(at + 8), rd.u32(at + 12), rd.u64(at + 16), rd.u64(at + 24)});
                      }
                  },
                  [&](uint64_t at, uint64_t count, std::vector<uint64_t>& stack) {
                      for (uint64_t k = 0; k < count; ++k, at += 24) stack.push_back(rd.u64(at + 16));
                  });
    if (info.blocks.size() != n_items)
        bad_file("the R-tree holds " + std::to_string(info.blocks.size()) + " leaf items, its itemCount says " + std::to_string(n_items));
    std::stable_sort(info.blocks.begin(), info.blocks.end(), [](const Block& a, const Block& b) { return a.data_offset < b.data_offset; });
    for (uint64_t k = 0; k < info.blocks.size(); ++k) {
        const Block& b = info.blocks[k];
        if (b.data_offset < info.full_data_offset || b.data_offset > info.full_index_offset || b.data_size > info.full_index_offset - b.data_offset)
            bad_file("block " + std::to_string(k) + " at byte " + std::to_string(b.data_offset) + " lies outside [fullDataOffset, fullIndexOffset)");
        if (b.data_size >= (1ull << 32)) bad_file("block " + std::to_string(k) + " has 2^32 bytes or more");
        if (k && info.blocks[k - 1].data_offset + info.blocks[k - 1].data_size > b.data_offset)
            bad_file("blocks " + std::to_string(k - 1) + " and " + std::to_string(k) + " overlap");
    }
}

std::vector<uint64_t> select(const Info& info, const Region& rg, int64_t* chrom_id)
{
    std::vector<uint64_t> sel;
    *chrom_id = -1;
    if (!rg.any) {
        sel.resize(info.blocks.size());
        for (uint64_t k = 0; k < sel.size(); ++k) sel[k] = k;
        return sel;
    }
    for (uint64_t id = 0; id < info.chroms.size(); ++id)
        if (info.chroms[id].name == rg.chrom) { *chrom_id = (int64_t)id; break; }
    if (*chrom_id < 0) return sel;
    typedef std::pair<uint64_t, uint64_t> P;
    const P qs((uint64_t)*chrom_id, rg.whole ? 0 : rg.start), qe((uint64_t)*chrom_id, rg.whole ? 1ull << 32 : rg.end);
    for (uint64_t k = 0; k < info.blocks.size(); ++k) {
        const Block& b = info.blocks[k];
        if (P(b.start_chrom, b.start_base) < qe && P(b.end_chrom, b.end_base) > qs) sel.push_back(k);
    }
    return sel;
}

}  // namespace bbi
