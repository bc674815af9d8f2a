// tools/bbi_rec_check.cpp -- the record logic of bigwig2bed / bigbed2bed
// (starch_amd/csrc/bed_bbi_rec.hpp) run on the host, stage by stage as the kernels
// of bed_bbi_dev.hip run it: check, count, measure, place by a prefix sum, write.
// A plain C++ program without the device runtime, meant to be built with
// -fsanitize=address,undefined (tests/test_bbi_dev_cpu.py does): every block sits
// in a heap allocation of exactly its size and the output in one of exactly the
// measured bytes, so a read or a write past either is reported.
//
//   bbi_rec_check CASE      the case's lines to stdout; a bad block: exit status 3
//                           and  block N: reason  on stderr, nothing on stdout
//   bbi_rec_check --g FILE  FILE holds u32 bit patterns: the %g of each, a line each
// CASE (little-endian): u32 kind (1 bigWig, 2 bigBed), n_chroms, n_blocks, region
// mode, region chromId, 0; u64 region start, end; per chromosome u32 length and the
// name; per block u64 its number in the file's table, u64 length and the bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../starch_amd/csrc/bed_bbi_rec.hpp"

using namespace bbirec;

namespace {

struct Block {
    uint64_t index = 0, len = 0;
    std::unique_ptr<uint8_t[]> p;        // exactly len bytes
};

bool read_file(const char* path, std::vector<uint8_t>* out)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) out->insert(out->end(), buf, buf + k);
    fclose(f);
    return true;
}

uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }

struct Rec {               // a record found by the framing
    uint64_t block, at, len;   // bigWig: at is its number in the section; bigBed: its offset and bytes
};

int fail(uint64_t index, uint32_t kind)
{
    fprintf(stderr, "block %llu: %s\n", (unsigned long long)index, bad_text(kind));
    return 3;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "--g")) {
        std::vector<uint8_t> in;
        if (!read_file(argv[2], &in)) return 1;
        for (size_t k = 0; k + 4 <= in.size(); k += 4) {
            std::unique_ptr<uint8_t[]> t(new uint8_t[13]);     // what float_g promises to stay within
            const uint32_t n = fg::float_g(rd32(in.data() + k), t.get());
            fwrite(t.get(), 1, n, stdout);
            fputc('\n', stdout);
        }
        return 0;
    }
    if (argc != 2) return 1;
    std::vector<uint8_t> in;
    if (!read_file(argv[1], &in) || in.size() < 40) return 1;
    const uint8_t* h = in.data();
    const uint32_t kind = rd32(h), n_chroms = rd32(h + 4), n_blocks = rd32(h + 8);
    const Region rg{rd32(h + 12), rd32(h + 16), rd64(h + 24), rd64(h + 32)};
    size_t at = 40;
    std::vector<std::string> names(n_chroms);
    for (auto& nm : names) {
        const uint32_t l = rd32(h + at);
        nm.assign(reinterpret_cast<const char*>(h + at + 4), l);
        at += 4 + l;
    }
    std::vector<Block> blocks(n_blocks);
    for (auto& b : blocks) {
        b.index = rd64(h + at);
        b.len = rd64(h + at + 8);
        b.p.reset(new uint8_t[b.len]);
        memcpy(b.p.get(), h + at + 16, b.len);
        at += 16 + b.len;
    }
    // 1. every block checked and its records counted; the lowest bad block is the error
    std::vector<Rec> recs;
    for (uint64_t k = 0; k < blocks.size(); ++k) {
        const Block& b = blocks[k];
        if (kind == 1) {
            WigSec s;
            if (const uint32_t e = wig_section(b.p.get(), b.len, n_chroms, &s)) return fail(b.index, e);
            for (uint32_t i = 0; i < s.count; ++i) recs.push_back(Rec{k, i, 0});
        } else {
            for (uint64_t cur = 0, next = 0; cur < b.len; cur = next) {
                if (const uint32_t e = bed_next(b.p.get(), b.len, cur, &next)) return fail(b.index, e);
                recs.push_back(Rec{k, cur, next - cur});
            }
        }
    }
    // 2. every record checked and measured
    std::vector<uint64_t> ob(recs.size());
    for (size_t i = 0; i < recs.size(); ++i) {
        const Rec& r = recs[i];
        const Block& b = blocks[r.block];
        uint64_t s0 = 0, s1 = 0;
        uint32_t chrom = 0;
        if (kind == 1) {
            WigSec s;
            (void)wig_section(b.p.get(), b.len, n_chroms, &s);
            uint32_t bits = 0;
            if (const uint32_t e = wig_record(b.p.get(), s, (uint32_t)r.at, &s0, &s1, &bits)) return fail(b.index, e);
            chrom = s.chrom;
            ob[i] = region_keeps(rg, chrom, s0, s1) ? wig_line_len((uint32_t)names[chrom].size(), s0, s1, bits) : 0;
        } else {
            const uint8_t* p = b.p.get() + r.at;
            if (const uint32_t e = bed_record(p, n_chroms, &chrom, &s0, &s1)) return fail(b.index, e);
            if (bed_has_newline(p, kBedFixed, r.len - 1)) return fail(b.index, K_BED_NEWLINE);
            ob[i] = region_keeps(rg, chrom, s0, s1) ? bed_line_len((uint32_t)names[chrom].size(), s0, s1, r.len - kBedMinRecord) : 0;
        }
    }
    // 3. placed by an exclusive sum and written
    uint64_t total = 0;
    std::vector<uint64_t> off(recs.size());
    for (size_t i = 0; i < recs.size(); ++i) { off[i] = total; total += ob[i]; }
    std::unique_ptr<uint8_t[]> out(new uint8_t[total]);
    for (size_t i = 0; i < recs.size(); ++i) {
        if (!ob[i]) continue;
        const Rec& r = recs[i];
        const Block& b = blocks[r.block];
        uint64_t s0 = 0, s1 = 0, n = 0;
        uint32_t chrom = 0;
        if (kind == 1) {
            WigSec s;
            (void)wig_section(b.p.get(), b.len, n_chroms, &s);
            uint32_t bits = 0;
            (void)wig_record(b.p.get(), s, (uint32_t)r.at, &s0, &s1, &bits);
            const std::string& nm = names[s.chrom];
            n = wig_line_write(out.get() + off[i], reinterpret_cast<const uint8_t*>(nm.data()), (uint32_t)nm.size(), s0, s1, bits);
        } else {
            const uint8_t* p = b.p.get() + r.at;
            (void)bed_record(p, n_chroms, &chrom, &s0, &s1);
            const uint64_t rest = r.len - kBedMinRecord;
            const std::string& nm = names[chrom];
            n = bed_line_head(out.get() + off[i], reinterpret_cast<const uint8_t*>(nm.data()), (uint32_t)nm.size(), s0, s1, rest);
            memcpy(out.get() + off[i] + n, p + kBedFixed, rest);
            n += rest;
            out[off[i] + n++] = '\n';
        }
        if (n != ob[i]) {
            fprintf(stderr, "record %zu: measured %llu bytes, wrote %llu\n", i, (unsigned long long)ob[i], (unsigned long long)n);
            return 4;
        }
    }
    fwrite(out.get(), 1, total, stdout);
    return 0;
}
