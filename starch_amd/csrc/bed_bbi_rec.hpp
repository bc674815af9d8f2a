// starch_amd/csrc/bed_bbi_rec.hpp -- what bigwig2bed and bigbed2bed decide about
// the inflated bytes of a block, as __host__ __device__ functions on plain
// pointers and lengths: the check of a bigWig section and of each of its
// records, the step of a bigBed block's chain of records and the check of a
// record, the region's choice, and the text of a line (the definition:
// include/starch_amd.h).  No wave intrinsic and nothing of the device runtime:
// the kernels of bed_bbi_dev.hip are thin callers, and tools/bbi_rec_check.cpp
// runs the same functions on the host under a sanitizer.
// Every function reads only p[0, len) of what its caller names.
#pragma once
#include "float_g.hpp"

namespace bbirec {

enum : uint32_t {
    K_OK = 0, K_SEC_SHORT, K_SEC_TYPE, K_SEC_SIZE, K_CHROM, K_START_END, K_BED_SHORT, K_BED_NOZERO, K_BED_NEWLINE,
    K_BED_ORDER, K_COUNT
};

inline const char* bad_text(uint32_t k)
{
    switch (k) {
        case K_SEC_SHORT: return "the section is shorter than its 24-byte header";
        case K_SEC_TYPE: return "section type is not 1 (bedGraph), 2 (variableStep) or 3 (fixedStep)";
        case K_SEC_SIZE: return "the section's size is not what its itemCount announces";
        case K_CHROM: return "chromId is not below the chromosome count";
        case K_START_END: return "a record's start is not below its end";
        case K_BED_SHORT: return "fewer than 13 bytes are left for a record";
        case K_BED_NOZERO: return "the block does not end on a record's zero byte";
        case K_BED_NEWLINE: return "a newline in a record's rest";
        case K_BED_ORDER: return "a record's start is above its end";
        default: return "malformed block";
    }
}

constexpr uint32_t kWigHeader = 24;       // bytes of a section's header
constexpr uint32_t kBedFixed = 12;        // chromId, start, end of a bigBed record
constexpr uint32_t kBedMinRecord = 13;    // ... and the zero byte after an empty rest
constexpr uint32_t kNoChrom = 0xffffffffu;

STARCH_HD inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
STARCH_HD inline uint32_t rd32(const uint8_t* p) { return rd16(p) | (rd16(p + 2) << 16); }

STARCH_HD inline uint32_t dec_digits(uint64_t v)
{
    uint32_t d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}

// v in decimal at o; returns its digits
STARCH_HD inline uint32_t put_dec(uint8_t* o, uint64_t v)
{
    const uint32_t d = dec_digits(v);
    for (uint32_t k = d; k-- > 0;) { o[k] = (uint8_t)('0' + v % 10); v /= 10; }
    return d;
}

struct Region {            // mode 0: everything; 1: chromosome `chrom`; 2: [start, end) of it
    uint32_t mode, chrom;
    uint64_t start, end;
};

// a record on chromosome `chrom` from s to e is among the region's lines
STARCH_HD inline bool region_keeps(const Region& rg, uint32_t chrom, uint64_t s, uint64_t e)
{
    if (rg.mode == 0) return true;
    if (chrom != rg.chrom) return false;
    return rg.mode == 1 || (s < rg.end && e > rg.start);
}

// ---- bigWig ---------------------------------------------------------------------------
struct WigSec {
    uint32_t chrom, start, step, span, type, count, item;   // item: bytes of one
};

// the section p[0, len) against its own header and the chromosome count
STARCH_HD inline uint32_t wig_section(const uint8_t* p, uint64_t len, uint32_t n_chroms, WigSec* s)
{
    if (len < kWigHeader) return K_SEC_SHORT;
    s->chrom = rd32(p);
    s->start = rd32(p + 4);
    s->step = rd32(p + 12);
    s->span = rd32(p + 16);
    s->type = p[20];
    s->count = rd16(p + 22);
    if (s->type < 1 || s->type > 3) return K_SEC_TYPE;
    s->item = s->type == 1 ? 12u : (s->type == 2 ? 8u : 4u);
    if (len != (uint64_t)kWigHeader + (uint64_t)s->count * s->item) return K_SEC_SIZE;
    if (s->chrom >= n_chroms) return K_CHROM;
    return K_OK;
}

// Record i (below s.count) of the checked section p: its start and end in 64
// bits (a fixedStep start is chromStart + i * step, which may pass 2^32) and
// the bits of its value.
STARCH_HD inline uint32_t wig_record(const uint8_t* p, const WigSec& s, uint32_t i, uint64_t* a, uint64_t* b, uint32_t* bits)
{
    const uint8_t* it = p + kWigHeader + (uint64_t)i * s.item;
    if (s.type == 1) {
        *a = rd32(it);
        *b = rd32(it + 4);
        *bits = rd32(it + 8);
    } else if (s.type == 2) {
        *a = rd32(it);
        *b = *a + s.span;
        *bits = rd32(it + 4);
    } else {
        *a = (uint64_t)s.start + (uint64_t)i * s.step;
        *b = *a + s.span;
        *bits = rd32(it);
    }
    return *a < *b ? (uint32_t)K_OK : (uint32_t)K_START_END;
}

// bytes of the line  name TAB start TAB end TAB value NL
STARCH_HD inline uint64_t wig_line_len(uint32_t name_len, uint64_t a, uint64_t b, uint32_t bits)
{
    uint8_t t[16];
    return (uint64_t)name_len + dec_digits(a) + dec_digits(b) + fg::float_g(bits, t) + 4;
}

// the line at o, which has wig_line_len bytes; returns them
STARCH_HD inline uint64_t wig_line_write(uint8_t* o, const uint8_t* name, uint32_t name_len, uint64_t a, uint64_t b, uint32_t bits)
{
    uint64_t n = 0;
    for (uint32_t k = 0; k < name_len; ++k) o[n++] = name[k];
    o[n++] = '\t';
    n += put_dec(o + n, a);
    o[n++] = '\t';
    n += put_dec(o + n, b);
    o[n++] = '\t';
    uint8_t t[16];
    const uint32_t g = fg::float_g(bits, t);
    for (uint32_t k = 0; k < g; ++k) o[n++] = t[k];
    o[n++] = '\n';
    return n;
}

// ---- bigBed ---------------------------------------------------------------------------
// the first zero byte of p[lo, hi), or hi
STARCH_HD inline uint64_t bed_first_zero(const uint8_t* p, uint64_t lo, uint64_t hi)
{
    for (uint64_t q = lo; q < hi; ++q)
        if (p[q] == 0) return q;
    return hi;
}

// a record may begin at cur (below len) of a block of len bytes
STARCH_HD inline uint32_t bed_room(uint64_t len, uint64_t cur) { return len - cur < kBedMinRecord ? (uint32_t)K_BED_SHORT : (uint32_t)K_OK; }

// the record that begins at cur ends on the zero byte z (the first at cur + 12 or after; len: none)
STARCH_HD inline uint32_t bed_close(uint64_t len, uint64_t z, uint64_t* next)
{
    if (z >= len) return K_BED_NOZERO;
    *next = z + 1;
    return K_OK;
}

// The chain's step: the record at cur of the block p[0, len) and where the next
// one begins; the block ends exactly where *next == len.
STARCH_HD inline uint32_t bed_next(const uint8_t* p, uint64_t len, uint64_t cur, uint64_t* next)
{
    if (const uint32_t k = bed_room(len, cur)) return k;
    return bed_close(len, bed_first_zero(p, cur + kBedFixed, len), next);
}

// the fixed fields of the record p[0, 13 + rest)
STARCH_HD inline uint32_t bed_record(const uint8_t* p, uint32_t n_chroms, uint32_t* chrom, uint64_t* a, uint64_t* b)
{
    *chrom = rd32(p);
    *a = rd32(p + 4);
    *b = rd32(p + 8);
    if (*chrom >= n_chroms) return K_CHROM;
    return *a <= *b ? (uint32_t)K_OK : (uint32_t)K_BED_ORDER;
}

STARCH_HD inline bool bed_has_newline(const uint8_t* p, uint64_t lo, uint64_t hi)
{
    for (uint64_t q = lo; q < hi; ++q)
        if (p[q] == '\n') return true;
    return false;
}

// bytes of the line  name TAB start TAB end [TAB rest] NL
STARCH_HD inline uint64_t bed_line_len(uint32_t name_len, uint64_t a, uint64_t b, uint64_t rest)
{
    return (uint64_t)name_len + dec_digits(a) + dec_digits(b) + 3 + (rest ? rest + 1 : 0);
}

// the line's bytes before the rest (the TAB in front of a rest that is not empty included); returns them
STARCH_HD inline uint64_t bed_line_head(uint8_t* o, const uint8_t* name, uint32_t name_len, uint64_t a, uint64_t b, uint64_t rest)
{
    uint64_t n = 0;
    for (uint32_t k = 0; k < name_len; ++k) o[n++] = name[k];
    o[n++] = '\t';
    n += put_dec(o + n, a);
    o[n++] = '\t';
    n += put_dec(o + n, b);
    if (rest) o[n++] = '\t';
    return n;
}

}  // namespace bbirec
