// starch_amd/csrc/bed_bam.hpp -- host interface of bam2bed (bed_bam.hip): inflated
// BAM in HBM into the BED lines that sam2bed writes for its SAM text, unsorted; and
// the %g of a float32 in integer arithmetic, which host code may call too.
#pragma once
#include "bed_records.hpp"

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

// C's %g of the float32 with the bits `bits`, into o (13 bytes are enough);
// returns its length.  Exact for every bit pattern: the value m * 2^e is made a
// whole number in limbs of 10^9 -- m * 2^e itself, or for e < 0 m * 5^-e, which is
// the value times 10^-e -- and its six leading digits are rounded to nearest, ties
// to even, on all the digits below them.  No floating-point instruction.  A NaN
// prints nan whatever its sign.
__host__ __device__ inline uint32_t float_g(uint32_t bits, uint8_t* o)
{
    constexpr uint32_t kBase = 1000000000u;
    uint32_t n = 0;
    const uint32_t ex = (bits >> 23) & 255u, fr = bits & 0x7fffffu;
    if (ex == 255u && fr) { o[0] = 'n'; o[1] = 'a'; o[2] = 'n'; return 3; }
    if (bits >> 31) o[n++] = '-';
    if (ex == 255u) { o[n] = 'i'; o[n + 1] = 'n'; o[n + 2] = 'f'; return n + 3; }
    if (!ex && !fr) { o[n++] = '0'; return n; }
    const uint32_t m = ex ? (fr | 0x800000u) : fr;
    const int e = (ex ? (int)ex : 1) - 150;                  // the value is m * 2^e
    uint32_t L[13] = {m};                                    // m * 5^149 has 112 digits; 13 limbs hold 117
    int hi = 0;
    for (int left = e < 0 ? -e : e; left;) {
        const int step = left < (e < 0 ? 13 : 29) ? left : (e < 0 ? 13 : 29);   // 5^13 < 2^31, a limb < 2^30: below 2^62
        uint64_t mul = 1;
        for (int k = 0; k < step; ++k) mul *= e < 0 ? 5u : 2u;
        uint64_t carry = 0;
        for (int k = 0; k <= hi; ++k) {
            const uint64_t v = (uint64_t)L[k] * mul + carry;
            L[k] = (uint32_t)(v % kBase);
            carry = v / kBase;
        }
        while (carry) { L[++hi] = (uint32_t)(carry % kBase); carry /= kBase; }
        left -= step;
    }
    auto p10 = [](int k) { uint64_t v = 1; while (k-- > 0) v *= 10; return v; };
    int vd = 1;                                              // digits of V: the top limb, and the one below it when there is one
    for (uint32_t t = L[hi]; t >= 10; t /= 10) ++vd;
    int E = 9 * hi + vd - 1 - (e < 0 ? -e : 0);              // the decimal exponent of the leading digit
    uint64_t V = L[hi];
    bool sticky = false;
    if (hi) {
        V = V * kBase + L[hi - 1];
        vd += 9;
        for (int k = 0; k + 1 < hi; ++k) sticky |= L[k] != 0;
    }
    uint64_t D;
    if (vd <= 6) D = V * p10(6 - vd);
    else {
        const uint64_t q = p10(vd - 6), rem = V % q, half = q / 2;
        D = V / q;
        if (rem > half || (rem == half && (sticky || (D & 1)))) ++D;
        if (D == 1000000) { D = 100000; ++E; }
    }
    uint8_t d[6];
    for (int k = 6; k-- > 0; D /= 10) d[k] = (uint8_t)('0' + D % 10);
    int last = 5;                                            // trailing zeros are stripped
    while (last > 0 && d[last] == '0') --last;
    if (E < -4 || E >= 6) {
        o[n++] = d[0];
        if (last > 0) {
            o[n++] = '.';
            for (int k = 1; k <= last; ++k) o[n++] = d[k];
        }
        const int a = E < 0 ? -E : E;                        // at most 45
        o[n++] = 'e';
        o[n++] = E < 0 ? '-' : '+';
        o[n++] = (uint8_t)('0' + a / 10);
        o[n++] = (uint8_t)('0' + a % 10);
    } else if (E >= 0) {
        for (int k = 0; k <= E; ++k) o[n++] = d[k];
        if (last > E) {
            o[n++] = '.';
            for (int k = E + 1; k <= last; ++k) o[n++] = d[k];
        }
    } else {
        o[n++] = '0';
        o[n++] = '.';
        for (int k = -E - 1; k > 0; --k) o[n++] = '0';
        for (int k = 0; k <= last; ++k) o[n++] = d[k];
    }
    return n;
}

}  // namespace bam
