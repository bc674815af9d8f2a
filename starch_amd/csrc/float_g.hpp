// starch_amd/csrc/float_g.hpp -- C's %g of a float32 in integer arithmetic, for
// kernels and host code alike (bed_bam.hip's f tags, bed_bbi_rec.hpp's bigWig
// values).  It includes nothing of the device runtime, so a plain C++ compiler
// takes it too: STARCH_HD is __host__ __device__ under hipcc and empty elsewhere.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define STARCH_HD __host__ __device__
#else
#define STARCH_HD
#endif

namespace fg {

// C's %g of the float32 with the bits `bits`, into o (13 bytes are enough);
// returns its length.  Exact for every bit pattern: the value m * 2^e is made a
// whole number in limbs of 10^9 -- m * 2^e itself, or for e < 0 m * 5^-e, which is
// the value times 10^-e -- and its six leading digits are rounded to nearest, ties
// to even, on all the digits below them.  No floating-point instruction.  A NaN
// prints nan whatever its sign.
STARCH_HD inline uint32_t float_g(uint32_t bits, uint8_t* o)
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

}  // namespace fg
