// starch_amd/csrc/gz_adler.hpp -- Adler-32 (RFC 1950) from pieces: __host__
// __device__ functions, so that a kernel over the inflated blocks of a bigWig /
// bigBed file and the host run the same arithmetic: k_tab_adler (gz_inflate.hip) on the
// device, starch_bbi_adler32_host (api_bed.hip) on the host.
//
// A piece x[0, n) is summed without the leading 1 of Adler-32:
//   a = sum x[i],   w = sum i * x[i],   b = n * a - w = sum (n - i) * x[i]
// and kept as (a mod M, b mod M, n) with M = 65521.  Two pieces side by side
// fold as adler32_combine does: a = a1 + a2, b = b1 + n2 * a1 + b2 (mod M).  The
// Adler-32 of the whole is s1 = 1 + a, s2 = n + b (mod M), s2 << 16 | s1.
//
// Widths.  a and w are accumulated unreduced in 64 bits: for bytes of 0xff a
// piece of n bytes gives a = 255 n and w = 255 n (n - 1) / 2, which stays below
// 2^64 for every n up to kAdlerMaxPiece = 2^20 (w < 2^48), and n * a < 2^48
// too.  (zlib's 32-bit s2 is safe for 5552 bytes only; nothing here is 32 bits
// wide before it has been reduced.)  After the reduction every value is below
// M < 2^16, and a fold multiplies (n2 mod M) * a1 < 2^32 in 64 bits.  A piece
// of kAdlerPiece bytes is meant for one wave: a lane sums 16-byte runs 1024
// bytes apart, at most 255 * 64 in a and 255 * 64 * 4095 in w per lane.
#pragma once
#include "common.hpp"

namespace gz {

constexpr uint32_t kAdlerMod = 65521;
constexpr uint32_t kAdlerPiece = 4096;           // bytes of a piece meant for one wave
constexpr uint32_t kAdlerLanes = 64;             // shares of a piece
constexpr uint32_t kAdlerRun = 16;               // consecutive bytes of a share
constexpr uint32_t kAdlerMaxPiece = 1u << 20;

struct AdlerSum {
    uint32_t a, b;       // mod kAdlerMod
    uint64_t n;
};

// Share `lane` of kAdlerLanes of the piece x[0, n): the runs of kAdlerRun bytes
// at lane * kAdlerRun, + kAdlerLanes * kAdlerRun, ...; added to *a and *w.
__host__ __device__ inline void adler_share(const uint8_t* x, uint32_t n, uint32_t lane, uint64_t* a, uint64_t* w)
{
    uint64_t sa = 0, sw = 0;
    for (uint32_t i = lane * kAdlerRun; i < n; i += kAdlerLanes * kAdlerRun) {
        const uint32_t e = n - i < kAdlerRun ? n - i : kAdlerRun;
        for (uint32_t j = 0; j < e; ++j) {
            const uint32_t v = x[i + j];
            sa += v;
            sw += (uint64_t)(i + j) * v;
        }
    }
    *a += sa;
    *w += sw;
}

// the piece of n bytes whose shares sum to a and w
__host__ __device__ inline AdlerSum adler_piece(uint64_t a, uint64_t w, uint32_t n)
{
    return AdlerSum{(uint32_t)(a % kAdlerMod), (uint32_t)(((uint64_t)n * a - w) % kAdlerMod), n};
}

// x then y
__host__ __device__ inline AdlerSum adler_fold(const AdlerSum& x, const AdlerSum& y)
{
    const uint64_t b = (uint64_t)x.b + (y.n % kAdlerMod) * (uint64_t)x.a + y.b;
    return AdlerSum{(x.a + y.a) % kAdlerMod, (uint32_t)(b % kAdlerMod), x.n + y.n};
}

__host__ __device__ inline uint32_t adler_value(const AdlerSum& s)
{
    const uint32_t s1 = (1u + s.a) % kAdlerMod, s2 = (uint32_t)((s.n % kAdlerMod + s.b) % kAdlerMod);
    return (s2 << 16) | s1;
}

// Adler-32 of x[0, n) from pieces of `piece` bytes (1 .. kAdlerMaxPiece), every
// piece summed in its kAdlerLanes shares.
inline uint32_t adler32_pieces(const uint8_t* x, uint64_t n, uint32_t piece)
{
    AdlerSum s{0, 0, 0};
    for (uint64_t at = 0; at < n; at += piece) {
        const uint32_t len = (uint32_t)(n - at < piece ? n - at : piece);
        uint64_t a = 0, w = 0;
        for (uint32_t lane = 0; lane < kAdlerLanes; ++lane) adler_share(x + at, len, lane, &a, &w);
        s = adler_fold(s, adler_piece(a, w, len));
    }
    return adler_value(s);
}

}  // namespace gz
