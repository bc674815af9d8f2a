// starch_amd/csrc/gz_crc.hpp -- the CRC-32 machinery that the gzip encoder
// (gz_deflate.hip) and the inflater (gz_inflate.hip) share: the byte-at-a-time
// table, and the GF(2) arithmetic that joins the CRC registers of adjacent
// pieces.  A register here has init 0 and no final xor; the gzip CRC-32 of n
// bytes with register R is ~(R ^ 0xffffffff * x^(8n)).
//
// __constant__ data belongs to the translation unit that includes this header
// (each .hip file is its own code object), so each of them uploads its copy:
// upload_crc_tables(), once per device.
#pragma once
#include <atomic>

#include "common.hpp"

namespace gz {
namespace {

__constant__ uint32_t c_crc_tab[256];          // reflected CRC-32 (poly 0xEDB88320), byte at a time
__constant__ uint32_t c_x8pow[48];             // x^(8 * 2^k) mod P (reflected CRC-32)

// GF(2) product of two CRC-32 register values (reflected: bit 31 is x^0)
__host__ __device__ inline uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & m) p ^= b;
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}

__device__ __forceinline__ uint32_t x8n(uint64_t n)   // x^(8n) mod P
{
    uint32_t r = 1u << 31;                     // x^0
    for (int k = 0; n; ++k, n >>= 1)
        if (n & 1u) r = gf_mul(r, c_x8pow[k]);
    return r;
}

// CRC register (init 0, no final xor) of A||B from those of A and B
__device__ __forceinline__ uint32_t crc_cat(uint32_t ra, uint32_t rb, uint64_t len_b)
{
    return gf_mul(ra, x8n(len_b)) ^ rb;
}

void upload_crc_tables()
{
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load() & bit) return;
    // x^8 mod P, then squarings: x^(8 * 2^k)
    uint32_t pw[48];
    uint32_t x8 = 1u << 23;                      // reflected x^8
    for (int k = 0; k < 48; ++k) { pw[k] = x8; x8 = gf_mul(x8, x8); }
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int j = 0; j < 8; ++j) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
        tab[i] = c;
    }
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_x8pow), pw, sizeof(pw)));
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_crc_tab), tab, sizeof(tab)));
    done.fetch_or(bit);
}

}  // namespace
}  // namespace gz
