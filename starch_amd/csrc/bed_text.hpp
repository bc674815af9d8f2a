// starch_amd/csrc/bed_text.hpp -- device helpers of every BED command that writes
// text (bed_map, bed_mapel, bed_mapscore, bed_closest, bed_setops, and through
// bed_records.hpp bed_convert and bed_align; sort_bed.hip takes line_beg): line
// bounds, decimal numbers in and out, and the output cursor of a thread with the
// copies it leaves to its wave.
#pragma once
#include "common.hpp"
#include "sort_bed.hpp"

namespace bt {

constexpr uint64_t kLimit = 0x7fffffffffffffffull;   // the largest coordinate

__device__ __forceinline__ uint64_t line_beg(const uint64_t* __restrict__ line_end, uint64_t i) { return i ? line_end[i - 1] : 0; }

__device__ __forceinline__ uint32_t dec_digits(uint64_t v)
{
    uint32_t d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}

__device__ __forceinline__ void put_dec(uint8_t* o, uint64_t v, uint32_t d)
{
    for (uint32_t k = d; k-- > 0;) { o[k] = (uint8_t)('0' + v % 10); v /= 10; }
}

// the k bytes at s are the word w
__device__ __forceinline__ bool is_word(const uint8_t* __restrict__ s, const char* w, uint32_t k)
{
    for (uint32_t j = 0; j < k; ++j)
        if (s[j] != (uint8_t)w[j]) return false;
    return true;
}

// decimal field s[b, e): 0, or kEmpty, kDigit, kRange (20 digits or more, or above 2^63-1)
template <uint32_t kEmpty, uint32_t kDigit, uint32_t kRange>
__device__ __forceinline__ uint32_t parse_coord(const uint8_t* __restrict__ s, uint32_t b, uint32_t e, uint64_t* v)
{
    if (b == e) return kEmpty;
    for (uint32_t p = b; p < e; ++p)
        if ((uint32_t)s[p] - '0' > 9u) return kDigit;
    if (e - b > 19) return kRange;
    uint64_t x = 0;
    for (uint32_t p = b; p < e; ++p) x = x * 10 + ((uint32_t)s[p] - '0');   // 19 digits: below 10^19 < 2^64
    if (x > kLimit) return kRange;
    *v = x;
    return 0;
}

__device__ __forceinline__ bool is_blank(uint8_t c) { return c == ' ' || c == '\t'; }

// One thread's output cursor, and the copies it leaves to its wave: a copy of
// sb::kWaveCopyBytes or more is not made by the thread but noted in the slot
// the caller names (a slot holds one copy) and made by wave_copy_tails.
template <int kSlots = 1>
struct Writer {
    uint8_t* out;
    uint64_t o;
    const uint8_t* big_src[kSlots] = {};
    uint64_t big_dst[kSlots] = {}, big_len[kSlots] = {};
    __device__ __forceinline__ void bytes(const uint8_t* __restrict__ s, uint64_t n)
    {
        for (uint64_t p = 0; p < n; ++p) out[o + p] = s[p];
        o += n;
    }
    __device__ __forceinline__ void tab() { out[o++] = '\t'; }
    __device__ __forceinline__ void delim(const uint8_t* d, uint32_t len)
    {
        for (uint32_t k = 0; k < len; ++k) out[o++] = d[k];
    }
    __device__ __forceinline__ void dec(uint64_t v, uint32_t d)   // d = dec_digits(v)
    {
        put_dec(out + o, v, d);
        o += d;
    }
    __device__ __forceinline__ void dec(uint64_t v) { dec(v, dec_digits(v)); }
    // n bytes at s: written here when short, left to the wave in `slot` when long
    __device__ __forceinline__ void copy(int slot, const uint8_t* __restrict__ s, uint64_t n)
    {
        if (n >= sb::kWaveCopyBytes) { big_src[slot] = s; big_dst[slot] = o; big_len[slot] = n; o += n; }
        else bytes(s, n);
    }
    // the last column and the '\n'
    __device__ __forceinline__ void tail(const uint8_t* __restrict__ s, uint64_t n)
    {
        copy(0, s, n);
        out[o++] = '\n';
    }
};

// the copies that the lanes of this wave left in w, made slot after slot and
// lane after lane by the whole wave (every lane of the wave calls this)
template <int kSlots>
__device__ __forceinline__ void wave_copy_tails(const Writer<kSlots>& w, uint8_t* __restrict__ out, int lane)
{
#pragma unroll
    for (int slot = 0; slot < kSlots; ++slot) {
        unsigned long long m = __ballot(w.big_len[slot] != 0);
        while (m) {
            const int l = __ffsll(m) - 1;
            m &= m - 1;
            const uint8_t* src = reinterpret_cast<const uint8_t*>(__shfl((uint64_t)reinterpret_cast<uintptr_t>(w.big_src[slot]), l, 64));
            const uint64_t dst = __shfl(w.big_dst[slot], l, 64), len = __shfl(w.big_len[slot], l, 64);
            for (uint64_t p = lane; p < len; p += 64) out[dst + p] = src[p];
        }
    }
}

}  // namespace bt
