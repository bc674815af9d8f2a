// starch_amd/csrc/bed_search.hpp -- the binary searches over ordered per-line
// arrays that bed_map.hip, bed_closest.hip and bed_mapel.hip share, and the
// per-chromosome bounds kernel of all three: device code only.
#pragma once
#include "common.hpp"

namespace bm {

// first index in [lo, hi) with v[index] >= x (hi: none)
__device__ __forceinline__ uint64_t lower(const uint64_t* __restrict__ v, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// first index in [lo, hi) with v[index] > x
__device__ __forceinline__ uint64_t upper(const uint64_t* __restrict__ v, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

constexpr int kBoundsThreads = 256;

// lo[c], c in [0, C]: the first of n ordered ranks that is >= c
static __global__ void __launch_bounds__(kBoundsThreads)
k_bm_bounds(const uint32_t* __restrict__ rank, uint64_t n, uint64_t C, uint64_t* __restrict__ lo_out)
{
    const uint64_t c = (uint64_t)blockIdx.x * kBoundsThreads + threadIdx.x;
    if (c > C) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (rank[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    lo_out[c] = lo;
}

}  // namespace bm
