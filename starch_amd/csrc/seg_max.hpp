// starch_amd/csrc/seg_max.hpp -- the segmented running maximum that
// bed_setops.hip (per-input merge) and bed_map.hip (a tile's largest window
// end per chromosome) share: device code only.
#pragma once
#include "common.hpp"

namespace so {

struct MF {          // the maximum since the last head (f: the range holds a head)
    uint64_t m;
    uint32_t f;
};
__device__ __forceinline__ MF comb(MF a, MF b) { return MF{b.f ? b.m : (a.m > b.m ? a.m : b.m), a.f | b.f}; }

__device__ __forceinline__ MF wave_incl_mf(MF v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        MF o;
        o.m = __shfl_up(v.m, d, 64);
        o.f = __shfl_up(v.f, d, 64);
        if (lane >= d) v = comb(o, v);
    }
    return v;
}

// exclusive scan over the block (all threads call it); sh_m, sh_f: blockDim.x / 64 entries
__device__ __forceinline__ MF block_excl_mf(MF v, uint64_t* sh_m, uint32_t* sh_f, MF* total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const MF inc = wave_incl_mf(v);
    MF exc;
    exc.m = __shfl_up(inc.m, 1, 64);
    exc.f = __shfl_up(inc.f, 1, 64);
    if (lane == 0) exc = MF{0, 0};
    if (lane == 63) { sh_m[wid] = inc.m; sh_f[wid] = inc.f; }
    __syncthreads();
    MF pre{0, 0};
    for (int w = 0; w < wid; ++w) pre = comb(pre, MF{sh_m[w], sh_f[w]});
    if (total) {
        MF tot = pre;
        for (int w = wid; w < nw; ++w) tot = comb(tot, MF{sh_m[w], sh_f[w]});
        *total = tot;
    }
    __syncthreads();
    return comb(pre, exc);
}

}  // namespace so
