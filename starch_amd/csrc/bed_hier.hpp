// starch_amd/csrc/bed_hier.hpp -- the hierarchy of maxima over an array of stops
// that bed_closest.hip and bed_mapel.hip share: level k holds the maximum of
// every aligned group of kFanout^k stops, up to the level with one item.  The
// level kernel and the host-side builder (device code: for .hip files only);
// the fan-out is bed_closest.hpp's, the walks over it stay with their callers.
#pragma once
#include <string>

#include "../../include/starch_amd.h"
#include "bed_closest.hpp"

namespace bc {

constexpr int kLevelThreads = 256;

struct Hier {
    const uint64_t* lev[kMaxLevels];   // lev[0]: the stops themselves
    uint64_t cnt[kMaxLevels];
    int nlev;
};

// out[g] = the largest of in[g * kFanout, min((g + 1) * kFanout, n))
static __global__ void __launch_bounds__(kLevelThreads)
k_bc_level(const uint64_t* __restrict__ in, uint64_t n, uint64_t groups, uint64_t* __restrict__ out)
{
    const uint64_t g = (uint64_t)blockIdx.x * kLevelThreads + threadIdx.x;
    if (g >= groups) return;
    const uint64_t b = g << kFanShift, e = b + kFanout < n ? b + kFanout : n;
    uint64_t m = 0;
    for (uint64_t k = b; k < e; ++k) m = in[k] > m ? in[k] : m;
    out[g] = m;
}

// The levels above the n > 0 stops S, one after the other in buf.  Throws
// STARCH_ERR_INTERNAL with `tool` in front when kMaxLevels do not reach one item.
static inline void build_hier(const uint64_t* S, uint64_t n, DevBuf& buf, hipStream_t st, const char* tool, Hier* h)
{
    uint64_t total = 0, c = n;
    int nlev = 1;
    while (c > 1) { c = ceil_div(c, kFanout); total += c; ++nlev; }
    if (nlev > kMaxLevels) throw StarchError(STARCH_ERR_INTERNAL, std::string(tool) + ": too many levels");
    uint64_t* hb = buf.as<uint64_t>(total);
    h->nlev = nlev;
    h->lev[0] = S;
    h->cnt[0] = n;
    for (int k = 1; k < nlev; ++k) {
        const uint64_t groups = ceil_div(h->cnt[k - 1], kFanout);
        hipLaunchKernelGGL(k_bc_level, dim3(blocks_for(groups, kLevelThreads)), dim3(kLevelThreads), 0, st, h->lev[k - 1],
                           h->cnt[k - 1], groups, hb);
        h->lev[k] = hb;
        h->cnt[k] = groups;
        hb += groups;
    }
    HIP_CHECK(hipGetLastError());
}

}  // namespace bc
