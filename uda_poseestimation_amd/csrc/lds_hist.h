// The LDS histogram add shared by the kernels that count 256-bin histograms (strong_aug.hip, pixel_style.hip).
#pragma once
#include <hip/hip_runtime.h>

// ++h[v] for every active lane.  A wave whose lanes all bring one value - the black border a warp leaves, a flat background - adds its
// lane count once: 64 atomics on one LDS address would be served one after the other.
__device__ __forceinline__ void hist_add(unsigned int* h, unsigned int v) {
    const unsigned int first = __builtin_amdgcn_readfirstlane(v);
    if (__all(v == first)) {
        const unsigned long long m = __ballot(1);
        if ((int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(&h[first], (unsigned int)__popcll(m));
    } else {
        atomicAdd(&h[v], 1u);
    }
}
