// Order statistics on fp32 values, shared by heatmap.hip (kth_mask_k) and select.hip: the order-preserving key of a float and
// the k-th smallest of a strided vector by an MSB-first radix select.  (hm_better, the arg-max order: common.h)
#pragma once
#include "common.h"

// the sign-flip transform: a float's bits -> a uint32 that ascends with the value (-0 just below +0).  hm_key and pose_pair.h's order_key
__device__ __forceinline__ unsigned int hm_key_bits(unsigned int b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
// order-preserving float -> uint32 key (NaN -> 0xffffffff, the largest: torch.kthvalue's order)
__device__ __forceinline__ unsigned int hm_key(float v) { return v != v ? 0xffffffffu : hm_key_bits(__float_as_uint(v)); }
__device__ __forceinline__ float hm_unkey(unsigned int k) {
    if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// a k that was read from device memory, held inside the select's range 1 ... n
__device__ __forceinline__ int hm_kth_clamp(int k, int n) { return k < 1 ? 1 : (k > n ? n : k); }

// k-th smallest (1-indexed) of the n values base[i * stride], by ONE work-group (every thread calls it and gets the value).
// MSB-first radix select: 4 passes of 8 bits, each a 256-bin LDS histogram of the keys that still match the prefix found so
// far, then a scan of the bins for the one that holds rank k.  O(n) per pass (the previous rank-count form was O(n^2): 23 us
// at n = 512, ~0.7 ms at the n = 4096 of an 8-rank global batch); n = 4096 costs 16 key loads per thread in all.  Values are
// read from L2 each pass (n <= 65536 floats = 256 KiB).  NaN orders as the largest value: the result is then NaN.
// hist: 256 words of LDS, pick: 2 words of LDS.  The block size must be >= 64; 1 <= k <= n.
__device__ __forceinline__ float hm_kth_smallest(const float* __restrict__ base, size_t stride, int n, int k, unsigned int* hist,
                                                 unsigned int* pick) {
    unsigned int prefix = 0, pmask = 0, rank = (unsigned int)(k - 1);     // 0-based rank inside the surviving set
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const unsigned int key = hm_key(base[(size_t)i * stride]);
            if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            // wave 0: each lane owns 4 consecutive bins; exclusive prefix over lanes, then the owner of the rank reports
            const int b0 = threadIdx.x * 4;
            const unsigned int c0 = hist[b0], c1 = hist[b0 + 1], c2 = hist[b0 + 2], c3 = hist[b0 + 3];
            const unsigned int tot = c0 + c1 + c2 + c3;
            unsigned int incl = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned int up = __shfl_up(incl, o, 64);
                if ((int)threadIdx.x >= o) incl += up;
            }
            const unsigned int excl = incl - tot;
            if (rank >= excl && rank < incl) {
                unsigned int r = rank - excl;
                int b = b0;
                if (r >= c0) { r -= c0; ++b; if (r >= c1) { r -= c1; ++b; if (r >= c2) { r -= c2; ++b; } } }
                pick[0] = (unsigned int)b;
                pick[1] = r;
            }
        }
        __syncthreads();
        prefix |= pick[0] << shift;
        pmask |= 255u << shift;
        rank = pick[1];
        __syncthreads();
    }
    return hm_unkey(prefix);
}
