// What pose_nms.hip and pose_ap.hip share, each piece stated once: the per-joint term of object-key-point similarity and the rectangular
// form's area and mean (the bits of udapose_oks_matrix are the bits the AP matching compares with its thresholds), the finiteness test of
// the refusals and the 32-bit key that orders scores as both walks take them.  No FMA contraction inside: every step is one correctly
// rounded fp32 operation, whatever the including file's own setting.
#pragma once
#include <float.h>
#include "common.h"

constexpr unsigned int POSE_KEY_REFUSED = 0xffffffffu;

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }

// a key that orders poses as the walks do: smaller = earlier.  Scores descending (-0 = +0); every refused pose shares the last key
__device__ __forceinline__ unsigned int order_key(float score, bool refused) {
    if (refused) return POSE_KEY_REFUSED;
    const unsigned int u = __float_as_uint(score + 0.f);
    const unsigned int asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;      // (0xffffffff would need u = 0xffffffff, a NaN: refused)
}

// v_k = (2 sigma_k)^2
__device__ __forceinline__ float oks_sigma_sq(float sigma) {
#pragma clang fp contract(off)
    const float s2 = 2.f * sigma;
    return s2 * s2;
}

// expf(-e_k), e_k = d2 / v_k / A * 0.5f, d2 = dx * dx + dy * dy
__device__ __forceinline__ float oks_term(float2 pi, float2 pj, float v, float A) {
#pragma clang fp contract(off)
    const float dx = pi.x - pj.x, dy = pi.y - pj.y;
    const float d2 = dx * dx + dy * dy;
    const float e = d2 / v / A * 0.5f;
    return expf(-e);
}

// the rectangular form (COCO's convention): the label's area, and the mean over the label's nvis visible joints, 0 for none
__device__ __forceinline__ float oks_rect_area(float area_b) { return area_b + FLT_EPSILON; }
__device__ __forceinline__ float oks_rect_mean(float acc, int nvis) { return nvis ? acc / (float)nvis : 0.f; }
