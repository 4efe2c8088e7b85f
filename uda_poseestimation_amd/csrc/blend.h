// PIL's Image.blend(degenerate, image, factor) on one byte, the step every ImageEnhance class ends in: float32 d + f * (v - d), clipped
// to [0, 255], TRUNCATED to uint8.  Shared by the ColorJitter ops (augment.hip) and Sharpness (strong_aug.hip).
#pragma once
#include "common.h"

// no FMA contraction from here to the end of the including file: PIL rounds the product and the sum separately; a fused multiply-add lands
// on the other side of an integer for ~1 % of the bytes and the truncation to uint8 then differs
#pragma clang fp contract(off)

__device__ __forceinline__ unsigned char blend1(float d, float v, float f) {
    float prod = f * (v - d);
    asm volatile("" : "+v"(prod));        // (belt and braces: the product is pinned in a register, no contraction can cross this)
    const float t = d + prod;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (unsigned char)t);
}
