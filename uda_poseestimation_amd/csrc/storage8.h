// 8-channel groups of an NHWC activation tensor in its three storage types - the element type (bf16 / fp16), fp32 and the f16x2 split
// type sp32 (common.h) - <-> fp32 registers: the one statement of these loads and stores for pointwise.hip, adain.hip and adain_train.hip.
// st8<sp32> and st1<sp32> feed the saturation counter of the translation unit that includes this header (common.h: one counter per file that
// stores split values, each with its UDAPOSE_SP_SAT_READER; today pointwise.hip and adain.hip).
#pragma once
#include "common.h"

template <typename T> __device__ __forceinline__ void ld8(const T* p, float (&o)[8]);
template <> __device__ __forceinline__ void ld8<elem_t>(const elem_t* p, float (&o)[8]) {
    const elem8 v = *(const elem8*)p;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (float)v[e];
}
template <> __device__ __forceinline__ void ld8<float>(const float* p, float (&o)[8]) {
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = a[e]; o[4 + e] = b[e]; }
}
template <> __device__ __forceinline__ void ld8<sp32>(const sp32* p, float (&o)[8]) {      // 32 bytes = [8 h][8 l]
    const char* c = (const char*)p;
    sp_join8(*(const half8*)c, *(const half8*)(c + 16), o);
}
template <typename T> __device__ __forceinline__ void st8(T* p, const float (&v)[8]);
template <> __device__ __forceinline__ void st8<sp32>(sp32* p, const float (&v)[8]) {
    half8 h, l;
    sp_split8(v, h, l);
    char* c = (char*)p;
    *(half8*)c = h;
    *(half8*)(c + 16) = l;
}
template <> __device__ __forceinline__ void st8<elem_t>(elem_t* p, const float (&v)[8]) {
    elem8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (elem_t)v[e];
    *(elem8*)p = o;
}
template <> __device__ __forceinline__ void st8<float>(float* p, const float (&v)[8]) {
    *(f32x4*)p = (f32x4){v[0], v[1], v[2], v[3]};
    *(f32x4*)(p + 4) = (f32x4){v[4], v[5], v[6], v[7]};
}
// element i (any index) of a tensor
template <typename T> __device__ __forceinline__ float ld1(const T* p, size_t i) { return (float)p[i]; }
template <> __device__ __forceinline__ float ld1<sp32>(const sp32* p, size_t i) { return sp_load1(p, i); }
template <typename T> __device__ __forceinline__ void st1(T* p, size_t i, float v) { p[i] = (T)v; }
template <> __device__ __forceinline__ void st1<sp32>(sp32* p, size_t i, float v) { sp_store1(p, i, v); }

// 8 values kept in their STORAGE form (4 registers per 8 bf16 values, 8 per 8 floats or split values): adain_k's register cache
template <typename T> struct Raw8;
template <> struct Raw8<elem_t> { elem8 v; };
template <> struct Raw8<float> { f32x4 a, b; };
template <> struct Raw8<sp32> { half8 h, l; };
__device__ __forceinline__ void ldraw(const sp32* p, Raw8<sp32>& r) { const char* c = (const char*)p; r.h = *(const half8*)c; r.l = *(const half8*)(c + 16); }
__device__ __forceinline__ void unraw(const Raw8<sp32>& r, float (&o)[8]) { sp_join8(r.h, r.l, o); }
__device__ __forceinline__ void ldraw(const elem_t* p, Raw8<elem_t>& r) { r.v = *(const elem8*)p; }
__device__ __forceinline__ void ldraw(const float* p, Raw8<float>& r) { r.a = *(const f32x4*)p; r.b = *(const f32x4*)(p + 4); }
__device__ __forceinline__ void unraw(const Raw8<elem_t>& r, float (&o)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (float)r.v[e];
}
__device__ __forceinline__ void unraw(const Raw8<float>& r, float (&o)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = r.a[e]; o[4 + e] = r.b[e]; }
}

// 16-byte group i of an NHWC tensor with G groups per pixel -> (n, h, w, g)
__device__ __forceinline__ void nhwg_of(size_t i, int G, int H, int W, int& n, int& h, int& w, int& g) {
    g = (int)(i % G);
    size_t r = i / G;
    w = (int)(r % W); r /= W;
    h = (int)(r % H);
    n = (int)(r / H);
}
