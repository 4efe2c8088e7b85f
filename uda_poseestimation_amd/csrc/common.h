// Shared device/host helpers for the gfx950 (MI355X, CDNA4) kernels of the UDA pose hot path.
// wave = 64 lanes; MFMA 16x16x32 bf16; LDS 160 KiB/CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/udapose.h"      // the UDAPOSE_* return codes

// Storage / MFMA-operand element type of this build of the library.  The same sources are compiled twice:
//   libudapose_hip.so      elem_t = bf16  (v_mfma_f32_16x16x32_bf16)   - BASELINE.json's benched precision
//   libudapose_hip_f16.so  elem_t = fp16  (v_mfma_f32_16x16x32_f16)    - the reference's autocast dtype (train_human.py:280,414)
// Accumulation, BatchNorm statistics, master weights, gradients of weights and every loss are fp32 in both.
#if defined(UDAPOSE_ELEM_F16)
typedef _Float16 elem_t;
typedef __attribute__((ext_vector_type(8))) _Float16 elem8;
typedef __attribute__((ext_vector_type(4))) _Float16 elem4;
#define UDAPOSE_ELEM_KIND 1
#define UDAPOSE_MFMA_16x16x32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)
#else
typedef __bf16 elem_t;
typedef __attribute__((ext_vector_type(8))) __bf16 elem8;
typedef __attribute__((ext_vector_type(4))) __bf16 elem4;
#define UDAPOSE_ELEM_KIND 0
#define UDAPOSE_MFMA_16x16x32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
#endif
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// ---- "f16x2" storage: the fp32-grade precision mode (both builds of the library carry it; it does not depend on elem_t).
// A value v is kept as two fp16 numbers (h, l) with v = h + l * 2^-11 to ~2^-22 relative: h = fp16(v), l = fp16((v - h) * 2^11)
// (the remainder is scaled so that it stays in fp16's normal range whenever h does).  A product of two such values is
// h_a h_b + (h_a l_b + l_a h_b) 2^-11 + O(2^-22): THREE v_mfma_f32_16x16x32_f16 per 32-deep K step with two fp32 accumulators,
// against eight v_mfma_f32_16x16x4_f32 at a quarter of the rate each for the exact fp32 form (gfx950 has no xf32).
// Memory layout of a split tensor: every group of 8 consecutive channels is 32 bytes, [8 x h][8 x l] - byte for byte the
// footprint and the addressing of an fp32 NHWC tensor (element stride 4 bytes, 16-byte chunks), so the fp32 loaders of the
// igemm kernel and the 8-channel pointwise kernels serve it unchanged, and one 128-byte LDS row of 32 channels holds the
// MFMA fragments of lane group q as chunk 2q (h) and chunk 2q+1 (l).  Range: |v| <= 65504 (saturating).
typedef __attribute__((ext_vector_type(8))) _Float16 half8;
struct sp32 { unsigned int bits; };      // 4-byte stride type of a split tensor (never read as a scalar: groups of 8 only)
#define UDAPOSE_SP_SCALE 2048.f
#define UDAPOSE_SP_INV (1.f / 2048.f)
// Saturation counter of the f16x2 stores (round 4; VERDICT r3: the mode saturated silently): every store of a value outside fp16's
// range (|v| > 65504, or NaN, which the clamp below would turn into -65504) adds one to a device counter.  Device code is linked per
// source file, so every translation unit that stores split values owns a counter (UDAPOSE_SP_SAT_READER defines its host-side reader)
// and udapose_split_saturations sums them.  A saturating network is the exception: the atomic is behind a wave-uniform-in-practice branch.
static __device__ unsigned int g_sp_sat_count = 0u;
#define UDAPOSE_SP_SAT_READER(fn)                                                                          \
    unsigned long long fn(int reset) {                                                                     \
        unsigned int v = 0u, z = 0u;                                                                       \
        if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_sp_sat_count), sizeof(v)) != hipSuccess) return ~0ull;   \
        if (reset && v) (void)hipMemcpyToSymbol(HIP_SYMBOL(g_sp_sat_count), &z, sizeof(z));              \
        return v;                                                                                          \
    }
__device__ __forceinline__ void sp_split8(const float (&v)[8], half8& h, half8& l) {
    bool sat = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sat |= !(fabsf(v[e]) <= 65504.f);
        const float c = fminf(fmaxf(v[e], -65504.f), 65504.f);
        const _Float16 hh = (_Float16)c;
        h[e] = hh;
        l[e] = (_Float16)((c - (float)hh) * UDAPOSE_SP_SCALE);
    }
    if (sat) atomicAdd(&g_sp_sat_count, 1u);
}
__device__ __forceinline__ void sp_join8(const half8& h, const half8& l, float (&o)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (float)h[e] + (float)l[e] * UDAPOSE_SP_INV;
}
// element e (any index) of a split tensor
__device__ __forceinline__ float sp_load1(const void* base, size_t e) {
    const _Float16* g = (const _Float16*)((const char*)base + (e >> 3) * 32);
    return (float)g[e & 7] + (float)g[8 + (e & 7)] * UDAPOSE_SP_INV;
}
__device__ __forceinline__ void sp_store1(void* base, size_t e, float v) {
    _Float16* g = (_Float16*)((char*)base + (e >> 3) * 32);
    if (!(fabsf(v) <= 65504.f)) atomicAdd(&g_sp_sat_count, 1u);
    const float c = fminf(fmaxf(v, -65504.f), 65504.f);
    const _Float16 hh = (_Float16)c;
    g[e & 7] = hh;
    g[8 + (e & 7)] = (_Float16)((c - (float)hh) * UDAPOSE_SP_SCALE);
}

#define LDS_PTR(T, p) ((__attribute__((address_space(3))) T*)(p))

static inline int udapose_check_launch() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? UDAPOSE_OK : UDAPOSE_ERR_LAUNCH;
}

// Exact unsigned division by a runtime constant (mul-hi + shift), host-prepared.
struct FastDiv {
    uint32_t d, magic, shift;
};
static inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    f.d = d;
    if (d == 1) { f.magic = 0; f.shift = 0; return f; }
    uint32_t s = 0;
    while ((1u << s) < d) ++s;
    uint64_t m = ((((uint64_t)1 << 32) * (((uint64_t)1 << s) - d)) / d) + 1;
    f.magic = (uint32_t)m;
    f.shift = s;
    return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
    if (f.d == 1) return n;
    uint32_t t = __umulhi(n, f.magic);
    return (t + ((n - t) >> 1)) >> (f.shift - 1);
}

// XCD-aware work-group remap (MI355X: 8 XCDs, each with a private 4 MiB L2; work-groups are dealt round-robin, so b and
// b+8 share an L2).  Returns a bijective permutation of the linear block id that gives every XCD one CONTIGUOUS range of
// work ids, so that blocks which re-read the same operand panels hit the same L2 instead of each XCD streaming the whole
// working set from the Infinity Cache.  Placement is a speed matter only; results never depend on it.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t bid, uint32_t total) {
    const uint32_t q = total >> 3, r = total & 7u, xcd = bid & 7u, local = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
}

// Training-mode BatchNorm's scale and shift of one channel: z = y * sc + sh.  The forward (bn_finalize_k, bn_apply_chunk_k) and every
// backward that rebuilds the ReLU mask z > 0 from y instead of reading z (pointwise.hip relu == 2, the BS epilogue of igemm.hip) form
// them HERE, so the rebuilt mask is the forward's bit for bit.
__device__ __forceinline__ float bn_scale(float gamma, float invstd) { return gamma * invstd; }
__device__ __forceinline__ float bn_shift(float beta, float mean, float sc) { return beta - mean * sc; }
__device__ __forceinline__ void bn_scale_shift(float gamma, float beta, float mean, float invstd, float& sc, float& sh) {
    sc = bn_scale(gamma, invstd);
    sh = bn_shift(beta, mean, sc);
}
__device__ __forceinline__ void bn_scale_shift8(const float (&gamma)[8], const float (&beta)[8], const float (&mean)[8], const float (&invstd)[8],
                                                float (&sc)[8], float (&sh)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) bn_scale_shift(gamma[e], beta[e], mean[e], invstd[e], sc[e], sh[e]);
}

// torch's total order on floats for max / kthvalue: NaN is the LARGEST value (and all NaNs are equal); the first index wins a tie.
// The one arg-max order of every heat-map decode (heatmap.hip, softargmax.hip, flip.hip, refine.hip, pck_curve.hip, view_merge.hip).
__device__ __forceinline__ bool hm_better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    if (vn) return i < bi;
    return v > bv || (v == bv && i < bi);
}
// The wave arg-max: every lane brings its own best (value, flat index) and returns the wave's, under hm_better (a total order: the winner
// does not depend on the reduction tree).  view_merge_k runs it once per view and combines the waves in LDS tables of its own.
// (Both helpers reduce in locals and write the references once: updated through the references, the compiler keeps hm_better's branches
// where it otherwise selects - view_merge_k measured 0.9 us slower that way.)
__device__ __forceinline__ void hm_wave_best(float& bv, int& bi) {
    float v = bv;
    int i = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (hm_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    bv = v; bi = i;
}
// The block arg-max of argmax_rectify_k, sa_row, flip_merge_k, refine.hip and pck_curve.hip: hm_wave_best, then the WAVES waves' results
// combined through LDS; every thread returns the block's.  sv, si: WAVES entries of LDS.  Opens with a barrier: every thread of the
// block must reach the call.
template <int WAVES>
__device__ __forceinline__ void hm_block_best(float& bv, int& bi, float* sv, int* si) {
    hm_wave_best(bv, bi);
    __syncthreads();      // (sv, si may still be read from the previous reduction)
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    float v = sv[0];
    int i = si[0];
    for (int w = 1; w < WAVES; ++w)
        if (hm_better(sv[w], si[w], v, i)) { v = sv[w]; i = si[w]; }
    bv = v; bi = i;
}

// The wave sum (float, double, unsigned long long): six xor steps, every lane returns the wave's sum.  Lane 0 adds the same pairs in the same
// order as lane 0 of a __shfl_down tree (at each step lane i < offset holds a_i + a_(i + offset) in both).
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// The block sum in a fixed order: wave_sum, one LDS slot per wave, then the WAVES waves' sums added to zero in wave order,
// ((0 + w0) + w1) + ...; every thread returns the block's sum.  red: WAVES entries of LDS.  Barriers as hm_block_best: it opens with one
// (red may still be read from the previous reduction), so every thread of the block must reach the call, and the caller may rely on that
// barrier alone - none follows the last read of red.
template <int WAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = 0;
    for (int w = 0; w < WAVES; ++w) t += red[w];
    return t;
}

// The wave inclusive scan in lane order (int, unsigned int): six __shfl_up steps, lane l returns v_0 + ... + v_l.
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(v, o, 64);
        if ((int)(threadIdx.x & 63) >= o) v += up;
    }
    return v;
}
// The block inclusive scan in thread order: wave_scan_incl, one LDS slot per wave, then the sums of the waves before the thread's own added
// in wave order; every thread returns its prefix and gets the block's sum in `total`.  red: WAVES entries of LDS.  Barriers as block_sum: it
// opens with one, every thread of the block must reach the call, the caller may rely on that barrier alone, none follows the last read of red.
template <int WAVES, typename T>
__device__ __forceinline__ T block_scan_incl(T v, T* red, T& total) {
    v = wave_scan_incl(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T before = 0;
    total = 0;
    for (int w = 0; w < WAVES; ++w) {
        if (w < (int)(threadIdx.x >> 6)) before += red[w];
        total += red[w];
    }
    return v + before;
}
// v added to a 64-bit counter of device memory (an integer atomic; nothing is issued for v == 0): the evaluation meters' states
__device__ __forceinline__ void counter_add(long long* __restrict__ p, long long v) {
    if (v) atomicAdd((unsigned long long*)p, (unsigned long long)v);
}

// ReflectionPad2d(1)'s source index of position i (in [-1, n]) on an axis of n >= 2
__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
// sign(v) with sign(0) = 0 (NaN: 0)
__device__ __forceinline__ float sign_or_0(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// Blocks of a grid-stride launch over n items at `per` items per block: at least 1, at most `cap` (the caps decide speed: every file keeps its own)
constexpr size_t GRID_NO_CAP = 0x7fffffff;
static inline int grid_for(size_t n, int per, size_t cap) {
    const size_t b = (n + per - 1) / per;
    return (int)(b > cap ? cap : (b ? b : 1));
}
