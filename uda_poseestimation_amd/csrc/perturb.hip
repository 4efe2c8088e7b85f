// Gradient-direction perturbation of an image batch inside a norm ball: the step of FGSM / PGD style adversarial views.
// All operands fp32, [N][C][HW] contiguous; the same code in both builds of the library (no elem_t).
//
//   l2   (mode 0), per sample n:  u = g[n] / ||g[n]||_2;  d = (x[n] - x0[n]) + step * u;  if ||d||_2 > eps: d *= eps / ||d||_2;
//                                 out[n] = clamp(x0[n] + d)
//   linf (mode 1), per element:   d = clip((x - x0) + step * sign(g), -eps, eps);  out = clamp(x0 + d);  sign(0) = sign(NaN) = 0
//   x0 NULL: x0 = x.  step NULL: step = eps.  clamp = per-channel [lo[c], hi[c]] (both NULL: none).  eps, step: DEVICE scalars, read by the
//   launches, so a captured launch follows a host change of them.
//   Degenerate sample (its sum of squares of g is zero, inf or NaN - i.e. g[n] == 0, or holds a non-finite element, or squares that overflow):
//   out[n] = clamp(x[n]) - without a clamp x[n] bit for bit - and gnorm[n] = 0.  The rule is per SAMPLE wherever the sum of squares is formed:
//   always in l2, in linf when gnorm is asked for.  linf without gnorm is one launch with no reduction: there a non-finite g is handled per
//   element (sign(+-inf) = +-1, sign(NaN) = 0).
//
// Launches (256 threads, B = perturb_blocks(D) work-groups per sample, D = C * HW; work-group b owns the contiguous chunk b of its sample):
//   sumsq_k   partial[n][b] = sum of g^2 over the chunk                       (l2; linf with gnorm)
//   sumsq_k   partial2[n][b] = sum of d^2 over the chunk, d as above          (l2 with x0 or step given: the projection)
//   apply_k   out; work-group 0 of a sample also writes gnorm[n]
// The one-step form (l2, x0 NULL, step NULL: out = x + eps * u) has ||d|| = eps by construction and pays for no second norm: two launches.
//
// Summation order is fixed.  A thread adds the squares of its elements in index order (stride 256 accesses; the 4 lanes of a 16-byte access in
// order), a wave adds its 64 lanes by the xor butterfly, thread 0 adds the 4 waves in order, and every CONSUMER adds the B partials of its
// sample in index order (B <= 64 scalar loads per work-group).  No atomics, no allocation; every element of out and gnorm is written, and every
// workspace element a call reads it has written itself: two calls give the same bits, and the launches are capturable.
// A-priori error of the norm: every level is a pairwise or short sequential fp32 sum of non-negative terms - per thread at most
// ceil(D / (B * 256)) terms (<= 48 at 3 x 256 x 256 with 16-byte accesses: 4 per access, 12 accesses beyond D = 2^18), then 6 + 3 + (B - 1) levels - so
// relative error of the sum <= (terms per thread + 9 + B) * 2^-24 to first order, half of that for its square root.
//
// Scale invariance: g * 2^k gives the same out bits.  Every square scales by 2^(2k) exactly, so every partial and the total do; sqrtf is
// correctly rounded, so ||g|| scales by 2^k exactly; c = step / ||g|| (one correctly rounded division) scales by 2^-k exactly, and c * g is
// the same product.  This holds while no square of a non-zero element falls below the smallest normal number and the total stays finite:
// 2^-63 <= 2^k * |g_i| for every non-zero g_i, and 2^(2k) * sum g_i^2 < 2^128 (for |g_i| ~ 1 and D = 2^18: -63 <= k <= 54).  Outside it the
// result is still a valid perturbation (or the degenerate rule, on overflow); only the bit equality goes.
#include "common.h"
#include "pointwise.h"

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_MAX_B = 64;

// work-groups per sample and elements per work-group (a multiple of 4, so that 16-byte accesses never straddle two chunks)
inline int perturb_blocks(long long D) { const long long b = (D + 4095) / 4096; return (int)(b < 1 ? 1 : (b > PT_MAX_B ? PT_MAX_B : b)); }
inline long long perturb_chunk(long long D, int B) { const long long c = (D + B - 1) / B; return (c + 3) / 4 * 4; }

struct PtArgs {
    const float *x, *g, *x0, *lo, *hi, *eps, *step;
    float *out, *gnorm;
    const float *part_g, *part_d;       // [N][B] partial sums of squares read by this launch (NULL: not needed)
    float* part_out;                    // [N][B] partial sums this launch writes (sumsq_k)
    long long D, chunk;
    int HW, C, B, mode;
};

// the B partials of sample n, added in index order (a wave-uniform address: scalar loads)
__device__ __forceinline__ float sum_partials(const float* part, int n, int B) {
    float t = 0.f;
    for (int b = 0; b < B; ++b) t += part[(size_t)n * B + b];
    return t;
}
__device__ __forceinline__ bool usable(float s) { return s > 0.f && s < __builtin_inff(); }        // (false for NaN)
// the l2 displacement before the projection; ONE expression for the norm pass and the apply pass (the same bits in both)
__device__ __forceinline__ float l2_disp(float x, float x0, float g, float c) { return __fmaf_rn(c, g, x - x0); }

// MODE 0: sum of g^2.  MODE 1: sum of d^2, d = (x - x0) + (step / ||g||) * g (zero for a degenerate sample: never read).
template <int V, int MODE>
__global__ __launch_bounds__(PT_THREADS) void perturb_sumsq_k(PtArgs a) {
    const int n = blockIdx.x / a.B, b = blockIdx.x - n * a.B;
    const long long lo_i = (long long)b * a.chunk, hi_i = lo_i + a.chunk < a.D ? lo_i + a.chunk : a.D;
    const size_t base = (size_t)n * a.D;
    float c = 0.f;
    bool ok = true;
    if (MODE == 1) {
        const float sg = sum_partials(a.part_g, n, a.B);
        ok = usable(sg);
        c = ok ? __fdiv_rn(a.step ? *a.step : *a.eps, __fsqrt_rn(sg)) : 0.f;
    }
    const float* x0 = a.x0 ? a.x0 : a.x;
    float acc = 0.f;
    if (ok) {
        for (long long i = lo_i + (long long)threadIdx.x * V; i < hi_i; i += PT_THREADS * V) {
            if (V == 4) {
                const f32x4 g4 = *(const f32x4*)(a.g + base + i);
                if (MODE == 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = __fmaf_rn(g4[e], g4[e], acc);
                } else {
                    const f32x4 x4 = *(const f32x4*)(a.x + base + i), z4 = *(const f32x4*)(x0 + base + i);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float d = l2_disp(x4[e], z4[e], g4[e], c); acc = __fmaf_rn(d, d, acc); }
                }
            } else {
                const float g = a.g[base + i];
                if (MODE == 0) acc = __fmaf_rn(g, g, acc);
                else { const float d = l2_disp(a.x[base + i], x0[base + i], g, c); acc = __fmaf_rn(d, d, acc); }
            }
        }
    }
    __shared__ float red[PT_THREADS / 64];
    const float t = block_sum<PT_THREADS / 64>(acc, red);
    if (threadIdx.x == 0) a.part_out[(size_t)n * a.B + b] = t;
}

template <int V>
__global__ __launch_bounds__(PT_THREADS) void perturb_apply_k(PtArgs a) {
    const int n = blockIdx.x / a.B, b = blockIdx.x - n * a.B;
    const long long lo_i = (long long)b * a.chunk, hi_i = lo_i + a.chunk < a.D ? lo_i + a.chunk : a.D;
    const size_t base = (size_t)n * a.D;
    const float eps = *a.eps, step = a.step ? *a.step : eps;
    // sample-wide factors: c multiplies g (l2), f scales d (the projection); ok = false: the degenerate rule
    bool ok = true;
    float c = 0.f, f = 1.f, gn = 0.f;
    if (a.part_g) {
        const float sg = sum_partials(a.part_g, n, a.B);
        ok = usable(sg);
        if (ok) { gn = __fsqrt_rn(sg); c = __fdiv_rn(step, gn); }
        if (ok && a.part_d) {
            const float nd = __fsqrt_rn(sum_partials(a.part_d, n, a.B));
            if (nd > eps) f = __fdiv_rn(eps, nd);
        }
        if (a.gnorm && b == 0 && threadIdx.x == 0) a.gnorm[n] = gn;
    }
    const bool linf = a.mode == 1, clamp = a.lo != nullptr;
    const float* x0p = a.x0 ? a.x0 : a.x;
    for (long long i = lo_i + (long long)threadIdx.x * V; i < hi_i; i += PT_THREADS * V) {
        float xv[V], zv[V], gv[V], ov[V];
        if (V == 4) {
            const f32x4 x4 = *(const f32x4*)(a.x + base + i), g4 = *(const f32x4*)(a.g + base + i);
            const f32x4 z4 = a.x0 ? *(const f32x4*)(a.x0 + base + i) : x4;
#pragma unroll
            for (int e = 0; e < 4; ++e) { xv[e] = x4[e]; gv[e] = g4[e]; zv[e] = z4[e]; }
        } else {
            xv[0] = a.x[base + i]; gv[0] = a.g[base + i]; zv[0] = x0p[base + i];
        }
        float cl = 0.f, ch = 0.f;
        if (clamp) { const int ch_i = (int)(((uint32_t)i / (uint32_t)a.HW) % (uint32_t)a.C); cl = a.lo[ch_i]; ch = a.hi[ch_i]; }     // (V == 4 only where HW % 4 == 0: one channel per access)
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float o;
            if (!ok) o = xv[e];
            else if (linf) o = zv[e] + fminf(fmaxf(__fmaf_rn(step, sign_or_0(gv[e]), xv[e] - zv[e]), -eps), eps);
            else if (a.part_d) o = __fmaf_rn(f, l2_disp(xv[e], zv[e], gv[e], c), zv[e]);
            else o = __fmaf_rn(c, gv[e], xv[e]);            // the one-step form: x + eps * u
            ov[e] = clamp ? fminf(fmaxf(o, cl), ch) : o;
        }
        if (V == 4) { f32x4 o4; o4[0] = ov[0]; o4[1] = ov[1]; o4[2] = ov[2]; o4[3] = ov[3]; *(f32x4*)(a.out + base + i) = o4; }
        else a.out[base + i] = ov[0];
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// bytes of workspace udapose_perturb needs for these sizes (two [N][B] fp32 tables); < 0: an error code
long long perturb_ws_bytes(int N, int C, int HW) {
    if (N < 1 || C < 1 || HW < 1) return UDAPOSE_ERR_ARG;
    const long long D = (long long)C * HW;
    return 2ll * N * perturb_blocks(D) * (long long)sizeof(float);
}

int perturb(hipStream_t s, const float* x, const float* g, const float* x0, int N, int C, int HW, int mode, const float* eps, const float* step,
            const float* lo, const float* hi, void* ws, float* out, float* gnorm) {
    if (!x || !g || !eps || !out || N < 1 || C < 1 || HW < 1 || (mode != 0 && mode != 1) || (lo == nullptr) != (hi == nullptr)) return UDAPOSE_ERR_ARG;
    const long long D = (long long)C * HW;
    const int B = perturb_blocks(D);
    if ((long long)N * B > 0x7fffffffll || D > 0x7fffffffll - 4 * PT_THREADS) return UDAPOSE_ERR_UNSUPPORTED;
    const size_t bytes = (size_t)N * D * sizeof(float);
    if ((const char*)out < (const char*)g + bytes && (const char*)g < (const char*)out + bytes) return UDAPOSE_ERR_ARG;       // out overlaps g
    const bool need_norm = mode == 0 || gnorm != nullptr;
    const bool project = mode == 0 && (x0 != nullptr || step != nullptr);
    if (need_norm && (!ws || ((uintptr_t)ws & 3))) return UDAPOSE_ERR_ARG;
    PtArgs a{};
    a.x = x; a.g = g; a.x0 = x0; a.lo = lo; a.hi = hi; a.eps = eps; a.step = step; a.out = out; a.gnorm = gnorm;
    a.D = D; a.chunk = perturb_chunk(D, B); a.HW = HW; a.C = C; a.B = B; a.mode = mode;
    float* part_g = (float*)ws;
    float* part_d = part_g ? part_g + (size_t)N * B : nullptr;
    const bool vec = HW % 4 == 0 && aligned16(x) && aligned16(g) && aligned16(out) && (!x0 || aligned16(x0));
    const dim3 grid((unsigned)(N * B)), block(PT_THREADS);
    if (need_norm) {
        a.part_out = part_g;
        if (vec) hipLaunchKernelGGL((perturb_sumsq_k<4, 0>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((perturb_sumsq_k<1, 0>), grid, block, 0, s, a);
        a.part_g = part_g;
        if (project) {
            a.part_out = part_d;
            if (vec) hipLaunchKernelGGL((perturb_sumsq_k<4, 1>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((perturb_sumsq_k<1, 1>), grid, block, 0, s, a);
            a.part_d = part_d;
        }
        a.part_out = nullptr;
    }
    if (vec) hipLaunchKernelGGL((perturb_apply_k<4>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((perturb_apply_k<1>), grid, block, 0, s, a);
    return udapose_check_launch();
}
