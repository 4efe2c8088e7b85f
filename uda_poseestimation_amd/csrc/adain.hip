// AdaIN feature re-normalisation (lib/models/Style_net.py:4-29,167-168) on NHWC features (element type or fp32):
// out = alpha*((c-mu_c)/sd_c*sd_s+mu_s) + (1-alpha)*c with per-(n,c) statistics over H*W.  HBM-bound: the algorithmic minimum
// is content + style in, result out (201 MB for [32,512,32,32] fp32, 100 MB in bf16).
#include "style.h"
#include "storage8.h"

namespace {
constexpr int TPB = 256;

// One work-group of 1024 threads (16 waves: the CU's memory pipeline needs that many loads in flight - the 256-thread form
// of round 1 moved 2.1 TB/s) per (image, 64-channel slab): 8 channel groups x 128 pixel lanes, every lane moves 16 (bf16) or 32
// (fp32) contiguous bytes per pixel, a wave covers whole 128- / 256-byte pixel rows of the slab.  Pass 1 sweeps content and
// style once for the per-(n,c) sums (lane partials -> three xor steps inside the wave -> one LDS row per wave); the first
// CACHE pixels of each lane's content stay in registers, so for feature maps up to 128 * CACHE = 1024 pixels (relu4_1 of a
// 256x256 image: the training shape) pass 2 re-reads nothing: the kernel moves the algorithmic minimum (content + style in,
// result out).  Larger maps re-read the uncached remainder.  Unbiased variance + eps like the reference.
// The sums are taken about a per-channel pivot k = the channel's first pixel (every lane of a channel group loads the same 16 / 32
// bytes of pixel 0: one line, one extra load): sum (x - k) and sum (x - k)^2, mean = k + s1 / HW, var = (s2 - s1^2 / HW) / (HW - 1).
// The one-pass form about zero loses mean^2 / var of its precision (a channel at 100 +- 0.01 came out with a non-positive variance
// and NaN outputs); about a pivot inside the data the loss is at most 1 + max|x - mean|^2 / var, whatever the mean.
constexpr int ATPB = 1024, APL = ATPB / 8, CACHE = 8;

template <typename T>
__global__ __launch_bounds__(ATPB) void adain_k(const T* __restrict__ content, const T* __restrict__ style, T* __restrict__ out, int HWc, int HWs,
                                                int C, float eps, float alpha, const float* __restrict__ alpha_dev, float* __restrict__ stats_out) {
    if (alpha_dev) alpha = *alpha_dev;      // (a captured launch reads the step's blend factor from device memory)
    __shared__ float red[ATPB / 64][8][4][8];   // [wave][cg][stat][e]  16 KiB
    __shared__ float coef[64][2];
    __shared__ float piv[2][64];                // the pivots of content and style
    const int slabs = C / 64;
    const int n = blockIdx.x / slabs, sl = blockIdx.x % slabs;
    const int cg = threadIdx.x & 7, pl = threadIdx.x >> 3;
    const int c0 = sl * 64 + cg * 8;
    const T* cp = content + (size_t)n * HWc * C + c0;
    const T* sp = style + (size_t)n * HWs * C + c0;
    const int wave = threadIdx.x >> 6;
    Raw8<T> keep[CACHE];
    {   // content: sums about the pivot + register cache
        float s1[8], s2[8], kv[8];
        ld8<T>(cp, kv);
        if (pl == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) piv[0][cg * 8 + e] = kv[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s1[e] = s2[e] = 0.f;
#pragma unroll
        for (int k = 0; k < CACHE; ++k) {
            const int p = pl + k * APL;
            if (p < HWc) {
                float v[8];
                ldraw(cp + (size_t)p * C, keep[k]);
                unraw(keep[k], v);
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float d = v[e] - kv[e]; s1[e] += d; s2[e] += d * d; }
            }
        }
        for (int p = pl + CACHE * APL; p < HWc; p += APL) {
            float v[8];
            ld8<T>(cp + (size_t)p * C, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[e] - kv[e]; s1[e] += d; s2[e] += d * d; }
        }
        // lanes of a wave with equal cg (lane & 7) hold partials of the same channels: xor over lane bits 3..5
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int o = 8; o < 64; o <<= 1) { s1[e] += __shfl_xor(s1[e], o, 64); s2[e] += __shfl_xor(s2[e], o, 64); }
        if ((threadIdx.x & 63) < 8) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { red[wave][cg][0][e] = s1[e]; red[wave][cg][1][e] = s2[e]; }
        }
    }
    {   // style: sums only
        float s1[8], s2[8], kv[8];
        ld8<T>(sp, kv);
        if (pl == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) piv[1][cg * 8 + e] = kv[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s1[e] = s2[e] = 0.f;
        for (int p = pl; p < HWs; p += APL) {
            float v[8];
            ld8<T>(sp + (size_t)p * C, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[e] - kv[e]; s1[e] += d; s2[e] += d * d; }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int o = 8; o < 64; o <<= 1) { s1[e] += __shfl_xor(s1[e], o, 64); s2[e] += __shfl_xor(s2[e], o, 64); }
        if ((threadIdx.x & 63) < 8) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { red[wave][cg][2][e] = s1[e]; red[wave][cg][3][e] = s2[e]; }
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int g = threadIdx.x >> 3, e = threadIdx.x & 7;
        double a[4] = {0, 0, 0, 0};
        for (int k = 0; k < ATPB / 64; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] += (double)red[k][g][q][e];
        const double dc = a[0] / HWc, ds = a[2] / HWs;      // mean - pivot
        const double mc = (double)piv[0][threadIdx.x] + dc, ms = (double)piv[1][threadIdx.x] + ds;
        const double vc = (a[1] - a[0] * dc) / (HWc - 1) + eps, vs = (a[3] - a[2] * ds) / (HWs - 1) + eps;
        const float sdc = (float)sqrt(vc > 0 ? vc : 0), sds = (float)sqrt(vs > 0 ? vs : 0);
        // out = alpha*((x-mc)/sdc*sds+ms) + (1-alpha)*x = x*(alpha*sds/sdc + 1-alpha) + alpha*(ms - mc*sds/sdc)
        // (alpha == 0 returns the content bit for bit: x * 1 + (-0) keeps both zeros' signs, whatever the statistics are)
        coef[threadIdx.x][0] = alpha == 0.f ? 1.f : alpha * (sds / sdc) + (1.f - alpha);
        coef[threadIdx.x][1] = alpha == 0.f ? -0.f : alpha * ((float)ms - (float)mc * (sds / sdc));
        if (stats_out) {
            float* so = stats_out + ((size_t)n * C + sl * 64 + threadIdx.x) * 4;
            so[0] = (float)mc; so[1] = sdc; so[2] = (float)ms; so[3] = sds;
        }
    }
    __syncthreads();
    if (!out) return;                     // statistics only (calc_mean_std)
    float k0[8], k1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { k0[e] = coef[cg * 8 + e][0]; k1[e] = coef[cg * 8 + e][1]; }
    T* op = out + (size_t)n * HWc * C + c0;
#pragma unroll
    for (int k = 0; k < CACHE; ++k) {
        const int p = pl + k * APL;
        if (p < HWc) {
            float v[8], o[8];
            unraw(keep[k], v);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = v[e] * k0[e] + k1[e];
            st8<T>(op + (size_t)p * C, o);
        }
    }
    for (int p = pl + CACHE * APL; p < HWc; p += APL) {
        float v[8], o[8];
        ld8<T>(cp + (size_t)p * C, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = v[e] * k0[e] + k1[e];
        st8<T>(op + (size_t)p * C, o);
    }
}
}  // namespace

int adain_launch(hipStream_t s, const elem_t* content, const elem_t* style, elem_t* out, int N, int HWc, int HWs, int C, float eps, float alpha,
                 const float* alpha_dev, float* stats_out) {
    if (C % 64 || HWc < 2 || HWs < 2) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(adain_k<elem_t>, dim3(N * (C / 64)), dim3(ATPB), 0, s, content, style, out, HWc, HWs, C, eps, alpha, alpha_dev, stats_out);
    return udapose_check_launch();
}
int adain_launch_f32(hipStream_t s, const float* content, const float* style, float* out, int N, int HWc, int HWs, int C, float eps, float alpha,
                     const float* alpha_dev, float* stats_out) {
    if (C % 64 || HWc < 2 || HWs < 2) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(adain_k<float>, dim3(N * (C / 64)), dim3(ATPB), 0, s, content, style, out, HWc, HWs, C, eps, alpha, alpha_dev, stats_out);
    return udapose_check_launch();
}
int adain_launch_split(hipStream_t s, const void* content, const void* style, void* out, int N, int HWc, int HWs, int C, float eps, float alpha,
                       const float* alpha_dev, float* stats_out) {
    if (C % 64 || HWc < 2 || HWs < 2) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(adain_k<sp32>, dim3(N * (C / 64)), dim3(ATPB), 0, s, (const sp32*)content, (const sp32*)style, (sp32*)out, HWc, HWs, C, eps, alpha,
                       alpha_dev, stats_out);
    return udapose_check_launch();
}

UDAPOSE_SP_SAT_READER(sp_sat_read_adain)
