// Merge of the k re-warped teacher views by agreement (the definitions are in include/udapose.h): per (sample, joint) plane
// the views' peaks, the medoid peak, the views within `radius` of it, their mean (or the plain mean of all views), an agreement gate for the
// consistency mask and, on request, the views' variance.  ONE launch in place of mean_views_k; no atomics, a fixed summation order, integer
// outputs that are exact.
// One work-group of 256 threads owns one plane; a thread owns the pixel quads 4t, 4t + 1024, ... of it.
//   pass 1: every thread keeps a running (max, first index) per view over its pixels (the first index wins a tie, NaN is the largest value: the
//           order of udapose_heatmap_argmax), reduced per wave by shuffles and across the four waves through 64 bytes of LDS per view.
//   decide: every thread reads the k reduced peaks back (a broadcast read) and forms validity, the k x k table of squared distances, the
//           medoid, the inlier mask, spread2 and agree from them - a few dozen integer operations on wave-uniform values, repeated by every
//           wave so that no second barrier and no broadcast of the mask is needed; thread 0 stores them.
//   pass 2: the views are read again (k * H * W * 4 bytes, <= 295 KB per plane, just read: they sit in L2) and the mean of the inliers is
//           stored.  The plain mean does not depend on the peaks: with mode "mean" and no energy pass 2 is folded into pass 1 and every
//           view is read once.  The views are never staged in LDS (a 96 x 96 plane of 8 views would take a CU's whole LDS for one group).
// 512 planes are 2 waves per SIMD: the launch is bound by the latency of a thread's loads, not by bandwidth.  Both passes therefore issue the
// loads of U quads per view before they use the first (U = 4 for up to four views, 2 for up to eight; the register arrays are sized by the
// view class KM = 2 / 4 / 8, the loops over views stay guarded by the runtime k).
// A quad is one 16-byte access when H * W % 4 == 0 and every pointer is 16-byte aligned (VEC), four element accesses cut at the plane's end
// otherwise; the pixels, their order within a thread and every reduction are the same in both forms, and so are all output bits.
#include "data.h"

namespace {
constexpr int TPB = 256;
constexpr int MAXV = 8;
struct MergeViews { const float* p[MAXV]; };        // by value in the kernel arguments: a captured launch holds the pointers

struct MergeOut {
    float* mean;
    int* peaks;          // [k][R][2] (x, y)
    float* maxvals;      // [k][R]
    int* inliers;        // [R] bit v: view v
    int* n_inliers;      // [R]
    int* spread2;        // [R]
    float* agree;        // [R] 0 / 1
    float* energy;       // [R]
};

// n (1..4) pixels of every view from element `at` on; the rest of the quad reads as 0 and is never used
template <bool VEC, int KM>
__device__ __forceinline__ void load_quad(const MergeViews& v, int k, size_t at, int n, float (&x)[KM][4]) {
#pragma unroll
    for (int j = 0; j < KM; ++j) {
        if (j < k) {
            if (VEC) {
                const f32x4 q = *(const f32x4*)(v.p[j] + at);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[j][e] = q[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[j][e] = e < n ? v.p[j][at + e] : 0.f;
            }
        }
    }
}
template <bool VEC>
__device__ __forceinline__ void store_quad(float* dst, int n, const float (&o)[4]) {
    if (VEC) {
        *(f32x4*)dst = (f32x4){o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (e < n) dst[e] = o[e];
    }
}
// the mean of the views named by `mask` (wave-uniform, not empty): added in view order, divided by their number.  Sums and one division
// only - nothing here can be contracted into a fused multiply-add, so the bits are those of mean_views_k.
template <int KM>
__device__ __forceinline__ void masked_mean(const float (&x)[KM][4], int k, unsigned mask, float div, float (&o)[4]) {
    bool first = true;
#pragma unroll
    for (int j = 0; j < KM; ++j) {
        if (j < k && ((mask >> j) & 1u)) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = first ? x[j][e] : o[e] + x[j][e];
            first = false;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = o[e] / div;
}
// hm_better(v, i, bv, bi) for i > bi, a thread's own ascending sweep: a later pixel wins only with a larger value, or as the first NaN
__device__ __forceinline__ bool later_better(float v, float bv) { return v > bv || (v != v && bv == bv); }

template <bool VEC, int KM, int U>
__global__ __launch_bounds__(TPB) void view_merge_k(MergeViews v, int k, int H, int W, int trimmed, const float* __restrict__ radius_dev,
                                                    int min_views, MergeOut out, int R) {
    __shared__ float sv[TPB / 64][MAXV];
    __shared__ int si[TPB / 64][MAXV];
    __shared__ double se[TPB / 64];
    const size_t r = blockIdx.x;
    const int HW = H * W, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t base = r * (size_t)HW;
    const unsigned all = (1u << k) - 1u;
    const float fk = (float)k;
    const bool two_pass = trimmed || out.energy;

    // ---- pass 1: per-view (max, first index); the plain mean on the way when nothing else is asked of the values
    float bv[KM];
    int bi[KM];
#pragma unroll
    for (int j = 0; j < KM; ++j) { bv[j] = -INFINITY; bi[j] = 0x7fffffff; }
    for (int i0 = threadIdx.x * 4; i0 < HW; i0 += TPB * 4 * U) {
        float x[U][KM][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * TPB * 4;
            if (i < HW) load_quad<VEC, KM>(v, k, base + i, VEC ? 4 : (HW - i < 4 ? HW - i : 4), x[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * TPB * 4;
            if (i >= HW) continue;
            const int n = VEC ? 4 : (HW - i < 4 ? HW - i : 4);
#pragma unroll
            for (int j = 0; j < KM; ++j) {
                if (j < k) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < n && later_better(x[u][j][e], bv[j])) { bv[j] = x[u][j][e]; bi[j] = i + e; }
                }
            }
            if (!two_pass) {
                float o[4];
                masked_mean<KM>(x[u], k, all, fk, o);
                store_quad<VEC>(out.mean + base + i, n, o);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < KM; ++j) {
        if (j < k) {
            // (a thread whose pixels are all -inf has replaced nothing: its first pixel is its first maximum)
            if (bi[j] == 0x7fffffff && (int)threadIdx.x * 4 < HW) bi[j] = threadIdx.x * 4;
            hm_wave_best(bv[j], bi[j]);
            if (lane == 0) { sv[wave][j] = bv[j]; si[wave][j] = bi[j]; }
        }
    }
    __syncthreads();

    // ---- decide (every thread, on wave-uniform values)
    int px[KM], py[KM];
    unsigned valid = 0u;
#pragma unroll
    for (int j = 0; j < KM; ++j) {
        px[j] = py[j] = 0;
        if (j < k) {
            float m = sv[0][j];
            int ix = si[0][j];
#pragma unroll
            for (int w = 1; w < TPB / 64; ++w)
                if (hm_better(sv[w][j], si[w][j], m, ix)) { m = sv[w][j]; ix = si[w][j]; }
            px[j] = ix % W;
            py[j] = ix / W;
            if (m > 0.f) valid |= 1u << j;
            if (threadIdx.x == 0) {
                if (out.peaks) { out.peaks[((size_t)j * R + r) * 2] = px[j]; out.peaks[((size_t)j * R + r) * 2 + 1] = py[j]; }
                if (out.maxvals) out.maxvals[(size_t)j * R + r] = m;
            }
        }
    }
    int medoid = -1, best = 0x7fffffff, spread = 0;
#pragma unroll
    for (int a = 0; a < KM; ++a) {
        if (!((valid >> a) & 1u)) continue;
        int sum = 0;
#pragma unroll
        for (int b = 0; b < KM; ++b) {
            if (!((valid >> b) & 1u)) continue;
            const int dx = px[a] - px[b], dy = py[a] - py[b], d2 = dx * dx + dy * dy;
            sum += d2;
            spread = d2 > spread ? d2 : spread;
        }
        if (sum < best) { best = sum; medoid = a; }          // (ascending a and a strict <: the lowest view wins a tie)
    }
    unsigned inl = 0u;
    if (medoid >= 0) {
        const float rad = radius_dev[0], r2 = rad * rad;
        int mx = 0, my = 0;
#pragma unroll
        for (int j = 0; j < KM; ++j) if (j == medoid) { mx = px[j]; my = py[j]; }
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (!((valid >> j) & 1u)) continue;
            const int dx = px[j] - mx, dy = py[j] - my;
            if ((float)(dx * dx + dy * dy) <= r2) inl |= 1u << j;
        }
    }
    const int n_in = __popc(inl);
    if (threadIdx.x == 0) {
        if (out.inliers) out.inliers[r] = (int)inl;
        if (out.n_inliers) out.n_inliers[r] = n_in;
        if (out.spread2) out.spread2[r] = spread;
        if (out.agree) out.agree[r] = n_in >= min_views ? 1.f : 0.f;
    }
    if (!two_pass) return;

    // ---- pass 2: the mean of the inliers (of all views where there is none, or in mode "mean"), the variance of all views
    const unsigned use = (trimmed && n_in > 0) ? inl : all;
    const float div = (trimmed && n_in > 0) ? (float)n_in : fk;
    const bool want_e = out.energy != nullptr;
    double es = 0.0;
    for (int i0 = threadIdx.x * 4; i0 < HW; i0 += TPB * 4 * U) {
        float x[U][KM][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * TPB * 4;
            if (i < HW) load_quad<VEC, KM>(v, k, base + i, VEC ? 4 : (HW - i < 4 ? HW - i : 4), x[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * TPB * 4;
            if (i >= HW) continue;
            const int n = VEC ? 4 : (HW - i < 4 ? HW - i : 4);
            float o[4];
            masked_mean<KM>(x[u], k, use, div, o);
            store_quad<VEC>(out.mean + base + i, n, o);
            if (want_e) {
                float m[4];
                if (use == all) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) m[e] = o[e];
                } else {
                    masked_mean<KM>(x[u], k, all, fk, m);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < KM; ++j)
                        if (j < k) { const float d = x[u][j][e] - m[e]; s += d * d; }
                    if (e < n) es += (double)(s / fk);
                }
            }
        }
    }
    if (want_e) {
        // a thread's pixels in ascending index, the butterfly of a wave, the four waves in order: the same sum on every run
        es = wave_sum(es);
        if (lane == 0) se[wave] = es;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int w = 0; w < TPB / 64; ++w) t += se[w];
            out.energy[r] = (float)(t / (double)HW);
        }
    }
}

template <int KM, int U>
void launch(hipStream_t s, bool vec, const MergeViews& v, int k, int R, int H, int W, int trimmed, const float* radius_dev, int min_views,
            const MergeOut& out) {
    if (vec) hipLaunchKernelGGL((view_merge_k<true, KM, U>), dim3(R), dim3(TPB), 0, s, v, k, H, W, trimmed, radius_dev, min_views, out, R);
    else hipLaunchKernelGGL((view_merge_k<false, KM, U>), dim3(R), dim3(TPB), 0, s, v, k, H, W, trimmed, radius_dev, min_views, out, R);
}
}  // namespace

int affine_view_merge(hipStream_t s, const float* const* srcs, int k, int R, int H, int W, int mode, const float* radius_dev, int min_views,
                      float* mean, int* peaks, float* maxvals, int* inliers, int* n_inliers, int* spread2, float* agree, float* energy) {
    if (k < 1 || k > MAXV || !srcs || !mean || !radius_dev || min_views < 1 || min_views > k || R < 1 || H < 1 || W < 1) return UDAPOSE_ERR_ARG;
    if (mode != UDAPOSE_MERGE_MEAN && mode != UDAPOSE_MERGE_TRIMMED) return UDAPOSE_ERR_ARG;
    if (H > 2048 || W > 2048) return UDAPOSE_ERR_ARG;          // (squared peak distances stay exact in fp32, H * W in int)
    MergeViews v;
    for (int j = 0; j < MAXV; ++j) v.p[j] = j < k ? srcs[j] : nullptr;
    for (int j = 0; j < k; ++j) if (!v.p[j]) return UDAPOSE_ERR_ARG;
    const MergeOut out{mean, peaks, maxvals, inliers, n_inliers, spread2, agree, energy};
    bool vec = (H * W) % 4 == 0 && ((uintptr_t)mean & 15) == 0;
    for (int j = 0; j < k; ++j) vec = vec && ((uintptr_t)v.p[j] & 15) == 0;
    const int trimmed = mode == UDAPOSE_MERGE_TRIMMED;
    if (k <= 2) launch<2, 4>(s, vec, v, k, R, H, W, trimmed, radius_dev, min_views, out);
    else if (k <= 4) launch<4, 4>(s, vec, v, k, R, H, W, trimmed, radius_dev, min_views, out);
    else launch<8, 2>(s, vec, v, k, R, H, W, trimmed, radius_dev, min_views, out);
    return udapose_check_launch();
}
