// Sub-pixel key-point decodes (fp32 only: both builds of the library export identical code), one launch, one work-group per map:
//   mode 0 (quarter) : arg-max + a quarter pixel towards the higher neighbour (Simple Baselines)
//   mode 1 (DARK)    : arg-max + one Newton step on the logarithm of the Gaussian-blurred map (the definitions: include/udapose.h)
// The arg-max is argmax_rectify_k's: hm_better is a total order, so the winner does not depend on the reduction tree.  DARK stages the
// map in LDS while it looks for the arg-max, blurs it there (rows: A -> B, columns: B -> A) and takes max(g) and the 13 stencil values
// from A: g never reaches memory.  A and B are flat [H * W] arrays and a wave's lanes walk the flat index in both passes, so every
// ds_read_b32 of a 32-lane group covers 32 consecutive dwords = 32 different banks, in the column pass as in the row pass, whatever W is:
// no padding.  Taps are added in ascending order by the pixel's one owner thread, max(g) is reduced under hm_better's order again: no
// atomics, no scratch, and two calls give the same bits.
#include <math.h>
#include "conv_plan.h"      // max_dynamic_lds
#include "losses.h"

namespace {
constexpr int TPB = 256;
constexpr int MAX_TAPS = 31;
constexpr size_t LDS_BUDGET = (size_t)UDAPOSE_REFINE_MAX_PIXELS * 2 * sizeof(float);      // 150 KiB of the CU's 160
struct Taps { float t[MAX_TAPS]; };

// every thread returns the block's best (value, flat index) under hm_better: common.h's block arg-max
__device__ __forceinline__ void block_best(float& bv, int& bi, float* sv, int* si) { hm_block_best<TPB / 64>(bv, bi, sv, si); }

template <int MODE>
__global__ __launch_bounds__(TPB) void refine_decode_k(const float* __restrict__ hm, int H, int W, int ksize, const Taps taps,
                                                       float* __restrict__ coords, float* __restrict__ maxv, int* __restrict__ idx_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float sv[TPB / 64], st[MAX_TAPS];
    __shared__ int si[TPB / 64];
    const size_t r = blockIdx.x;
    if (MODE == 1 && threadIdx.x < MAX_TAPS) st[threadIdx.x] = taps.t[threadIdx.x];      // (published by block_best's barriers)
    const int HW = H * W;
    const float* h = hm + r * (size_t)HW;
    float* A = (float*)smem;          // the map, then g (MODE 1 only)
    float* B = A + HW;                // the row-blurred map
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < HW; i += TPB) {
        const float v = h[i];
        if (MODE == 1) A[i] = v;
        if (hm_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    block_best(bv, bi, sv, si);       // (its barriers also publish A)
    const float m = bv;
    const int ys = bi / W, xs = bi - ys * W;
    if (threadIdx.x == 0) {
        if (maxv) maxv[r] = m;
        if (idx_out) idx_out[r] = bi;
    }
    const bool pos = m > 0.f;
    float cx = pos ? (float)xs : 0.f, cy = pos ? (float)ys : 0.f;
    if (MODE == 0) {
        if (threadIdx.x != 0) return;
        if (pos && xs > 1 && xs < W - 1 && ys > 1 && ys < H - 1) {
            cx += 0.25f * sign_or_0(h[bi + 1] - h[bi - 1]);
            cy += 0.25f * sign_or_0(h[bi + W] - h[bi - W]);
        }
        coords[2 * r] = cx; coords[2 * r + 1] = cy;
        return;
    }
    // (uniform over the block: m, xs, ys are the same in every thread)
    if (!(pos && xs > 1 && xs < W - 2 && ys > 1 && ys < H - 2)) {
        if (threadIdx.x == 0) { coords[2 * r] = cx; coords[2 * r + 1] = cy; }
        return;
    }
    const int c = ksize >> 1;
    // rows: B[y][x] = sum_j t_j A[y][x + j - c], the taps that fall on the zero padding left out
    for (int i = threadIdx.x; i < HW; i += TPB) {
        const int y = i / W, x = i - y * W;
        float acc = 0.f;
        for (int j = 0; j < ksize; ++j) {
            const int xx = x + j - c;
            if (xx >= 0 && xx < W) acc = fmaf(st[j], A[i + j - c], acc);
        }
        B[i] = acc;
    }
    __syncthreads();
    // columns: g[y][x] = sum_j t_j B[y + j - c][x], over A; max(g) under hm_better's order (NaN is the largest)
    float gv = -INFINITY;
    int gi = 0x7fffffff;
    for (int i = threadIdx.x; i < HW; i += TPB) {
        const int y = i / W;
        float acc = 0.f;
        for (int j = 0; j < ksize; ++j) {
            const int yy = y + j - c;
            if (yy >= 0 && yy < H) acc = fmaf(st[j], B[i + (j - c) * W], acc);
        }
        A[i] = acc;
        if (hm_better(acc, i, gv, gi)) { gv = acc; gi = i; }
    }
    block_best(gv, gi, sv, si);       // (its barriers also publish g)
    if (threadIdx.x != 0) return;
    if (gv > 0.f) {
        const float scale = m / gv;
        auto L = [&](int dy, int dx) { return logf(fmaxf(A[bi + dy * W + dx] * scale, 1e-10f)); };
        const float g00 = L(0, 0);
        const float dx = 0.5f * (L(0, 1) - L(0, -1)), dy = 0.5f * (L(1, 0) - L(-1, 0));
        const float dxx = 0.25f * (L(0, 2) - 2.f * g00 + L(0, -2)), dyy = 0.25f * (L(2, 0) - 2.f * g00 + L(-2, 0));
        const float dxy = 0.25f * (L(1, 1) - L(-1, 1) - L(1, -1) + L(-1, -1));
        const float det = dxx * dyy - dxy * dxy;
        if (det != 0.f) {             // (a NaN determinant goes on and is caught as a NaN offset)
            const float ox = -(dyy * dx - dxy * dy) / det, oy = -(dxx * dy - dxy * dx) / det;
            if (fabsf(ox) <= 3.402823466e38f && fabsf(oy) <= 3.402823466e38f) { cx += ox; cy += oy; }
        }
    }
    coords[2 * r] = cx; coords[2 * r + 1] = cy;
}
}  // namespace

int refine_decode(hipStream_t s, const float* hm, int R, int H, int W, int mode, int kernel, float sigma, float* coords, float* maxv, int* idx) {
    if (!hm || !coords || R < 1 || H < 1 || W < 1 || (mode != 0 && mode != 1) || (long long)H * W > 0x7fffffffLL) return UDAPOSE_ERR_ARG;
    Taps taps = {};
    if (mode == 0) {
        hipLaunchKernelGGL(refine_decode_k<0>, dim3(R), dim3(TPB), 0, s, hm, H, W, 0, taps, coords, maxv, idx);
        return udapose_check_launch();
    }
    if (kernel < 3 || kernel > MAX_TAPS || (kernel & 1) == 0 || !(sigma <= 3.402823466e38f)) return UDAPOSE_ERR_ARG;
    if ((long long)H * W > UDAPOSE_REFINE_MAX_PIXELS) return UDAPOSE_ERR_ARG;
    const int c = kernel >> 1;
    const double sg = sigma > 0.f ? (double)sigma : 0.3 * (c - 1) + 0.8;
    double e[MAX_TAPS], sum = 0.0;
    for (int i = 0; i < kernel; ++i) { e[i] = exp(-(double)((i - c) * (i - c)) / (2.0 * sg * sg)); sum += e[i]; }
    for (int i = 0; i < kernel; ++i) taps.t[i] = (float)(e[i] / sum);
    max_dynamic_lds<refine_decode_k<1>>((int)LDS_BUDGET);
    const unsigned bytes = (unsigned)((size_t)H * W * 2 * sizeof(float) + 15) & ~15u;
    hipLaunchKernelGGL(refine_decode_k<1>, dim3(R), dim3(TPB), bytes, s, hm, H, W, kernel, taps, coords, maxv, idx);
    return udapose_check_launch();
}
