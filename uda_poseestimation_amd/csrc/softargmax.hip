// Soft-argmax key-point decode and coordinate losses (fp32 NCHW rows [R = B*K][H*W]), forward and backward.  The row family of
// softmax_loss.hip (softmax_rows.h): one 256-thread block per (b,k) row, f32x4 loads where H*W % 4 == 0 and the row is 16-byte aligned,
// a row of up to 4096 floats read once and kept in registers across the passes, sums in double, no atomics (two runs give the same
// bits), a tiny second launch for the reduction over rows.
// Per row h_i, i = y * W + x:  (x*, y*) = the first flat arg-max in argmax_rectify_k's order (hm_better: NaN is the largest value),
// m = h_i*;  O = the whole map (window < 0) or {|x - x*| <= window, |y - y*| <= window} clipped to the map;
// p_i = exp(beta (h_i - m)) / Z over O;  cx = sum p_i x_i, cy = sum p_i y_i (pixel-index units).  The arg-max is a constant of the
// gradient: dh_i = beta p_i ((x_i - cx) gx + (y_i - cy) gy) in O, 0 outside.  m = NaN / +-inf makes exp(beta (h - m)) NaN: NaN coordinates.
// The forward stores per row what the backward needs (arg-max index; m, 1 / Z, cx, cy), so the backward is one sweep.
#include "softmax_rows.h"
#include "losses.h"

namespace {
// O as inclusive column bounds and the flat range [lo, hi) of its lines: most pixels are turned away by two compares, before any division
struct Win {
    int x0, x1, lo, hi;
    __device__ __forceinline__ Win(int idx, int H, int W, int window) {
        if (window < 0) { x0 = 0; x1 = W - 1; lo = 0; hi = H * W; return; }
        const int ys = idx / W, xs = idx - ys * W;
        x0 = max(xs - window, 0); x1 = min(xs + window, W - 1);      // (the launcher clamps window to max(H, W): no overflow)
        lo = max(ys - window, 0) * W; hi = (min(ys + window, H - 1) + 1) * W;
    }
    // pixel i is in O: its column and line through x, y
    __device__ __forceinline__ bool has(int i, int W, int& x, int& y) const {
        if (i < lo || i >= hi) return false;
        y = i / W; x = i - y * W;
        return x >= x0 && x <= x1;
    }
};
__device__ __forceinline__ bool row_vec(const void* a, const void* b, int HW) {
    return (HW & 3) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

struct SaRow { int idx; float m, inv, cx, cy; double cxd, cyd; };      // cxd, cyd: the forward's own unrounded quotients
// stats [4][R]: m, 1 / Z, cx, cy
__device__ __forceinline__ void sa_store(const SaRow& s, int* idx, float* stats, size_t R, size_t r) {
    idx[r] = s.idx; stats[r] = s.m; stats[R + r] = s.inv; stats[2 * R + r] = s.cx; stats[3 * R + r] = s.cy;
}
__device__ __forceinline__ SaRow sa_load(const int* idx, const float* stats, size_t R, size_t r) {
    const float cx = stats[2 * R + r], cy = stats[3 * R + r];
    return SaRow{idx[r], stats[r], stats[R + r], cx, cy, (double)cx, (double)cy};
}

// arg-max, Z and the two first moments of one row; every thread returns the row's result
__device__ __forceinline__ SaRow sa_row(const Row& S, int H, int W, float beta, int window, double* red, float* sv, int* si) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    each2(S, S, [&](int i, float v, float) { if (hm_better(v, i, bv, bi)) { bv = v; bi = i; } });
    hm_block_best<TPB / 64>(bv, bi, sv, si);
    const Win w(bi, H, W, window);
    double z = 0.0, sx = 0.0, sy = 0.0, unused = 0.0;
    each2(S, S, [&](int i, float v, float) {
        int x, y;
        if (!w.has(i, W, x, y)) return;
        const double e = (double)expf(beta * (v - bv));
        z += e; sx += e * (double)x; sy += e * (double)y;
    });
    block_sum2_d(z, sx, red);
    block_sum2_d(sy, unused, red);
    const double cx = sx / z, cy = sy / z;
    return SaRow{bi, bv, (float)(1.0 / z), (float)cx, (float)cy, cx, cy};
}
// dh_i = beta p_i ((x_i - cx) gx + (y_i - cy) gy) in O, 0 outside: the full row is written
__device__ __forceinline__ void sa_sweep(const float* __restrict__ h, float* __restrict__ dh, int H, int W, float beta, int window, const SaRow& s,
                                         float gx, float gy) {
    const Win w(s.idx, H, W, window);
    row_map(h, nullptr, dh, H * W, row_vec(h, dh, H * W), [&](int i, float v, float) {
        int x, y;
        if (!w.has(i, W, x, y)) return 0.f;
        return beta * (expf(beta * (v - s.m)) * s.inv) * (((float)x - s.cx) * gx + ((float)y - s.cy) * gy);
    });
}
// l(d) and l'(d): norm 0 |d| (sign(0) = 0, as torch's abs), norm 1 0.5 d^2
__device__ __forceinline__ double coord_l(int norm, double d) { return norm == 0 ? fabs(d) : 0.5 * d * d; }
__device__ __forceinline__ double coord_dl(int norm, double d) { return norm == 0 ? (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d)) : d; }
__device__ __forceinline__ float coord_factor(const float* w, const unsigned char* mask, size_t r) {
    float f = 1.f;
    if (w) f *= w[r];
    if (mask) f *= mask[r] ? 1.f : 0.f;
    return f;
}

__global__ __launch_bounds__(TPB) void sa_fwd_k(const float* __restrict__ hm, int H, int W, float beta, int window, int R, float* __restrict__ coords,
                                                float* __restrict__ maxv, int* __restrict__ idx, float* __restrict__ stats) {
    __shared__ double red[2 * TPB / 64];
    __shared__ float sv[TPB / 64];
    __shared__ int si[TPB / 64];
    const size_t r = blockIdx.x;
    const int HW = H * W;
    const Row S(hm + r * HW, HW, row_vec(hm, hm, HW));
    const SaRow s = sa_row(S, H, W, beta, window, red, sv, si);
    if (threadIdx.x == 0) {
        coords[2 * r] = s.cx; coords[2 * r + 1] = s.cy;
        maxv[r] = s.m;
        sa_store(s, idx, stats, R, r);
    }
}
__global__ __launch_bounds__(TPB) void sa_bwd_k(const float* __restrict__ hm, const float* __restrict__ g, const int* __restrict__ idx,
                                                const float* __restrict__ stats, int H, int W, float beta, int window, int R, float* __restrict__ dh) {
    const size_t r = blockIdx.x;
    const size_t HW = (size_t)H * W;
    sa_sweep(hm + r * HW, dh + r * HW, H, W, beta, window, sa_load(idx, stats, R, r), g[2 * r], g[2 * r + 1]);
}
// rows[r] = f_r (l((cx - tx_r) / W) + l((cy - ty_r) / H)), f_r = weight[r] * (mask[r] != 0)
__global__ __launch_bounds__(TPB) void coord_fwd_k(const float* __restrict__ hm, const float* __restrict__ tgt, const float* __restrict__ w,
                                                   const unsigned char* __restrict__ mask, int H, int W, float beta, int window, int norm, int R,
                                                   float* __restrict__ rows, int* __restrict__ idx, float* __restrict__ stats) {
    __shared__ double red[2 * TPB / 64];
    __shared__ float sv[TPB / 64];
    __shared__ int si[TPB / 64];
    const size_t r = blockIdx.x;
    const int HW = H * W;
    const Row S(hm + r * HW, HW, row_vec(hm, hm, HW));
    const SaRow s = sa_row(S, H, W, beta, window, red, sv, si);
    if (threadIdx.x == 0) {
        const double dx = (s.cxd - (double)tgt[2 * r]) / W, dy = (s.cyd - (double)tgt[2 * r + 1]) / H;
        rows[r] = (float)(coord_l(norm, dx) + coord_l(norm, dy)) * coord_factor(w, mask, r);
        sa_store(s, idx, stats, R, r);
    }
}
// the sweep with gx = gscale / R * f_r * l'((cx - tx) / W) / W, gy likewise with H
__global__ __launch_bounds__(TPB) void coord_bwd_k(const float* __restrict__ hm, const float* __restrict__ tgt, const float* __restrict__ w,
                                                   const unsigned char* __restrict__ mask, const int* __restrict__ idx, const float* __restrict__ stats,
                                                   const float* __restrict__ gscale, int H, int W, float beta, int window, int norm, int R,
                                                   float* __restrict__ dh) {
    const size_t r = blockIdx.x;
    const size_t HW = (size_t)H * W;
    const SaRow s = sa_load(idx, stats, R, r);
    const double c = (double)(gscale ? gscale[0] : 1.f) / R * (double)coord_factor(w, mask, r);
    const double dx = ((double)s.cx - (double)tgt[2 * r]) / W, dy = ((double)s.cy - (double)tgt[2 * r + 1]) / H;
    sa_sweep(hm + r * HW, dh + r * HW, H, W, beta, window, s, (float)(c * coord_dl(norm, dx) / W), (float)(c * coord_dl(norm, dy) / H));
}

// beta finite and > 0; the window is clamped to the map (any window >= max(H, W) - 1 is the whole map round any arg-max)
bool sa_args(int R, int H, int W, float beta, int& window) {
    if (R <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || !(beta > 0.f) || !(beta <= 3.402823466e38f)) return false;
    const int cap = H > W ? H : W;
    if (window > cap) window = cap;
    return true;
}
}  // namespace

int sa_fwd(hipStream_t st, const float* hm, int R, int H, int W, float beta, int window, float* coords, float* maxv, int* idx, float* stats) {
    if (!hm || !coords || !maxv || !idx || !stats || !sa_args(R, H, W, beta, window)) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(sa_fwd_k, dim3(R), dim3(TPB), 0, st, hm, H, W, beta, window, R, coords, maxv, idx, stats);
    return udapose_check_launch();
}
int sa_bwd(hipStream_t st, const float* hm, const float* g, const int* idx, const float* stats, int R, int H, int W, float beta, int window,
           float* dh) {
    if (!hm || !g || !idx || !stats || !dh || !sa_args(R, H, W, beta, window)) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(sa_bwd_k, dim3(R), dim3(TPB), 0, st, hm, g, idx, stats, H, W, beta, window, R, dh);
    return udapose_check_launch();
}
// group: rows per output value (R for reduction='mean', K for the per-sample means of 'none'); norm 0 = l1, 1 = l2
int sa_coord_fwd(hipStream_t st, const float* hm, const float* tgt, const float* w, const unsigned char* mask, int R, int group, int H, int W,
                 float beta, int window, int norm, float* rows, int* idx, float* stats, float* out) {
    if (!hm || !tgt || !rows || !idx || !stats || !out || !sa_args(R, H, W, beta, window) || group < 1 || R % group || (norm != 0 && norm != 1))
        return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(coord_fwd_k, dim3(R), dim3(TPB), 0, st, hm, tgt, w, mask, H, W, beta, window, norm, R, rows, idx, stats);
    hipLaunchKernelGGL(reduce_rows_k, dim3(R / group), dim3(TPB), 0, st, rows, group, 0.f, (double)group, nullptr, 1, out, nullptr);
    return udapose_check_launch();
}
int sa_coord_bwd(hipStream_t st, const float* hm, const float* tgt, const float* w, const unsigned char* mask, const int* idx, const float* stats,
                 const float* gscale, int R, int H, int W, float beta, int window, int norm, float* dh) {
    if (!hm || !tgt || !idx || !stats || !dh || !sa_args(R, H, W, beta, window) || (norm != 0 && norm != 1)) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(coord_bwd_k, dim3(R), dim3(TPB), 0, st, hm, tgt, w, mask, idx, stats, gscale, H, W, beta, window, norm, R, dh);
    return udapose_check_launch();
}
