// Heat-map kernels (fp32 NCHW [B,K,H*W] rows): JointsMSE / consistency losses (fwd+bwd), arg-max decode, Gaussian
// "rectify" stamping, k-th value confidence mask, PCK.  Pure HBM sweeps: one pass over each operand, one block per
// (b,k) row where a per-row result is needed.  Deterministic (no atomics).
#include "losses.h"
#include "kth_select.h"

namespace {
constexpr int TPB = 256;

// rows[r] = 0.5 * w[r] * sum((p-g)^2) / HW           (JointsMSE 'none' rows; mean of rows = 'mean' loss)
// rows[r] = m[r] * sum((s-t)^2) / HW                  (ConsLoss: mode 1)
// `valid` (optional, ConsLoss(valid_mask=), loss.py:129-130): per-PIXEL selection [B][HW] shared by the Kc rows of an image;
// unselected pixels contribute nothing and the caller divides by the selected count instead of B*HW.
__global__ void sqdiff_rows_k(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ w,
                              const unsigned char* __restrict__ mask, int HW, float half, float* __restrict__ rows,
                              const unsigned char* __restrict__ valid, int Kc) {
    __shared__ double red[TPB / 64];
    const size_t r = blockIdx.x;
    const float* pa = a + r * HW;
    const float* pb = b + r * HW;
    double s = 0.0;
    if (valid) {
        const unsigned char* pv = valid + (r / Kc) * HW;
        for (int i = threadIdx.x; i < HW; i += TPB) { const float d = pv[i] ? pa[i] - pb[i] : 0.f; s += (double)(d * d); }
    } else if ((HW & 3) == 0) {
        for (int i = threadIdx.x * 4; i < HW; i += TPB * 4) {
            const f32x4 x = *(const f32x4*)(pa + i), y = *(const f32x4*)(pb + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = x[e] - y[e]; s += (double)(d * d); }
        }
    } else {
        for (int i = threadIdx.x; i < HW; i += TPB) { const float d = pa[i] - pb[i]; s += (double)(d * d); }
    }
    const double t = block_sum<TPB / 64>(s, red);
    if (threadIdx.x == 0) {
        float f = half;
        if (w) f *= w[r];
        if (mask) f *= mask[r] ? 1.f : 0.f;
        rows[r] = (float)(t / HW) * f;
    }
}
// out = sum(rows) / R, or - with a pixel selection - sum(rows) * HW / (Kc * count): rows carry sum/HW, the mean runs over
// the `count` selected (b, h, w) positions of loss_map = mean over the Kc channels
__global__ void mean_rows_k(const float* __restrict__ rows, int R, float* __restrict__ out, const float* __restrict__ count, int HW, int Kc) {
    __shared__ double red[TPB / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < R; i += TPB) s += (double)rows[i];
    const double t = block_sum<TPB / 64>(s, red);
    if (threadIdx.x == 0) out[0] = count ? (float)(t * HW / ((double)Kc * (double)count[0])) : (float)(t / R);
}
// count[0] = number of non-zero bytes of m[0..n)
__global__ void mask_count_k(const unsigned char* __restrict__ m, size_t n, float* __restrict__ count) {
    __shared__ double red[TPB / 64];
    double s = 0.0;
    for (size_t i = threadIdx.x; i < n; i += TPB) s += m[i] ? 1.0 : 0.0;
    const double t = block_sum<TPB / 64>(s, red);
    if (threadIdx.x == 0) count[0] = (float)t;
}
// da = gscale[0] * coef * f[r] * (a-b), f = w or mask (or 1).  E elements per thread and step: 4 (16-byte loads; the launcher sees to
// HW % 4 == 0, so a quad lies in one row) or 1, for maps whose pixel count is no multiple of 4 (rows are then not 16-byte aligned).
template <int E>
__global__ void sqdiff_bwd_k(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ w,
                             const unsigned char* __restrict__ mask, const float* __restrict__ gscale, float coef, int HW,
                             size_t total, float* __restrict__ da, const unsigned char* __restrict__ valid, const float* __restrict__ count, int Kc) {
    typedef float vec __attribute__((ext_vector_type(E)));
    float gs = gscale ? gscale[0] : 1.f;
    if (count) gs *= (float)(((double)(total / HW) / Kc) * HW / (double)count[0]);     // B*HW / count: the mean runs over the selected pixels
    for (size_t i = ((size_t)blockIdx.x * TPB + threadIdx.x) * E; i < total; i += (size_t)gridDim.x * TPB * E) {
        const size_t r = i / HW;
        float f = gs * coef;
        if (w) f *= w[r];
        if (mask) f *= mask[r] ? 1.f : 0.f;
        const vec x = *(const vec*)(a + i), y = *(const vec*)(b + i);
        vec o;
#pragma unroll
        for (int e = 0; e < E; ++e) o[e] = f * (x[e] - y[e]);
        if (valid) {
            const unsigned char* pv = valid + (r / Kc) * HW + (i - r * HW);
#pragma unroll
            for (int e = 0; e < E; ++e) if (!pv[e]) o[e] = 0.f;
        }
        *(vec*)(da + i) = o;
    }
}

// (hm_better, the arg-max order: common.h; hm_key / hm_unkey, the k-th value order: kth_select.h)

// per row: max value, first flat arg-max, (x,y) zeroed when max <= 0  (utils.py:54-75 / keypoint_detection.py:9-37);
// optionally stamps the rectify patch (utils.py:77-109) into out (full row written: zeros elsewhere).
__global__ void argmax_rectify_k(const float* __restrict__ hm, int H, int W, float* __restrict__ maxv, int* __restrict__ idx_out,
                                 float* __restrict__ preds, float* __restrict__ rect, const float* __restrict__ patch, int rad) {
    __shared__ float sv[TPB / 64];
    __shared__ int si[TPB / 64];
    const size_t r = blockIdx.x;
    const int HW = H * W;
    const float* p = hm + r * HW;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < HW; i += TPB) {
        const float v = p[i];
        if (hm_better(v, i, bv, bi)) { bv = v; bi = i; }      // (NaN counts as the maximum, first index on ties: torch / numpy)
    }
    hm_block_best<TPB / 64>(bv, bi, sv, si);
    const bool pos = bv > 0.f;
    const int mx = pos ? bi % W : 0, my = pos ? bi / W : 0;
    if (threadIdx.x == 0) {
        if (maxv) maxv[r] = bv;
        if (idx_out) idx_out[r] = bi;
        if (preds) { preds[r * 2] = (float)mx; preds[r * 2 + 1] = (float)my; }
    }
    if (rect) {
        // reference quirk kept: bounds test compares x with H and y with W (utils.py:89)
        const bool skip = (mx >= H) || (my >= W);
        const int size = 2 * rad + 1;
        float* o = rect + r * HW;
        for (int i = threadIdx.x; i < HW; i += TPB) {
            const int y = i / W, x = i % W;
            const int gx = x - (mx - rad), gy = y - (my - rad);
            float v = 0.f;
            // image range: x in [max(0,ulx), min(brx,H)), y in [max(0,uly), min(bry,W))  (reference's h/w usage)
            if (!skip && gx >= 0 && gx < size && gy >= 0 && gy < size && x < H && y < W) v = patch[gy * size + gx];
            o[i] = v;
        }
    }
}

// k-th smallest (1-indexed) of n values, then mask[i] = (tm[i]*act[i]) > thr  (train_human.py:429-430), in ONE work-group:
// hm_kth_smallest (kth_select.h) over the contiguous vector.  NaN orders as the largest value and a NaN threshold gives an
// all-false mask, exactly like torch.kthvalue + `>`.  k_dev (hm_kth_mask_dev): k is read from device memory - one uniform load, the same
// for every thread - and held inside 1 ... n, so that a captured launch follows a host change of mask_ratio.
__global__ void kth_mask_k(const float* __restrict__ act, const float* __restrict__ tm, int n, int k, float* __restrict__ thr_out,
                           unsigned char* __restrict__ mask, const float* __restrict__ act_local, int n_local, const int* __restrict__ k_dev) {
    __shared__ unsigned int hist[256];
    __shared__ unsigned int pick[2];
    if (k_dev) k = hm_kth_clamp(k_dev[0], n);
    const float thr = hm_kth_smallest(act, 1, n, k, hist, pick);
    if (threadIdx.x == 0 && thr_out) thr_out[0] = thr;
    const float* al = act_local ? act_local : act;
    const int nl = act_local ? n_local : n;
    for (int i = threadIdx.x; i < nl; i += blockDim.x) mask[i] = ((tm ? tm[i] : 1.f) * al[i]) > thr ? 1 : 0;
}

// PCK from decoded coordinates (keypoint_detection.py:40-94): per key-point hits / counts over the batch.
__global__ void pck_k(const float* __restrict__ pred, const float* __restrict__ gt, int B, int K, float nh, float nw, float thr,
                      float* __restrict__ acc, float* __restrict__ avg_cnt) {
    // single block; thread per key-point
    __shared__ float s_acc[256];
    const int c = threadIdx.x;
    float a = -1.f;
    if (c < K) {
        int hits = 0, n = 0;
        for (int b = 0; b < B; ++b) {
            const float tx = gt[(b * K + c) * 2], ty = gt[(b * K + c) * 2 + 1];
            if (tx > 1.f && ty > 1.f) {
                const float dx = pred[(b * K + c) * 2] / nh - tx / nh, dy = pred[(b * K + c) * 2 + 1] / nw - ty / nw;
                ++n;
                hits += sqrtf(dx * dx + dy * dy) < thr;
            }
        }
        a = n ? (float)hits / n : -1.f;
        acc[c] = a;
    }
    s_acc[c] = a;
    __syncthreads();
    if (c == 0) {
        float t = 0.f; int cnt = 0;
        for (int i = 0; i < K; ++i) if (s_acc[i] >= 0.f) { t += s_acc[i]; ++cnt; }
        avg_cnt[0] = cnt ? t / cnt : 0.f;
        avg_cnt[1] = (float)cnt;
    }
}
}  // namespace

// valid / count / Kc: optional per-pixel selection [R/Kc][HW] of ConsLoss(valid_mask=) and its device-resident count (hm_mask_count)
int hm_sqdiff_rows(hipStream_t s, const float* a, const float* b, const float* w, const unsigned char* mask, int R, int HW, float half,
                   float* rows, float* mean_out, const unsigned char* valid, const float* count, int Kc) {
    if (valid && (!count || Kc < 1 || R % Kc)) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(sqdiff_rows_k, dim3(R), dim3(TPB), 0, s, a, b, w, mask, HW, half, rows, valid, Kc);
    if (mean_out) hipLaunchKernelGGL(mean_rows_k, dim3(1), dim3(TPB), 0, s, rows, R, mean_out, valid ? count : nullptr, HW, Kc);
    return udapose_check_launch();
}
int hm_sqdiff_bwd(hipStream_t s, const float* a, const float* b, const float* w, const unsigned char* mask, const float* gscale, float coef,
                  int R, int HW, float* da, const unsigned char* valid, const float* count, int Kc) {
    if (valid && (!count || Kc < 1 || R % Kc)) return UDAPOSE_ERR_ARG;
    const size_t total = (size_t)R * HW;
    const int E = HW % 4 ? 1 : 4;
    size_t blocks = (total / E + TPB - 1) / TPB;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(E == 4 ? sqdiff_bwd_k<4> : sqdiff_bwd_k<1>, dim3((int)blocks), dim3(TPB), 0, s, a, b, w, mask, gscale, coef, HW, total, da,
                       valid, valid ? count : nullptr, Kc);
    return udapose_check_launch();
}
int hm_mask_count(hipStream_t s, const unsigned char* m, size_t n, float* count) {
    hipLaunchKernelGGL(mask_count_k, dim3(1), dim3(TPB), 0, s, m, n, count);
    return udapose_check_launch();
}
int hm_argmax_rectify(hipStream_t s, const float* hm, int R, int H, int W, float* maxv, int* idx, float* preds, float* rect, const float* patch,
                      int rad) {
    hipLaunchKernelGGL(argmax_rectify_k, dim3(R), dim3(TPB), 0, s, hm, H, W, maxv, idx, preds, rect, patch, rad);
    return udapose_check_launch();
}
int hm_kth_mask(hipStream_t s, const float* act, const float* tm, int n, int k, float* thr_out, unsigned char* mask, const float* act_local,
                int n_local) {
    if (k < 1 || k > n || n > (1 << 22)) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(kth_mask_k, dim3(1), dim3(1024), 0, s, act, tm, n, k, thr_out, mask, act_local, n_local, nullptr);
    return udapose_check_launch();
}
// the same launch with k in device memory (the host checked its range when it uploaded it; the kernel holds it inside 1 ... n)
int hm_kth_mask_dev(hipStream_t s, const float* act, const float* tm, int n, const int* k_dev, float* thr_out, unsigned char* mask,
                    const float* act_local, int n_local) {
    if (!act || !k_dev || !mask || n < 1 || n > (1 << 22) || (act_local && n_local < 0)) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(kth_mask_k, dim3(1), dim3(1024), 0, s, act, tm, n, 0, thr_out, mask, act_local, n_local, k_dev);
    return udapose_check_launch();
}
int hm_pck(hipStream_t s, const float* pred, const float* gt, int B, int K, float nh, float nw, float thr, float* acc, float* avg_cnt) {
    if (K > 256) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(pck_k, dim3(1), dim3(256), 0, s, pred, gt, B, K, nh, nw, thr, acc, avg_cnt);
    return udapose_check_launch();
}
