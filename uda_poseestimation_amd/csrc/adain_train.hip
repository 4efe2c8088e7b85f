// Backward of the AdaIN style network's decoder pre-training step (reference adain/net.py:102-162, adain/function.py:3-11):
// the data and weight gradients of the reflection-padded 3x3 convolutions (with and without the nearest x2 upsample), the
// ceil-mode 2x2 max-pool backward, bias gradients, and the mean/std style loss and MSE content loss with their gradients.
// 16-bit NHWC activations and gradients (the build's element type), fp32 accumulation, fp32 weight gradients and losses.
//
// Reflect convolutions are run on the PADDED grid: a reflect-padded 3x3 conv over the logical map Hl x Wl (Hl = H << upsample)
// is a pad-0 3x3 conv over the (Hl+2) x (Wl+2) padded map.  Its data gradient is the existing implicit-GEMM dgrad of that
// pad-0 geometry into a padded buffer, followed by the fold below (reflection adjoint, upsample adjoint, ReLU mask, loss
// terms).  Its weight gradient gathers the padded input once (the forward's own addressing) and runs the existing LDS-DMA
// weight-gradient kernels on it with per-split partial tiles that one launch adds in split order: every reduction here is
// bit-reproducible (no atomics in arrival order).
#include "style.h"
#include "storage8.h"

namespace {
constexpr int TPB = 256;

constexpr size_t GRID_CAP = 65535u * 8;      // blocks of a grid-stride sweep

// padded rows (of Hl + 2) that land on logical row l after ReflectionPad2d(1): l + 1, plus 0 when l == 1, plus Hl + 1 when l == Hl - 2
__device__ __forceinline__ int pad_sources(int l, int Hl, int (&r)[3]) {
    int n = 0;
    if (l == 1) r[n++] = 0;
    r[n++] = l + 1;
    if (l == Hl - 2) r[n++] = Hl + 1;
    return n;
}

// x [N,H,W,C] -> P [N,Hl+2,Wl+2,C], P[n,py,px] = x[n, reflect(py-1, Hl) >> up, reflect(px-1, Wl) >> up]
__global__ void reflect_gather_k(const elem_t* __restrict__ x, elem_t* __restrict__ P, int N, int H, int W, int C, int up) {
    const int G = C >> 3, Hl = H << up, Wl = W << up, Hp = Hl + 2, Wp = Wl + 2;
    const size_t total = (size_t)N * Hp * Wp * G;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        int n, py, px, g;
        nhwg_of(i, G, Hp, Wp, n, py, px, g);
        const int sy = reflect1(py - 1, Hl) >> up, sx = reflect1(px - 1, Wl) >> up;
        *(elem8*)(P + i * 8) = *(const elem8*)(x + (((size_t)n * H + sy) * W + sx) * C + g * 8);
    }
}

// One thread per (n, y, x, 8 channels) of the physical map [N,H,W,C]:
//   g = fold(dP) (+ style-loss gradient) (+ content-loss gradient) (+ add_nchw) ; dx = mask ? g * (x > 0) : g
// fold: padded-grid gradient dP [N,Hl+2,Wl+2,C] -> logical (reflection adjoint, fixed summation order) -> physical (sum of each 2x2
// block when up).  Style term (mean/std loss of adain/net.py:137-146, std = sqrt(unbiased var + eps)):
//   gs_s * 2/(N*C) * [(m - m_t)/HW + (sd - sd_t) * (x - m) / ((HW - 1) * sd)],  stats [N][C][4] = (m, sd, m_t, sd_t)
// Content term: gs_c * c_scale * (x - t)  (c_scale = 2 / numel: nn.MSELoss).  gs_* are device scalars (the upstream gradients).
__global__ void fold_k(const elem_t* __restrict__ dP, int up, const elem_t* __restrict__ x, int mask, const float* __restrict__ stats,
                       const float* __restrict__ gs_s, const elem_t* __restrict__ t, const float* __restrict__ gs_c, float c_scale,
                       const float* __restrict__ add_nchw, int add_c, elem_t* __restrict__ dx, int N, int H, int W, int C, float term_scale) {
    const int G = C >> 3, Hl = H << up, Wl = W << up, Wp = Wl + 2;
    const size_t total = (size_t)N * H * W * G;
    const float ks = stats ? term_scale * gs_s[0] * 2.f / ((float)N * (float)C) : 0.f;
    const float kc = t ? term_scale * gs_c[0] * c_scale : 0.f;
    const float HW = (float)H * (float)W;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        int n, y, xw, g;
        nhwg_of(i, G, H, W, n, y, xw, g);
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        if (dP) {
            const size_t img = (size_t)n * (Hl + 2);
            for (int a = 0; a <= up; ++a) {
                int rows[3];
                const int nr = pad_sources((y << up) + a, Hl, rows);
                for (int b = 0; b <= up; ++b) {
                    int cols[3];
                    const int nc = pad_sources((xw << up) + b, Wl, cols);
                    for (int ri = 0; ri < nr; ++ri)
                        for (int ci = 0; ci < nc; ++ci) {
                            float v[8];
                            ld8(dP + ((img + rows[ri]) * Wp + cols[ci]) * C + g * 8, v);
#pragma unroll
                            for (int e = 0; e < 8; ++e) acc[e] += v[e];
                        }
                }
            }
        }
        float xv[8];
        if (x) ld8(x + i * 8, xv);
        if (stats) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float* st = stats + ((size_t)n * C + g * 8 + e) * 4;
                const float m = st[0], sd = st[1];
                acc[e] += ks * ((m - st[2]) / HW + (sd - st[3]) * (xv[e] - m) / ((HW - 1.f) * sd));
            }
        }
        if (t) {
            float tv[8];
            ld8(t + i * 8, tv);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += kc * (xv[e] - tv[e]);
        }
        if (add_nchw) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = g * 8 + e;
                if (c < add_c) acc[e] += term_scale * add_nchw[(((size_t)n * add_c + c) * H + y) * W + xw];
            }
        }
        if (mask) {
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = xv[e] > 0.f ? acc[e] : 0.f;
        }
        st8(dx + i * 8, acc);
    }
}

// MaxPool2d(2, 2, ceil_mode=True) backward, one thread per input (n, iy, ix, 8 channels): the gradient of output (iy/2, ix/2) goes to
// the FIRST maximum of its (clipped) window in scan order - torch's rule (`val > maxval || isnan(val)`), ties after ReLU included.
// mask: also apply the producer's ReLU mask (x > 0).
__global__ void maxpool2x2_ceil_bwd_k(const elem_t* __restrict__ x, const elem_t* __restrict__ dy, elem_t* __restrict__ dx, int N, int H, int W,
                                      int C, int mask) {
    const int G = C >> 3, Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const size_t total = (size_t)N * H * W * G;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        int n, iy, ix, g;
        nhwg_of(i, G, H, W, n, iy, ix, g);
        const int oy = iy >> 1, ox = ix >> 1, me = (iy & 1) * 2 + (ix & 1);
        float best[8];
        int arg[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { best[e] = -INFINITY; arg[e] = -1; }
        float mine[8];
        for (int k = 0; k < 4; ++k) {
            const int h = oy * 2 + (k >> 1), w = ox * 2 + (k & 1);
            if (h >= H || w >= W) continue;
            float v[8];
            ld8(x + (((size_t)n * H + h) * W + w) * C + g * 8, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (arg[e] < 0 || v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; arg[e] = k; }
                if (k == me) mine[e] = v[e];
            }
        }
        float d[8], o[8];
        ld8(dy + (((size_t)n * Ho + oy) * Wo + ox) * C + g * 8, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (arg[e] == me && (!mask || mine[e] > 0.f)) ? d[e] : 0.f;
        st8(dx + i * 8, o);
    }
}

// bias gradient, stage 1: rows [b*BG_ROWS, ...) of dy [M][C] -> part[b][C] (fixed lane order inside the work-group)
constexpr int BG_ROWS = 2048;
__global__ __launch_bounds__(TPB) void colsum_part_k(const elem_t* __restrict__ dy, float* __restrict__ part, int M, int C) {
    __shared__ float red[TPB][9];
    const int G = C >> 3;                      // C <= 8 * TPB (host-checked)
    const int lanes = TPB / G;                 // row lanes per channel group
    const int g = threadIdx.x % G, rl = threadIdx.x / G;
    const int r0 = blockIdx.x * BG_ROWS, r1 = min(M, r0 + BG_ROWS);
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    if (rl < lanes)
        for (int m = r0 + rl; m < r1; m += lanes) {
            float v[8];
            ld8(dy + (size_t)m * C + g * 8, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += v[e];
        }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[threadIdx.x][e] = s[e];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += TPB) {
        const int gg = c >> 3, e = c & 7;
        float a = 0.f;
        for (int l = 0; l < lanes; ++l) a += red[l * G + gg][e];
        part[(size_t)blockIdx.x * C + c] = a;
    }
}
// stage 2 (and the weight-gradient split sum): out[i] = sum_k part[k * stride + src(i)] in split order
__global__ void colsum_final_k(const float* __restrict__ part, float* __restrict__ out, int nparts, int C, int c_valid, float out_scale) {
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c >= c_valid) return;
    float a = 0.f;
    for (int k = 0; k < nparts; ++k) a += part[(size_t)k * C + c];
    out[c] = a * out_scale;
}
// weight-gradient split sum: parts [ks][Co][T][Ci] -> dw [co_valid][Ci][T] (torch Conv2d layout), splits added in order
__global__ void wsplit_sum_k(const float* __restrict__ parts, float* __restrict__ dw, int ks, int Co, int T, int Ci, int co_valid, float out_scale) {
    const size_t n = (size_t)co_valid * Ci * T, stride = (size_t)Co * T * Ci;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
        const int t = (int)(i % T);
        const size_t r = i / T;
        const int ci = (int)(r % Ci), co = (int)(r / Ci);
        const size_t src = ((size_t)co * T + t) * Ci + ci;
        float a = 0.f;
        for (int k = 0; k < ks; ++k) a += parts[k * stride + src];
        dw[i] = a * out_scale;
    }
}

// MSE of two 16-bit tensors of n elements (n % 8 == 0): fixed grid of partial sums, then one ordered sum
constexpr int MSE_BLOCKS = 512;
__global__ __launch_bounds__(TPB) void mse_part_k(const elem_t* __restrict__ a, const elem_t* __restrict__ b, float* __restrict__ part, size_t n8) {
    __shared__ float red[TPB / 64];
    float s = 0.f;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n8; i += (size_t)MSE_BLOCKS * TPB) {
        float va[8], vb[8];
        ld8(a + i * 8, va);
        ld8(b + i * 8, vb);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = va[e] - vb[e]; s += d * d; }
    }
    const float t = block_sum<TPB / 64>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}
__global__ __launch_bounds__(TPB) void mse_final_k(const float* __restrict__ part, float* __restrict__ out, float inv_n) {
    __shared__ float red[TPB / 64];
    float s = 0.f;
    for (int i = threadIdx.x; i < MSE_BLOCKS; i += TPB) s += part[i];
    const float t = block_sum<TPB / 64>(s, red);
    if (threadIdx.x == 0) out[0] = t * inv_n;
}

// style loss term from the statistics [R = N*C][4] = (m, sd, m_t, sd_t): out (+)= (sum (m - m_t)^2 + (sd - sd_t)^2) / R
__global__ __launch_bounds__(TPB) void style_loss_k(const float* __restrict__ stats, float* __restrict__ out, int R, int accumulate) {
    __shared__ float red[TPB / 64];
    float s = 0.f;
    for (int i = threadIdx.x; i < R; i += TPB) {
        const float* st = stats + (size_t)i * 4;
        const float dm = st[0] - st[2], ds = st[1] - st[3];
        s += dm * dm + ds * ds;
    }
    const float t = block_sum<TPB / 64>(s, red);
    if (threadIdx.x == 0) out[0] = (accumulate ? out[0] : 0.f) + t / (float)R;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool reflect3_ok(const ConvGeom& g) {
    return g.reflect && !g.transposed && g.KH == 3 && g.KW == 3 && g.stride == 1 && g.pad == 1 && g.Ci % 64 == 0 && g.Co % 64 == 0 &&
           (g.Hi << g.upsample) >= 2 && (g.Wi << g.upsample) >= 2;
}
// the pad-0 3x3 conv over the padded grid that the reflect conv g is
ConvGeom padded_geom(const ConvGeom& g) {
    ConvGeom p = g;
    p.Hi = (g.Hi << g.upsample) + 2;
    p.Wi = (g.Wi << g.upsample) + 2;
    p.pad = 0;
    p.reflect = 0;
    p.upsample = 0;
    return p;
}
size_t padded_bytes(const ConvGeom& g) {
    const ConvGeom p = padded_geom(g);
    return align256((size_t)p.N * p.Hi * p.Wi * p.Ci * sizeof(elem_t));
}
}  // namespace

size_t conv_bwd_ws_bytes(const ConvGeom& g) {
    if (!reflect3_ok(g)) return 0;
    const ConvGeom p = padded_geom(g);
    const int ks = wgrad_parts_plan(p.N * p.Ho() * p.Wo(), p.Ci, p.Co, 9, nullptr);
    return padded_bytes(g) + align256((size_t)ks * p.Co * 9 * p.Ci * sizeof(float));
}

int conv_bwd_prepare(const ConvGeom& g) {
    if (!reflect3_ok(g)) return UDAPOSE_ERR_UNSUPPORTED;
    const ConvGeom p = padded_geom(g);
    if (!get_tap_plan(p, 0) || !get_tap_plan(p, 1)) return UDAPOSE_ERR_UNSUPPORTED;
    return UDAPOSE_OK;
}

int conv_dgrad_reflect_padded(hipStream_t s, const ConvGeom& g, const elem_t* dy, const elem_t* w_bwd, elem_t* dP) {
    if (!reflect3_ok(g) || !dy || !w_bwd || !dP) return reflect3_ok(g) ? UDAPOSE_ERR_ARG : UDAPOSE_ERR_UNSUPPORTED;
    return conv_dgrad(s, padded_geom(g), dy, w_bwd, dP, nullptr, 0);
}

int reflect_fold(hipStream_t s, const elem_t* dP, int up, const elem_t* x, int mask, const float* stats, const float* gs_s, const elem_t* t,
                 const float* gs_c, float c_scale, const float* add_nchw, int add_c, elem_t* dx, int N, int H, int W, int C, float term_scale) {
    if (!dx || C % 8 || N < 1 || H < 1 || W < 1) return UDAPOSE_ERR_ARG;
    if (dP && ((H << up) < 2 || (W << up) < 2)) return UDAPOSE_ERR_ARG;
    if ((mask || stats || t) && !x) return UDAPOSE_ERR_ARG;
    if ((stats && (!gs_s || H * W < 2)) || (t && !gs_c) || (add_nchw && (add_c < 1 || add_c > C))) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(fold_k, dim3(grid_for((size_t)N * H * W * (C / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, dP, up, x, mask, stats, gs_s, t, gs_c, c_scale, add_nchw,
                       add_c, dx, N, H, W, C, term_scale);
    return udapose_check_launch();
}

int conv_dgrad_reflect(hipStream_t s, const ConvGeom& g, const elem_t* dy, const elem_t* w_bwd, elem_t* dx, const elem_t* mask_src, void* ws) {
    if (!ws) return UDAPOSE_ERR_ARG;
    const int rc = conv_dgrad_reflect_padded(s, g, dy, w_bwd, (elem_t*)ws);
    if (rc != UDAPOSE_OK) return rc;
    return reflect_fold(s, (const elem_t*)ws, g.upsample, mask_src, mask_src != nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr, 0, dx,
                        g.N, g.Hi, g.Wi, g.Ci, 1.f);
}

int conv_wgrad_reflect(hipStream_t s, const ConvGeom& g, const elem_t* dy, const elem_t* x, float* dw, int co_valid, void* ws, float out_scale) {
    if (!reflect3_ok(g)) return UDAPOSE_ERR_UNSUPPORTED;
    if (!dy || !x || !dw || !ws || co_valid < 1 || co_valid > g.Co) return UDAPOSE_ERR_ARG;
    const ConvGeom p = padded_geom(g);
    elem_t* P = (elem_t*)ws;
    float* parts = (float*)((char*)ws + padded_bytes(g));
    hipLaunchKernelGGL(reflect_gather_k, dim3(grid_for((size_t)p.N * p.Hi * p.Wi * (p.Ci / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, x, P, g.N, g.Hi, g.Wi, g.Ci,
                       g.upsample);
    int rc = udapose_check_launch();
    if (rc != UDAPOSE_OK) return rc;
    WgParams wp;
    rc = conv_wgrad_params(p, dy, P, parts, -1, &wp, nullptr);
    if (rc != UDAPOSE_OK) return rc;
    rc = wgrad_launch_parts(wp, parts, s);
    if (rc != UDAPOSE_OK) return rc;
    hipLaunchKernelGGL(wsplit_sum_k, dim3(grid_for((size_t)co_valid * g.Ci * 9, TPB, GRID_CAP)), dim3(TPB), 0, s, parts, dw, wp.ksplit, g.Co, 9, g.Ci, co_valid, out_scale);
    return udapose_check_launch();
}

int maxpool2x2_ceil_bwd(hipStream_t s, const elem_t* x, const elem_t* dy, elem_t* dx, int N, int H, int W, int C, int mask) {
    if (!x || !dy || !dx || C % 8 || N < 1 || H < 1 || W < 1) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(maxpool2x2_ceil_bwd_k, dim3(grid_for((size_t)N * H * W * (C / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, x, dy, dx, N, H, W, C, mask);
    return udapose_check_launch();
}

size_t bias_grad_ws_bytes(long long M, int C) { return (size_t)((M + BG_ROWS - 1) / BG_ROWS) * C * sizeof(float); }

int bias_grad(hipStream_t s, const elem_t* dy, float* db, long long M, int C, int c_valid, void* ws, float out_scale) {
    if (!dy || !db || !ws || M < 1 || C % 8 || C > 8 * TPB || c_valid < 1 || c_valid > C) return UDAPOSE_ERR_ARG;
    const int nb = (int)((M + BG_ROWS - 1) / BG_ROWS);
    hipLaunchKernelGGL(colsum_part_k, dim3(nb), dim3(TPB), 0, s, dy, (float*)ws, (int)M, C);
    int rc = udapose_check_launch();
    if (rc != UDAPOSE_OK) return rc;
    hipLaunchKernelGGL(colsum_final_k, dim3((c_valid + TPB - 1) / TPB), dim3(TPB), 0, s, (const float*)ws, db, nb, C, c_valid, out_scale);
    return udapose_check_launch();
}

size_t feat_mse_ws_bytes() { return MSE_BLOCKS * sizeof(float); }

int feat_mse_fwd(hipStream_t s, const elem_t* a, const elem_t* b, long long n, float* out, void* ws) {
    if (!a || !b || !out || !ws || n < 8 || n % 8) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(mse_part_k, dim3(MSE_BLOCKS), dim3(TPB), 0, s, a, b, (float*)ws, (size_t)(n / 8));
    int rc = udapose_check_launch();
    if (rc != UDAPOSE_OK) return rc;
    hipLaunchKernelGGL(mse_final_k, dim3(1), dim3(TPB), 0, s, (const float*)ws, out, (float)(1.0 / (double)n));
    return udapose_check_launch();
}

int style_stat_loss(hipStream_t s, const float* stats, int R, float* out, int accumulate) {
    if (!stats || !out || R < 1) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(style_loss_k, dim3(1), dim3(TPB), 0, s, stats, out, R, accumulate);
    return udapose_check_launch();
}
