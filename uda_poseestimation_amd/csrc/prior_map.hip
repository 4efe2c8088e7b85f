// Skeleton-prior maps (the reference's generate_prior_map, utils.py:111-145) and the pairwise joint-distance statistics that feed them.
// The reference materialises five [B][K][K][H][W] tensors; here one launch reads B*K decoded coordinates and two K x K tables and writes
// the [B][K][H][W] result once.  fp32 throughout the map (the statistics accumulate in fp64), no atomics, no scratch, nothing allocated.
#include "losses.h"
#include <math.h>

namespace {
constexpr int PM_TPB = 256;      // pixels of one image per work-group
constexpr int PM_JB = 8;         // outputs j accumulated in registers per pass over i
constexpr int PM_KMAX = 64;
constexpr int PD_TPB = 256;

// w[i][j], the weight of joint i's ring in output j.  Default mode: soft-max over i of -std[i][j] / gamma with the diagonal set to epsilon
// first (utils.py:139-141; max subtracted, so std = +inf weighs exactly 0).  v3: 1 / (1 + std[i][j]) (utils.py:132).  One thread per column.
__global__ void prior_weights_k(const float* __restrict__ sd, int K, float gamma, float epsilon, int v3, float* __restrict__ w) {
    const int j = threadIdx.x;
    if (j >= K) return;
    if (v3) {
        for (int i = 0; i < K; ++i) w[i * K + j] = 1.f / (1.f + sd[i * K + j]);
        return;
    }
    float mx = -INFINITY;
    for (int i = 0; i < K; ++i) {
        const float v = i == j ? epsilon : -sd[i * K + j] / gamma;
        mx = fmaxf(mx, v);
    }
    float sum = 0.f;
    for (int i = 0; i < K; ++i) {
        const float v = i == j ? epsilon : -sd[i * K + j] / gamma;
        sum += expf(v - mx);
    }
    for (int i = 0; i < K; ++i) {
        const float v = i == j ? epsilon : -sd[i * K + j] / gamma;
        w[i * K + j] = expf(v - mx) / sum;
    }
}

// out[b][j][y][x] = sum_i f[i][j] exp(-(d_i - mean[i][j])^2 / (2 sigma^2)),  d_i = |(x, y) - (cx_i, cy_i)|,  f = w (default) or conf[b][i] * w (v3);
// times hm[b][j][y][x] when hm is given.  A work-group owns PM_TPB consecutive pixels of one image: it stages the image's coordinates and both
// tables (f already multiplied by the confidences) in LDS, rows padded to a multiple of PM_JB with zero weights, and every thread owns one pixel:
// per pass of PM_JB outputs it walks i, forms d_i once (a correctly rounded square root of an exact integer: the reference's own number) and
// issues one v_exp_f32 per term with log2(e) / (2 sigma^2) folded into c2.  The table reads are wave-uniform LDS broadcasts; stores run along x.
__global__ void __launch_bounds__(PM_TPB) prior_map_k(const float* __restrict__ coords, const float* __restrict__ conf, const float* __restrict__ mean,
                                                      const float* __restrict__ w, const float* __restrict__ hm, int K, int Kp, int HW, int W,
                                                      int blocks_per_image, float c2, float* __restrict__ out) {
    extern __shared__ float lds[];
    float* s_mean = lds;                 // [K][Kp]
    float* s_w = lds + K * Kp;           // [K][Kp]
    float* s_cx = s_w + K * Kp;          // [K]
    float* s_cy = s_cx + K;              // [K]
    const int b = blockIdx.x / blocks_per_image;
    const int p = (blockIdx.x - b * blocks_per_image) * PM_TPB + threadIdx.x;
    for (int e = threadIdx.x; e < K * Kp; e += PM_TPB) {
        const int i = e / Kp, j = e - i * Kp;
        float m = 0.f, f = 0.f;
        if (j < K) {
            m = mean[i * K + j];
            f = w[i * K + j];
            if (conf) f = conf[(size_t)b * K + i] * f;      // (utils.py:134: the table times the confidence, then times the target)
        }
        s_mean[e] = m;
        s_w[e] = f;
    }
    for (int i = threadIdx.x; i < K; i += PM_TPB) {
        s_cx[i] = coords[((size_t)b * K + i) * 2];
        s_cy[i] = coords[((size_t)b * K + i) * 2 + 1];
    }
    __syncthreads();
    if (p >= HW) return;
    const int y = p / W;
    const float fx = (float)(p - y * W), fy = (float)y;
    const size_t base = (size_t)b * K * HW + p;
    for (int j0 = 0; j0 < K; j0 += PM_JB) {
        float acc[PM_JB];
#pragma unroll
        for (int e = 0; e < PM_JB; ++e) acc[e] = 0.f;
        for (int i = 0; i < K; ++i) {
            const float dx = fx - s_cx[i], dy = fy - s_cy[i];
            const float d = sqrtf(dx * dx + dy * dy);
            const float* pm = s_mean + i * Kp + j0;
            const float* pw = s_w + i * Kp + j0;
#pragma unroll
            for (int e = 0; e < PM_JB; ++e) {
                const float u = d - pm[e];
                acc[e] += pw[e] * __builtin_amdgcn_exp2f(-(u * u) * c2);
            }
        }
#pragma unroll
        for (int e = 0; e < PM_JB; ++e) {
            const int j = j0 + e;
            if (j < K) {
                const size_t o = base + (size_t)j * HW;
                out[o] = hm ? hm[o] * acc[e] : acc[e];
            }
        }
    }
}

// acc[0..2][i][j] += (count, sum d, sum d^2) over the samples m where joints i and j are both visible; d in fp64 from the fp32 coordinates.
// One work-group per pair: every thread adds its samples m = t, t + PD_TPB, ... in order, the partials meet in a fixed LDS tree, and thread 0
// alone adds the result into acc - the same batches in the same order give the same bits.
__global__ void __launch_bounds__(PD_TPB) pair_dist_accumulate_k(const float* __restrict__ coords, const unsigned char* __restrict__ vis, int M, int K,
                                                                 double* __restrict__ acc) {
    __shared__ double red[3][PD_TPB];
    const int i = blockIdx.x / K, j = blockIdx.x - i * K;
    double n = 0.0, s1 = 0.0, s2 = 0.0;
    for (int m = threadIdx.x; m < M; m += PD_TPB) {
        const size_t r = (size_t)m * K;
        if (vis[r + i] && vis[r + j]) {
            const double dx = (double)coords[(r + i) * 2] - (double)coords[(r + j) * 2];
            const double dy = (double)coords[(r + i) * 2 + 1] - (double)coords[(r + j) * 2 + 1];
            const double d2 = dx * dx + dy * dy;
            n += 1.0;
            s1 += sqrt(d2);
            s2 += d2;
        }
    }
    red[0][threadIdx.x] = n; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int o = PD_TPB / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const size_t KK = (size_t)K * K;
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q * KK + blockIdx.x] += red[q][0];
    }
}

// mean = sum d / n, std = sqrt(max(sum d^2 / n - mean^2, 0)) (population), both rounded to fp32 once; a pair never seen: mean 0, std +inf
__global__ void pair_dist_finish_k(const double* __restrict__ acc, int KK, float* __restrict__ mean, float* __restrict__ sd) {
    for (int p = threadIdx.x; p < KK; p += blockDim.x) {
        const double n = acc[p];
        if (n > 0.0) {
            const double mu = acc[KK + p] / n;
            double var = acc[2 * KK + p] / n - mu * mu;
            if (!(var > 0.0)) var = 0.0;
            mean[p] = (float)mu;
            sd[p] = (float)sqrt(var);
        } else {
            mean[p] = 0.f;
            sd[p] = INFINITY;
        }
    }
}
}  // namespace

static int pm_check_k(int K) {
    if (K < 1) return UDAPOSE_ERR_ARG;
    if (K > PM_KMAX) return UDAPOSE_ERR_UNSUPPORTED;
    return UDAPOSE_OK;
}

int pm_weights(hipStream_t s, const float* sd, int K, float gamma, float epsilon, int v3, float* w) {
    if (!sd || !w) return UDAPOSE_ERR_ARG;
    if (const int e = pm_check_k(K)) return e;
    if (!v3 && (!isfinite(gamma) || gamma == 0.f || epsilon != epsilon)) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(prior_weights_k, dim3(1), dim3(PM_KMAX), 0, s, sd, K, gamma, epsilon, v3 ? 1 : 0, w);
    return udapose_check_launch();
}

int pm_map(hipStream_t s, const float* coords, const float* conf, const float* mean, const float* w, const float* hm, int B, int K, int H, int W,
           float sigma, int v3, float* out) {
    if (!coords || !mean || !w || !out || (v3 && !conf)) return UDAPOSE_ERR_ARG;
    if (const int e = pm_check_k(K)) return e;
    if (B < 1 || H < 1 || W < 1 || !isfinite(sigma) || !(sigma > 0.f)) return UDAPOSE_ERR_ARG;
    const long long HW = (long long)H * W;
    if (HW > (1ll << 30)) return UDAPOSE_ERR_UNSUPPORTED;
    const long long bpi = (HW + PM_TPB - 1) / PM_TPB;
    if (bpi * B > 0x7fffffffll) return UDAPOSE_ERR_UNSUPPORTED;
    const int Kp = (K + PM_JB - 1) / PM_JB * PM_JB;
    const size_t lds = (size_t)(2 * K * Kp + 2 * K) * sizeof(float);       // 33 280 bytes at K = 64
    const float c2 = (float)(1.4426950408889634 / (2.0 * (double)sigma * (double)sigma));
    hipLaunchKernelGGL(prior_map_k, dim3((unsigned)(bpi * B)), dim3(PM_TPB), lds, s, coords, v3 ? conf : nullptr, mean, w, hm, K, Kp, (int)HW, W, (int)bpi,
                       c2, out);
    return udapose_check_launch();
}

int pm_pair_accumulate(hipStream_t s, const float* coords, const unsigned char* vis, int M, int K, double* acc) {
    if (!coords || !vis || !acc || M < 1) return UDAPOSE_ERR_ARG;
    if (const int e = pm_check_k(K)) return e;
    hipLaunchKernelGGL(pair_dist_accumulate_k, dim3(K * K), dim3(PD_TPB), 0, s, coords, vis, M, K, acc);
    return udapose_check_launch();
}

int pm_pair_finish(hipStream_t s, const double* acc, int K, float* mean, float* sd) {
    if (!acc || !mean || !sd) return UDAPOSE_ERR_ARG;
    if (const int e = pm_check_k(K)) return e;
    hipLaunchKernelGGL(pair_dist_finish_k, dim3(1), dim3(PD_TPB), 0, s, acc, K * K, mean, sd);
    return udapose_check_launch();
}
