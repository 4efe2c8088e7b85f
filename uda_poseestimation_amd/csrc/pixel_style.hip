// Histogram matching and colour-statistics transfer as style bridges without weights (lib/models/pixel_style.py).
// fp32 NCHW images in and out, nothing depends on the library's element type.  A plane is one (n, c) channel; HW = H W <= 2^24.
//
// LEVEL of a pixel:  l = (int) min(max(rint(fmaf(x, std_c, mean_c) * 255), 0), 255)   (std 1, mean 0 without normalisation)
//   evaluated in fp32 exactly as written; the clamp comes before the cast, so out-of-range, infinite and NaN pixels land on a bound.
// SUMMARY of a batch: int32 words, per sample a row of C * 256 (+ 8 when C == 3) words:
//   words [c * 256 + k]          the count of level k in channel c (uint32)
//   words [768 .. 773] (C == 3)  three uint64 (low word first): sum l_0 l_1, sum l_0 l_2, sum l_1 l_2; words 774, 775 stay zero
//   All integer: a clear kernel zeroes the buffer (never a memset node), then every work-group counts PIXEL_SHARE pixels of a plane
//   (of a sample's three planes when C == 3) in LDS and adds its counts with integer atomics - exact whatever the order.
// TRANSFER: out = x + alpha (T - l) inv_c, inv_c = 1 / (255 std_c), then the optional clamp.  Every work-group rebuilds what its plane
//   (sample) needs from the two summaries, in fp64 from the integers, rounded once to fp32:
//   hist      tab[k] = T(k) - k, the histogram-matching recipe of scikit-image's match_histograms on integer cumulative counts
//   meanstd   T - l = A l + B,  A = g - 1, B = 255 (mu_s - g mu_c), g = sqrt(var_s + eps) / sqrt(var_c + eps)   (unbiased variances, raw units)
//   cholesky  T_a - l_a = sum_b K[a][b] l_b + K[a][3],  K = [L_s L_c^-1 - I | 255 (mu_s - L_s L_c^-1 mu_c)],  L = chol(Sigma + eps I)
//   and then streams PIXEL_SHARE pixels: per pixel d = tab[l] | fmaf(A, l, B) | three fmaf, t = alpha d, out = t == 0 ? x : fmaf(t, inv_c, x).
// There are no floating-point atomics in this file.
#include "style.h"
#include "lds_hist.h"

namespace {
constexpr int TPB = 256;                        // one thread per level where a table is built
constexpr int SHARE = UDAPOSE_PIXEL_SHARE;      // pixels of a plane per work-group, both kernels
constexpr int CROSS_WORDS = 8;
static_assert(TPB == 256 && SHARE % (4 * TPB) == 0, "a thread per level; a share is whole float4 rounds");

__host__ __device__ inline int row_words(int C) { return C * 256 + (C == 3 ? CROSS_WORDS : 0); }

__device__ __forceinline__ float level_f(float x, float sd, float mu) {
    const float v = rintf(fmaf(x, sd, mu) * 255.f);
    return fminf(fmaxf(v, 0.f), 255.f);         // (fmaxf of a NaN and 0 is 0)
}

// n floats from `a` (and written to `b`, or b == a): `head` of them one by one up to the first 16-byte boundary, then nvec float4, then the rest.
// Without a common boundary everything goes one by one (head = n).
struct Span {
    int head, nvec;
};
__device__ __forceinline__ Span span_of(const void* a, const void* b, int n, bool planes_agree) {
    Span s{n, 0};
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b;
    if (planes_agree && ((ua ^ ub) & 15) == 0) {
        const int h = (int)(((16 - (ua & 15)) & 15) >> 2);
        if (h <= n) {
            s.head = h;
            s.nvec = (n - h) >> 2;
        }
    }
    return s;
}

__device__ __forceinline__ float& lane_of(float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

__global__ __launch_bounds__(TPB) void pixel_clear_k(unsigned int* __restrict__ p, long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < n) p[i] = 0u;
}

// NCH == 3: a work-group counts one share of the three planes of a sample (C == 3) and their cross sums; NCH == 1: one share of a plane.
template <int NCH>
__global__ __launch_bounds__(TPB) void pixel_summary_k(const float* __restrict__ x, unsigned int* __restrict__ sum, int C, int HW, int nchunk,
                                                       const float* __restrict__ mean, const float* __restrict__ stdv) {
    __shared__ unsigned int hist[NCH * 256];
    __shared__ unsigned long long wsum[3][TPB / 64];
    const int t = threadIdx.x;
    const int grp = blockIdx.x / nchunk, chunk = blockIdx.x - grp * nchunk;
    const int p0 = chunk * SHARE, n = min(SHARE, HW - p0);
    const long long plane0 = (long long)grp * NCH;
    const int c0 = (int)(plane0 % C);
    for (int i = t; i < NCH * 256; i += TPB) hist[i] = 0u;
    __syncthreads();
    float sd[NCH], mu[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        sd[j] = stdv ? stdv[c0 + j] : 1.f;
        mu[j] = mean ? mean[c0 + j] : 0.f;
    }
    const float* base = x + (size_t)plane0 * HW + p0;
    const Span sp = span_of(base, base, n, NCH == 1 || (HW & 3) == 0);
    unsigned long long x01 = 0, x02 = 0, x12 = 0;
    auto count = [&](const float (&v)[NCH]) {
        unsigned int l[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            l[j] = (unsigned int)level_f(v[j], sd[j], mu[j]);
            hist_add(hist + 256 * j, l[j]);
        }
        if (NCH == 3) {
            x01 += l[0] * l[NCH > 1 ? 1 : 0];
            x02 += l[0] * l[NCH > 2 ? 2 : 0];
            x12 += l[NCH > 1 ? 1 : 0] * l[NCH > 2 ? 2 : 0];
        }
    };
    for (int i = t; i < sp.head; i += TPB) {
        float v[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) v[j] = base[(size_t)j * HW + i];
        count(v);
    }
    for (int q = t; q < sp.nvec; q += TPB) {
        float4 a[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) a[j] = *reinterpret_cast<const float4*>(base + (size_t)j * HW + sp.head + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float v[NCH];
#pragma unroll
            for (int j = 0; j < NCH; ++j) v[j] = lane_of(a[j], k);
            count(v);
        }
    }
    for (int i = sp.head + 4 * sp.nvec + t; i < n; i += TPB) {
        float v[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) v[j] = base[(size_t)j * HW + i];
        count(v);
    }
    if (NCH == 3) {                                     // per-thread 64-bit sums, six xor steps, then the waves in order
        x01 = wave_sum(x01);
        x02 = wave_sum(x02);
        x12 = wave_sum(x12);
        if ((t & 63) == 0) {
            wsum[0][t >> 6] = x01;
            wsum[1][t >> 6] = x02;
            wsum[2][t >> 6] = x12;
        }
    }
    __syncthreads();
    unsigned int* row = sum + (size_t)(plane0 / C) * row_words(C) + (size_t)c0 * 256;
    for (int i = t; i < NCH * 256; i += TPB) {
        const unsigned int h = hist[i];
        if (h != 0u) atomicAdd(&row[i], h);
    }
    if (NCH == 3 && t < 3) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < TPB / 64; ++w) s += wsum[t][w];
        if (s != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(row + 768) + t, s);
    }
}

// first index of the non-decreasing c[0 .. 255] whose entry is >= v (lower) or > v (upper); 256 when there is none
__device__ __forceinline__ int lower_bound256(const unsigned int* c, unsigned int v) {
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int upper_bound256(const unsigned int* c, unsigned int v) {
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// unbiased variance or covariance in raw units from exact integers: (n X - Sa Sb) / (n (n - 1) 255^2); both products are below 2^64
__device__ __forceinline__ double cov_of(unsigned long long n, unsigned long long X, unsigned long long Sa, unsigned long long Sb) {
    const unsigned long long P = n * X, Q = Sa * Sb;
    const double num = P >= Q ? (double)(P - Q) : -(double)(Q - P);
    return num / ((double)n * (double)(n - 1) * 65025.0);
}

struct Chol3 {
    double l11, l21, l31, l22, l32, l33;
};
// S = (s11, s21, s31, s22, s32, s33), the lower triangle
__device__ __forceinline__ Chol3 chol3(const double* S) {
    Chol3 L;
    L.l11 = sqrt(S[0]);
    L.l21 = S[1] / L.l11;
    L.l31 = S[2] / L.l11;
    L.l22 = sqrt(S[3] - L.l21 * L.l21);
    L.l32 = (S[4] - L.l31 * L.l21) / L.l22;
    L.l33 = sqrt(S[5] - L.l31 * L.l31 - L.l32 * L.l32);
    return L;
}

// MODE 0 hist, 1 meanstd: a work-group owns one share of a plane; 2 cholesky: one share of a sample's three planes
template <int MODE>
__global__ __launch_bounds__(TPB) void pixel_transfer_k(const float* __restrict__ content, const unsigned int* __restrict__ sum_c,
                                                        const unsigned int* __restrict__ sum_s, float* __restrict__ out, int C, int HW, int nchunk,
                                                        double eps, float alpha, const float* __restrict__ alpha_dev, const float* __restrict__ lo,
                                                        const float* __restrict__ hi, const float* __restrict__ mean, const float* __restrict__ stdv) {
    constexpr int NCH = MODE == 2 ? 3 : 1;
    __shared__ unsigned int scan[2][2][256];            // [buffer][content, style][level]
    __shared__ float tab[256];
    __shared__ unsigned long long mom[2][3][2];         // [content, style][channel][sum l, sum l^2]
    __shared__ float coef[12];
    const int t = threadIdx.x;
    const int grp = blockIdx.x / nchunk, chunk = blockIdx.x - grp * nchunk;
    const int p0 = chunk * SHARE, n = min(SHARE, HW - p0);
    const long long plane0 = (long long)grp * NCH;
    const int c0 = (int)(plane0 % C);
    const size_t roff = (size_t)(plane0 / C) * row_words(C);
    const unsigned int* rc = sum_c + roff;
    const unsigned int* rs = sum_s + roff;
    const float a = alpha_dev ? alpha_dev[0] : alpha;

    if (MODE == 0) {
        const unsigned int hc = rc[c0 * 256 + t], hs = rs[c0 * 256 + t];
        scan[0][0][t] = hc;
        scan[0][1][t] = hs;
        __syncthreads();
        int cur = 0;
        for (int off = 1; off < 256; off <<= 1) {       // inclusive prefix sums of both histograms (eight steps: ends in buffer 0)
            const unsigned int vc = scan[cur][0][t] + (t >= off ? scan[cur][0][t - off] : 0u);
            const unsigned int vs = scan[cur][1][t] + (t >= off ? scan[cur][1][t - off] : 0u);
            scan[cur ^ 1][0][t] = vc;
            scan[cur ^ 1][1][t] = vs;
            __syncthreads();
            cur ^= 1;
        }
        const unsigned int* Cs = scan[cur][1];
        float d = 0.f;                                  // (a level the content does not hold is never looked up)
        if (hc != 0u) {
            const unsigned int q = scan[cur][0][t], total = Cs[255];
            if (q >= total) {
                d = (float)(lower_bound256(Cs, total) - t);                 // the last occupied style level
            } else {
                // the first level whose cumulative count exceeds q: occupied, < 256 (the min only keeps summaries that are not histograms of
                // H W pixels inside the table)
                const int u = min(upper_bound256(Cs, q), 255);
                const unsigned int below = u > 0 ? Cs[u - 1] : 0u;
                if (below == 0u) {
                    d = (float)(u - t);                                     // q < Cs[v_0]
                } else {
                    const int vj = lower_bound256(Cs, below);               // the occupied level at which the count reached `below`
                    const double T = (double)vj + (double)(q - below) / (double)(Cs[u] - below) * (double)(u - vj);
                    d = (float)(T - (double)t);
                }
            }
        }
        tab[t] = d;
    } else {
        const int lane = t & 63;
        for (int idx = t >> 6; idx < 2 * NCH; idx += TPB / 64) {
            const int img = idx / NCH, j = idx - img * NCH;
            const unsigned int* h = (img ? rs : rc) + (c0 + j) * 256;
            unsigned long long s1 = 0, s2 = 0;
            for (int k = lane; k < 256; k += 64) {
                const unsigned long long hv = h[k];
                s1 += hv * (unsigned long long)k;
                s2 += hv * (unsigned long long)(k * k);
            }
            s1 = wave_sum(s1);
            s2 = wave_sum(s2);
            if (lane == 0) {
                mom[img][j][0] = s1;
                mom[img][j][1] = s2;
            }
        }
        __syncthreads();
        if (t == 0) {
            const unsigned long long nn = (unsigned long long)HW;
            const double dn = 255.0 * (double)HW;
            if (MODE == 1) {
                const double mu_c = (double)mom[0][0][0] / dn, mu_s = (double)mom[1][0][0] / dn;
                const double var_c = cov_of(nn, mom[0][0][1], mom[0][0][0], mom[0][0][0]);
                const double var_s = cov_of(nn, mom[1][0][1], mom[1][0][0], mom[1][0][0]);
                const double g = sqrt(var_s + eps) / sqrt(var_c + eps);
                coef[0] = (float)(g - 1.0);
                coef[1] = (float)(255.0 * (mu_s - g * mu_c));
            } else {
                double mu[2][3], S[2][6];
                for (int img = 0; img < 2; ++img) {
                    const unsigned long long* X = reinterpret_cast<const unsigned long long*>((img ? rs : rc) + 768);
                    const unsigned long long x01 = X[0], x02 = X[1], x12 = X[2];
                    const unsigned long long s0 = mom[img][0][0], s1 = mom[img][1][0], s2 = mom[img][2][0];
                    mu[img][0] = (double)s0 / dn;
                    mu[img][1] = (double)s1 / dn;
                    mu[img][2] = (double)s2 / dn;
                    S[img][0] = cov_of(nn, mom[img][0][1], s0, s0) + eps;
                    S[img][1] = cov_of(nn, x01, s1, s0);
                    S[img][2] = cov_of(nn, x02, s2, s0);
                    S[img][3] = cov_of(nn, mom[img][1][1], s1, s1) + eps;
                    S[img][4] = cov_of(nn, x12, s2, s1);
                    S[img][5] = cov_of(nn, mom[img][2][1], s2, s2) + eps;
                }
                const Chol3 Lc = chol3(S[0]), Ls = chol3(S[1]);
                // the inverse of the lower-triangular L_c in closed form, then M = L_s L_c^-1 (lower triangular)
                const double i11 = 1.0 / Lc.l11, i22 = 1.0 / Lc.l22, i33 = 1.0 / Lc.l33;
                const double i21 = -Lc.l21 * i11 * i22, i32 = -Lc.l32 * i22 * i33;
                const double i31 = (Lc.l21 * Lc.l32 - Lc.l31 * Lc.l22) * i11 * i22 * i33;
                double M[3][3];
                M[0][0] = Ls.l11 * i11;
                M[0][1] = 0.0;
                M[0][2] = 0.0;
                M[1][0] = Ls.l21 * i11 + Ls.l22 * i21;
                M[1][1] = Ls.l22 * i22;
                M[1][2] = 0.0;
                M[2][0] = Ls.l31 * i11 + Ls.l32 * i21 + Ls.l33 * i31;
                M[2][1] = Ls.l32 * i22 + Ls.l33 * i32;
                M[2][2] = Ls.l33 * i33;
                for (int r = 0; r < 3; ++r) {
                    for (int b = 0; b < 3; ++b) coef[4 * r + b] = (float)(M[r][b] - (r == b ? 1.0 : 0.0));
                    coef[4 * r + 3] = (float)(255.0 * (mu[1][r] - (M[r][0] * mu[0][0] + M[r][1] * mu[0][1] + M[r][2] * mu[0][2])));
                }
            }
        }
    }
    __syncthreads();

    float sd[NCH], mu[NCH], inv[NCH], vlo[NCH], vhi[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        sd[j] = stdv ? stdv[c0 + j] : 1.f;
        mu[j] = mean ? mean[c0 + j] : 0.f;
        inv[j] = (float)(1.0 / (255.0 * (double)sd[j]));
        vlo[j] = lo ? lo[c0 + j] : 0.f;
        vhi[j] = lo ? hi[c0 + j] : 0.f;
    }
    float K[MODE == 2 ? 12 : 2];
#pragma unroll
    for (int i = 0; i < (MODE == 2 ? 12 : 2); ++i) K[i] = MODE == 0 ? 0.f : coef[i];
    const bool clamp = lo != nullptr;
    auto pixel = [&](const float (&v)[NCH], float (&o)[NCH]) {
        float l[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) l[j] = level_f(v[j], sd[j], mu[j]);
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            float d;
            if (MODE == 0) d = tab[(int)l[j]];
            else if (MODE == 1) d = fmaf(K[0], l[j], K[1]);
            else d = fmaf(K[4 * j], l[0], fmaf(K[4 * j + 1], l[NCH > 1 ? 1 : 0], fmaf(K[4 * j + 2], l[NCH > 2 ? 2 : 0], K[4 * j + 3])));
            const float td = a * d;
            float r = td == 0.f ? v[j] : fmaf(td, inv[j], v[j]);            // (alpha == 0, or nothing to move: x to the bit)
            if (clamp) r = fmaxf(fminf(r, vhi[j]), vlo[j]);
            o[j] = r;
        }
    };
    const size_t off = (size_t)plane0 * HW + p0;
    const float* src = content + off;
    float* dst = out + off;
    const Span sp = span_of(src, dst, n, NCH == 1 || (HW & 3) == 0);
    for (int i = t; i < sp.head; i += TPB) {
        float v[NCH], o[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) v[j] = src[(size_t)j * HW + i];
        pixel(v, o);
#pragma unroll
        for (int j = 0; j < NCH; ++j) dst[(size_t)j * HW + i] = o[j];
    }
    for (int q = t; q < sp.nvec; q += TPB) {
        float4 in[NCH], res[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) in[j] = *reinterpret_cast<const float4*>(src + (size_t)j * HW + sp.head + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float v[NCH], o[NCH];
#pragma unroll
            for (int j = 0; j < NCH; ++j) v[j] = lane_of(in[j], k);
            pixel(v, o);
#pragma unroll
            for (int j = 0; j < NCH; ++j) lane_of(res[j], k) = o[j];
        }
#pragma unroll
        for (int j = 0; j < NCH; ++j) *reinterpret_cast<float4*>(dst + (size_t)j * HW + sp.head + 4 * q) = res[j];
    }
    for (int i = sp.head + 4 * sp.nvec + t; i < n; i += TPB) {
        float v[NCH], o[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) v[j] = src[(size_t)j * HW + i];
        pixel(v, o);
#pragma unroll
        for (int j = 0; j < NCH; ++j) dst[(size_t)j * HW + i] = o[j];
    }
}

// UDAPOSE_OK, or why these sizes are refused (before any launch)
int pixel_check(int N, int C, int H, int W) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return UDAPOSE_ERR_ARG;
    const long long HW = (long long)H * W;
    if (HW > UDAPOSE_PIXEL_MAX_HW) return UDAPOSE_ERR_UNSUPPORTED;                 // uint32 counts, and n * sum l^2 below 2^64
    const long long nchunk = (HW + SHARE - 1) / SHARE;
    if ((long long)N * C * nchunk > 0x7fffffffLL || (long long)N * row_words(C) > 0x7fffffffLL) return UDAPOSE_ERR_UNSUPPORTED;
    return UDAPOSE_OK;
}
}  // namespace

long long pixel_summary_bytes(int N, int C) {
    if (N <= 0 || C <= 0 || (long long)N * row_words(C) > 0x7fffffffLL) return UDAPOSE_ERR_ARG;
    return (long long)N * row_words(C) * 4;
}

int pixel_summary(hipStream_t s, const float* x, int N, int C, int H, int W, const float* mean, const float* stdv, void* summary) {
    const int e = pixel_check(N, C, H, W);
    if (e != UDAPOSE_OK) return e;
    if (!x || !summary || ((uintptr_t)summary & 7) || ((uintptr_t)x & 3) || !mean != !stdv) return UDAPOSE_ERR_ARG;
    const int HW = H * W, nchunk = (HW + SHARE - 1) / SHARE;
    const long long words = (long long)N * row_words(C);
    unsigned int* sum = (unsigned int*)summary;
    hipLaunchKernelGGL(pixel_clear_k, dim3((unsigned)((words + TPB - 1) / TPB)), dim3(TPB), 0, s, sum, words);
    if (C == 3)
        hipLaunchKernelGGL(pixel_summary_k<3>, dim3((unsigned)(N * nchunk)), dim3(TPB), 0, s, x, sum, C, HW, nchunk, mean, stdv);
    else
        hipLaunchKernelGGL(pixel_summary_k<1>, dim3((unsigned)(N * C * nchunk)), dim3(TPB), 0, s, x, sum, C, HW, nchunk, mean, stdv);
    return udapose_check_launch();
}

int pixel_transfer(hipStream_t s, const float* content, const void* sum_c, const void* sum_s, float* out, int N, int C, int H, int W, int mode, double eps,
                   float alpha, const float* alpha_dev, const float* lo, const float* hi, const float* mean, const float* stdv) {
    const int e = pixel_check(N, C, H, W);
    if (e != UDAPOSE_OK) return e;
    if (!content || !sum_c || !sum_s || !out || ((uintptr_t)sum_c & 7) || ((uintptr_t)sum_s & 7) || ((uintptr_t)content & 3) || ((uintptr_t)out & 3))
        return UDAPOSE_ERR_ARG;
    if (!lo != !hi || !mean != !stdv) return UDAPOSE_ERR_ARG;
    if (mode < UDAPOSE_PIXEL_HIST || mode > UDAPOSE_PIXEL_CHOLESKY) return UDAPOSE_ERR_ARG;
    if (mode == UDAPOSE_PIXEL_CHOLESKY && C != 3) return UDAPOSE_ERR_ARG;
    if (mode != UDAPOSE_PIXEL_HIST && ((long long)H * W < 2 || !(eps > 0.0) || !(eps < 1e300))) return UDAPOSE_ERR_ARG;
    const int HW = H * W, nchunk = (HW + SHARE - 1) / SHARE;
    const unsigned int* sc = (const unsigned int*)sum_c;
    const unsigned int* ss = (const unsigned int*)sum_s;
    if (mode == UDAPOSE_PIXEL_HIST)
        hipLaunchKernelGGL(pixel_transfer_k<0>, dim3((unsigned)(N * C * nchunk)), dim3(TPB), 0, s, content, sc, ss, out, C, HW, nchunk, eps, alpha, alpha_dev,
                           lo, hi, mean, stdv);
    else if (mode == UDAPOSE_PIXEL_MEANSTD)
        hipLaunchKernelGGL(pixel_transfer_k<1>, dim3((unsigned)(N * C * nchunk)), dim3(TPB), 0, s, content, sc, ss, out, C, HW, nchunk, eps, alpha, alpha_dev,
                           lo, hi, mean, stdv);
    else
        hipLaunchKernelGGL(pixel_transfer_k<2>, dim3((unsigned)(N * nchunk)), dim3(TPB), 0, s, content, sc, ss, out, C, HW, nchunk, eps, alpha, alpha_dev, lo,
                           hi, mean, stdv);
    return udapose_check_launch();
}
