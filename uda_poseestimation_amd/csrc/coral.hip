// CORAL (covariance alignment of source and target heat-maps; the reference's lib/models/loss.py:176-208) through n x n Gram matrices.
// src, tgt: fp32 NCHW [n][K][H][W]; X = the (down-sampled) maps flattened to n x D, D = K*Ho*Wo; Xc = the batch-centred X.
//   Cs = Xs_c^T Xs_c / (n-1)  (D x D: never formed)          ||Cs - Ct||_F^2 = sum(Gss^2 + Gtt^2 - 2 Gst^2) / (n-1)^2 =: S
//   Gab = Xa_c Xb_c^T = Hc (Xa Xb^T) Hc   (n x n, Hc = I - 11^T/n)        loss = sqrt(S) / (4 D^2)
//   d loss / d Xs = k (Gss Xs - Gst Xt),  d loss / d Xt = k (Gtt Xt - Gst^T Xs),  k = 1 / (2 D^2 sqrt(S) (n-1)^2)
// Z = [src; tgt] is the stacked 2n x D data, its rows padded with zeros to MP = a multiple of 32 (at most 128: n <= 64).
//   coral_gram_k    persistent grid (<= 256 work-groups, each a contiguous run of 64-column tiles): raw Z Z^T by exact-fp32 MFMA
//                   (v_mfma_f32_32x32x2_f32), the upper 32x32 blocks only, one partial per work-group, no atomics.  An MFMA accumulator is an
//                   fp32 fma chain, so a chain is kept to 16 products: four interleaved accumulators per tile, added in fp64 into the
//                   work-group's running partial, which is written as fp64
//   coral_sum_k     the partials added in fp64 in work-group order - eight runs of consecutive work-groups per element, the eight run sums added
//                   in order: a fixed association, so two runs agree to the bit.  (One work-group adding 256 partials of 24 KB took 97 us: profiles/coral.txt, last section.)
//   coral_finish_k  one work-group, fp64: centring, S, the loss, the fp32 coefficient matrix
//                   coef [MP][MP] = k [Gss, -Gst; -Gst^T, Gtt] (all zero where S == 0: a zero gradient where torch gives NaN)
//   coral_bwd_k     the same grid: d(down-sampled Z) tile = coef . Z tile by MFMA, times the upstream gradient, scattered to full resolution
// Down-sampling (F.interpolate(scale_factor=1/d, mode='bilinear'), folded into the loads): Ho x Wo = floor(H/d) x floor(W/d); even d: the mean of
// the central 2x2 pixels of each d x d block (rows and columns d/2-1, d/2); odd d: the centre pixel.  The backward hands 0.25 of an element's
// gradient to each of its four pixels (all of it to the centre pixel) and writes an explicit 0 to every other pixel of the full-resolution
// gradient: footprints are disjoint and cover the map (the last block of a row / column takes the remainder), so nothing is cleared beforehand.
#include "losses.h"

namespace {
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int CT = 256;         // threads per work-group of the two streaming kernels (4 waves)
constexpr int TK = 64;          // columns of one LDS tile
constexpr int LPG = TK + 2;     // LDS row pitch of the Gram kernel (words): lane l reads [row l&31][col k + (l>>5)] - bank 2 (l&31) + (l>>5)
constexpr int LPB = TK + 32;    // ... of the backward: lane l reads [row k + (l>>5)][col l&31] - bank (l&31) + 32 (l>>5)
constexpr int GRID_MAX = 256;
constexpr int FT = 1024;        // threads of the finish kernel

struct CoralGeo {
    int N, M, K, H, W, d, Ho, Wo;
    unsigned Dd, HoWo;          // columns after down-sampling; pixels of one down-sampled map
    size_t img;                 // K*H*W: floats of one image
    FastDiv fHoWo, fWo;
};

// element (row r of Z, column c) of the down-sampled data; r < M, c < Dd
__device__ __forceinline__ float coral_load(const float* __restrict__ src, const float* __restrict__ tgt, const CoralGeo& g, int r, unsigned c) {
    const float* base = r < g.N ? src + (size_t)r * g.img : tgt + (size_t)(r - g.N) * g.img;
    if (g.d == 1) return base[c];
    const unsigned k = fdiv(c, g.fHoWo), rem = c - k * g.HoWo, ho = fdiv(rem, g.fWo), wo = rem - ho * (unsigned)g.Wo;
    const int o = (g.d - 1) >> 1;       // odd d: the centre; even d: d/2 - 1, the first of the two central rows / columns
    const float* p = base + ((size_t)k * g.H + ho * g.d + o) * g.W + wo * g.d + o;
    if (g.d & 1) return p[0];
    return 0.25f * ((p[0] + p[1]) + (p[g.W] + p[g.W + 1]));
}
// the gradient v of element (r, c) to its footprint of the full-resolution gradient
__device__ __forceinline__ void coral_scatter(float* __restrict__ dsrc, float* __restrict__ dtgt, const CoralGeo& g, int r, unsigned c, float v) {
    float* base = r < g.N ? dsrc + (size_t)r * g.img : dtgt + (size_t)(r - g.N) * g.img;
    if (g.d == 1) { base[c] = v; return; }
    const unsigned k = fdiv(c, g.fHoWo), rem = c - k * g.HoWo, ho = fdiv(rem, g.fWo), wo = rem - ho * (unsigned)g.Wo;
    const int y0 = ho * g.d, y1 = (int)ho == g.Ho - 1 ? g.H : y0 + g.d;
    const int x0 = wo * g.d, x1 = (int)wo == g.Wo - 1 ? g.W : x0 + g.d;
    const int o = (g.d - 1) >> 1, cy = y0 + o, cx = x0 + o;
    const bool odd = g.d & 1;
    const float q = odd ? v : 0.25f * v;
    float* pk = base + (size_t)k * g.H * g.W;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            const bool hit = odd ? (y == cy && x == cx) : ((y == cy || y == cy + 1) && (x == cx || x == cx + 1));
            pk[(size_t)y * g.W + x] = hit ? q : 0.f;
        }
}
// block blk of the upper triangle of RB x RB blocks, row by row: (0,0) (0,1) .. (0,RB-1) (1,1) ..
__device__ __host__ __forceinline__ void coral_block(int RB, int blk, int& bi, int& bj) {
    bi = 0;
    while (blk >= RB - bi) { blk -= RB - bi; ++bi; }
    bj = bi + blk;
}

// Raw Gram partials.  part [gridDim.x][NB][32][32] doubles, NB = RB (RB+1) / 2.  Wave w owns blocks w, w+4, w+8; every wave reads the whole
// tile.  The next tile's elements are fetched into registers while this one is multiplied.
template <int RB>
__global__ __launch_bounds__(CT) void coral_gram_k(const float* __restrict__ src, const float* __restrict__ tgt, CoralGeo g, int ntiles,
                                                    double* __restrict__ part) {
    constexpr int MP = RB * 32, PER = MP * TK / CT, NB = RB * (RB + 1) / 2, NQ = (NB + 3) / 4, NA = 4;
    __shared__ float tile[MP * LPG];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, lr = l & 31, lh = l >> 5;
    const int t0 = (int)((long long)blockIdx.x * ntiles / gridDim.x), t1 = (int)((long long)(blockIdx.x + 1) * ntiles / gridDim.x);
    const int cc = t & (TK - 1), r0 = t >> 6;          // this thread's column of the tile, and its first row (rows r0, r0+4, ..)
    float pre[PER];
    auto fetch = [&](int ti) {
        const unsigned c = (unsigned)ti * TK + cc;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int r = i * 4 + r0;
            pre[i] = (r < g.M && c < g.Dd) ? coral_load(src, tgt, g, r, c) : 0.f;
        }
    };
    double sum[NQ][16];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) sum[q][e] = 0.0;
    if (t0 < t1) fetch(t0);
    for (int ti = t0; ti < t1; ++ti) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i) tile[(i * 4 + r0) * LPG + cc] = pre[i];
        __syncthreads();
        if (ti + 1 < t1) fetch(ti + 1);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int blk = w + 4 * q;
            if (blk < NB) {
                int bi, bj;
                coral_block(RB, blk, bi, bj);
                const float* pa = tile + (32 * bi + lr) * LPG + lh;
                const float* pb = tile + (32 * bj + lr) * LPG + lh;
                f32x16 acc[NA];
#pragma unroll
                for (int i = 0; i < NA; ++i)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
#pragma unroll
                for (int k = 0; k < TK; k += 2 * NA)
#pragma unroll
                    for (int i = 0; i < NA; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[k + 2 * i], pb[k + 2 * i], acc[i], 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 16; ++e) sum[q][e] += ((double)acc[0][e] + (double)acc[1][e]) + ((double)acc[2][e] + (double)acc[3][e]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int blk = w + 4 * q;
        if (blk < NB) {
            double* o = part + ((size_t)blockIdx.x * NB + blk) * 1024;
#pragma unroll
            for (int e = 0; e < 16; ++e) o[((e & 3) + 8 * (e >> 2) + 4 * lh) * 32 + lr] = sum[q][e];
        }
    }
}

// sum[e] = the G partials of element e (e < NB * 1024) added in work-group order.  A work-group takes 32 consecutive elements; thread (run, el)
// adds the partials of its run of work-groups [run G / 8, (run + 1) G / 8) in order, then the eight run sums are added in order.
constexpr int SUM_T = 256, SUM_EL = 32, SUM_RUNS = SUM_T / SUM_EL;
__global__ __launch_bounds__(SUM_T) void coral_sum_k(const double* __restrict__ part, int G, int nel, double* __restrict__ sum) {
    __shared__ double runs[SUM_RUNS][SUM_EL];
    const int el = threadIdx.x & (SUM_EL - 1), run = threadIdx.x / SUM_EL;
    const int e = blockIdx.x * SUM_EL + el;            // nel is a multiple of 1024: never out of range
    const int g0 = run * G / SUM_RUNS, g1 = (run + 1) * G / SUM_RUNS;
    double s = 0.0;
#pragma unroll 8
    for (int gi = g0; gi < g1; ++gi) s += part[(size_t)gi * nel + e];
    runs[run][el] = s;
    __syncthreads();
    if (run == 0) {
#pragma unroll
        for (int r = 1; r < SUM_RUNS; ++r) s += runs[r][el];
        sum[e] = s;
    }
}

// One work-group, fp64.  Gd [MP][MP] doubles (workspace): the raw, then the centred stacked Gram.
__global__ __launch_bounds__(FT) void coral_finish_k(const double* __restrict__ sum, int RB, int N, double Dd, double* __restrict__ Gd,
                                                     float* __restrict__ coef, float* __restrict__ loss) {
    __shared__ double R[2 * 128], T[4], red[FT / 64], Ssh;
    const int t = threadIdx.x, M = 2 * N, MP = RB * 32, NB = RB * (RB + 1) / 2;
    const double n = (double)N;
    // the upper blocks, mirrored into the full symmetric matrix
    for (int e = t; e < NB * 1024; e += FT) {
        const int blk = e >> 10, ii = (e >> 5) & 31, jj = e & 31;
        int bi, bj;
        coral_block(RB, blk, bi, bj);
        const int row = 32 * bi + ii, col = 32 * bj + jj;
        if (row >= M || col >= M) continue;
        const double s = sum[e];
        Gd[row * MP + col] = s;
        if (bi != bj) Gd[col * MP + row] = s;
    }
    __syncthreads();
    // R[i][b] = sum over the columns j of part b (0: src, 1: tgt) of G[i][j]; T[a][b] = sum over the rows of part a
    for (int e = t; e < 2 * M; e += FT) {
        const int i = e >> 1, b = e & 1;
        double s = 0.0;
        for (int j = b * N; j < (b + 1) * N; ++j) s += Gd[i * MP + j];
        R[e] = s;
    }
    __syncthreads();
    if (t < 4) {
        const int a = t >> 1, b = t & 1;
        double s = 0.0;
        for (int i = a * N; i < (a + 1) * N; ++i) s += R[i * 2 + b];
        T[t] = s;
    }
    __syncthreads();
    // Hc G Hc per n x n part (G is symmetric: the column sums of part (a, b) are the row sums R[j][a]); per (i, j) the four parts together, so that
    // src == tgt gives S = 0 exactly
    double acc = 0.0;
    for (int e = t; e < N * N; e += FT) {
        const int i = e / N, j = e - i * N;
        double gc[4];
#pragma unroll
        for (int ab = 0; ab < 4; ++ab) {
            const int a = ab >> 1, b = ab & 1, gi = a * N + i, gj = b * N + j;
            gc[ab] = Gd[gi * MP + gj] - R[gi * 2 + b] / n - R[gj * 2 + a] / n + T[ab] / (n * n);
            Gd[gi * MP + gj] = gc[ab];
        }
        // (as products of sum and difference: exactly 0 for equal parts, whatever the compiler contracts into an fma)
        acc += (gc[0] - gc[1]) * (gc[0] + gc[1]) + (gc[3] - gc[2]) * (gc[3] + gc[2]);
    }
    acc = wave_sum(acc);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int i = 0; i < FT / 64; ++i) s += red[i];
        s /= (n - 1.0) * (n - 1.0);
        Ssh = s > 0.0 ? s : 0.0;
        loss[0] = (float)(sqrt(Ssh) / (4.0 * Dd * Dd));
    }
    __syncthreads();
    const double S = Ssh;
    const double k = S > 0.0 ? 1.0 / (2.0 * Dd * Dd * sqrt(S) * (n - 1.0) * (n - 1.0)) : 0.0;
    for (int e = t; e < MP * MP; e += FT) {
        const int i = e / MP, j = e - i * MP;
        float v = 0.f;
        if (i < M && j < M && k != 0.0) v = (float)(((i >= N) == (j >= N) ? k : -k) * Gd[e]);
        coef[e] = v;
    }
}

// d(down-sampled Z)[i][c] = sum_j coef[i][j] Z[j][c].  A wave owns one 32-row block of the output (its coefficients stay in registers) and
// every CG-th 32-column half of the tile.
template <int RB>
__global__ __launch_bounds__(CT) void coral_bwd_k(const float* __restrict__ src, const float* __restrict__ tgt, const float* __restrict__ coef,
                                                   const float* __restrict__ gscale, CoralGeo g, int ntiles, float* __restrict__ dsrc,
                                                   float* __restrict__ dtgt) {
    constexpr int MP = RB * 32, PER = MP * TK / CT, RBW = RB == 1 ? 1 : RB == 2 ? 2 : 4, CG = 4 / RBW, NSUB = TK / 32;
    __shared__ float tile[MP * LPB];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, lr = l & 31, lh = l >> 5;
    const int t0 = (int)((long long)blockIdx.x * ntiles / gridDim.x), t1 = (int)((long long)(blockIdx.x + 1) * ntiles / gridDim.x);
    const int cc = t & (TK - 1), r0 = t >> 6;
    const int bi = w % RBW, cg = w / RBW;
    const bool active = bi < RB;
    const float gs = gscale ? gscale[0] : 1.f;
    float a[MP / 2];
#pragma unroll
    for (int s = 0; s < MP / 2; ++s) a[s] = active ? coef[(32 * bi + lr) * MP + 2 * s + lh] : 0.f;
    float pre[PER];
    auto fetch = [&](int ti) {
        const unsigned c = (unsigned)ti * TK + cc;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int r = i * 4 + r0;
            pre[i] = (r < g.M && c < g.Dd) ? coral_load(src, tgt, g, r, c) : 0.f;
        }
    };
    if (t0 < t1) fetch(t0);
    for (int ti = t0; ti < t1; ++ti) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i) tile[(i * 4 + r0) * LPB + cc] = pre[i];
        __syncthreads();
        if (ti + 1 < t1) fetch(ti + 1);
        f32x16 acc[NSUB];
#pragma unroll
        for (int q = 0; q < NSUB; ++q) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;
            const int cj = cg + q * CG;
            if (active && cj < NSUB) {
                const float* pb = tile + lh * LPB + 32 * cj + lr;
#pragma unroll
                for (int s = 0; s < MP / 2; ++s) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], pb[2 * s * LPB], acc[q], 0, 0, 0);
            }
        }
        __syncthreads();        // every wave has read the data: the tile now takes the gradients
#pragma unroll
        for (int q = 0; q < NSUB; ++q) {
            const int cj = cg + q * CG;
            if (active && cj < NSUB) {
#pragma unroll
                for (int e = 0; e < 16; ++e) tile[(32 * bi + (e & 3) + 8 * (e >> 2) + 4 * lh) * LPB + 32 * cj + lr] = acc[q][e] * gs;
            }
        }
        __syncthreads();
        const unsigned c = (unsigned)ti * TK + cc;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int r = i * 4 + r0;
            if (r < g.M && c < g.Dd) coral_scatter(dsrc, dtgt, g, r, c, tile[r * LPB + cc]);
        }
    }
}

// geometry, the padded row blocks, tiles and grid; false: refused arguments
bool coral_geo(int N, int K, int H, int W, int down, CoralGeo& g, int& RB, int& ntiles, int& grid) {
    if (N < 2 || N > 64 || K < 1 || H < 1 || W < 1 || down < 1) return false;
    const int Ho = H / down, Wo = W / down;
    if (Ho < 1 || Wo < 1) return false;
    const unsigned long long img = (unsigned long long)K * H * W;
    if (img > 0x7fffffffull) return false;
    g.N = N; g.M = 2 * N; g.K = K; g.H = H; g.W = W; g.d = down; g.Ho = Ho; g.Wo = Wo;
    g.HoWo = (unsigned)Ho * Wo;
    g.Dd = (unsigned)K * g.HoWo;
    g.img = (size_t)img;
    g.fHoWo = make_fastdiv(g.HoWo);
    g.fWo = make_fastdiv((unsigned)Wo);
    RB = (2 * N + 31) / 32;
    ntiles = (int)((g.Dd + TK - 1) / TK);
    grid = ntiles < GRID_MAX ? ntiles : GRID_MAX;
    return true;
}
}  // namespace

// workspace (doubles): [MP*MP: the stacked Gram][NB * 1024: the summed upper blocks][grid * NB * 1024: the partials]
long long coral_ws_bytes(int N, int K, int H, int W, int down) {
    CoralGeo g;
    int RB, ntiles, grid;
    if (!coral_geo(N, K, H, W, down, g, RB, ntiles, grid)) return UDAPOSE_ERR_ARG;
    const long long MP = RB * 32, NB = RB * (RB + 1) / 2;
    return MP * MP * 8 + (long long)(grid + 1) * NB * 1024 * 8;
}
int coral_fwd(hipStream_t st, const float* src, const float* tgt, int N, int K, int H, int W, int down, void* ws, float* coef, float* loss) {
    CoralGeo g;
    int RB, ntiles, grid;
    if (!src || !tgt || !ws || !coef || !loss || !coral_geo(N, K, H, W, down, g, RB, ntiles, grid)) return UDAPOSE_ERR_ARG;
    double* Gd = (double*)ws;
    const int nel = RB * (RB + 1) / 2 * 1024;
    double* sum = Gd + (size_t)RB * 32 * RB * 32;
    double* part = sum + nel;
    switch (RB) {
    case 1: hipLaunchKernelGGL(coral_gram_k<1>, dim3(grid), dim3(CT), 0, st, src, tgt, g, ntiles, part); break;
    case 2: hipLaunchKernelGGL(coral_gram_k<2>, dim3(grid), dim3(CT), 0, st, src, tgt, g, ntiles, part); break;
    case 3: hipLaunchKernelGGL(coral_gram_k<3>, dim3(grid), dim3(CT), 0, st, src, tgt, g, ntiles, part); break;
    default: hipLaunchKernelGGL(coral_gram_k<4>, dim3(grid), dim3(CT), 0, st, src, tgt, g, ntiles, part); break;
    }
    hipLaunchKernelGGL(coral_sum_k, dim3(nel / SUM_EL), dim3(SUM_T), 0, st, part, grid, nel, sum);
    hipLaunchKernelGGL(coral_finish_k, dim3(1), dim3(FT), 0, st, sum, RB, N, (double)g.Dd, Gd, coef, loss);
    return udapose_check_launch();
}
int coral_bwd(hipStream_t st, const float* src, const float* tgt, const float* coef, const float* gscale, int N, int K, int H, int W, int down,
              float* dsrc, float* dtgt) {
    CoralGeo g;
    int RB, ntiles, grid;
    if (!src || !tgt || !coef || !dsrc || !dtgt || !coral_geo(N, K, H, W, down, g, RB, ntiles, grid)) return UDAPOSE_ERR_ARG;
    switch (RB) {
    case 1: hipLaunchKernelGGL(coral_bwd_k<1>, dim3(grid), dim3(CT), 0, st, src, tgt, coef, gscale, g, ntiles, dsrc, dtgt); break;
    case 2: hipLaunchKernelGGL(coral_bwd_k<2>, dim3(grid), dim3(CT), 0, st, src, tgt, coef, gscale, g, ntiles, dsrc, dtgt); break;
    case 3: hipLaunchKernelGGL(coral_bwd_k<3>, dim3(grid), dim3(CT), 0, st, src, tgt, coef, gscale, g, ntiles, dsrc, dtgt); break;
    default: hipLaunchKernelGGL(coral_bwd_k<4>, dim3(grid), dim3(CT), 0, st, src, tgt, coef, gscale, g, ntiles, dsrc, dtgt); break;
    }
    return udapose_check_launch();
}
