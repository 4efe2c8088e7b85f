// Fourier Domain Adaptation (Yang & Soatto, CVPR 2020) as a style bridge without weights: the content image keeps its phase and takes
// the style image's amplitude on the (2b+1) x (2b+1) lowest spatial frequencies.  Only that window changes, so no FFT is taken:
//   out = content + IDFT2(dF),   dF = alpha (A_style - A_content) F_content / |F_content|  on |u|, |v| <= b
// needs (2b+1) x (b+1) direct DFT coefficients per plane (real input: Hermitian symmetry) and a synthesis of the same rank.
// fp32 throughout, nothing depends on the library's element type.  A plane is one (n, c) channel of a contiguous NCHW fp32 tensor.
//
// Twiddles: every work-group builds cos / sin of 2 pi t / W (t < W) and 2 pi t / H (t < H) in LDS from the fp64 sincospi, rounded once to
// fp32; a phase is looked up at (v x) mod W or (u y) mod H, reduced exactly in integers.
// Order of every sum is fixed (no atomics): two runs, and a plane alone or inside a batch, give the same bits.
//   spectrum, per work-group of FDA_ROWS rows:  R[y, v] = sum_x x[y, x] e^{-2 pi i v x / W}   one wave per row and eight v: lane l adds x = l, l + 64, ...
//                                                                                               in order, then six xor steps (beyond 256 pixels:
//                                                                                               the next 256 the same way, added behind)
//                                               P[u, v] = sum_{y in group} R[y, v] e^{-2 pi i u y / H}      in row order
//   then per coefficient                        G[u, v] = sum_{groups} P[u, v]                              in group order
//   apply, per work-group of FDA_ROWS rows:     dF on the window (from the two spectra), S[y, v] = sum_u dF[u, v] e^{+2 pi i u y / H} in u order,
//                                               out[y, x] = content + (Re S[y, 0] + 2 sum_{v = 1..b} Re(S[y, v] e^{2 pi i v x / W})) / (H W)
// Every image row is read from HBM once per kernel (the spectrum's waves re-read it per eight v from L1 / L2).
#include "style.h"

#define FDA_TPB 1024    // 16 waves per work-group: a group's latency chains (row sums, S, pixels) overlap; sums do not depend on it
#define FDA_SUM_TPB 256
#define FDA_ROWS 32     // image rows per work-group, both kernels; a function of nothing, so a plane's sums never depend on the batch
#define FDA_VT 8        // coefficients v a wave forms at a time
#define FDA_RG 8        // rows of one pixel column that a thread of the apply kernel carries
#define FDA_XG 4        // runs of 64 pixels whose phases a wave keeps in registers
static_assert(FDA_VT == 8, "the wave sum below is written for 16 values");

static_assert(((2 * UDAPOSE_FDA_MAX_B + 1) * (UDAPOSE_FDA_MAX_B + 1) + FDA_ROWS * (UDAPOSE_FDA_MAX_B + 1) + 2 * UDAPOSE_FDA_MAX_DIM) * 8 <= 150 * 1024,
              "the apply kernel's LDS (dF, S and both twiddle tables at the largest window and image) must fit 150 KiB");

__device__ __forceinline__ void fda_tables(float2* twW, float2* twH, int W, int H) {
    for (int t = threadIdx.x; t < W; t += FDA_TPB) {
        double s, c;
        sincospi(2.0 * (double)t / (double)W, &s, &c);
        twW[t] = make_float2((float)c, (float)s);
    }
    for (int t = threadIdx.x; t < H; t += FDA_TPB) {
        double s, c;
        sincospi(2.0 * (double)t / (double)H, &s, &c);
        twH[t] = make_float2((float)c, (float)s);
    }
}

// part [planes][nblk][(2b+1)(b+1)]: the coefficients of one group of rows
__global__ __launch_bounds__(FDA_TPB) void fda_spectrum_part_k(const float* __restrict__ x, float2* __restrict__ part, int H, int W, int b, int nblk) {
    extern __shared__ float2 fda_lds[];
    float2* twW = fda_lds;
    float2* twH = twW + W;
    float2* R = twH + H;                                // [FDA_ROWS][b + 1]
    const int plane = blockIdx.x / nblk, blk = blockIdx.x - plane * nblk;
    const int y0 = blk * FDA_ROWS, rows = min(FDA_ROWS, H - y0), nv = b + 1;
    fda_tables(twW, twH, W, H);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* img = x + (size_t)plane * H * W;
    // A wave owns FDA_VT coefficients v and a range of the group's rows, and keeps the phases of its lanes' pixels in registers across those
    // rows (they do not depend on the row): per row and pixel only the loads and the multiply-adds remain.
    const int nt = (nv + FDA_VT - 1) / FDA_VT, ng = (W + 64 * FDA_XG - 1) / (64 * FDA_XG);
    const int nsplit = max(1, (FDA_TPB / 64) / nt), rps = (rows + nsplit - 1) / nsplit;
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
    const int jo = (h4 ? 4 : 0) + (h3 ? 2 : 0) + (h2 ? 1 : 0);     // the lane ends up with the sum of v0 + jo, real (h5 = 0) or imaginary part
    for (int item = wave; item < nt * nsplit; item += FDA_TPB / 64) {
        const int v0 = (item / nsplit) * FDA_VT, r0 = (item % nsplit) * rps, r1 = min(rows, r0 + rps);
        for (int g = 0; g < ng; ++g) {
            float2 tw[FDA_XG][FDA_VT];
#pragma unroll
            for (int k = 0; k < FDA_XG; ++k) {
                const int xx = (g * FDA_XG + k) * 64 + lane;
                int t = xx < W ? (int)(((unsigned)v0 * (unsigned)xx) % (unsigned)W) : 0;
#pragma unroll
                for (int j = 0; j < FDA_VT; ++j) {      // (v beyond b: a valid phase, a result nobody stores; x beyond W: zero)
                    tw[k][j] = xx < W ? twW[t] : make_float2(0.f, 0.f);
                    t += xx;
                    if (t >= W) t -= W;
                }
            }
            for (int r = r0; r < r1; ++r) {
                const float* row = img + (size_t)(y0 + r) * W;
                float a[2 * FDA_VT];
#pragma unroll
                for (int j = 0; j < 2 * FDA_VT; ++j) a[j] = 0.f;
#pragma unroll
                for (int k = 0; k < FDA_XG; ++k) {      // x = lane, lane + 64, ... in order
                    const int xx = (g * FDA_XG + k) * 64 + lane;
                    const float val = xx < W ? row[xx] : 0.f;
#pragma unroll
                    for (int j = 0; j < FDA_VT; ++j) {
                        a[j] = fmaf(val, tw[k][j].x, a[j]);
                        a[FDA_VT + j] = fmaf(-val, tw[k][j].y, a[FDA_VT + j]);
                    }
                }
                // the six xor steps (32, 16, .. 1) of a wave sum, for all 16 values at once: at each of the first four steps a lane keeps
                // the half of its values that its lane bit selects and hands the other half over - the sums a full butterfly forms, on fewer lanes
                float b8[8], b4[4], b2[2];
#pragma unroll
                for (int i = 0; i < 8; ++i) b8[i] = (h5 ? a[i + 8] : a[i]) + __shfl_xor(h5 ? a[i] : a[i + 8], 32, 64);
#pragma unroll
                for (int i = 0; i < 4; ++i) b4[i] = (h4 ? b8[i + 4] : b8[i]) + __shfl_xor(h4 ? b8[i] : b8[i + 4], 16, 64);
#pragma unroll
                for (int i = 0; i < 2; ++i) b2[i] = (h3 ? b4[i + 2] : b4[i]) + __shfl_xor(h3 ? b4[i] : b4[i + 2], 8, 64);
                float s1 = (h2 ? b2[1] : b2[0]) + __shfl_xor(h2 ? b2[0] : b2[1], 4, 64);
                s1 += __shfl_xor(s1, 2, 64);
                s1 += __shfl_xor(s1, 1, 64);
                if ((lane & 3) == 0 && v0 + jo < nv) {
                    float* p = (float*)&R[r * nv + v0 + jo] + (h5 ? 1 : 0);
                    *p = g == 0 ? s1 : *p + s1;         // (images wider than 64 FDA_XG pixels: the next run of pixels, in order)
                }
            }
        }
    }
    __syncthreads();
    const int nc = (2 * b + 1) * nv;
    float2* out = part + (size_t)blockIdx.x * nc;
    for (int j = threadIdx.x; j < nc; j += FDA_TPB) {
        const int ui = j / nv, v = j - ui * nv, u = ui - b;
        const int step = u < 0 ? u + H : u;             // (|u| <= b < H)
        int t = ((u * y0) % H + H) % H;
        float re = 0.f, im = 0.f;
        for (int r = 0; r < rows; ++r) {                // (a + i c)(cos - i sin)
            const float2 a = R[r * nv + v], w = twH[t];
            re = fmaf(a.x, w.x, fmaf(a.y, w.y, re));
            im = fmaf(a.y, w.x, fmaf(-a.x, w.y, im));
            t += step;
            if (t >= H) t -= H;
        }
        out[j] = make_float2(re, im);
    }
}

__global__ __launch_bounds__(FDA_SUM_TPB) void fda_spectrum_sum_k(const float2* __restrict__ part, float2* __restrict__ spec, int nc, int nblk, long long total) {
    const long long i = (long long)blockIdx.x * FDA_SUM_TPB + threadIdx.x;
    if (i >= total) return;
    const long long plane = i / nc;
    const int j = (int)(i - plane * nc);
    const float2* p = part + (size_t)plane * nblk * nc + j;
    float2 g = p[0];
    for (int k = 1; k < nblk; ++k) {
        const float2 a = p[(size_t)k * nc];
        g.x += a.x;
        g.y += a.y;
    }
    spec[i] = g;
}

__global__ __launch_bounds__(FDA_TPB) void fda_apply_k(const float* __restrict__ content, const float2* __restrict__ spec_c, const float2* __restrict__ spec_s,
                                                       float* __restrict__ out, int C, int H, int W, int b, int nblk, float alpha,
                                                       const float* __restrict__ alpha_dev, const float* __restrict__ lo, const float* __restrict__ hi,
                                                       const float* __restrict__ mean, const float* __restrict__ stdv) {
    extern __shared__ float2 fda_lds[];
    const int nv = b + 1, nc = (2 * b + 1) * nv;
    float2* twW = fda_lds;
    float2* twH = twW + W;
    float2* dF = twH + H;                               // [2b + 1][b + 1]
    float2* S = dF + nc;                                // [b + 1][FDA_ROWS]
    const int plane = blockIdx.x / nblk, blk = blockIdx.x - plane * nblk, c = plane % C;
    const int y0 = blk * FDA_ROWS, rows = min(FDA_ROWS, H - y0);
    const float a = alpha_dev ? alpha_dev[0] : alpha;
    const float hw = (float)H * (float)W;
    fda_tables(twW, twH, W, H);
    const float2* sc = spec_c + (size_t)plane * nc;
    const float2* ss = spec_s + (size_t)plane * nc;
    for (int j = threadIdx.x; j < nc; j += FDA_TPB) {
        float2 gc = sc[j], gs = ss[j];
        float scale = a;
        if (mean && j == b * nv) {                      // the DC coefficient of the raw image std x + mean; its dF back in normalised units
            const float sd = stdv[c], off = mean[c] * hw;
            gc = make_float2(fmaf(sd, gc.x, off), sd * gc.y);
            gs = make_float2(fmaf(sd, gs.x, off), sd * gs.y);
            scale = a / sd;
        }
        const float ac = hypotf(gc.x, gc.y), as = hypotf(gs.x, gs.y);
        float px = 1.f, py = 0.f;                       // |F_content| == 0: the phase of np.angle(0) == 0
        if (ac != 0.f) {
            px = gc.x / ac;
            py = gc.y / ac;
        }
        const float m = scale * (as - ac);              // alpha == 0, or equal spectra: exactly zero
        dF[j] = make_float2(m * px, m * py);
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < rows * nv; idx += FDA_TPB) {
        const int r = idx / nv, v = idx - r * nv, y = y0 + r;
        int t = (H - (b * y) % H) % H;                  // u = -b
        float re = 0.f, im = 0.f;
        for (int ui = 0; ui <= 2 * b; ++ui) {           // (d + i e)(cos + i sin)
            const float2 d = dF[ui * nv + v], w = twH[t];
            re = fmaf(d.x, w.x, fmaf(-d.y, w.y, re));
            im = fmaf(d.x, w.y, fmaf(d.y, w.x, im));
            t += y;
            if (t >= H) t -= H;
        }
        S[v * FDA_ROWS + r] = make_float2(re, im);
    }
    __syncthreads();
    // A thread owns one pixel column of FDA_RG rows: the phase of (v, x) is read once for those rows, their S[., v] are adjacent in LDS.
    const float inv = 1.f / hw;
    const size_t base = ((size_t)plane * H + y0) * W;
    const float vlo = lo ? lo[c] : 0.f, vhi = lo ? hi[c] : 0.f;
    const int ngr = (rows + FDA_RG - 1) / FDA_RG;
    for (int idx = threadIdx.x; idx < ngr * W; idx += FDA_TPB) {
        const int rg = idx / W, xx = idx - rg * W, rb = rg * FDA_RG;
        float acc[FDA_RG];
#pragma unroll
        for (int r = 0; r < FDA_RG; ++r) acc[r] = 0.f;
        int t = xx;
        for (int v = 1; v <= b; ++v) {
            const float2 w = twW[t];
            const float2* Sv = S + v * FDA_ROWS + rb;   // (rows beyond the image: values nobody stores)
#pragma unroll
            for (int r = 0; r < FDA_RG; ++r) {
                const float2 sv = Sv[r];
                acc[r] = fmaf(sv.x, w.x, fmaf(-sv.y, w.y, acc[r]));
            }
            t += xx;
            if (t >= W) t -= W;
        }
#pragma unroll
        for (int r = 0; r < FDA_RG; ++r) {
            if (rb + r < rows) {
                const size_t e = base + (size_t)(rb + r) * W + xx;
                float o = fmaf(inv, S[rb + r].x + 2.f * acc[r], content[e]);
                if (lo) o = fmaxf(fminf(o, vhi), vlo);
                out[e] = o;
            }
        }
    }
}

// UDAPOSE_OK, or why these sizes are refused (before any launch)
static int fda_check(long long planes, int H, int W, int b) {
    if (planes <= 0 || H <= 0 || W <= 0 || b < 0) return UDAPOSE_ERR_ARG;
    if (2LL * b + 1 > (H < W ? H : W)) return UDAPOSE_ERR_ARG;      // the window must stay below the Nyquist row / column
    if (b > UDAPOSE_FDA_MAX_B || H > UDAPOSE_FDA_MAX_DIM || W > UDAPOSE_FDA_MAX_DIM) return UDAPOSE_ERR_UNSUPPORTED;
    if (planes * ((H + FDA_ROWS - 1) / FDA_ROWS) > 0x7fffffffLL) return UDAPOSE_ERR_UNSUPPORTED;
    return UDAPOSE_OK;
}

long long fda_ws_bytes(int planes, int H, int W, int b) {
    const int e = fda_check(planes, H, W, b);
    if (e != UDAPOSE_OK) return e;
    return (long long)planes * ((H + FDA_ROWS - 1) / FDA_ROWS) * (2 * b + 1) * (b + 1) * (long long)sizeof(float2);
}

int fda_spectrum(hipStream_t s, const float* x, int planes, int H, int W, int b, void* ws, float* spec) {
    const int e = fda_check(planes, H, W, b);
    if (e != UDAPOSE_OK) return e;
    if (!x || !ws || !spec || ((uintptr_t)ws & 7) || ((uintptr_t)spec & 7)) return UDAPOSE_ERR_ARG;
    max_dynamic_lds<fda_spectrum_part_k>(150 * 1024);
    const int nblk = (H + FDA_ROWS - 1) / FDA_ROWS, nc = (2 * b + 1) * (b + 1);
    const unsigned lds = (unsigned)((W + H + FDA_ROWS * (b + 1)) * sizeof(float2));
    hipLaunchKernelGGL(fda_spectrum_part_k, dim3(planes * nblk), dim3(FDA_TPB), lds, s, x, (float2*)ws, H, W, b, nblk);
    const long long total = (long long)planes * nc;
    hipLaunchKernelGGL(fda_spectrum_sum_k, dim3((unsigned)((total + FDA_SUM_TPB - 1) / FDA_SUM_TPB)), dim3(FDA_SUM_TPB), 0, s, (const float2*)ws, (float2*)spec, nc, nblk,
                       total);
    return udapose_check_launch();
}

int fda_apply(hipStream_t s, const float* content, const float* spec_c, const float* spec_s, float* out, int planes, int C, int H, int W, int b, float alpha,
              const float* alpha_dev, const float* lo, const float* hi, const float* mean, const float* stdv) {
    const int e = fda_check(planes, H, W, b);
    if (e != UDAPOSE_OK) return e;
    if (!content || !spec_c || !spec_s || !out || ((uintptr_t)spec_c & 7) || ((uintptr_t)spec_s & 7)) return UDAPOSE_ERR_ARG;
    if (C <= 0 || planes % C || !lo != !hi || !mean != !stdv) return UDAPOSE_ERR_ARG;
    max_dynamic_lds<fda_apply_k>(150 * 1024);
    const int nblk = (H + FDA_ROWS - 1) / FDA_ROWS, nv = b + 1;
    const unsigned lds = (unsigned)((W + H + (2 * b + 1) * nv + FDA_ROWS * nv) * sizeof(float2));
    hipLaunchKernelGGL(fda_apply_k, dim3(planes * nblk), dim3(FDA_TPB), lds, s, content, (const float2*)spec_c, (const float2*)spec_s, out, C, H, W, b, nblk,
                       alpha, alpha_dev, lo, hi, mean, stdv);
    return udapose_check_launch();
}
