// Memory-bound kernels of the pose network for gfx950: layout conversion, weight packing, training-mode BatchNorm
// (finalize / apply / backward), 3x3 s2 and 2x2 ceil max-pooling.  All activation tensors are NHWC bf16 and every
// thread moves 16 bytes (8 channels) per access.  These kernels are HBM-roofline bound (8 TB/s peak).
#include <stdlib.h>
#include <type_traits>
#include "pointwise.h"
#include "storage8.h"

namespace {

constexpr int TPB = 256;
constexpr size_t GRID_CAP = 8192;      // blocks of a grid-stride sweep

// ------------------------------------------------------------------ layout conversion
// 'strict' plans (net.hip): the f16x2 forward also leaves the fp16 tensors the 16-bit backward reads ("shadows").  One 16-byte store each:
// an fp16 rounding of 8 fp32 values (the pre-BN y), and the split store whose h half is ALSO the fp16 shadow of z (returned for the mask)
__device__ __forceinline__ void st8_f16(_Float16* p, const float (&v)[8]) {
    half8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (_Float16)v[e];
    *(half8*)p = o;
}
__device__ __forceinline__ half8 st8_split_shadow(sp32* p, _Float16* h16, const float (&v)[8]) {
    half8 h, l;
    sp_split8(v, h, l);
    char* c = (char*)p;
    *(half8*)c = h;
    *(half8*)(c + 16) = l;
    *(half8*)h16 = h;
    return h;
}
// ReLU bit mask of 8 stored fp16 values (bit e: value e > 0, what a reader of the fp16 z sees)
__device__ __forceinline__ unsigned char mask_of(const half8& h) {
    unsigned mb = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) mb |= ((float)h[e] > 0.f ? 1u : 0u) << e;
    return (unsigned char)mb;
}
// the same of 8 fp32 values as a reader of their 16-bit stored form sees them (bit e: the STORED value of channel e is > 0)
__device__ __forceinline__ unsigned char mask_of_stored(const float (&o)[8]) {
    unsigned mb = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) mb |= ((float)(elem_t)o[e] > 0.f ? 1u : 0u) << e;
    return (unsigned char)mb;
}

// src NCHW fp32 [N,C,HW] -> dst NHWC [N,HW,Cp] (channels >= C zero-filled); one thread per (pixel, 8-channel group)
// (SH: T is sp32 and dst16 receives the fp16 image as well - a 'strict' plan's x8 for the stem's weight gradient)
template <typename T, bool SH = false>
__global__ void nchw_f32_to_nhwc_k(const float* __restrict__ src, T* __restrict__ dst, int N, int C, int HW, int Cp,
                                   _Float16* __restrict__ dst16 = nullptr) {
    const int G = Cp >> 3;
    const size_t total = (size_t)N * HW * G;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        const size_t pix = i % ((size_t)N * HW);      // pixel fastest: coalesced plane reads
        const int g = (int)(i / ((size_t)N * HW));
        const size_t n = pix / HW, hw = pix % HW;
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = g * 8 + e;
            o[e] = c < C ? src[(n * C + c) * HW + hw] : 0.f;
        }
        if constexpr (SH) (void)st8_split_shadow((sp32*)(dst + pix * Cp + g * 8), dst16 + pix * Cp + g * 8, o);
        else st8<T>(dst + pix * Cp + g * 8, o);
    }
}

// src NHWC (fp32 or bf16) [N,HW,Cs] -> dst NCHW fp32 [N,C,HW], optional per-channel clamp (style-net output)
template <typename T>
__global__ void nhwc_to_nchw_f32_k(const T* __restrict__ src, float* __restrict__ dst, int N, int C, int HW, int Cs,
                                   const float* __restrict__ lo, const float* __restrict__ hi) {
    const size_t total = (size_t)N * HW;
    for (size_t pix = (size_t)blockIdx.x * TPB + threadIdx.x; pix < total; pix += (size_t)gridDim.x * TPB) {
        const size_t n = pix / HW, hw = pix % HW;
        for (int c = 0; c < C; ++c) {
            float v = ld1<T>(src, pix * Cs + c);
            if (lo) v = fmaxf(fminf(v, hi[c]), lo[c]);
            dst[(n * C + c) * HW + hw] = v;
        }
    }
}

// ------------------------------------------------------------------ weight packing (fp32 master -> bf16 GEMM layouts)
__global__ void cast_f32_bf16_k(const float* __restrict__ src, elem_t* __restrict__ dst, size_t n8) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n8; i += (size_t)gridDim.x * TPB) {
        const f32x4 a = *(const f32x4*)(src + i * 8), b = *(const f32x4*)(src + i * 8 + 4);
        elem8 o = {(elem_t)a[0], (elem_t)a[1], (elem_t)a[2], (elem_t)a[3], (elem_t)b[0], (elem_t)b[1], (elem_t)b[2], (elem_t)b[3]};
        *(elem8*)(dst + i * 8) = o;
    }
}
// src [A][T][B] fp32 -> dst [B][T][A] (bf16 or fp32) (32x32 LDS-tiled transpose per tap); grid = (B/32, A/32, T)
template <typename D>
__global__ void transpose_cast_k(const float* __restrict__ src, D* __restrict__ dst, int A, int T, int B) {
    __shared__ float tile[32][33];
    const int t = blockIdx.z, b0 = blockIdx.x * 32, a0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int a = a0 + r, b = b0 + tx;
        tile[r][tx] = (a < A && b < B) ? src[((size_t)a * T + t) * B + b] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int b = b0 + r, a = a0 + tx;
        if (a < A && b < B) st1<D>(dst, ((size_t)b * T + t) * A + a, tile[tx][r]);
    }
}
// One launch packs every weight of a network: a job is either a contiguous cast (T == 0: n elements) or a per-tap
// transpose [A][T][B] fp32 -> [B][T][A] bf16; block b works on job blk_job[b], sub-block blk_sub[b].
// kind: bit 0 = transpose, bit 1 = f16x2 split output (the fp32-grade plans) instead of the element type.
struct PackJob { const float* src; elem_t* dst; int A, T, B, kind; long long n; };
__global__ void pack_multi_k(const PackJob* __restrict__ jobs, const int* __restrict__ blk_job, const int* __restrict__ blk_sub) {
    __shared__ float tile[32][33];
    const PackJob j = jobs[blk_job[blockIdx.x]];
    const int sub = blk_sub[blockIdx.x];
    if ((j.kind & 1) == 0) {
        const long long base = (long long)sub * 8192;           // 8192 elements per block
        for (long long i = base + threadIdx.x * 8; i < base + 8192 && i < j.n; i += TPB * 8) {
            const f32x4 a = *(const f32x4*)(j.src + i), b = *(const f32x4*)(j.src + i + 4);
            if (j.kind & 2) {
                const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
                st8<sp32>((sp32*)j.dst + i, v);
            } else {
                elem8 o = {(elem_t)a[0], (elem_t)a[1], (elem_t)a[2], (elem_t)a[3], (elem_t)b[0], (elem_t)b[1], (elem_t)b[2], (elem_t)b[3]};
                *(elem8*)(j.dst + i) = o;
            }
        }
        return;
    }
    const int tb = (j.B + 31) / 32, ta = (j.A + 31) / 32;
    const int t = sub / (ta * tb), rem = sub % (ta * tb);
    const int a0 = (rem / tb) * 32, b0 = (rem % tb) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int a = a0 + r, b = b0 + tx;
        tile[r][tx] = (a < j.A && b < j.B) ? j.src[((size_t)a * j.T + t) * j.B + b] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int b = b0 + r, a = a0 + tx;
        if (a < j.A && b < j.B) {
            if (j.kind & 2) sp_store1(j.dst, ((size_t)b * j.T + t) * j.A + a, tile[tx][r]);
            else j.dst[((size_t)b * j.T + t) * j.A + a] = (elem_t)tile[tx][r];
        }
    }
}

// generic strided gather with zero padding: dst[a][kh][kwp][bp] bf16 <- src[a*sa + kh*skh + kw*skw + b*sb] (kw<KW, b<B)
template <typename D>
__global__ void pack_strided_k(const float* __restrict__ src, D* __restrict__ dst, int A, int KH, int KWp, int KW, int Bp, int B,
                               long sa, long skh, long skw, long sb) {
    const size_t total = (size_t)A * KH * KWp * Bp;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        const int b = (int)(i % Bp);
        size_t r = i / Bp;
        const int kw = (int)(r % KWp); r /= KWp;
        const int kh = (int)(r % KH);
        const int a = (int)(r / KH);
        float v = 0.f;
        if (kw < KW && b < B) v = src[a * sa + kh * skh + kw * skw + b * sb];
        st1<D>(dst, i, v);
    }
}
// inverse of pack_strided for gradients: dst[a*sa + kh*skh + kw*skw + b*sb] (beta*dst +) = src[a][kh][kwp][bp] (fp32)
__global__ void unpack_strided_k(const float* __restrict__ src, float* __restrict__ dst, int A, int KH, int KWp, int KW, int Bp, int B,
                                 long sa, long skh, long skw, long sb, float beta) {
    const size_t total = (size_t)A * KH * KW * B;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        const int b = (int)(i % B);
        size_t r = i / B;
        const int kw = (int)(r % KW); r /= KW;
        const int kh = (int)(r % KH);
        const int a = (int)(r / KH);
        const float v = src[(((size_t)a * KH + kh) * KWp + kw) * Bp + b];
        float* d = dst + (a * sa + kh * skh + kw * skw + b * sb);
        *d = (beta != 0.f ? beta * *d : 0.f) + v;
    }
}

// ------------------------------------------------------------------ BatchNorm (training mode)
// Column sums of a partial-sum slab [rows][2][C]: block = 32 channels x 32 row lanes (1024 threads), 128-byte coalesced
// row segments, fp64 accumulation, LDS tree over the row lanes.  Result for channel c0+cl in (s1, s2) of lanes rl == 0.
#ifndef UDAPOSE_FIN_C
#define UDAPOSE_FIN_C 8
#endif
constexpr int FIN_C = UDAPOSE_FIN_C;    // channels per block.  8 (32-byte row segments, C/8 blocks of 256 threads): the finalize kernels sit in
                                        // every layer's dependency chain and are pure latency - 4x the blocks of the 128-byte-segment form (32)
                                        // measured -0.1 ms per step (profiles/r2_ab_runs.txt); 4 / 16 channels and more row lanes measured slower
#ifndef UDAPOSE_FIN_RL
#define UDAPOSE_FIN_RL 32
#endif
constexpr int FIN_RL = UDAPOSE_FIN_RL;  // row lanes per block
constexpr int FIN_T = FIN_C * FIN_RL;
__device__ __forceinline__ void slab_colsum(const float* __restrict__ slab, int rows, int C, int c, bool cvalid, double& s1, double& s2,
                                            double (*red)[FIN_C][2]) {
    const int cl = threadIdx.x % FIN_C, rl = threadIdx.x / FIN_C;
    double a = 0.0, b = 0.0;
    if (cvalid) {
        // 8, then 4 independent row loads in flight per thread (the loop is pure latency: 1024 slab rows = 32 per lane); the
        // additions keep the order of the 4-row form, so the sums are bit-identical to it
        int r = rl;
        for (; r + 7 * FIN_RL < rows; r += 8 * FIN_RL) {
            const float* q = slab + (size_t)r * 2 * C + c;
            const size_t st = (size_t)FIN_RL * 2 * C;
            const float a0 = q[0], b0 = q[C], a1 = q[st], b1 = q[st + C];
            const float a2 = q[2 * st], b2 = q[2 * st + C], a3 = q[3 * st], b3 = q[3 * st + C];
            const float a4 = q[4 * st], b4 = q[4 * st + C], a5 = q[5 * st], b5 = q[5 * st + C];
            const float a6 = q[6 * st], b6 = q[6 * st + C], a7 = q[7 * st], b7 = q[7 * st + C];
            a += ((double)a0 + (double)a1) + ((double)a2 + (double)a3);
            b += ((double)b0 + (double)b1) + ((double)b2 + (double)b3);
            a += ((double)a4 + (double)a5) + ((double)a6 + (double)a7);
            b += ((double)b4 + (double)b5) + ((double)b6 + (double)b7);
        }
        for (; r + 3 * FIN_RL < rows; r += 4 * FIN_RL) {
            const float* q = slab + (size_t)r * 2 * C + c;
            const size_t st = (size_t)FIN_RL * 2 * C;
            const float a0 = q[0], b0 = q[C], a1 = q[st], b1 = q[st + C];
            const float a2 = q[2 * st], b2 = q[2 * st + C], a3 = q[3 * st], b3 = q[3 * st + C];
            a += ((double)a0 + (double)a1) + ((double)a2 + (double)a3);
            b += ((double)b0 + (double)b1) + ((double)b2 + (double)b3);
        }
        for (; r < rows; r += FIN_RL) {
            a += (double)slab[(size_t)r * 2 * C + c];
            b += (double)slab[(size_t)r * 2 * C + C + c];
        }
    }
    red[rl][cl][0] = a; red[rl][cl][1] = b;
    __syncthreads();
    for (int st = FIN_RL / 2; st > 0; st >>= 1) {
        if (rl < st) { red[rl][cl][0] += red[rl + st][cl][0]; red[rl][cl][1] += red[rl + st][cl][1]; }
        __syncthreads();
    }
    s1 = red[0][cl][0]; s2 = red[0][cl][1];
}
// The building blocks of the BatchNorm kernels below.  Each expression that several kernels must agree on bit for bit is stated once here
// (the scale / shift pair itself: bn_scale_shift, common.h); device code is compiled with the default contraction, so a * b + c fuses.
// batch statistics of one channel from its fp64 sums: mean and clamped biased variance; from the variance, invstd and the unbiased variance.
// (three functions, so that a kernel forms each value where it did before they were shared: the finalize kernels are pure latency)
__device__ __forceinline__ void bn_stats_finish(double s1, double s2, double count, double& mean, double& var) {
    mean = s1 / count;
    var = s2 / count - mean * mean;
    if (var < 0.0) var = 0.0;
}
__device__ __forceinline__ float bn_invstd(double var, float eps) { return (float)(1.0 / sqrt(var + (double)eps)); }
__device__ __forceinline__ double bn_unbiased_var(double var, double count) { return count > 1.0 ? var * count / (count - 1.0) : var; }
// momentum update of one channel's running statistics, like torch.nn.BatchNorm2d in train()
__device__ __forceinline__ void bn_running_update1(float* __restrict__ rm, float* __restrict__ rv, int c, float momentum, float mean, float unb) {
    rm[c] = (1.f - momentum) * rm[c] + momentum * mean;
    rv[c] = (1.f - momentum) * rv[c] + momentum * unb;
}
// the forward's two scalar steps ...
__device__ __forceinline__ float bn_affine(float v, float sc, float sh) { return v * sc + sh; }
__device__ __forceinline__ float bn_relu(float o, int relu) { return (relu && o < 0.f) ? 0.f : o; }
// ... and o = [relu]( v * sc + sh [+ res] ): the forward of 8 channels, before the rounding of the store
template <typename T>
__device__ __forceinline__ void bn_apply8(const float (&v)[8], const float (&sc)[8], const float (&sh)[8], const T* __restrict__ res, size_t off, int relu,
                                          float (&o)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = bn_affine(v[e], sc[e], sh[e]);
    if (res) {
        float r[8];
        ld8<T>(res + off, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += r[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = bn_relu(o[e], relu);
}
// ... and its store at element offset off: z, the 'strict' fp16 shadow z16 (SH) and the ReLU bit mask of the stored values at mask[mi]
template <typename T, bool SH>
__device__ __forceinline__ void bn_store8(T* __restrict__ z, _Float16* __restrict__ z16, unsigned char* __restrict__ mask, size_t off, size_t mi,
                                          const float (&o)[8]) {
    if constexpr (SH) {
        const half8 h = st8_split_shadow(z + off, z16 + off, o);
        if (mask) mask[mi] = mask_of(h);
    } else {
        st8<T>(z + off, o);
        if constexpr (sizeof(T) == sizeof(elem_t)) {
            if (mask) mask[mi] = mask_of_stored(o);
        }
    }
}
// pixels [p0, p1) of work-group sp when each takes P of npix
__device__ __forceinline__ void pix_range(size_t sp, int P, size_t npix, size_t& p0, size_t& p1) {
    p0 = sp * P;
    p1 = p0 + P;
    if (p1 > npix) p1 = npix;
}
// Streaming kernels (bn_apply_k, bn_bwd_apply_pre_k) walk i = first, first + istep, .. < iend over the tensor's n8 16-byte groups, G per pixel row.
// xcd (launcher: TPB % G == 0, gridDim.x % 8 == 0): work-group b runs on XCD b mod 8 (round-robin dealing), and XCD k takes the
// k-th EIGHTH of the pixel rows - the rows the implicit GEMM's work-groups on XCD k wrote just before and will read next (each
// XCD owns a contiguous range of m-tiles there): y comes from, and z stays in, that XCD's L2 (tools/probe/l2_handoff.hip)
__device__ __forceinline__ void xcd_stream_range(size_t n8, int G, int xcd, size_t& i, size_t& iend, size_t& istep) {
    i = (size_t)blockIdx.x * TPB + threadIdx.x, iend = n8, istep = (size_t)gridDim.x * TPB;
    if (xcd) {
        const size_t rows = n8 / G, per = (rows + 7) / 8;
        const unsigned x = blockIdx.x & 7u, local = blockIdx.x >> 3, nb = gridDim.x >> 3;
        const unsigned RB = TPB / G;
        size_t rend = (size_t)(x + 1) * per;
        if (rend > rows) rend = rows;
        i = ((size_t)x * per + (size_t)local * RB + threadIdx.x / G) * G + threadIdx.x % G;
        iend = rend * G;
        istep = (size_t)nb * RB * G;
    }
}
// Chunked kernels, grid (C/64, S): the work-group's 64-channel chunk and pixel range sp.
// xcd: the (chunk, pixel range) pairs are dealt so that XCD k gets the k-th EIGHTH of the pixel rows (all chunks of it) - the rows
// the implicit GEMMs' work-groups on XCD k produced and will consume (igemm.hip: each XCD owns a contiguous range of m-tiles):
// y is then read from, and z left in, that XCD's L2 (tools/probe/l2_handoff.hip: 17.9 against 6.7 TB/s across a kernel boundary)
__device__ __forceinline__ void xcd_chunk_of(int xcd, int& chunk, int& sp) {
    chunk = blockIdx.x, sp = blockIdx.y;
    if (xcd) {
        const uint32_t w = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
        sp = (int)(w / gridDim.x);
        chunk = (int)(w - (uint32_t)sp * gridDim.x);
    }
}
// Chunked kernels' prelude: fp64 column sums of the work-group's 64 channels of a partial-sum slab [rows][2][C] (rows <= 128: <= 64 KB of
// L2-resident data, read as 16-byte vectors), 8 row groups of 32 threads; part[rg][st * 64 + col] = row group rg's sum of statistic st.
// The order of the loads and of the additions is part of the result.
__device__ __forceinline__ void slab_colsum64(const float* __restrict__ slab, int rows, int C, int chunk, double (*part)[128]) {
    const int q = threadIdx.x & 31, rg = threadIdx.x >> 5;          // 16-byte column quad (16 per statistic), row group
    const float* base = slab + (size_t)(q >> 4) * C + chunk * 64 + (q & 15) * 4;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int r = rg;
    for (; r + 56 < rows; r += 64) {      // eight independent 16-byte loads in flight (same order of additions as the four-load form)
        const f32x4 u = *(const f32x4*)(base + (size_t)r * 2 * C), v = *(const f32x4*)(base + (size_t)(r + 8) * 2 * C);
        const f32x4 w = *(const f32x4*)(base + (size_t)(r + 16) * 2 * C), x = *(const f32x4*)(base + (size_t)(r + 24) * 2 * C);
        const f32x4 u2 = *(const f32x4*)(base + (size_t)(r + 32) * 2 * C), v2 = *(const f32x4*)(base + (size_t)(r + 40) * 2 * C);
        const f32x4 w2 = *(const f32x4*)(base + (size_t)(r + 48) * 2 * C), x2 = *(const f32x4*)(base + (size_t)(r + 56) * 2 * C);
        a0 += ((double)u[0] + (double)v[0]) + ((double)w[0] + (double)x[0]);
        a1 += ((double)u[1] + (double)v[1]) + ((double)w[1] + (double)x[1]);
        a2 += ((double)u[2] + (double)v[2]) + ((double)w[2] + (double)x[2]);
        a3 += ((double)u[3] + (double)v[3]) + ((double)w[3] + (double)x[3]);
        a0 += ((double)u2[0] + (double)v2[0]) + ((double)w2[0] + (double)x2[0]);
        a1 += ((double)u2[1] + (double)v2[1]) + ((double)w2[1] + (double)x2[1]);
        a2 += ((double)u2[2] + (double)v2[2]) + ((double)w2[2] + (double)x2[2]);
        a3 += ((double)u2[3] + (double)v2[3]) + ((double)w2[3] + (double)x2[3]);
    }
    for (; r + 24 < rows; r += 32) {      // four independent 16-byte loads in flight
        const f32x4 u = *(const f32x4*)(base + (size_t)r * 2 * C), v = *(const f32x4*)(base + (size_t)(r + 8) * 2 * C);
        const f32x4 w = *(const f32x4*)(base + (size_t)(r + 16) * 2 * C), x = *(const f32x4*)(base + (size_t)(r + 24) * 2 * C);
        a0 += ((double)u[0] + (double)v[0]) + ((double)w[0] + (double)x[0]);
        a1 += ((double)u[1] + (double)v[1]) + ((double)w[1] + (double)x[1]);
        a2 += ((double)u[2] + (double)v[2]) + ((double)w[2] + (double)x[2]);
        a3 += ((double)u[3] + (double)v[3]) + ((double)w[3] + (double)x[3]);
    }
    for (; r < rows; r += 8) {
        const f32x4 u = *(const f32x4*)(base + (size_t)r * 2 * C);
        a0 += (double)u[0]; a1 += (double)u[1]; a2 += (double)u[2]; a3 += (double)u[3];
    }
    part[rg][q * 4 + 0] = a0; part[rg][q * 4 + 1] = a1; part[rg][q * 4 + 2] = a2; part[rg][q * 4 + 3] = a3;
}
// Finalize: reduce the conv epilogue's partial sums in fp64, produce scale/shift and saved mean/invstd, update running
// stats (momentum, unbiased variance) exactly like torch.nn.BatchNorm2d in train().
__global__ __launch_bounds__(FIN_T) void bn_finalize_k(const float* __restrict__ slab, int rows, int C, double count, const float* __restrict__ gamma,
                              const float* __restrict__ beta, float* __restrict__ running_mean, float* __restrict__ running_var,
                              long long* __restrict__ nbt, float momentum, float eps, float* __restrict__ scale,
                              float* __restrict__ shift, float* __restrict__ save_mean, float* __restrict__ save_invstd,
                              const float* __restrict__ pre_bias = nullptr) {
    __shared__ double red[FIN_RL][FIN_C][2];
    const int c = blockIdx.x * FIN_C + (threadIdx.x % FIN_C);
    if (blockIdx.x == 0 && threadIdx.x == 0 && nbt) *nbt += 1;
    double s1, s2;
    slab_colsum(slab, rows, C, c, c < C, s1, s2, red);
    if ((threadIdx.x / FIN_C) != 0 || c >= C) return;
    double mean, var;
    bn_stats_finish(s1, s2, count, mean, var);
    // pre_bias: the producing convolution adds a per-channel bias AFTER its statistics epilogue (the sums are those of the raw
    // accumulators): the mean of what it stored is shifted by it, the variance is not (Upsampling(bias=True), pose_resnet.py:15,41)
    if (pre_bias) mean += (double)pre_bias[c];
    const float invstd = bn_invstd(var, eps);
    const float sc = bn_scale(gamma[c], invstd);
    scale[c] = sc;
    shift[c] = bn_shift(beta[c], (float)mean, sc);
    save_mean[c] = (float)mean;
    save_invstd[c] = invstd;
    const double unb = bn_unbiased_var(var, count);
    save_invstd[C + c] = (float)unb;          // third saved vector: unbiased variance (deferred running-stat update)
    if (running_mean) bn_running_update1(running_mean, running_var, c, momentum, (float)mean, (float)unb);
}
// deferred running-statistics update of one BN layer from its saved batch statistics [3][C] (mean, invstd, unbiased var):
// used when a forward ran concurrently with another forward of the same module and must not race on the buffers
__global__ void bn_running_update_k(const float* __restrict__ save, int C, float* __restrict__ rm, float* __restrict__ rv,
                                    long long* __restrict__ nbt, float momentum) {
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c == 0 && nbt) *nbt += 1;
    if (c >= C) return;
    bn_running_update1(rm, rv, c, momentum, save[c], save[2 * C + c]);
}
// y += x over n floats (n % 4 == 0): sum of the two per-pass flat gradient buffers
__global__ void axpy_k(float* __restrict__ y, const float* __restrict__ x, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n4; i += (size_t)gridDim.x * TPB) {
        f32x4 a = *(f32x4*)(y + i * 4);
        const f32x4 b = *(const f32x4*)(x + i * 4);
        a[0] += b[0]; a[1] += b[1]; a[2] += b[2]; a[3] += b[3];
        *(f32x4*)(y + i * 4) = a;
    }
}
__global__ void axpy_tail_k(float* __restrict__ y, const float* __restrict__ x, int n) {
    if ((int)threadIdx.x < n) y[threadIdx.x] += x[threadIdx.x];
}
// eval mode: scale/shift from running statistics
__global__ void bn_eval_coeff_k(int C, const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ rm,
                                const float* __restrict__ rv, float eps, float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c >= C) return;
    const float sc = gamma[c] / sqrtf(rv[c] + eps);
    scale[c] = sc;
    shift[c] = beta[c] - rm[c] * sc;
}

// z = [relu]( y*scale[c] + shift[c] [+ res] ), NHWC (bf16 or fp32 storage), 8 channels per thread
// (TY: storage of the conv output y; T: storage of the residual and of z - the f16x2 mode keeps y in fp32 and z split)
// (SH, 'strict' plans: T = sp32, TY = float; also y16 = fp16(y), z16 = the h half of z and, where mask is given, the ReLU bit mask of z16)
template <typename T, typename TY = T, bool SH = false>
__global__ void bn_apply_k(const TY* __restrict__ y, const T* __restrict__ res, T* __restrict__ z, size_t n8, int C,
                           const float* __restrict__ scale, const float* __restrict__ shift, int relu, unsigned char* __restrict__ mask = nullptr,
                           int xcd = 0, _Float16* __restrict__ y16 = nullptr, _Float16* __restrict__ z16 = nullptr) {
    const int G = C >> 3;
    // the launcher keeps gridDim.x * TPB a multiple of G (G is a power of two <= TPB, or the grid is one block per G-aligned
    // stride), so a thread's channel group never changes: its coefficients are loaded once
    const int c0 = (int)(((size_t)blockIdx.x * TPB + threadIdx.x) % G) * 8;
    float sc[8], sh[8];
    ld8<float>(scale + c0, sc);
    ld8<float>(shift + c0, sh);
    size_t i, iend, istep;
    xcd_stream_range(n8, G, xcd, i, iend, istep);
    for (; i < iend; i += istep) {
        float v[8], o[8];
        ld8<TY>(y + i * 8, v);
        if constexpr (SH) st8_f16(y16 + i * 8, v);
        bn_apply8<T>(v, sc, sh, res, i * 8, relu, o);
        bn_store8<T, SH>(z, z16, mask, i * 8, i, o);
    }
}

// output height / width of the 3x3 stride-2 pad-1 max-pool
__host__ __device__ inline int pool3x3s2_out(int H) { return (H + 2 - 3) / 2 + 1; }
// The gradient entering the stem's BatchNorm, gathered on the fly from the gradient of the 3x3 stride-2 max-pool's OUTPUT and the
// saved winning taps (the <= 4 windows that contain the pixel, fp32 sum, rounded to the storage type; no atomics) - the full-resolution
// gradient tensor (67 MB per pass at 256x256, b=32) is never written or re-read; maxpool3x3s2_bwd_k writes exactly these values where a
// plan does keep that tensor.  pix = flat NHW index of the pool INPUT.
struct PoolSrc { const elem_t* dy; const unsigned char* idx; int H, W; };
__device__ __forceinline__ void pool_grad8(const PoolSrc& ps, size_t pix, int C, int c0, float (&d)[8]) {
    const int w = (int)(pix % ps.W);
    const size_t r = pix / ps.W;
    const int h = (int)(r % ps.H);
    const size_t n = r / ps.H;
    const int Ho = pool3x3s2_out(ps.H), Wo = pool3x3s2_out(ps.W);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int ho = h >> 1; ho <= ((h + 1) >> 1); ++ho)       // windows with ho in {h/2, h/2 + 1 if h odd}: 2ho-1 <= h <= 2ho+1
        for (int wo = w >> 1; wo <= ((w + 1) >> 1); ++wo) {
            if (ho >= Ho || wo >= Wo) continue;
            const int kh = h - (ho * 2 - 1), kw = w - (wo * 2 - 1);
            if (kh < 0 || kh > 2 || kw < 0 || kw > 2) continue;
            const size_t o = ((n * Ho + ho) * Wo + wo) * C + c0;
            const unsigned long long pk = *(const unsigned long long*)(ps.idx + o);
            const elem8 dd = *(const elem8*)(ps.dy + o);
            const unsigned tap = (unsigned)(kh * 3 + kw);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (((pk >> (8 * e)) & 0xFF) == tap) acc[e] += (float)dd[e];
        }
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = (float)(elem_t)acc[e];
}

// ---- building blocks of the BatchNorm backward.  The gradient entering it (DZ) may be kept in fp32 near the loss, where
// g - mean(g) - xhat*mean(g*xhat) cancels most of g and bf16 rounding of g would dominate the result.
// scale / shift for the ReLU mask rebuilt from y (relu == 2: the forward's own, z is not read); zero otherwise
__device__ __forceinline__ void bn_bwd_mask_coef8(int relu, const float* __restrict__ gamma, const float* __restrict__ beta, int c0, const float (&mu)[8],
                                                  const float (&is)[8], float (&sc)[8], float (&sh)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { sc[e] = 0.f; sh[e] = 0.f; }
    if (relu == 2) {
        float ga[8], be[8];
        ld8<float>(gamma + c0, ga);
        ld8<float>(beta + c0, be);
        bn_scale_shift8(ga, be, mu, is, sc, sh);
    }
}
// the stored z of a 16-byte group where the mask is read from it (relu == 1)
__device__ __forceinline__ elem8 bn_bwd_ldz8(int relu, const elem_t* __restrict__ z, size_t off) {
    elem8 zz = {};
    if (relu == 1) zz = *(const elem8*)(z + off);
    return zz;
}
// g = d under the ReLU mask: relu 0 none, 1 the stored z > 0, 2 y * sc + sh > 0 (the forward's z rebuilt: bn_bwd_mask_coef8)
__device__ __forceinline__ float bn_bwd_g(int relu, float d, float y, float z, float sc, float sh) {
    float gv = d;
    if (relu == 1 && !(z > 0.f)) gv = 0.f;
    if (relu == 2 && !(y * sc + sh > 0.f)) gv = 0.f;
    return gv;
}
__device__ __forceinline__ float bn_xhat(float y, float mu, float is) { return (y - mu) * is; }
// dy = ca*(g - cb - xhat*cc)
__device__ __forceinline__ elem_t bn_bwd_dy(float g, float y, float mu, float is, float ca, float cb, float cc) {
    const float xh = bn_xhat(y, mu, is);
    return (elem_t)(ca * (g - cb - xh * cc));
}
// 8 channels of a pixel, element by element (the order the expressions are formed in is kept per element):
// the reduce's s1 += g, s2 += g * xhat
__device__ __forceinline__ void bn_bwd_sums8(int relu, const float (&d)[8], const elem8& yy, const elem8& zz, const float (&sc)[8], const float (&sh)[8],
                                             const float (&mu)[8], const float (&is)[8], float (&s1)[8], float (&s2)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float gv = bn_bwd_g(relu, d[e], (float)yy[e], (float)zz[e], sc[e], sh[e]);
        s1[e] += gv;
        s2[e] += gv * bn_xhat((float)yy[e], mu[e], is[e]);
    }
}
// the apply's dy and g (the masked d, for the skip branch)
__device__ __forceinline__ void bn_bwd_g8_dy8(int relu, const float (&d)[8], const elem8& yy, const elem8& zz, const float (&sc)[8], const float (&sh)[8],
                                              const float (&mu)[8], const float (&is)[8], const float (&ca)[8], const float (&cb)[8],
                                              const float (&cc)[8], elem8& o, elem8& go) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float gv = bn_bwd_g(relu, d[e], (float)yy[e], (float)zz[e], sc[e], sh[e]);
        o[e] = bn_bwd_dy(gv, (float)yy[e], mu[e], is[e], ca[e], cb[e], cc[e]);
        go[e] = (elem_t)gv;
    }
}
// dy of an already masked g
__device__ __forceinline__ elem8 bn_bwd_dy8(const float (&g)[8], const elem8& yy, const float (&mu)[8], const float (&is)[8], const float (&ca)[8],
                                            const float (&cb)[8], const float (&cc)[8]) {
    elem8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = bn_bwd_dy(g[e], (float)yy[e], mu[e], is[e], ca[e], cb[e], cc[e]);
    return o;
}
// apply coefficients of one channel from its sums over the M = count pixels: ca = gamma*invstd, cb = sum(g)/M, cc = sum(g*xhat)/M
__device__ __forceinline__ void bn_bwd_coef(float gamma, float invstd, double s1, double s2, double count, float& ca, float& cb, float& cc) {
    ca = bn_scale(gamma, invstd);
    cb = (float)(s1 / count);
    cc = (float)(s2 / count);
}
// dgamma, dbeta (beta_acc*old + new) of channel c from s1 = sum(g), s2 = sum(g*xhat)
__device__ __forceinline__ void bwd_param_acc(float* __restrict__ dgamma, float* __restrict__ dbeta, int c, float beta_acc, double s1, double s2) {
    dgamma[c] = (beta_acc != 0.f ? beta_acc * dgamma[c] : 0.f) + (float)s2;
    dbeta[c] = (beta_acc != 0.f ? beta_acc * dbeta[c] : 0.f) + (float)s1;
}
// chunked kernels: a thread's apply coefficients from the chunk totals tot[2][64] = (sum(g), sum(g*xhat)) of its 64 channels
__device__ __forceinline__ void chunk_bwd_coef8(const double (*tot)[64], int cg, double count, const float (&ga)[8], const float (&is)[8], float (&ca)[8],
                                                float (&cb)[8], float (&cc)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) bn_bwd_coef(ga[e], is[e], tot[0][cg * 8 + e], tot[1][cg * 8 + e], count, ca[e], cb[e], cc[e]);
}

// Backward reduce: per-channel sum(g) and sum(g*xhat), g = dz * (z>0) when relu.  Partial slab [blocks][2][C].
// Requires C/8 to be a power of two <= 256 (thread's channel group is loop-invariant).
template <typename DZ, bool POOL = false>
__global__ void bn_bwd_reduce_k(const DZ* __restrict__ dz, const elem_t* __restrict__ z, const elem_t* __restrict__ y,
                                size_t npix, int C, const float* __restrict__ mean, const float* __restrict__ invstd, int relu,
                                float* __restrict__ slab, int pix_per_block, const float* __restrict__ gamma, const float* __restrict__ beta,
                                PoolSrc ps = PoolSrc{nullptr, nullptr, 0, 0}) {
    __shared__ float red[TPB][17];
    const int G = C >> 3;
    const int g = threadIdx.x % G, prow = threadIdx.x / G, pstep = TPB / G;
    const int c0 = g * 8;
    float mu[8], is[8], s1[8], s2[8], sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { mu[e] = mean[c0 + e]; is[e] = invstd[c0 + e]; s1[e] = 0.f; s2[e] = 0.f; }
    bn_bwd_mask_coef8(relu, gamma, beta, c0, mu, is, sc, sh);
    size_t p0, p1;
    pix_range(blockIdx.x, pix_per_block, npix, p0, p1);
    for (size_t p = p0 + prow; p < p1; p += pstep) {
        const size_t off = p * C + c0;
        float d[8];
        if constexpr (POOL) pool_grad8(ps, p, C, c0, d);
        else ld8<DZ>(dz + off, d);
        const elem8 yy = *(const elem8*)(y + off);
        bn_bwd_sums8(relu, d, yy, bn_bwd_ldz8(relu, z, off), sc, sh, mu, is, s1, s2);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[threadIdx.x][e] = s1[e]; red[threadIdx.x][8 + e] = s2[e]; }
    __syncthreads();
    if (threadIdx.x < G) {
        float a[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) a[e] = 0.f;
        for (int k = 0; k < pstep; ++k)
#pragma unroll
            for (int e = 0; e < 16; ++e) a[e] += red[threadIdx.x + k * G][e];
        float* sp = slab + (size_t)blockIdx.x * 2 * C;
#pragma unroll
        for (int e = 0; e < 8; ++e) { sp[c0 + e] = a[e]; sp[C + c0 + e] = a[8 + e]; }
    }
}
// Finalize backward: dgamma, dbeta and the apply coefficients coef[3][C] = (ca, cb, cc).
__global__ __launch_bounds__(FIN_T) void bn_bwd_finalize_k(const float* __restrict__ slab, int rows, int C, double count, const float* __restrict__ gamma,
                                  const float* __restrict__ invstd, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                  float beta_acc, float* __restrict__ coef) {
    __shared__ double red[FIN_RL][FIN_C][2];
    const int c = blockIdx.x * FIN_C + (threadIdx.x % FIN_C);
    double s1, s2;
    slab_colsum(slab, rows, C, c, c < C, s1, s2, red);
    if ((threadIdx.x / FIN_C) != 0 || c >= C) return;
    if (dgamma) bwd_param_acc(dgamma, dbeta, c, beta_acc, s1, s2);
    bn_bwd_coef(gamma[c], invstd[c], s1, s2, count, coef[c], coef[C + c], coef[2 * C + c]);
}
// dy = ca*(g - cb - xhat*cc); optionally also write g (masked dz) for the skip branch
template <typename DZ, bool POOL = false>
__global__ void bn_bwd_apply_k(const DZ* __restrict__ dz, const elem_t* __restrict__ z, const elem_t* __restrict__ y,
                               elem_t* __restrict__ dy, elem_t* __restrict__ gout, size_t n8, int C, const float* __restrict__ mean,
                               const float* __restrict__ invstd, const float* __restrict__ coef, int relu, const float* __restrict__ gamma,
                               const float* __restrict__ beta, PoolSrc ps = PoolSrc{nullptr, nullptr, 0, 0}) {
    const int G = C >> 3;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n8; i += (size_t)gridDim.x * TPB) {
        const int c0 = (int)(i % G) * 8;
        float d[8];
        if constexpr (POOL) pool_grad8(ps, i / G, C, c0, d);
        else ld8<DZ>(dz + i * 8, d);
        const elem8 yy = *(const elem8*)(y + i * 8);
        const elem8 zz = bn_bwd_ldz8(relu, z, i * 8);
        // per-channel coefficients as 16-byte loads (8 consecutive channels), per iteration: the channel group changes with i
        float mu[8], is[8], ca[8], cb[8], cc[8], sc[8], sh[8];
        ld8<float>(mean + c0, mu);
        ld8<float>(invstd + c0, is);
        ld8<float>(coef + c0, ca);
        ld8<float>(coef + C + c0, cb);
        ld8<float>(coef + 2 * C + c0, cc);
        bn_bwd_mask_coef8(relu, gamma, beta, c0, mu, is, sc, sh);
        elem8 o, go;
        bn_bwd_g8_dy8(relu, d, yy, zz, sc, sh, mu, is, ca, cb, cc, o, go);
        *(elem8*)(dy + i * 8) = o;
        if (gout) *(elem8*)(gout + i * 8) = go;
    }
}

// ---- channel-chunked BN forward: finalize + apply in one launch (wide, small-spatial layers) ---------------------------
// Work-group = 64 channels x one pixel range, grid (C/64, S).  Prelude: the work-group column-sums its 64 channels of the conv
// epilogue's partial-statistics slab ([rows][2][C], rows <= 128 since the igemm adds its wave rows itself) in fp64 with a fixed
// order (slab_colsum64) and derives scale / shift with the functions bn_finalize_k uses; the sp == 0 work-groups also write the
// saved statistics and the running-statistics update.  Then it streams its pixels.
// (TY / TZ: element types of the pre-BN conv output and of the residual / output: elem_t, elem_t in the 16-bit modes; float, sp32 in the
// f16x2 mode, whose convolutions leave y in fp32 and whose activations are split tensors)
// (SH: the 'strict' form of the f16x2 instance - y16 / z16 / mask as in bn_apply_k)
template <typename TY, typename TZ, bool SH = false>
__global__ __launch_bounds__(TPB) void bn_apply_chunk_k(const TY* __restrict__ y, const TZ* __restrict__ res, TZ* __restrict__ z,
                                                        size_t npix, int C, const float* __restrict__ slab, int rows, double count,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                        float momentum, float* __restrict__ running_mean, float* __restrict__ running_var,
                                                        long long* __restrict__ nbt, float* __restrict__ save, int relu, int P,
                                                        unsigned char* __restrict__ mask, int xcd, _Float16* __restrict__ y16 = nullptr,
                                                        _Float16* __restrict__ z16 = nullptr) {
    __shared__ double part[8][128];
    __shared__ float scs[64], shs[64];
    int chunk, sp;
    xcd_chunk_of(xcd, chunk, sp);
    slab_colsum64(slab, rows, C, chunk, part);
    __syncthreads();
    if (threadIdx.x < 64) {
        const int col = threadIdx.x, c = chunk * 64 + col;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) { s1 += part[k][col]; s2 += part[k][64 + col]; }
        double mean, var;
        bn_stats_finish(s1, s2, count, mean, var);
        const float invstd = bn_invstd(var, eps);
        const float sc = bn_scale(gamma[c], invstd);
        scs[col] = sc;
        shs[col] = bn_shift(beta[c], (float)mean, sc);
        if (sp == 0) {
            const double unb = bn_unbiased_var(var, count);
            save[c] = (float)mean;
            save[C + c] = invstd;
            save[2 * C + c] = (float)unb;
            if (running_mean) bn_running_update1(running_mean, running_var, c, momentum, (float)mean, (float)unb);
            if (c == 0 && nbt) *nbt += 1;
        }
    }
    __syncthreads();
    const int cg = threadIdx.x & 7, prow = threadIdx.x >> 3;
    const int c0 = chunk * 64 + cg * 8;
    float sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { sc[e] = scs[cg * 8 + e]; sh[e] = shs[cg * 8 + e]; }
    size_t p0, p1;
    pix_range(sp, P, npix, p0, p1);
    for (size_t p = p0 + prow; p < p1; p += 32) {
        const size_t off = p * C + c0;
        float v[8], o[8];
        ld8<TY>(y + off, v);
        if constexpr (SH) st8_f16(y16 + off, v);
        bn_apply8<TZ>(v, sc, sh, res, off, relu, o);
        bn_store8<TZ, SH>(z, z16, mask, off, off >> 3, o);
    }
}

// ---- channel-chunked BN backward (wide, small-spatial layers: C >= 256, <= 32 K pixels) ------------------------------
// Work-group = 64 channels (one 128-byte segment of every pixel row) x one pixel range; grid (C/64, S).  The reduce writes
// S partial rows per chunk ([chunk][S][2][64] floats, <= 32 KB per chunk), and every apply work-group sums its chunk's rows
// itself (fp64, fixed order) before streaming: the separate finalize launch (6-7 us on the critical path of every layer)
// is gone, at the price of a <= 32 KB L2-resident prelude per work-group.
template <typename DZ>
__global__ __launch_bounds__(TPB) void bn_bwd_reduce_chunk_k(const DZ* __restrict__ dz, const elem_t* __restrict__ z, const elem_t* __restrict__ y,
                                                             size_t npix, int C, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, int relu, float* __restrict__ slab, int P,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta) {
    __shared__ float red[32][8][17];
    const int chunk = blockIdx.x, sp = blockIdx.y, S = gridDim.y;
    const int cg = threadIdx.x & 7, prow = threadIdx.x >> 3;
    const int c0 = chunk * 64 + cg * 8;
    float mu[8], is[8], s1[8], s2[8], sc[8], sh[8];
    ld8<float>(mean + c0, mu);
    ld8<float>(invstd + c0, is);
#pragma unroll
    for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
    bn_bwd_mask_coef8(relu, gamma, beta, c0, mu, is, sc, sh);
    size_t p0, p1;
    pix_range(sp, P, npix, p0, p1);
    for (size_t p = p0 + prow; p < p1; p += 32) {
        const size_t off = p * C + c0;
        float d[8];
        ld8<DZ>(dz + off, d);
        const elem8 yy = *(const elem8*)(y + off);
        bn_bwd_sums8(relu, d, yy, bn_bwd_ldz8(relu, z, off), sc, sh, mu, is, s1, s2);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[prow][cg][e] = s1[e]; red[prow][cg][8 + e] = s2[e]; }
    __syncthreads();
    if (threadIdx.x < 128) {
        const int g = threadIdx.x >> 4, e = threadIdx.x & 15;
        float a = 0.f;
        for (int k = 0; k < 32; ++k) a += red[k][g][e];
        slab[(((size_t)chunk * S + sp) * 2 + (e >> 3)) * 64 + g * 8 + (e & 7)] = a;
    }
}
template <typename DZ>
__global__ __launch_bounds__(TPB) void bn_bwd_apply_chunk_k(const DZ* __restrict__ dz, const elem_t* __restrict__ z, const elem_t* __restrict__ y,
                                                            elem_t* __restrict__ dy, elem_t* __restrict__ gout, size_t npix, int C,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd, int relu,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ slab, int P, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, float beta_acc) {
    __shared__ double tot[2][64];
    const int chunk = blockIdx.x, sp = blockIdx.y, S = gridDim.y;
    if (threadIdx.x < 128) {
        const int st = threadIdx.x >> 6, col = threadIdx.x & 63;
        const float* q = slab + ((size_t)chunk * S * 2 + st) * 64 + col;
        double a = 0.0;
        int k = 0;
        for (; k + 4 <= S; k += 4)        // four independent loads in flight; the order of the fp64 additions is fixed
            a += ((double)q[(size_t)k * 128] + (double)q[(size_t)(k + 1) * 128]) + ((double)q[(size_t)(k + 2) * 128] + (double)q[(size_t)(k + 3) * 128]);
        for (; k < S; ++k) a += (double)q[(size_t)k * 128];
        tot[st][col] = a;
    }
    __syncthreads();
    if (sp == 0 && threadIdx.x < 64 && dgamma) bwd_param_acc(dgamma, dbeta, chunk * 64 + threadIdx.x, beta_acc, tot[0][threadIdx.x], tot[1][threadIdx.x]);
    const int cg = threadIdx.x & 7, prow = threadIdx.x >> 3;
    const int c0 = chunk * 64 + cg * 8;
    float mu[8], is[8], ga[8], ca[8], cb[8], cc[8], sc[8], sh[8];
    ld8<float>(mean + c0, mu);
    ld8<float>(invstd + c0, is);
    ld8<float>(gamma + c0, ga);
    chunk_bwd_coef8(tot, cg, (double)npix, ga, is, ca, cb, cc);
    bn_bwd_mask_coef8(relu, gamma, beta, c0, mu, is, sc, sh);
    size_t p0, p1;
    pix_range(sp, P, npix, p0, p1);
    for (size_t p = p0 + prow; p < p1; p += 32) {
        const size_t off = p * C + c0;
        float d[8];
        ld8<DZ>(dz + off, d);
        const elem8 yy = *(const elem8*)(y + off);
        elem8 o, go;
        bn_bwd_g8_dy8(relu, d, yy, bn_bwd_ldz8(relu, z, off), sc, sh, mu, is, ca, cb, cc, o, go);
        *(elem8*)(dy + off) = o;
        if (gout) *(elem8*)(gout + off) = go;
    }
}

// dy = ca*(g - cb - xhat*cc) for an already masked g (pre-reduced form, layers the chunked kernel does not take): the grid
// keeps gridDim.x * TPB a multiple of C/8 (bn_apply_grid), so a thread's 8 channels never change and its 40 coefficients are
// loaded once instead of per 16-byte access; no integer division in the loop.
template <typename DZ>
__global__ __launch_bounds__(TPB) void bn_bwd_apply_pre_k(const DZ* __restrict__ g, const elem_t* __restrict__ y, elem_t* __restrict__ dy, size_t n8,
                                                          int C, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          const float* __restrict__ coef, int xcd = 0) {
    const int G = C >> 3;
    const int c0 = (int)(((size_t)blockIdx.x * TPB + threadIdx.x) % G) * 8;
    float mu[8], is[8], ca[8], cb[8], cc[8];
    ld8<float>(mean + c0, mu);
    ld8<float>(invstd + c0, is);
    ld8<float>(coef + c0, ca);
    ld8<float>(coef + C + c0, cb);
    ld8<float>(coef + 2 * C + c0, cc);
    size_t i, iend, istep;
    xcd_stream_range(n8, G, xcd, i, iend, istep);
    for (; i < iend; i += istep) {
        float d[8];
        ld8<DZ>(g + i * 8, d);
        const elem8 yy = *(const elem8*)(y + i * 8);
        *(elem8*)(dy + i * 8) = bn_bwd_dy8(d, yy, mu, is, ca, cb, cc);
    }
}

// ---- BN backward whose reduction was done by the producing dgrad's epilogue (igemm.hip, BS mode) -----------------------
// dz already carries the ReLU mask (g), and slab[rows][2][C] holds one partial row of (sum g, sum g*xhat) per m-tile of that
// dgrad launch.  Work-group = 64 channels x one pixel range, grid (C/64, S): prelude = fp64 column sums of the work-group's 64
// channels (slab_colsum64, rows <= 128), then dy = ca*(g - cb - xhat*cc).
template <typename DZ>
__global__ __launch_bounds__(TPB) void bn_bwd_apply_pre_chunk_k(const DZ* __restrict__ g, const elem_t* __restrict__ y, elem_t* __restrict__ dy,
                                                                size_t npix, int C, const float* __restrict__ mean,
                                                                const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                const float* __restrict__ slab, int rows, int P, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, float beta_acc, int xcd) {
    __shared__ double part[8][128];
    __shared__ double tot[2][64];
    int chunk, sp;
    xcd_chunk_of(xcd, chunk, sp);
    slab_colsum64(slab, rows, C, chunk, part);
    __syncthreads();
    if (threadIdx.x < 128) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) a += part[k][threadIdx.x];
        tot[threadIdx.x >> 6][threadIdx.x & 63] = a;
    }
    __syncthreads();
    if (sp == 0 && threadIdx.x < 64 && dgamma) bwd_param_acc(dgamma, dbeta, chunk * 64 + threadIdx.x, beta_acc, tot[0][threadIdx.x], tot[1][threadIdx.x]);
    const int cg = threadIdx.x & 7, prow = threadIdx.x >> 3;
    const int c0 = chunk * 64 + cg * 8;
    float mu[8], is[8], ga[8], ca[8], cb[8], cc[8];
    ld8<float>(mean + c0, mu);
    ld8<float>(invstd + c0, is);
    ld8<float>(gamma + c0, ga);
    chunk_bwd_coef8(tot, cg, (double)npix, ga, is, ca, cb, cc);
    size_t p0, p1;
    pix_range(sp, P, npix, p0, p1);
    for (size_t p = p0 + prow; p < p1; p += 32) {
        const size_t off = p * C + c0;
        float d[8];
        ld8<DZ>(g + off, d);
        const elem8 yy = *(const elem8*)(y + off);
        *(elem8*)(dy + off) = bn_bwd_dy8(d, yy, mu, is, ca, cb, cc);
    }
}

// ------------------------------------------------------------------ max pooling (NHWC bf16)
// The 3x3 stride-2 pad-1 window (ho, wo) of 8 channels: the maximum of tap(v) over the in-range taps and the winning tap (0..8, first
// max in (kh,kw) scan order, a NaN wins: like ATen).  tap transforms a loaded value before it competes.
template <typename T, typename F>
__device__ __forceinline__ void pool3x3s2_scan(const T* __restrict__ x, int n, int ho, int wo, int g, int H, int W, int C, const F& tap, float (&best)[8],
                                               unsigned char (&bi)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { best[e] = -INFINITY; bi[e] = 0; }
    bool first = true;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int h = ho * 2 - 1 + kh, w = wo * 2 - 1 + kw;
            if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
                float v[8];
                ld8<T>(x + (((size_t)n * H + h) * W + w) * C + g * 8, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float f = tap(v[e], e);
                    if (first || f > best[e] || f != f) { best[e] = f; bi[e] = (unsigned char)(kh * 3 + kw); }
                }
                first = false;
            }
        }
}
// the 8 winning taps of a 16-byte group as stored: one byte per channel
__device__ __forceinline__ unsigned long long pack_taps(const unsigned char (&bi)[8]) {
    unsigned long long pk = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) pk |= (unsigned long long)bi[e] << (8 * e);
    return pk;
}
// the per-tap transforms of channel e's value: none (the plain pool), and the stem's BatchNorm + ReLU (bn_apply8's steps without a residual)
// with the rounding of bn_apply_k's 16-bit store
struct TapIdentity {
    __device__ __forceinline__ float operator()(float v, int) const { return v; }
};
struct TapBnRelu {
    float sc[8], sh[8];
    __device__ __forceinline__ float operator()(float v, int e) const { return (float)(elem_t)bn_relu(bn_affine(v, sc[e], sh[e]), 1); }
};
// 3x3 stride 2 pad 1 (ResNet stem).  Saves the winning tap per element.
// (SH, 'strict' plans: T = sp32 and y16 receives the pooled fp16 map, the h half of y)
template <typename T, bool SH = false>
__global__ void maxpool3x3s2_fwd_k(const T* __restrict__ x, T* __restrict__ y, unsigned char* __restrict__ idx, int N, int H,
                                   int W, int C, int Ho, int Wo, _Float16* __restrict__ y16 = nullptr) {
    const int G = C >> 3;
    const size_t total = (size_t)N * Ho * Wo * G;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        int n, ho, wo, g;
        nhwg_of(i, G, Ho, Wo, n, ho, wo, g);
        float best[8];
        unsigned char bi[8];
        pool3x3s2_scan<T>(x, n, ho, wo, g, H, W, C, TapIdentity{}, best, bi);
        if constexpr (SH) (void)st8_split_shadow(y + i * 8, y16 + i * 8, best);     // ('strict': the pooled fp16 map, T = sp32)
        else st8<T>(y + i * 8, best);
        if (idx) *(unsigned long long*)(idx + i * 8) = pack_taps(bi);
    }
}
// The stem's BatchNorm apply + ReLU + 3x3 stride-2 max-pool in ONE sweep: z = relu(y*scale + shift) is formed per tap in registers by
// TapBnRelu - bn_affine and bn_relu, the scalar steps bn_apply8 is made of - and rounded to the storage type (so values, ties and winning
// taps are exactly those of bn_apply_k followed by maxpool3x3s2_fwd_k) and never written: the backward recomputes the ReLU mask from y.
// Saves one 67 MB write and one (1.5x amplified) read per pass.
__global__ void bn_relu_maxpool3x3s2_k(const elem_t* __restrict__ x, elem_t* __restrict__ y, unsigned char* __restrict__ idx, int N, int H, int W,
                                       int C, int Ho, int Wo, const float* __restrict__ scale, const float* __restrict__ shift) {
    const int G = C >> 3;
    const size_t total = (size_t)N * Ho * Wo * G;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        int n, ho, wo, g;
        nhwg_of(i, G, Ho, Wo, n, ho, wo, g);
        TapBnRelu bn;
        ld8<float>(scale + g * 8, bn.sc);
        ld8<float>(shift + g * 8, bn.sh);
        float best[8];
        unsigned char bi[8];
        pool3x3s2_scan<elem_t>(x, n, ho, wo, g, H, W, C, bn, best, bi);
        st8<elem_t>(y + i * 8, best);
        *(unsigned long long*)(idx + i * 8) = pack_taps(bi);
    }
}
// gather-style backward (no atomics): each input pixel checks the <=4 windows that contain it
__global__ void maxpool3x3s2_bwd_k(const elem_t* __restrict__ dy, const unsigned char* __restrict__ idx, elem_t* __restrict__ dx, int N,
                                   int H, int W, int C) {
    const int G = C >> 3;
    const size_t total = (size_t)N * H * W * G;
    const PoolSrc ps{dy, idx, H, W};
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        float d[8];
        pool_grad8(ps, i / G, C, (int)(i % G) * 8, d);
        st8<elem_t>(dx + i * 8, d);
    }
}
// 2x2 stride 2 ceil-mode (VGG encoder, inference only)
template <typename T>
__global__ void maxpool2x2_ceil_k(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C, int Ho, int Wo) {
    const int G = C >> 3;
    const size_t total = (size_t)N * Ho * Wo * G;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        int n, ho, wo, g;
        nhwg_of(i, G, Ho, Wo, n, ho, wo, g);
        float best[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) best[e] = -INFINITY;
        for (int kh = 0; kh < 2; ++kh)
            for (int kw = 0; kw < 2; ++kw) {
                const int h = ho * 2 + kh, w = wo * 2 + kw;
                if (h < H && w < W) {
                    float v[8];
                    ld8<T>(x + (((size_t)n * H + h) * W + w) * C + g * 8, v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float f = v[e];
                        if (f > best[e] || f != f) best[e] = f;     // (a NaN wins, as in maxpool3x3s2_fwd_k and ATen; fmaxf would drop it)
                    }
                }
            }
        st8<T>(y + i * 8, best);
    }
}

// per-plane sums of an NCHW fp32 tensor over (n, hw): out[c] (beta*old +) = sum  (head bias gradient)
__global__ __launch_bounds__(1024) void plane_sum_k(const float* __restrict__ x, float* __restrict__ out, int N, int C, int HW, float beta) {
    const int c = blockIdx.x;
    double s = 0.0;
    if ((HW & 3) == 0) {
        const int hw4 = HW >> 2;
        for (int i = threadIdx.x; i < hw4; i += 1024) {
            int n = 0;
            for (; n + 4 <= N; n += 4) {          // four independent 16-byte loads in flight
                const f32x4 a = *(const f32x4*)(x + ((size_t)n * C + c) * HW + 4 * i);
                const f32x4 b = *(const f32x4*)(x + ((size_t)(n + 1) * C + c) * HW + 4 * i);
                const f32x4 d = *(const f32x4*)(x + ((size_t)(n + 2) * C + c) * HW + 4 * i);
                const f32x4 e = *(const f32x4*)(x + ((size_t)(n + 3) * C + c) * HW + 4 * i);
                s += (double)((a[0] + a[1]) + (a[2] + a[3])) + (double)((b[0] + b[1]) + (b[2] + b[3])) +
                     (double)((d[0] + d[1]) + (d[2] + d[3])) + (double)((e[0] + e[1]) + (e[2] + e[3]));
            }
            for (; n < N; ++n) {
                const f32x4 a = *(const f32x4*)(x + ((size_t)n * C + c) * HW + 4 * i);
                s += (double)((a[0] + a[1]) + (a[2] + a[3]));
            }
        }
    } else {
        for (int n = 0; n < N; ++n)
            for (int i = threadIdx.x; i < HW; i += 1024) s += (double)x[((size_t)n * C + c) * HW + i];
    }
    __shared__ double red[16];
    const double t = block_sum<16>(s, red);
    if (threadIdx.x == 0) {
        out[c] = (beta != 0.f ? beta * out[c] : 0.f) + (float)t;
    }
}

}  // namespace

// ------------------------------------------------------------------ host launchers (internal C++ API; C-ABI wrappers in capi.hip)
int pw_nchw_f32_to_nhwc_bf16(hipStream_t s, const float* src, elem_t* dst, int N, int C, int HW, int Cp) {
    if (Cp % 8) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(nchw_f32_to_nhwc_k<elem_t>, dim3(grid_for((size_t)N * HW * (Cp / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, src, dst, N, C, HW, Cp);
    return udapose_check_launch();
}
int pw_nchw_f32_to_nhwc_f32(hipStream_t s, const float* src, float* dst, int N, int C, int HW, int Cp) {
    if (Cp % 8) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(nchw_f32_to_nhwc_k<float>, dim3(grid_for((size_t)N * HW * (Cp / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, src, dst, N, C, HW, Cp);
    return udapose_check_launch();
}
int pw_nchw_f32_to_nhwc_split(hipStream_t s, const float* src, void* dst, int N, int C, int HW, int Cp, void* dst16) {
    if (Cp % 8) return UDAPOSE_ERR_ARG;
    if (dst16)      // ('strict' plans: the fp16 image for the 16-bit backward in the same pass)
        hipLaunchKernelGGL((nchw_f32_to_nhwc_k<sp32, true>), dim3(grid_for((size_t)N * HW * (Cp / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, src, (sp32*)dst, N, C, HW, Cp,
                           (_Float16*)dst16);
    else
        hipLaunchKernelGGL(nchw_f32_to_nhwc_k<sp32>, dim3(grid_for((size_t)N * HW * (Cp / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, src, (sp32*)dst, N, C, HW, Cp);
    return udapose_check_launch();
}
// src_is_f32: 0 = element type, 1 = fp32, 2 = f16x2 split
int pw_nhwc_to_nchw_f32(hipStream_t s, const void* src, int src_is_f32, float* dst, int N, int C, int HW, int Cs, const float* lo, const float* hi) {
    if (src_is_f32 == 2)
        hipLaunchKernelGGL(nhwc_to_nchw_f32_k<sp32>, dim3(grid_for((size_t)N * HW, TPB, GRID_CAP)), dim3(TPB), 0, s, (const sp32*)src, dst, N, C, HW, Cs, lo, hi);
    else if (src_is_f32)
        hipLaunchKernelGGL(nhwc_to_nchw_f32_k<float>, dim3(grid_for((size_t)N * HW, TPB, GRID_CAP)), dim3(TPB), 0, s, (const float*)src, dst, N, C, HW, Cs, lo, hi);
    else
        hipLaunchKernelGGL(nhwc_to_nchw_f32_k<elem_t>, dim3(grid_for((size_t)N * HW, TPB, GRID_CAP)), dim3(TPB), 0, s, (const elem_t*)src, dst, N, C, HW, Cs, lo, hi);
    return udapose_check_launch();
}
int pw_cast_f32_bf16(hipStream_t s, const float* src, elem_t* dst, size_t n) {
    if (n % 8) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(cast_f32_bf16_k, dim3(grid_for(n / 8, TPB, GRID_CAP)), dim3(TPB), 0, s, src, dst, n / 8);
    return udapose_check_launch();
}
int pw_transpose_cast(hipStream_t s, const float* src, elem_t* dst, int A, int T, int B) {
    hipLaunchKernelGGL(transpose_cast_k<elem_t>, dim3((B + 31) / 32, (A + 31) / 32, T), dim3(TPB), 0, s, src, dst, A, T, B);
    return udapose_check_launch();
}
int pw_transpose_f32(hipStream_t s, const float* src, float* dst, int A, int T, int B) {
    hipLaunchKernelGGL(transpose_cast_k<float>, dim3((B + 31) / 32, (A + 31) / 32, T), dim3(TPB), 0, s, src, dst, A, T, B);
    return udapose_check_launch();
}
// fp32 -> f16x2 split, n % 8 == 0 (src == dst allowed: every thread reads its 32 bytes before it writes them)
__global__ void f32_to_split_k(const float* src, sp32* dst, size_t n8) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n8; i += (size_t)gridDim.x * TPB) {
        float v[8];
        ld8<float>(src + i * 8, v);
        st8<sp32>(dst + i * 8, v);
    }
}
__global__ void split_to_f32_k(const sp32* src, float* dst, size_t n8) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n8; i += (size_t)gridDim.x * TPB) {
        float v[8];
        ld8<sp32>(src + i * 8, v);
        st8<float>(dst + i * 8, v);
    }
}
int pw_f32_to_split(hipStream_t s, const float* src, void* dst, size_t n) {
    if (n % 8) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(f32_to_split_k, dim3(grid_for(n / 8, TPB, GRID_CAP)), dim3(TPB), 0, s, src, (sp32*)dst, n / 8);
    return udapose_check_launch();
}
int pw_split_to_f32(hipStream_t s, const void* src, float* dst, size_t n) {
    if (n % 8) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(split_to_f32_k, dim3(grid_for(n / 8, TPB, GRID_CAP)), dim3(TPB), 0, s, (const sp32*)src, dst, n / 8);
    return udapose_check_launch();
}
int pw_transpose_split(hipStream_t s, const float* src, void* dst, int A, int T, int B) {
    hipLaunchKernelGGL(transpose_cast_k<sp32>, dim3((B + 31) / 32, (A + 31) / 32, T), dim3(TPB), 0, s, src, (sp32*)dst, A, T, B);
    return udapose_check_launch();
}
int pw_pack_strided_split(hipStream_t s, const float* src, void* dst, int A, int KH, int KWp, int KW, int Bp, int B, long sa, long skh, long skw, long sb) {
    hipLaunchKernelGGL(pack_strided_k<sp32>, dim3(grid_for((size_t)A * KH * KWp * Bp, TPB, GRID_CAP)), dim3(TPB), 0, s, src, (sp32*)dst, A, KH, KWp, KW, Bp, B, sa, skh, skw, sb);
    return udapose_check_launch();
}
int pw_pack_multi(hipStream_t s, const void* jobs, const int* blk_job, const int* blk_sub, int nblocks) {
    if (nblocks <= 0) return UDAPOSE_OK;
    hipLaunchKernelGGL(pack_multi_k, dim3(nblocks), dim3(TPB), 0, s, (const PackJob*)jobs, blk_job, blk_sub);
    return udapose_check_launch();
}
int pw_pack_strided(hipStream_t s, const float* src, elem_t* dst, int A, int KH, int KWp, int KW, int Bp, int B, long sa, long skh, long skw, long sb) {
    hipLaunchKernelGGL(pack_strided_k<elem_t>, dim3(grid_for((size_t)A * KH * KWp * Bp, TPB, GRID_CAP)), dim3(TPB), 0, s, src, dst, A, KH, KWp, KW, Bp, B, sa, skh, skw, sb);
    return udapose_check_launch();
}
int pw_pack_strided_f32(hipStream_t s, const float* src, float* dst, int A, int KH, int KWp, int KW, int Bp, int B, long sa, long skh, long skw, long sb) {
    hipLaunchKernelGGL(pack_strided_k<float>, dim3(grid_for((size_t)A * KH * KWp * Bp, TPB, GRID_CAP)), dim3(TPB), 0, s, src, dst, A, KH, KWp, KW, Bp, B, sa, skh, skw, sb);
    return udapose_check_launch();
}
int pw_unpack_strided(hipStream_t s, const float* src, float* dst, int A, int KH, int KWp, int KW, int Bp, int B, long sa, long skh, long skw, long sb, float beta) {
    hipLaunchKernelGGL(unpack_strided_k, dim3(grid_for((size_t)A * KH * KW * B, TPB, GRID_CAP)), dim3(TPB), 0, s, src, dst, A, KH, KWp, KW, Bp, B, sa, skh, skw, sb, beta);
    return udapose_check_launch();
}
int pw_bn_finalize(hipStream_t s, const float* slab, int rows, int C, double count, const float* gamma, const float* beta, float* rm, float* rv,
                   long long* nbt, float momentum, float eps, float* scale, float* shift, float* save_mean, float* save_invstd, const float* pre_bias) {
    hipLaunchKernelGGL(bn_finalize_k, dim3((C + FIN_C - 1) / FIN_C), dim3(FIN_T), 0, s, slab, rows, C, count, gamma, beta, rm, rv, nbt, momentum, eps, scale, shift,
                       save_mean, save_invstd, pre_bias);
    return udapose_check_launch();
}
// launch geometry of the channel-chunked kernels, grid (chunks, S): 64-channel chunks x S pixel ranges of P pixels (a multiple of the 32 pixel
// rows a work-group covers per iteration), about `target` work-groups in all (a policy value <= 1 means the default, 1024; others are tuning)
struct ChunkGeom { int chunks, S, P; };
static ChunkGeom chunk_geometry(size_t npix, int C, int target) {
    const int chunks = C / 64;
    int S = (target > 1 ? target : 1024) / chunks;
    if (S > 64) S = 64;
    if (S < 1) S = 1;
    int P = (int)((npix + S - 1) / S);
    P = (P + 31) & ~31;
    S = (int)((npix + P - 1) / P);
    return {chunks, S, P};
}
// whether pw_bn_train_fused* take a layer, and how (enabled: Policy::bn_fwd_chunked; bit 30: XCD-aligned pixel ranges).
// layer3 / layer4 / the first deconv (<= 8 K pixels, <= 128 slab rows): measured -0.1 ms per step; with the 32 K-pixel
// layers included the 128-byte row segments of the chunked layout cost what the saved launches gain
static bool fused_fwd_geometry(size_t npix, int C, int rows, int enabled, ChunkGeom& g, int& xcd) {
    xcd = (enabled >> 30) & 1;
    enabled &= ~(1 << 30);
    if (!enabled || C < 256 || C % 64 || npix > 8192 || npix < 1024 || rows > 128) return false;
    g = chunk_geometry(npix, C, enabled);
    return true;
}
// finalize + apply in one launch where the chunked form applies; returns 1 when it took the layer, 0 when the caller must use
// pw_bn_finalize + pw_bn_apply, < 0 on error
int pw_bn_train_fused(hipStream_t s, const elem_t* y, const elem_t* res, elem_t* z, size_t npix, int C, const float* slab, int rows,
                      const float* gamma, const float* beta, float* rm, float* rv, long long* nbt, float momentum, float eps, float* save,
                      int relu, int enabled, unsigned char* mask) {
    ChunkGeom g;
    int xcd;
    if (!fused_fwd_geometry(npix, C, rows, enabled, g, xcd)) return 0;
    hipLaunchKernelGGL((bn_apply_chunk_k<elem_t, elem_t>), dim3(g.chunks, g.S), dim3(TPB), 0, s, y, res, z, npix, C, slab, rows, (double)npix, gamma, beta, eps,
                       momentum, rm, rv, nbt, save, relu, g.P, mask, xcd);
    return udapose_check_launch() == UDAPOSE_OK ? 1 : UDAPOSE_ERR_LAUNCH;
}
// the same for the f16x2 mode: y fp32 (the split convolutions' pre-BN output), res / z split tensors.  On the teacher's forward - the
// critical path of a step in the reference precision mix - this removes one launch (bn_finalize_k) per BatchNorm of layer3 / layer4 / deconv1.
int pw_bn_train_fused_split(hipStream_t s, const float* y, const void* res, void* z, size_t npix, int C, const float* slab, int rows,
                            const float* gamma, const float* beta, float* rm, float* rv, long long* nbt, float momentum, float eps, float* save,
                            int relu, int enabled, void* y16, void* z16, unsigned char* mask) {
    ChunkGeom g;
    int xcd;
    if (!fused_fwd_geometry(npix, C, rows, enabled, g, xcd)) return 0;
    if (y16)        // ('strict' plans: y16 / z16 / mask are the fp16 tensors the 16-bit backward reads, written in the same pass)
        hipLaunchKernelGGL((bn_apply_chunk_k<float, sp32, true>), dim3(g.chunks, g.S), dim3(TPB), 0, s, y, (const sp32*)res, (sp32*)z, npix, C, slab, rows,
                           (double)npix, gamma, beta, eps, momentum, rm, rv, nbt, save, relu, g.P, mask, xcd, (_Float16*)y16, (_Float16*)z16);
    else
        hipLaunchKernelGGL((bn_apply_chunk_k<float, sp32>), dim3(g.chunks, g.S), dim3(TPB), 0, s, y, (const sp32*)res, (sp32*)z, npix, C, slab, rows, (double)npix,
                           gamma, beta, eps, momentum, rm, rv, nbt, save, relu, g.P, (unsigned char*)nullptr, xcd);
    return udapose_check_launch() == UDAPOSE_OK ? 1 : UDAPOSE_ERR_LAUNCH;
}
// the same for every BN layer of a net in one launch: jobs[blockIdx.x], channels blockIdx.y*TPB..; save = act + save_off
__global__ void bn_running_update_multi_k(const BnRunJob* __restrict__ jobs, const char* __restrict__ act, float momentum) {
    const BnRunJob j = jobs[blockIdx.x];
    const int c = blockIdx.y * TPB + threadIdx.x;
    if (c == 0 && j.nbt) *j.nbt += 1;
    if (c >= j.C) return;
    const float* save = (const float*)(act + j.save_off);
    bn_running_update1(j.rm, j.rv, c, momentum, save[c], save[2 * j.C + c]);
}
int pw_bn_running_update_multi(hipStream_t s, const BnRunJob* d_jobs, int njobs, int maxC, const void* act, float momentum) {
    hipLaunchKernelGGL(bn_running_update_multi_k, dim3(njobs, grid_for(maxC, TPB, GRID_NO_CAP)), dim3(TPB), 0, s, d_jobs, (const char*)act, momentum);
    return udapose_check_launch();
}
int pw_bn_running_update(hipStream_t s, const float* save, int C, float* rm, float* rv, long long* nbt, float momentum) {
    hipLaunchKernelGGL(bn_running_update_k, dim3(grid_for(C, TPB, GRID_NO_CAP)), dim3(TPB), 0, s, save, C, rm, rv, nbt, momentum);
    return udapose_check_launch();
}
// clears several ranges in one launch: grid (jobs, 32); replaces one hipMemsetAsync node per split weight gradient
__global__ void zero_multi_k(const ZeroJob* __restrict__ jobs, char* __restrict__ base) {
    const ZeroJob j = jobs[blockIdx.x];
    u32x4* p = (u32x4*)(base + j.off);
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (long long i = (long long)blockIdx.y * TPB + threadIdx.x; i < j.n16; i += (long long)gridDim.y * TPB) p[i] = z;
}
int pw_zero_multi(hipStream_t s, const ZeroJob* d_jobs, int njobs, void* base) {
    if (njobs <= 0) return UDAPOSE_OK;
    hipLaunchKernelGGL(zero_multi_k, dim3(njobs, 32), dim3(TPB), 0, s, d_jobs, (char*)base);
    return udapose_check_launch();
}
// one range cleared by a kernel (common.h: why not hipMemsetAsync): 16-byte stores over the aligned body, 4-byte stores over the ragged ends
__global__ void zero_k(unsigned int* __restrict__ p, size_t head, size_t n16, size_t tail) {
    const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x, step = (size_t)gridDim.x * TPB;
    if (t < head) p[t] = 0u;
    u32x4* b = (u32x4*)(p + head);
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (size_t i = t; i < n16; i += step) b[i] = z;
    if (t < tail) p[head + n16 * 4 + t] = 0u;
}
int pw_zero(hipStream_t s, void* p, size_t bytes) {
    if (!bytes) return UDAPOSE_OK;
    if (!p || (bytes & 3) || ((uintptr_t)p & 3)) return UDAPOSE_ERR_ARG;
    size_t words = bytes / 4, head = ((16 - ((uintptr_t)p & 15)) & 15) / 4;
    if (head > words) head = words;
    const size_t n16 = (words - head) / 4, tail = (words - head) & 3;
    size_t g = (n16 + TPB - 1) / TPB;
    if (g > 1024) g = 1024;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(zero_k, dim3((unsigned)g), dim3(TPB), 0, s, (unsigned int*)p, head, n16, tail);
    return udapose_check_launch();
}
// Deterministic split reductions of the grouped weight-gradient launches (net.hip build_wg_group): split z of a layer stored its partial tile at
// part + z * stride; dst = beta * dst + ((p0 + p1) + p2) + ... in split order.  One block per UDAPOSE_SPLIT_SUM_CHUNK elements of a job (blk: (job, chunk) pairs).
// (pair form: blocks [nblk, 2 nblk) run the same jobs on the second pass's workspace and gradient base - the two passes of one plan in ONE launch)
__global__ __launch_bounds__(TPB) void split_sum_k(const SumJob* __restrict__ jobs, const int* __restrict__ blk, int nblk, char* __restrict__ ws, char* __restrict__ gbase,
                                                   char* __restrict__ ws2, char* __restrict__ gbase2) {
    int bi = blockIdx.x;
    if (bi >= nblk) { bi -= nblk; ws = ws2; gbase = gbase2; }
    const SumJob j = jobs[blk[2 * bi]];
    const unsigned c0 = (unsigned)blk[2 * bi + 1] * UDAPOSE_SPLIT_SUM_CHUNK;
    const unsigned c1 = c0 + UDAPOSE_SPLIT_SUM_CHUNK < j.n ? c0 + UDAPOSE_SPLIT_SUM_CHUNK : j.n;
    const float* part = (const float*)(ws + j.part_off);
    float* dst = (float*)((j.dst_ws ? ws : gbase) + j.dst_off);
    if (((((uintptr_t)part) | ((uintptr_t)dst)) & 15) == 0 && (j.stride & 3u) == 0 && (j.n & 3u) == 0) {
        for (unsigned e = c0 + threadIdx.x * 4u; e < c1; e += TPB * 4u) {
            f32x4 a = *(const f32x4*)(part + e);
#pragma unroll 8
            for (int z = 1; z < j.ks; ++z) a += *(const f32x4*)(part + (size_t)z * j.stride + e);        // (loads hoisted in groups of eight, adds in split order)
            if (j.beta != 0.f) a = *(const f32x4*)(dst + e) + a;
            *(f32x4*)(dst + e) = a;
        }
    } else {
        for (unsigned e = c0 + threadIdx.x; e < c1; e += TPB) {
            float a = part[e];
            for (int z = 1; z < j.ks; ++z) a += part[(size_t)z * j.stride + e];
            if (j.beta != 0.f) a = dst[e] + a;
            dst[e] = a;
        }
    }
}
int pw_split_sum(hipStream_t s, const SumJob* d_jobs, const int* d_blk, int nblk, void* ws, void* grad_base, void* ws2, void* grad_base2) {
    if (nblk <= 0) return UDAPOSE_OK;
    hipLaunchKernelGGL(split_sum_k, dim3(ws2 ? 2 * nblk : nblk), dim3(TPB), 0, s, d_jobs, d_blk, nblk, (char*)ws, (char*)grad_base, (char*)ws2, (char*)grad_base2);
    return udapose_check_launch();
}
int pw_axpy(hipStream_t s, float* y, const float* x, size_t n) {
    const size_t n4 = n / 4;
    if (n4) hipLaunchKernelGGL(axpy_k, dim3(grid_for(n4, TPB, GRID_CAP)), dim3(TPB), 0, s, y, x, n4);
    if (n % 4) hipLaunchKernelGGL(axpy_tail_k, dim3(1), dim3(64), 0, s, y + n4 * 4, x + n4 * 4, (int)(n % 4));
    return udapose_check_launch();
}
int pw_bn_eval_coeff(hipStream_t s, int C, const float* gamma, const float* beta, const float* rm, const float* rv, float eps, float* scale, float* shift) {
    hipLaunchKernelGGL(bn_eval_coeff_k, dim3(grid_for(C, TPB, GRID_NO_CAP)), dim3(TPB), 0, s, C, gamma, beta, rm, rv, eps, scale, shift);
    return udapose_check_launch();
}
// grid of bn_apply_k: every thread must keep its channel group over the grid-stride loop -> (grid * TPB) % (C/8) == 0
static int bn_apply_grid(size_t n8, int C) {
    const int G = C / 8;
    int g = grid_for(n8, TPB, GRID_CAP);
    if (g > 2048) g = 2048;             // 8 work-groups per CU: threads of the large tensors loop, coefficients stay in registers
    if ((TPB % G) != 0) {               // C/8 not a divisor of the block size (e.g. C = 24): round the grid to a multiple of G
        g = (g / G) * G;
        if (g < G) g = G;
    }
    return g;
}
// XCD-aligned rows in bn_apply_k / bn_bwd_apply_pre_k: needs whole rows per block pass, a grid that is a multiple of the 8 XCDs and enough
// rows to give every XCD work (n8 = 16-byte groups of the tensor)
int pw_bn_apply_xcd_ok(size_t n8, int C) {
    const int grid = bn_apply_grid(n8, C), G = C / 8;
    return (TPB % G) == 0 && (grid % 8) == 0 && (n8 / G) >= (size_t)8 * (TPB / G);
}
int pw_bn_apply(hipStream_t s, const elem_t* y, const elem_t* res, elem_t* z, size_t n, int C, const float* scale, const float* shift, int relu,
                unsigned char* mask, int xcd) {
    if (C % 8 || n % 8) return UDAPOSE_ERR_ARG;
    const int grid = bn_apply_grid(n / 8, C);
    const int ok = xcd && pw_bn_apply_xcd_ok(n / 8, C);
    hipLaunchKernelGGL(bn_apply_k<elem_t>, dim3(grid), dim3(TPB), 0, s, y, res, z, n / 8, C, scale, shift, relu, mask, ok);
    return udapose_check_launch();
}
// f16x2 mode: y fp32 (the conv epilogue's fp32 output), residual and z split.  'strict' plans (y16 given): the same pass also writes
// y16 = fp16(y), z16 = the h half of z and the ReLU bit mask (when given), with the XCD row mapping of pw_bn_apply (xcd)
int pw_bn_apply_split(hipStream_t s, const float* y, const void* res, void* z, size_t n, int C, const float* scale, const float* shift, int relu,
                      void* y16, void* z16, unsigned char* mask, int xcd) {
    if (C % 8 || n % 8) return UDAPOSE_ERR_ARG;
    if (y16) {
        const int grid = bn_apply_grid(n / 8, C);
        const int ok = xcd && pw_bn_apply_xcd_ok(n / 8, C);
        hipLaunchKernelGGL((bn_apply_k<sp32, float, true>), dim3(grid), dim3(TPB), 0, s, y, (const sp32*)res, (sp32*)z, n / 8, C, scale, shift, relu, mask,
                           ok, (_Float16*)y16, (_Float16*)z16);
        return udapose_check_launch();
    }
    hipLaunchKernelGGL((bn_apply_k<sp32, float>), dim3(bn_apply_grid(n / 8, C)), dim3(TPB), 0, s, y, (const sp32*)res, (sp32*)z, n / 8, C, scale, shift, relu,
                       (unsigned char*)nullptr);
    return udapose_check_launch();
}
int pw_bn_apply_f32(hipStream_t s, const float* y, const float* res, float* z, size_t n, int C, const float* scale, const float* shift, int relu) {
    if (C % 8 || n % 8) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(bn_apply_k<float>, dim3(bn_apply_grid(n / 8, C)), dim3(TPB), 0, s, y, res, z, n / 8, C, scale, shift, relu, (unsigned char*)nullptr);
    return udapose_check_launch();
}
int pw_bn_bwd_rows(size_t npix) {
    // upper bound used to size the scratch slab; the launch picks rows = min(1024, ceil(npix / pixels-per-iteration))
    return (int)(npix < 1024 ? (npix < 1 ? 1 : npix) : 1024);
}
// the layers the channel-chunked backward forms take (wide, small-spatial; the pre-reduced form also needs a slab of <= 128 rows)
int pw_bn_bwd_takes_chunked(size_t npix, int C, int chunked) { return chunked && C >= 256 && npix <= 32768 && npix >= 1024; }
int pw_bn_bwd_pre_takes_chunked(size_t npix, int C, int rows, int chunked) {
    return pw_bn_bwd_takes_chunked(npix, C, chunked & ~(3 << 29)) && rows <= 128;
}
// grid of the streaming reduce (bn_bwd_reduce_k): one slab row per block, each over ppb pixels
struct ReduceGeom { int rows, ppb; };
static ReduceGeom stream_reduce_geometry(size_t npix, int G) {
    const int pstep = TPB / G;                                  // pixels a block covers per iteration
    size_t want = (npix + pstep - 1) / pstep;
    if (want > 1024) want = 1024;
    const int rows = (int)(want < 1 ? 1 : want);
    return {rows, (int)((npix + rows - 1) / rows)};
}
static void launch_bwd_finalize(hipStream_t s, const float* slab, int rows, int C, size_t npix, const float* gamma, const float* invstd, float* dgamma,
                                float* dbeta, float beta_acc, float* coef) {
    hipLaunchKernelGGL(bn_bwd_finalize_k, dim3((C + FIN_C - 1) / FIN_C), dim3(FIN_T), 0, s, slab, rows, C, (double)npix, gamma, invstd, dgamma, dbeta, beta_acc, coef);
}
// f(typed pointer): the gradient entering a BN backward is fp32 or the element type; pointee_t names the kernels' DZ inside f
template <typename F>
static void with_grad_type(const void* g, int is_f32, F&& f) {
    if (is_f32) f((const float*)g);
    else f((const elem_t*)g);
}
template <typename P> using pointee_t = std::remove_const_t<std::remove_pointer_t<P>>;
int pw_bn_bwd(hipStream_t s, const void* dz, int dz_is_f32, const elem_t* z, const elem_t* y, elem_t* dy, elem_t* gout, size_t npix, int C,
              const float* gamma, const float* mean, const float* invstd, int relu, float* slab, float* coef, float* dgamma, float* dbeta,
              float beta_acc, const float* beta, int chunked) {
    // chunked (Policy::bn_bwd_chunked): 0 restores reduce / finalize / apply everywhere
    if (relu == 2 && !beta) return UDAPOSE_ERR_ARG;
    if (relu == 1 && !z) return UDAPOSE_ERR_ARG;
    const int G = C / 8;
    if (C % 8 || G > 256 || (G & (G - 1))) return UDAPOSE_ERR_UNSUPPORTED;
    if (pw_bn_bwd_takes_chunked(npix, C, chunked)) {
        // channel-chunked form without a finalize launch (see bn_bwd_reduce_chunk_k)
        const ChunkGeom cg = chunk_geometry(npix, C, 1024);
        const dim3 grid(cg.chunks, cg.S);
        with_grad_type(dz, dz_is_f32, [&](auto d) {
            using DZ = pointee_t<decltype(d)>;
            hipLaunchKernelGGL(bn_bwd_reduce_chunk_k<DZ>, grid, dim3(TPB), 0, s, d, z, y, npix, C, mean, invstd, relu, slab, cg.P, gamma, beta);
            hipLaunchKernelGGL(bn_bwd_apply_chunk_k<DZ>, grid, dim3(TPB), 0, s, d, z, y, dy, gout, npix, C, mean, invstd, relu, gamma, beta, slab, cg.P, dgamma,
                               dbeta, beta_acc);
        });
        return udapose_check_launch();
    }
    const ReduceGeom rg = stream_reduce_geometry(npix, G);
    with_grad_type(dz, dz_is_f32, [&](auto d) {
        using DZ = pointee_t<decltype(d)>;
        hipLaunchKernelGGL(bn_bwd_reduce_k<DZ>, dim3(rg.rows), dim3(TPB), 0, s, d, z, y, npix, C, mean, invstd, relu, slab, rg.ppb, gamma, beta);
        launch_bwd_finalize(s, slab, rg.rows, C, npix, gamma, invstd, dgamma, dbeta, beta_acc, coef);
        hipLaunchKernelGGL(bn_bwd_apply_k<DZ>, dim3(grid_for(npix * G, TPB, GRID_CAP)), dim3(TPB), 0, s, d, z, y, dy, gout, npix * G, C, mean, invstd, coef, relu, gamma, beta);
    });
    return udapose_check_launch();
}
// BN backward after a dgrad that already masked dz and reduced it (DgradBnStat): slab[rows][2][C] -> dgamma / dbeta and
// dy = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)).  One launch for the wide, small-spatial layers, finalize + apply otherwise.
int pw_bn_bwd_pre(hipStream_t s, const void* g, int g_is_f32, const elem_t* y, elem_t* dy, size_t npix, int C, const float* gamma, const float* mean,
                  const float* invstd, const float* slab, int rows, float* coef, float* dgamma, float* dbeta, float beta_acc, int chunked,
                  int legacy) {
    const int G = C / 8;
    if (C % 8 || G > 256 || (G & (G - 1)) || rows < 1) return UDAPOSE_ERR_UNSUPPORTED;
    const int xcd = (chunked >> 30) & 1, xcd_stream = (chunked >> 29) & 1;     // (bit 30: XCD-aligned pixel ranges in the chunked form; bit 29: in the streaming form too)
    chunked &= ~(3 << 29);
    if (pw_bn_bwd_pre_takes_chunked(npix, C, rows, chunked)) {
        const ChunkGeom cg = chunk_geometry(npix, C, chunked);
        with_grad_type(g, g_is_f32, [&](auto d) {
            hipLaunchKernelGGL(bn_bwd_apply_pre_chunk_k<pointee_t<decltype(d)>>, dim3(cg.chunks, cg.S), dim3(TPB), 0, s, d, y, dy, npix, C, mean, invstd, gamma, slab,
                               rows, cg.P, dgamma, dbeta, beta_acc, xcd);
        });
        return udapose_check_launch();
    }
    launch_bwd_finalize(s, slab, rows, C, npix, gamma, invstd, dgamma, dbeta, beta_acc, coef);
    if (legacy) {
        with_grad_type(g, g_is_f32, [&](auto d) {
            hipLaunchKernelGGL(bn_bwd_apply_k<pointee_t<decltype(d)>>, dim3(grid_for(npix * G, TPB, GRID_CAP)), dim3(TPB), 0, s, d, (const elem_t*)nullptr, y, dy, (elem_t*)nullptr,
                               npix * G, C, mean, invstd, coef, 0, gamma, (const float*)nullptr);
        });
        return udapose_check_launch();
    }
    const int grid = bn_apply_grid(npix * G, C);
    const int ok = xcd_stream && pw_bn_apply_xcd_ok(npix * G, C);
    with_grad_type(g, g_is_f32, [&](auto d) {
        hipLaunchKernelGGL(bn_bwd_apply_pre_k<pointee_t<decltype(d)>>, dim3(grid), dim3(TPB), 0, s, d, y, dy, npix * G, C, mean, invstd, coef, ok);
    });
    return udapose_check_launch();
}
int pw_maxpool3x3s2_fwd(hipStream_t s, const elem_t* x, elem_t* y, unsigned char* idx, int N, int H, int W, int C) {
    const int Ho = pool3x3s2_out(H), Wo = pool3x3s2_out(W);
    hipLaunchKernelGGL(maxpool3x3s2_fwd_k<elem_t>, dim3(grid_for((size_t)N * Ho * Wo * (C / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, x, y, idx, N, H, W, C, Ho, Wo);
    return udapose_check_launch();
}
int pw_bn_relu_maxpool3x3s2(hipStream_t s, const elem_t* x, elem_t* y, unsigned char* idx, int N, int H, int W, int C, const float* scale,
                            const float* shift) {
    if (C % 8 || !idx) return UDAPOSE_ERR_ARG;
    const int Ho = pool3x3s2_out(H), Wo = pool3x3s2_out(W);
    hipLaunchKernelGGL(bn_relu_maxpool3x3s2_k, dim3(grid_for((size_t)N * Ho * Wo * (C / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, x, y, idx, N, H, W, C, Ho, Wo, scale, shift);
    return udapose_check_launch();
}
// BN backward (relu mask recomputed from y) whose incoming gradient is the max-pool backward of (pool_dy, pool_idx), gathered on the
// fly: reduce -> finalize -> apply; H x W = the pool's input size, npix = N*H*W
int pw_bn_bwd_pooled(hipStream_t s, const elem_t* pool_dy, const unsigned char* pool_idx, int H, int W, const elem_t* y, elem_t* dy, size_t npix, int C,
                     const float* gamma, const float* mean, const float* invstd, float* slab, float* coef, float* dgamma, float* dbeta, float beta_acc,
                     const float* beta) {
    const int G = C / 8;
    if (C % 8 || G > 256 || (G & (G - 1)) || !beta || npix % ((size_t)H * W)) return UDAPOSE_ERR_UNSUPPORTED;
    const PoolSrc ps{pool_dy, pool_idx, H, W};
    const ReduceGeom rg = stream_reduce_geometry(npix, G);
    hipLaunchKernelGGL((bn_bwd_reduce_k<elem_t, true>), dim3(rg.rows), dim3(TPB), 0, s, (const elem_t*)nullptr, (const elem_t*)nullptr, y, npix, C, mean, invstd,
                       2, slab, rg.ppb, gamma, beta, ps);
    launch_bwd_finalize(s, slab, rg.rows, C, npix, gamma, invstd, dgamma, dbeta, beta_acc, coef);
    hipLaunchKernelGGL((bn_bwd_apply_k<elem_t, true>), dim3(grid_for(npix * G, TPB, GRID_CAP)), dim3(TPB), 0, s, (const elem_t*)nullptr, (const elem_t*)nullptr, y, dy,
                       (elem_t*)nullptr, npix * G, C, mean, invstd, coef, 2, gamma, beta, ps);
    return udapose_check_launch();
}
int pw_maxpool3x3s2_fwd_f32(hipStream_t s, const float* x, float* y, unsigned char* idx, int N, int H, int W, int C) {
    const int Ho = pool3x3s2_out(H), Wo = pool3x3s2_out(W);
    hipLaunchKernelGGL(maxpool3x3s2_fwd_k<float>, dim3(grid_for((size_t)N * Ho * Wo * (C / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, x, y, idx, N, H, W, C, Ho, Wo);
    return udapose_check_launch();
}
int pw_maxpool3x3s2_fwd_split(hipStream_t s, const void* x, void* y, unsigned char* idx, int N, int H, int W, int C, void* y16) {
    const int Ho = pool3x3s2_out(H), Wo = pool3x3s2_out(W);
    if (y16) {      // ('strict' plans: the pooled fp16 map as well)
        hipLaunchKernelGGL((maxpool3x3s2_fwd_k<sp32, true>), dim3(grid_for((size_t)N * Ho * Wo * (C / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, (const sp32*)x, (sp32*)y, idx, N, H, W,
                           C, Ho, Wo, (_Float16*)y16);
        return udapose_check_launch();
    }
    hipLaunchKernelGGL(maxpool3x3s2_fwd_k<sp32>, dim3(grid_for((size_t)N * Ho * Wo * (C / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, (const sp32*)x, (sp32*)y, idx, N, H, W, C, Ho, Wo);
    return udapose_check_launch();
}
int pw_maxpool2x2_ceil_split(hipStream_t s, const void* x, void* y, int N, int H, int W, int C) {
    if (C % 8) return UDAPOSE_ERR_ARG;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    hipLaunchKernelGGL(maxpool2x2_ceil_k<sp32>, dim3(grid_for((size_t)N * Ho * Wo * (C / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, (const sp32*)x, (sp32*)y, N, H, W, C, Ho, Wo);
    return udapose_check_launch();
}
int pw_maxpool3x3s2_bwd(hipStream_t s, const elem_t* dy, const unsigned char* idx, elem_t* dx, int N, int H, int W, int C) {
    hipLaunchKernelGGL(maxpool3x3s2_bwd_k, dim3(grid_for((size_t)N * H * W * (C / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, dy, idx, dx, N, H, W, C);
    return udapose_check_launch();
}
int pw_maxpool2x2_ceil(hipStream_t s, const elem_t* x, elem_t* y, int N, int H, int W, int C) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    hipLaunchKernelGGL(maxpool2x2_ceil_k<elem_t>, dim3(grid_for((size_t)N * Ho * Wo * (C / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, x, y, N, H, W, C, Ho, Wo);
    return udapose_check_launch();
}
int pw_maxpool2x2_ceil_f32(hipStream_t s, const float* x, float* y, int N, int H, int W, int C) {
    if (C % 8) return UDAPOSE_ERR_ARG;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    hipLaunchKernelGGL(maxpool2x2_ceil_k<float>, dim3(grid_for((size_t)N * Ho * Wo * (C / 8), TPB, GRID_CAP)), dim3(TPB), 0, s, x, y, N, H, W, C, Ho, Wo);
    return udapose_check_launch();
}
int pw_plane_sum(hipStream_t s, const float* x, float* out, int N, int C, int HW, float beta) {
    hipLaunchKernelGGL(plane_sum_k, dim3(C), dim3(1024), 0, s, x, out, N, C, HW, beta);
    return udapose_check_launch();
}

UDAPOSE_SP_SAT_READER(sp_sat_read_pointwise)
