// Row machinery shared by the per-(b,k)-row heat-map kernels of softmax_loss.hip and softargmax.hip: one 256-thread block per row of HW
// fp32 values, a row of up to 4096 floats read ONCE and kept in registers across passes (longer or ragged rows are re-read, L2-resident),
// operands read as f32x4 where HW % 4 == 0 and the rows are 16-byte aligned (element by element otherwise), block sums in double, no
// atomics, and the tiny second launch that reduces over rows.  Everything lives in the including file's unnamed namespace.
#pragma once
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int REG_V = 4;     // f32x4 per thread kept in registers: rows of up to REG_V * TPB * 4 = 4096 floats

// sums of two values over the block (red: 2 * TPB / 64 doubles)
__device__ __forceinline__ void block_sum2_d(double& a, double& b, double* red) {
    a = wave_sum(a);
    b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a; red[TPB / 64 + (threadIdx.x >> 6)] = b; }
    __syncthreads();
    double ta = 0.0, tb = 0.0;
    for (int i = 0; i < TPB / 64; ++i) { ta += red[i]; tb += red[TPB / 64 + i]; }
    __syncthreads();
    a = ta; b = tb;
}
// maxima of two values over the block; fmaxf drops NaN here, the NaN comes back through exp(s - max)
__device__ __forceinline__ void block_max2_f(float& a, float& b, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a = fmaxf(a, __shfl_xor(a, o, 64)); b = fmaxf(b, __shfl_xor(b, o, 64)); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a; red[TPB / 64 + (threadIdx.x >> 6)] = b; }
    __syncthreads();
    float ta = red[0], tb = red[TPB / 64];
    for (int i = 1; i < TPB / 64; ++i) { ta = fmaxf(ta, red[i]); tb = fmaxf(tb, red[TPB / 64 + i]); }
    __syncthreads();
    a = ta; b = tb;
}

// One row of HW floats as this thread sees it: its share in registers when the row is short and 16-byte aligned, memory otherwise.
// vec: the row may be read as f32x4 (HW % 4 == 0 keeps every row of a 16-byte aligned tensor aligned; a caller that cannot vouch for the
// base pointer passes its own test).
struct Row {
    const float* p;
    int HW;
    bool vec, inreg;
    f32x4 v[REG_V];
    __device__ __forceinline__ Row(const float* p_, int HW_) : Row(p_, HW_, (HW_ & 3) == 0) {}
    __device__ __forceinline__ Row(const float* p_, int HW_, bool vec_) : p(p_), HW(HW_), vec(vec_), inreg(vec_ && HW_ <= REG_V * TPB * 4) {
        if (inreg) {
#pragma unroll
            for (int j = 0; j < REG_V; ++j) {
                const int i = (j * TPB + (int)threadIdx.x) * 4;
                v[j] = i < HW ? *(const f32x4*)(p + i) : (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
    }
};
// f(i, a_i, b_i) over this thread's elements of two rows of the same length (b may be the same row as a)
template <class F>
__device__ __forceinline__ void each2(const Row& a, const Row& b, F&& f) {
    const int HW = a.HW;
    if (a.inreg) {
#pragma unroll
        for (int j = 0; j < REG_V; ++j) {
            const int i = (j * TPB + (int)threadIdx.x) * 4;
            if (i < HW) {
#pragma unroll
                for (int e = 0; e < 4; ++e) f(i + e, a.v[j][e], b.v[j][e]);
            }
        }
    } else if (a.vec) {
        for (int i = threadIdx.x * 4; i < HW; i += TPB * 4) {
            const f32x4 x = *(const f32x4*)(a.p + i), y = *(const f32x4*)(b.p + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) f(i + e, x[e], y[e]);
        }
    } else {
        for (int i = threadIdx.x; i < HW; i += TPB) f(i, a.p[i], b.p[i]);
    }
}

// Reduction over rows, one block per group of n rows: out[g] = sum of the selected rows / denominator.  thr > 0 selects rows[i] < thr
// (EntLoss's threshold) and divides by their number; count (a device scalar: the valid_mask's selected positions) divides by Kc * count;
// otherwise by denom.  cnt_out[0] = number of selected rows (0 / 0 = NaN for an empty selection, as tensor([]).mean()).
__global__ __launch_bounds__(TPB) void reduce_rows_k(const float* __restrict__ rows, int n, float thr, double denom, const float* __restrict__ count,
                                                     int Kc, float* __restrict__ out, float* __restrict__ cnt_out) {
    __shared__ double red[2 * TPB / 64];
    const float* p = rows + (size_t)blockIdx.x * n;
    double s = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < n; i += TPB) {
        const float v = p[i];
        if (!(thr > 0.f) || v < thr) { s += (double)v; c += 1.0; }
    }
    block_sum2_d(s, c, red);
    if (threadIdx.x == 0) {
        const double d = count ? (double)Kc * (double)count[0] : (thr > 0.f ? c : denom);
        out[blockIdx.x] = (float)(s / d);
        if (cnt_out) cnt_out[0] = (float)c;
    }
}

// d[i] = f(i, a[i], b[i]) over one row (b may be null: f gets a[i] twice); vec: as in Row, for all three pointers
template <class F>
__device__ __forceinline__ void row_map(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ d, int HW, bool vec, F&& f) {
    if (vec) {
        for (int i = threadIdx.x * 4; i < HW; i += TPB * 4) {
            const f32x4 x = *(const f32x4*)(a + i), y = b ? *(const f32x4*)(b + i) : x;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = f(i + e, x[e], y[e]);
            *(f32x4*)(d + i) = o;
        }
    } else {
        for (int i = threadIdx.x; i < HW; i += TPB) d[i] = f(i, a[i], b ? b[i] : a[i]);
    }
}
template <class F>
__device__ __forceinline__ void row_map(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ d, int HW, F&& f) {
    row_map(a, b, d, HW, (HW & 3) == 0, f);
}
}  // namespace
