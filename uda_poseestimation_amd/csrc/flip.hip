// Flip-test evaluation kernels (fp32 only: both builds of the library export identical code).
//   hflip_k / hflip_scalar_k : mirror every row of an image batch, optionally behind a copy of the batch (one launch, no torch.cat)
//   flip_merge_k             : flip the heat-maps of the mirrored batch back (columns reversed, left / right channels swapped, optional
//                              one-pixel shift), average them with the plain batch's and decode the result in the same pass
// Pure HBM sweeps: every operand is read once, every output written once.  No atomics, no scratch: capturable.
#include "losses.h"

namespace {
constexpr int TPB = 256;

// dst[mirror half][row][x] = src[row][W-1-x]; with keep, dst[row] = src[row] as well.  One thread per 16-byte group of a row: the
// group at columns 4j..4j+3 lands reversed at columns W-4-4j..W-1-4j, so both the read and the write of a wave are contiguous.
__global__ void hflip_k(const float* __restrict__ src, float* __restrict__ dst, size_t rows, int W4, size_t mirror_off, int keep) {
    const size_t total = rows * (size_t)W4;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        const size_t r = i / (size_t)W4;
        const int j = (int)(i - r * (size_t)W4);
        const f32x4 v = *(const f32x4*)(src + i * 4);
        if (keep) *(f32x4*)(dst + i * 4) = v;
        *(f32x4*)(dst + mirror_off + (r * (size_t)W4 + (size_t)(W4 - 1 - j)) * 4) = (f32x4){v[3], v[2], v[1], v[0]};
    }
}
// the same element by element: W % 4 != 0 (rows are then not 16-byte aligned) or unaligned base pointers
__global__ void hflip_scalar_k(const float* __restrict__ src, float* __restrict__ dst, size_t rows, int W, size_t mirror_off, int keep) {
    const size_t total = rows * (size_t)W;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        const size_t r = i / (size_t)W;
        const int x = (int)(i - r * (size_t)W);
        const float v = src[i];
        if (keep) dst[i] = v;
        dst[mirror_off + r * (size_t)W + (size_t)(W - 1 - x)] = v;
    }
}

// One work-group per (n, k) plane.  s[y][x] = f[n][perm[k]][y][c(x)], c(x) = W-1-x, or with the one-pixel shift W-x for x >= 1 and
// W-1 for x = 0 (column 0 keeps the flipped-back value); out = s (mode 0) or (a + s) * 0.5f (mode 1).  The arg-max of the values just
// written is reduced exactly as argmax_rectify_k does: hm_better is a total order, so the winner does not depend on the reduction tree.
// (a and out carry no __restrict__: out may be a)
__global__ void flip_merge_k(const float* a, const float* __restrict__ f, const int* __restrict__ perm, int K, int H, int W,
                             int shift, int mode, float* out, float* __restrict__ maxv, int* __restrict__ idx_out,
                             float* __restrict__ preds) {
    __shared__ float sv[TPB / 64];
    __shared__ int si[TPB / 64];
    const size_t r = blockIdx.x;
    const int k = (int)(r % (size_t)K);
    int pk = perm ? perm[k] : k;
    if (pk < 0 || pk >= K) pk = k;                // a bad table entry never moves the read outside f
    const int HW = H * W;
    const float* pf = f + (r - (size_t)k + (size_t)pk) * HW;
    const float* pa = a + r * HW;                 // (only dereferenced in mode 1)
    float* po = out + r * HW;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < HW; i += TPB) {
        const int y = i / W, x = i - y * W;
        const int c = shift ? (x ? W - x : W - 1) : W - 1 - x;
        float v = pf[y * W + c];
        if (mode) v = (pa[i] + v) * 0.5f;
        po[i] = v;
        if (hm_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    if (!maxv && !idx_out && !preds) return;      // (uniform over the grid)
    hm_block_best<TPB / 64>(bv, bi, sv, si);
    if (threadIdx.x == 0) {
        const bool pos = bv > 0.f;
        if (maxv) maxv[r] = bv;
        if (idx_out) idx_out[r] = bi;
        if (preds) { preds[r * 2] = pos ? (float)(bi % W) : 0.f; preds[r * 2 + 1] = pos ? (float)(bi / W) : 0.f; }
    }
}

inline bool ranges_overlap(const void* p, size_t pn, const void* q, size_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qn && b < a + pn;
}
}  // namespace

int flip_hbatch(hipStream_t s, const float* src, float* dst, int N, size_t rows_per_image, int W, int keep_original) {
    if (!src || !dst || N < 0 || W < 0 || (keep_original != 0 && keep_original != 1)) return UDAPOSE_ERR_ARG;
    if (N == 0 || rows_per_image == 0 || W == 0) return UDAPOSE_OK;
    if (rows_per_image > SIZE_MAX / 16 / (size_t)N / (size_t)W) return UDAPOSE_ERR_ARG;
    const size_t rows = (size_t)N * rows_per_image;
    const size_t n = rows * (size_t)W, bytes = n * sizeof(float);
    if (ranges_overlap(src, bytes, dst, keep_original ? 2 * bytes : bytes)) return UDAPOSE_ERR_ARG;
    const size_t mirror_off = keep_original ? n : 0;
    const bool vec = (W % 4) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0;
    const size_t work = vec ? n / 4 : n;
    size_t blocks = (work + TPB - 1) / TPB;
    if (blocks > 8192) blocks = 8192;
    if (vec)
        hipLaunchKernelGGL(hflip_k, dim3((unsigned)blocks), dim3(TPB), 0, s, src, dst, rows, W / 4, mirror_off, keep_original);
    else
        hipLaunchKernelGGL(hflip_scalar_k, dim3((unsigned)blocks), dim3(TPB), 0, s, src, dst, rows, W, mirror_off, keep_original);
    return udapose_check_launch();
}

int flip_merge(hipStream_t s, const float* a, const float* f, const int* perm, int N, int K, int H, int W, int shift, int mode, float* out,
               float* maxv, int* idx, float* preds) {
    if (!f || !out || N < 0 || K < 1 || H < 1 || W < 1 || (shift != 0 && shift != 1) || (mode != 0 && mode != 1)) return UDAPOSE_ERR_ARG;
    if (mode == 1 && !a) return UDAPOSE_ERR_ARG;
    if ((long long)H * W > 0x7fffffffLL || (long long)N * K > 0x7fffffffLL) return UDAPOSE_ERR_ARG;
    if (N == 0) return UDAPOSE_OK;
    const size_t bytes = (size_t)N * K * H * W * sizeof(float);
    if (ranges_overlap(out, bytes, f, bytes)) return UDAPOSE_ERR_ARG;       // a plane of f is read by two work-groups (k and perm[k])
    if (mode == 1 && out != a && ranges_overlap(out, bytes, a, bytes)) return UDAPOSE_ERR_ARG;      // (out == a: same thread, same element)
    hipLaunchKernelGGL(flip_merge_k, dim3((unsigned)(N * K)), dim3(TPB), 0, s, mode ? a : f, f, perm, K, H, W, shift, mode, out, maxv, idx, preds);
    return udapose_check_launch();
}
