// The strong student view (FixMatch / RandAugment colour ops and RandomErasing) for a whole batch, byte for byte PIL's results on uint8 NHWC
// images like augment.hip.  One op code per image and launch; codes continue udapose_aug_color_op's (0 none, 1-3 ImageEnhance):
//   4 autocontrast  ImageOps.autocontrast(img), cutoff 0      } per-channel table built from the image's own histogram
//   5 equalize      ImageOps.equalize(img)                    }
//   6 posterize     ImageOps.posterize(img, bits)               table i & ~(2^(8-bits) - 1)
//   7 solarize      ImageOps.solarize(img, threshold)           table i < cut ? i : 255 - i, cut = ceil(threshold) from the host
//   8 sharpness     ImageEnhance.Sharpness(img).enhance(f)      blend(SMOOTH(img), img, f), SMOOTH = the 3x3 kernel (1,1,1,1,5,1,1,1,1) / 13
// An image whose code belongs to another kernel is left alone.  RandomErasing (lib/transforms/__init__.py:134-179) fills a box of the
// normalised fp32 NCHW tensor.
#include "data.h"
#include "lds_hist.h"   // hist_add
#include "blend.h"      // blend1; and NO FMA contraction in this file: the stencil and the blend round every product and every sum separately

namespace {
constexpr int TPB = 256;
constexpr int TAB_TPB = 1024;      // point_table_k: one work-group per image
constexpr int LUT = 768;           // 3 channels x 256 entries, bytes

__device__ __forceinline__ bool is_point_op(int o) { return o >= 4 && o <= 7; }

// lut[n][c][i] of every image whose op is 4..7.  Ops 4 and 5 first count the image's three 256-bin histograms in LDS (integer atomics:
// exact, whatever the order); the table is then one entry per thread.
//   autocontrast: lo / hi = first / last filled bin (LDS atomicMin / atomicMax over the filled bins); hi <= lo -> identity; else
//     int(i * scale + offset) in fp64, scale = inv_scale[hi - lo - 1] = 255.0 / (hi - lo) as the host's Python divided it,
//     offset = -lo * scale; product and sum are rounded separately, truncation toward zero, clip.  (Contraction is off in this
//     file and the product is pinned besides: HIP's __dmul_rn / __dadd_rn are plain operators in a header compiled with contraction on,
//     and their pair came out of the compiler as one v_fma_f64.)
//   equalize: integers.  The filled bins are <= 1 exactly when hi <= lo; the counts sum to HW (no mask), so step = (HW - h[hi]) / 255;
//     step == 0 -> identity; else (step / 2 + sum_{j<i} h[j]) / step, clipped to 255 (the entry can be 256; Image.point clips it).
//     uint32 holds step / 2 + HW for every HW the launcher admits.  The running sum is a serial loop per entry over LDS (256 x 256 / 2
//     reads per channel): small beside the 3 HW atomics of the histogram.
__global__ void __launch_bounds__(TAB_TPB) point_table_k(const unsigned char* __restrict__ img, const int* __restrict__ op,
                                                         const int* __restrict__ param, const double* __restrict__ inv_scale,
                                                         unsigned char* __restrict__ lut, int HW) {
    __shared__ unsigned int hist[LUT];
    __shared__ int lo[3], hi[3];
    const int n = blockIdx.x, o = op[n];
    if (!is_point_op(o)) return;                       // (uniform over the block: every barrier below is reached by all or by none)
    const int t = threadIdx.x, c = t >> 8, i = t & 255;
    unsigned char* out = lut + (size_t)n * LUT;
    if (o >= 6) {
        if (t < LUT) {
            const int p = param[n];
            out[t] = (unsigned char)(o == 6 ? (i & ~((1 << (8 - p)) - 1)) : (i < p ? i : 255 - i));
        }
        return;
    }
    if (t < LUT) hist[t] = 0u;
    if (t < 3) { lo[t] = 256; hi[t] = -1; }
    __syncthreads();
    const unsigned char* p = img + (size_t)n * HW * 3;
    // groups of 4 pixels = three dwords where the image starts on a dword; what is left, or all of an image that does not, by bytes
    const int G = ((uintptr_t)p & 3) == 0 ? HW >> 2 : 0;
    const unsigned int* pw = (const unsigned int*)p;
    unsigned int* hr = hist;
    unsigned int* hg = hist + 256;
    unsigned int* hb = hist + 512;
    for (int g = t; g < G; g += TAB_TPB) {
        const unsigned int w0 = pw[3 * g], w1 = pw[3 * g + 1], w2 = pw[3 * g + 2];      // r g b r | g b r g | b r g b
        hist_add(hr, w0 & 255u); hist_add(hg, (w0 >> 8) & 255u); hist_add(hb, (w0 >> 16) & 255u); hist_add(hr, w0 >> 24);
        hist_add(hg, w1 & 255u); hist_add(hb, (w1 >> 8) & 255u); hist_add(hr, (w1 >> 16) & 255u); hist_add(hg, w1 >> 24);
        hist_add(hb, w2 & 255u); hist_add(hr, (w2 >> 8) & 255u); hist_add(hg, (w2 >> 16) & 255u); hist_add(hb, w2 >> 24);
    }
    for (int k = G * 4 + t; k < HW; k += TAB_TPB) {
        hist_add(hr, p[(size_t)k * 3]); hist_add(hg, p[(size_t)k * 3 + 1]); hist_add(hb, p[(size_t)k * 3 + 2]);
    }
    __syncthreads();
    if (t < LUT && hist[t] != 0u) { atomicMin(&lo[c], i); atomicMax(&hi[c], i); }
    __syncthreads();
    if (t >= LUT) return;
    const int l = lo[c], h = hi[c];
    int v = i;
    if (h > l) {
        if (o == 4) {
            const double scale = inv_scale[h - l - 1];
            const double offset = -(double)l * scale;
            double prod = (double)i * scale;
            asm volatile("" : "+v"(prod));             // (the pin of blend1: the product is rounded before the sum sees it)
            const double x = prod + offset;            // |x| <= 65025: the conversion below is exact truncation
            const int ix = (int)x;
            v = ix < 0 ? 0 : (ix > 255 ? 255 : ix);
        } else {
            const unsigned int step = ((unsigned int)HW - hist[c * 256 + h]) / 255u;
            if (step != 0u) {
                unsigned int acc = step >> 1;
                for (int j = 0; j < i; ++j) acc += hist[c * 256 + j];
                const unsigned int q = acc / step;
                v = q > 255u ? 255 : (int)q;
            }
        }
    }
    out[t] = (unsigned char)v;
}

// img[n][i][c] = lut[n][c][img[n][i][c]] in place, for the images whose op is 4..7; grid (chunks, N)
__global__ void point_apply_k(unsigned char* __restrict__ img, const int* __restrict__ op, const unsigned char* __restrict__ lut, int HW) {
    __shared__ unsigned char tab[LUT];
    const int n = blockIdx.y;
    if (!is_point_op(op[n])) return;
    for (int k = threadIdx.x; k < LUT; k += TPB) tab[k] = lut[(size_t)n * LUT + k];
    __syncthreads();
    unsigned char* p = img + (size_t)n * HW * 3;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < HW; i += gridDim.x * TPB) {
        unsigned char* q = p + (size_t)i * 3;
        const unsigned char r = tab[q[0]], g = tab[256 + q[1]], b = tab[512 + q[2]];
        q[0] = r; q[1] = g; q[2] = b;
    }
}

// dst[n] = src[n] for the images whose op is 8 (the stencil reads neighbours: it works from a copy)
__global__ void sharp_copy_k(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, const int* __restrict__ op, int HW) {
    const int n = blockIdx.y;
    if (op[n] != 8) return;
    const unsigned char* s = src + (size_t)n * HW * 3;
    unsigned char* d = dst + (size_t)n * HW * 3;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < HW; i += gridDim.x * TPB) {
        d[(size_t)i * 3] = s[(size_t)i * 3]; d[(size_t)i * 3 + 1] = s[(size_t)i * 3 + 1]; d[(size_t)i * 3 + 2] = s[(size_t)i * 3 + 2];
    }
}

// libImaging's clip8 on the filter's float sum
__device__ __forceinline__ float smooth_clip8(float v) { return v <= 0.f ? 0.f : (v >= 255.f ? 255.f : (float)(unsigned char)v); }

// One channel of libImaging's ImagingFilter3x3 with SMOOTH's kernel at an interior pixel: float32 coefficients float32(1 / 13) and
// float32(5 / 13), the sum starts at 0.5f, a row's three products are added left to right and the row's sum is then added, top row first
// (the other row order gave the same bytes on 10^7 bytes of random, dark, low-contrast and saturated images: DESIGN.md 4.20).
// p = the pixel's byte of this channel, rs = bytes per image row.
__device__ __forceinline__ float smooth1(const unsigned char* p, size_t rs) {
    const float k1 = (float)(1.0 / 13.0), k5 = (float)(5.0 / 13.0);
    const unsigned char* a = p - rs;
    const unsigned char* b = p + rs;
    float ss = 0.5f;
    ss += ((float)a[-3] * k1 + (float)a[0] * k1) + (float)a[3] * k1;
    ss += ((float)p[-3] * k1 + (float)p[0] * k5) + (float)p[3] * k1;
    ss += ((float)b[-3] * k1 + (float)b[0] * k1) + (float)b[3] * k1;
    return smooth_clip8(ss);
}

// img[n] = blend(SMOOTH(src[n]), src[n], factor[n]) at the interior pixels of the images whose op is 8 (src = the copy of img); the
// one-pixel border keeps its bytes: SMOOTH copies it and blend(v, v, f) = v.  H, W >= 3.
__global__ void sharpness_k(const unsigned char* __restrict__ src, unsigned char* __restrict__ img, const int* __restrict__ op,
                            const float* __restrict__ factor, int H, int W) {
    const int n = blockIdx.y;
    if (op[n] != 8) return;
    const float f = factor[n];
    const size_t rs = (size_t)W * 3;
    const unsigned char* s = src + (size_t)n * H * rs;
    unsigned char* d = img + (size_t)n * H * rs;
    const int Wi = W - 2, cnt = (H - 2) * Wi;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < cnt; i += gridDim.x * TPB) {
        const int y = i / Wi + 1, x = i - (y - 1) * Wi + 1;
        const size_t o = (size_t)y * rs + (size_t)x * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[o + c] = blend1(smooth1(s + o + c, rs), (float)s[o + c], f);
    }
}

// x[n][c][top + r][left + q] = v_c for r < h, q < w, box[n] = (top, left, h, w); an empty box or one that leaves the image: untouched
__global__ void erase_f32_k(float* __restrict__ x, const int* __restrict__ box, float v0, float v1, float v2, int H, int W) {
    const int n = blockIdx.y;
    const int top = box[n * 4], left = box[n * 4 + 1], h = box[n * 4 + 2], w = box[n * 4 + 3];
    if (h <= 0 || w <= 0 || top < 0 || left < 0 || h > H - top || w > W - left) return;
    float* xn = x + (size_t)n * 3 * H * W;
    const int area = h * w;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < area; i += gridDim.x * TPB) {
        const int r = i / w, q = i - r * w;
        const size_t o = (size_t)(top + r) * W + left + q;
        xn[o] = v0;
        xn[(size_t)H * W + o] = v1;
        xn[(size_t)2 * H * W + o] = v2;
    }
}

int sweep_chunks(long long elems) {
    const long long gx = (elems + TPB - 1) / TPB;
    return (int)(gx > 256 ? 256 : (gx < 1 ? 1 : gx));
}
}  // namespace

// ops 4..7 of img [N][HW][3] uint8 in place: the table build (one work-group per image), then the look-up sweep.  Two launches were kept:
// a fused kernel would either run one work-group per image for the sweep too, or have every chunk of an image count the whole histogram.
int aug_point_op(hipStream_t s, unsigned char* img, const int* op, const int* param, const double* inv_scale, unsigned char* lut, int N, int HW) {
    if (N <= 0 || HW <= 0) return UDAPOSE_ERR_ARG;
    if (HW > UDAPOSE_AUG_MAX_HW) return UDAPOSE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(point_table_k, dim3(N), dim3(TAB_TPB), 0, s, (const unsigned char*)img, op, param, inv_scale, lut, HW);
    hipLaunchKernelGGL(point_apply_k, dim3(sweep_chunks(HW), N), dim3(TPB), 0, s, img, op, (const unsigned char*)lut, HW);
    return udapose_check_launch();
}

// op 8 of img [N][H][W][3] uint8 through tmp (same size): copy, then stencil + blend back into img
int aug_sharpness_u8(hipStream_t s, unsigned char* img, unsigned char* tmp, const int* op, const float* factor, int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return UDAPOSE_ERR_ARG;
    if ((long long)H * W > UDAPOSE_AUG_MAX_HW) return UDAPOSE_ERR_UNSUPPORTED;
    if (H < 3 || W < 3) return UDAPOSE_OK;             // (PIL's filter returns a copy, and blending an image with itself returns it)
    hipLaunchKernelGGL(sharp_copy_k, dim3(sweep_chunks((long long)H * W), N), dim3(TPB), 0, s, (const unsigned char*)img, tmp, op, H * W);
    hipLaunchKernelGGL(sharpness_k, dim3(sweep_chunks((long long)(H - 2) * (W - 2)), N), dim3(TPB), 0, s, (const unsigned char*)tmp, img, op,
                       factor, H, W);
    return udapose_check_launch();
}

int aug_erase_f32(hipStream_t s, float* x, const int* box, float v0, float v1, float v2, int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return UDAPOSE_ERR_ARG;
    if ((long long)H * W > UDAPOSE_AUG_MAX_HW) return UDAPOSE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(erase_f32_k, dim3(sweep_chunks((long long)H * W), N), dim3(TPB), 0, s, x, box, v0, v1, v2, H, W);
    return udapose_check_launch();
}
