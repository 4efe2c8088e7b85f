// Top-down inference geometry (fp32 only: both builds of the library export identical code).
//   box_crop_k        : rotated / padded / non-square box crops of uint8 NHWC frames, resized to Ho x Wo: the device counterpart of the
//                       reference's crop + Resize (lib/datasets/util.py:87-123) and crop_ori (util.py:235-287), as NCHW fp32 normalised
//                       and / or NHWC uint8, optionally followed by the column-reversed crops (the flip test's 2M batch) from the same reads
//   coords_to_image_k : heat-map pixels of a crop -> pixels of its frame
// Geometry.  Pixel i of a frame covers [i, i + 1), its centre is i + 0.5.  box = (cx, cy, bw, bh, rot_deg); sx = bw / Wo, sy = bh / Ho,
// (c, s) = (cos, sin)(rot): exact from a table for multiples of 90 degrees, else the fp64 value rounded to fp32.  Output pixel (u, v) is the
// mean of tx * ty bilinear samples, tx = clamp(ceil(bw / Wo), 1, 8), ty likewise: sample (i, j) sits at
//   dx = ((u + (i + 0.5) / tx) - Wo / 2) * sx,  dy = ((v + (j + 0.5) / ty) - Ho / 2) * sy,  X = cx + c dx - s dy,  Y = cy + s dx + c dy
// and reads x0 = floor(X - 0.5) with weight X - 0.5 - x0 on x0 + 1 (the same in y); a tap outside the frame contributes 0 (zero padding in
// pixel values, ahead of the normalisation).  The samples are added j-major in a fixed order: no atomics, bit-reproducible.  A box more than
// 8 times the output size is under-sampled (the tap cap).
// One work-group = one 32 x 8 output tile of one box.  The tile's source footprint (its four corners mapped, one pixel of margin, clipped to
// the frame plus its zero border) is staged in LDS as one dword per pixel when it has at most LDS_PIXELS pixels: the packed RGB rows are
// read with aligned dword loads, a pixel read once per tile whatever the tap count.  Larger footprints, and frames whose base address is not
// dword-aligned, gather their taps from global memory.  Everything a box needs is read from device memory: a captured launch follows new boxes.
#include "data.h"

// no FMA contraction: the staged and the gathering form of a tile must give the same bits (the compiler contracts the two instantiations of
// the sample loop differently: 27 ulp apart on a value near 0 when it may), and a crop must not depend on which form its tiles took
#pragma clang fp contract(off)

namespace {
constexpr int TPB = 256, TW = 32, TH = 8;
constexpr int LDS_PIXELS = 8192;      // 32 KiB: four work-groups per CU beside the 160 KiB

struct BoxGeom {
    float cx, cy, sx, sy, c, s;
    int tx, ty;
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }

// (cos, sin) of rot degrees
__device__ __forceinline__ void box_trig(float rot, float& c, float& s) {
    float r = fmodf(rot, 360.f);
    if (r < 0.f) r += 360.f;
    if (r == 0.f || r == 360.f) { c = 1.f; s = 0.f; }
    else if (r == 90.f) { c = 0.f; s = 1.f; }
    else if (r == 180.f) { c = -1.f; s = 0.f; }
    else if (r == 270.f) { c = 0.f; s = -1.f; }
    else {
        const double a = (double)rot * (3.14159265358979323846 / 180.0);
        c = (float)cos(a);
        s = (float)sin(a);
    }
}
__device__ __forceinline__ int box_taps(float scale) {
    const float t = ceilf(scale);
    return t < 1.f ? 1 : (t > 8.f ? 8 : (int)t);
}
// false: the box is refused (a non-finite field, a side that is not positive)
__device__ __forceinline__ bool box_geom(const float* __restrict__ b, int Ho, int Wo, BoxGeom& g) {
    const float cx = b[0], cy = b[1], bw = b[2], bh = b[3], rot = b[4];
    if (!(finite_f(cx) && finite_f(cy) && finite_f(bw) && finite_f(bh) && finite_f(rot)) || !(bw > 0.f) || !(bh > 0.f)) return false;
    g.cx = cx; g.cy = cy;
    g.sx = bw / (float)Wo;
    g.sy = bh / (float)Ho;
    g.tx = box_taps(g.sx);
    g.ty = box_taps(g.sy);
    box_trig(rot, g.c, g.s);
    return true;
}

// what thread 0 works out once per tile
struct TileSetup {
    BoxGeom g;
    int ok;            // the box is accepted
    int staged;        // the footprint is in LDS
    int x_lo, y_lo, w, h;
};

// the taps of one sample from the LDS image (one dword per pixel, byte 0 = R; the zero border is part of it)
struct LdsTaps {
    const unsigned int* img;
    int x_lo, y_lo, w, h;
    __device__ __forceinline__ unsigned int at(int x, int y) const {
        const int ix = min(max(x - x_lo, 0), w - 1), iy = min(max(y - y_lo, 0), h - 1);      // (never outside the image: the margin covers rounding)
        return img[iy * w + ix];
    }
};
// the same from global memory
struct GlobalTaps {
    const unsigned char* frame;
    int Hs, Ws;
    __device__ __forceinline__ unsigned int at(int x, int y) const {
        if (x < 0 || x >= Ws || y < 0 || y >= Hs) return 0u;
        const unsigned char* p = frame + ((size_t)y * Ws + x) * 3;
        return (unsigned int)p[0] | ((unsigned int)p[1] << 8) | ((unsigned int)p[2] << 16);
    }
};

template <typename Taps>
__device__ __forceinline__ void box_pixel(const Taps& t, const BoxGeom& g, int u, int v, int Ho, int Wo, int Hs, int Ws, float (&acc)[3]) {
    acc[0] = acc[1] = acc[2] = 0.f;
    const float hw = (float)Wo / 2.f, hh = (float)Ho / 2.f;
    const float xmax = (float)Ws + 0.5f, ymax = (float)Hs + 0.5f;
    for (int j = 0; j < g.ty; ++j) {
        const float dy = (((float)v + ((float)j + 0.5f) / (float)g.ty) - hh) * g.sy;
        for (int i = 0; i < g.tx; ++i) {
            const float dx = (((float)u + ((float)i + 0.5f) / (float)g.tx) - hw) * g.sx;
            const float X = g.cx + g.c * dx - g.s * dy, Y = g.cy + g.s * dx + g.c * dy;
            // all four taps outside the frame (or a position that overflowed): the sample is 0
            if (!(X >= -0.5f && X < xmax && Y >= -0.5f && Y < ymax)) continue;
            const float fx0 = floorf(X - 0.5f), fy0 = floorf(Y - 0.5f);
            const float wx = X - 0.5f - fx0, wy = Y - 0.5f - fy0;
            const int x0 = (int)fx0, y0 = (int)fy0;
            const unsigned int p00 = t.at(x0, y0), p01 = t.at(x0 + 1, y0), p10 = t.at(x0, y0 + 1), p11 = t.at(x0 + 1, y0 + 1);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float a = (float)((p00 >> (8 * ch)) & 255u), b = (float)((p01 >> (8 * ch)) & 255u);
                const float cc = (float)((p10 >> (8 * ch)) & 255u), d = (float)((p11 >> (8 * ch)) & 255u);
                const float top = (1.f - wx) * a + wx * b, bot = (1.f - wx) * cc + wx * d;
                acc[ch] += (1.f - wy) * top + wy * bot;
            }
        }
    }
    const float n = (float)(g.tx * g.ty);
    acc[0] /= n; acc[1] /= n; acc[2] /= n;
}

__global__ __launch_bounds__(TPB) void box_crop_k(const unsigned char* __restrict__ frames, int F, int Hs, int Ws, const int* __restrict__ frame_idx,
                                                  const float* __restrict__ boxes, int M, int Ho, int Wo, int tiles_x,
                                                  const float* __restrict__ mean3, const float* __restrict__ std3, int mirror, int aligned,
                                                  float* __restrict__ out_f32, unsigned char* __restrict__ out_u8,
                                                  unsigned char* __restrict__ status) {
    __shared__ unsigned int img[LDS_PIXELS];
    __shared__ TileSetup ts;
    const int m = blockIdx.y;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int u0 = tile_x * TW, v0 = tile_y * TH;
    const int u1 = min(u0 + TW, Wo), v1 = min(v0 + TH, Ho);
    const int f = frame_idx[m];
    if (threadIdx.x == 0) {
        TileSetup t;
        t.staged = 0; t.x_lo = t.y_lo = 0; t.w = t.h = 1;
        t.ok = box_geom(boxes + (size_t)m * 5, Ho, Wo, t.g) && f >= 0 && f < F;
        if (t.ok && aligned) {
            // the tile's corners in the frame: every sample of the tile lies inside their bounding box
            const BoxGeom& g = t.g;
            const float dx0 = ((float)u0 - (float)Wo / 2.f) * g.sx, dx1 = ((float)u1 - (float)Wo / 2.f) * g.sx;
            const float dy0 = ((float)v0 - (float)Ho / 2.f) * g.sy, dy1 = ((float)v1 - (float)Ho / 2.f) * g.sy;
            float xa = INFINITY, xb = -INFINITY, ya = INFINITY, yb = -INFINITY;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float dx = (k & 1) ? dx1 : dx0, dy = (k & 2) ? dy1 : dy0;
                const float X = g.cx + g.c * dx - g.s * dy, Y = g.cy + g.s * dx + g.c * dy;
                xa = fminf(xa, X); xb = fmaxf(xb, X); ya = fminf(ya, Y); yb = fmaxf(yb, Y);
            }
            // taps floor(X - 0.5) .. + 1, one pixel of margin for rounding; clipped to the frame and its zero border (-1 .. Ws, -1 .. Hs)
            xa = fmaxf(floorf(xa - 0.5f) - 1.f, -1.f); xb = fminf(floorf(xb - 0.5f) + 2.f, (float)Ws);
            ya = fmaxf(floorf(ya - 0.5f) - 1.f, -1.f); yb = fminf(floorf(yb - 0.5f) + 2.f, (float)Hs);
            if (xb >= xa && yb >= ya) {      // (false as well for a NaN of an overflowed corner, and for a tile wholly outside the frame)
                const float w = xb - xa + 1.f, h = yb - ya + 1.f;
                if (w * h <= (float)LDS_PIXELS) {
                    t.staged = 1;
                    t.x_lo = (int)xa; t.y_lo = (int)ya; t.w = (int)w; t.h = (int)h;
                }
            }
        }
        ts = t;
        if (blockIdx.x == 0) status[m] = t.ok ? 0 : 1;
    }
    __syncthreads();
    const int ok = ts.ok, staged = ts.staged;
    const unsigned char* frame = frames + (size_t)(ok ? f : 0) * Hs * Ws * 3;
    if (staged) {
        const int x_lo = ts.x_lo, y_lo = ts.y_lo, w = ts.w, h = ts.h;
        // the in-frame part: rows ya .. yb, columns xa .. xb; row y's bytes are [rb + xa * 3, rb + (xb + 1) * 3) of the frames buffer
        const int xa = max(x_lo, 0), xb = min(x_lo + w - 1, Ws - 1), ya = max(y_lo, 0), yb = min(y_lo + h - 1, Hs - 1);
        if (xa != x_lo || ya != y_lo || xb - xa + 1 != w || yb - ya + 1 != h) {      // (uniform) part of the footprint is the zero border
            for (int p = threadIdx.x; p < w * h; p += TPB) img[p] = 0u;
            __syncthreads();
        }
        if (xb >= xa && yb >= ya) {
            const size_t total = (size_t)F * Hs * Ws * 3;
            const int nd = ((xb - xa + 1) * 3 + 3) / 4 + 1;      // dwords that cover a row's bytes at any alignment
            const int rows = yb - ya + 1;
            unsigned char* img8 = (unsigned char*)img;
            for (int q = threadIdx.x; q < rows * nd; q += TPB) {
                const int r = q / nd, jd = q - r * nd;
                const int y = ya + r;
                const size_t rb = ((size_t)f * Hs + y) * (size_t)Ws * 3;      // byte offset of (y, 0)
                const size_t b0 = rb + (size_t)xa * 3, b1 = rb + (size_t)(xb + 1) * 3;
                const size_t d = (b0 >> 2) + jd;
                if (d * 4 >= b1) continue;
                unsigned int word;
                if (d * 4 + 4 <= total) word = *(const unsigned int*)(frames + d * 4);
                else {      // the last, partial dword of the buffer: nothing is read past its end
                    word = 0u;
                    for (size_t e = d * 4; e < total; ++e) word |= (unsigned int)frames[e] << (8 * (e - d * 4));
                }
                unsigned char* row = img8 + (size_t)(y - y_lo) * w * 4;      // LDS bytes of footprint row y, column x_lo first
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const size_t a = d * 4 + e;
                    if (a >= b0 && a < b1) {
                        const unsigned int k = (unsigned int)(a - rb), px = k / 3u, ch = k - px * 3u;
                        row[(px - (unsigned int)x_lo) * 4u + ch] = (unsigned char)(word >> (8 * e));      // (px >= xa >= x_lo)
                    }
                }
            }
        }
        __syncthreads();
    }
    const int lx = threadIdx.x & (TW - 1), ly = threadIdx.x / TW;
    const int u = u0 + lx, v = v0 + ly;
    if (u >= Wo || v >= Ho) return;
    float acc[3] = {0.f, 0.f, 0.f};
    if (ok) {
        const BoxGeom g = ts.g;
        if (staged) box_pixel(LdsTaps{img, ts.x_lo, ts.y_lo, ts.w, ts.h}, g, u, v, Ho, Wo, Hs, Ws, acc);
        else box_pixel(GlobalTaps{frame, Hs, Ws}, g, u, v, Ho, Wo, Hs, Ws, acc);
    }
    const size_t HW = (size_t)Ho * Wo;
    const int um = Wo - 1 - u;
    if (out_f32) {
        float* o = out_f32 + (size_t)m * 3 * HW + (size_t)v * Wo;
        float* om = out_f32 + ((size_t)M + m) * 3 * HW + (size_t)v * Wo;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float z = to_tensor_norm(acc[ch], mean3[ch], std3[ch]);
            o[ch * HW + u] = z;
            if (mirror) om[ch * HW + um] = z;
        }
    }
    if (out_u8) {
        unsigned char* o = out_u8 + ((size_t)m * HW + (size_t)v * Wo + u) * 3;
        unsigned char* om = out_u8 + (((size_t)M + m) * HW + (size_t)v * Wo + um) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const unsigned char z = (unsigned char)fminf(255.f, floorf(acc[ch] + 0.5f));
            o[ch] = z;
            if (mirror) om[ch] = z;
        }
    }
}

// out[m][k] = (cx, cy) + R(rot) (((x stride_x, y stride_y) - (Wo / 2, Ho / 2)) * (sx, sy)): one thread per key point
__global__ void coords_to_image_k(const float* __restrict__ coords, const float* __restrict__ boxes, int M, int K, float stride_x, float stride_y,
                                  int Ho, int Wo, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= (size_t)M * K) return;
    const float* b = boxes + (i / (size_t)K) * 5;
    const float sx = b[2] / (float)Wo, sy = b[3] / (float)Ho;
    float c, s;
    box_trig(b[4], c, s);
    const float dx = (coords[i * 2] * stride_x - (float)Wo / 2.f) * sx, dy = (coords[i * 2 + 1] * stride_y - (float)Ho / 2.f) * sy;
    out[i * 2] = b[0] + c * dx - s * dy;
    out[i * 2 + 1] = b[1] + s * dx + c * dy;
}
}  // namespace

int box_crop(hipStream_t s, const unsigned char* frames, int F, int Hs, int Ws, const int* frame_idx, const float* boxes, int M, int Ho, int Wo,
             const float* mean3, const float* std3, int mirror, float* out_f32, unsigned char* out_u8, unsigned char* status) {
    if (!frames || !frame_idx || !boxes || !status || (!out_f32 && !out_u8) || (out_f32 && (!mean3 || !std3))) return UDAPOSE_ERR_ARG;
    if (F < 1 || M < 1 || Ho < 1 || Ho > 1024 || Wo < 1 || Wo > 1024 || Hs < 1 || Hs > 8192 || Ws < 1 || Ws > 8192) return UDAPOSE_ERR_ARG;
    if (mirror != 0 && mirror != 1) return UDAPOSE_ERR_ARG;
    if (M > 65535) return UDAPOSE_ERR_ARG;      // (grid y)
    const int tiles_x = (Wo + TW - 1) / TW, tiles_y = (Ho + TH - 1) / TH;
    const int aligned = ((uintptr_t)frames & 3u) == 0;
    hipLaunchKernelGGL(box_crop_k, dim3(tiles_x * tiles_y, M), dim3(TPB), 0, s, frames, F, Hs, Ws, frame_idx, boxes, M, Ho, Wo, tiles_x, mean3, std3,
                       mirror, aligned, out_f32, out_u8, status);
    return udapose_check_launch();
}

int box_coords_to_image(hipStream_t s, const float* coords, const float* boxes, int M, int K, float stride_x, float stride_y, int Ho, int Wo,
                        float* out) {
    if (!coords || !boxes || !out || M < 1 || K < 1 || Ho < 1 || Wo < 1) return UDAPOSE_ERR_ARG;
    if ((long long)M * K > 0x7fffffffLL) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(coords_to_image_k, dim3(grid_for((size_t)M * K, TPB, GRID_NO_CAP)), dim3(TPB), 0, s, coords, boxes, M, K, stride_x, stride_y,
                       Ho, Wo, out);
    return udapose_check_launch();
}
