// Data gradient of the stem convolution (7x7, stride 2, pad 3, 64 channels of dy -> the 3 image channels): what carries a loss's
// gradient through PoseResNet to its INPUT.
//   dx[n][c][iy][ix] = sum over co, ky, kx with 2*oy + ky - 3 == iy and 2*ox + kx - 3 == ix of dy[n][oy][ox][co] * w[co][c][ky][kx]
// dy NHWC [N][H/2][W/2][64] in the element type, w the fp32 master weight in its channels-last layout [64][7][7][3] (rounded to the
// element type here: every data gradient of a plan reads element-type weights), dx fp32 NCHW [N][3][H][W], every element written.
//
// Form.  An even input row receives the filter rows ky = 1, 3, 5 and an odd one ky = 0, 2, 4, 6, so the 2x2 output "quad" (qy, qx) -
// rows 2qy, 2qy+1, columns 2qx, 2qx+1 - reads exactly the 4x4 window of dy at rows qy-1 .. qy+2, columns qx-1 .. qx+2: window row wy holds
// filter row ky = py + 5 - 2*wy of output-row parity py (the one missing tap, py = 0 / wy = 3, is a zero weight), columns alike.  That is
// a GEMM: M = the quads, 12 output columns (py, px, c) padded to 16, K = 16 window pixels x 64 channels = 1024 = 32 steps of
// v_mfma_f32_16x16x32: three quarters of the MFMA columns work, against 3 of 16 for a per-pixel form.
//
// One work-group (4 waves) owns 16x16 quads = 32x32 pixels of one image: the 19x19 dy pixels they read are staged in LDS once (16-byte
// slots XOR-swizzled by the pixel index, so that the 16 lanes a ds_read_b128 serves per cycle hit 16 different slots), the B operand
// [32 steps][64 lanes][8 channels] (32 KB) is built in LDS once per work-group from the fp32 weights, and the grid is at most two
// work-groups per CU which walk the tiles.  A wave owns 4 quad rows (4 accumulators) and reads each B fragment once for the four.
// No atomics, no workspace, one fixed summation order: capturable, bit-reproducible.
#include "net.h"      // prof_before / prof_after

namespace {
constexpr int SD_TQ = 16;                       // quads per tile side
constexpr int SD_TP = SD_TQ + 3;                // dy pixels per tile side: one before, two behind
constexpr int SD_A_BYTES = SD_TP * SD_TP * 128;
constexpr int SD_B_BYTES = 32 * 64 * 16;
constexpr int SD_THREADS = 256;
constexpr int SD_A_UNITS = SD_TP * SD_TP * 8;   // 16-byte slots of the staged tile

// byte offset of 16-byte channel slot `slot` (8 channels) of tile pixel P
__device__ __forceinline__ int sd_a_off(int P, int slot) { return P * 128 + ((slot ^ (P & 7)) << 4); }

// VEC: floats per store (4: W % 4 == 0 and dx 16-byte aligned; 2: dx 8-byte aligned; 1: any dx)
template <int VEC>
__global__ __launch_bounds__(SD_THREADS) void stem_dgrad_k(const elem_t* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx, int QH,
                                                           int QW, int tiles_x, int tiles_y, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem;
    char* Bs = smem + SD_A_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = 2 * QH, W = 2 * QW;

    // B[k = (wy*4 + wx)*64 + co][col = (py*2 + px)*3 + c] = round(w[co][ky][kx][c]) for ky = py + 5 - 2*wy, kx = px + 5 - 2*wx: every weight
    // has exactly one place, the rest of the image is zero.  Stored as the lanes read it: [k step][lane = (k%32/8)*16 + col][k%8]
    for (int i = tid; i < SD_B_BYTES / 16; i += SD_THREADS) ((uint4*)Bs)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    for (int i = tid; i < 64 * 49 * 3; i += SD_THREADS) {
        const int c = i % 3, t = i / 3, kx = t % 7, t2 = t / 7, ky = t2 % 7, co = t2 / 7;
        const int py = 1 - (ky & 1), wy = (py + 5 - ky) >> 1, px = 1 - (kx & 1), wx = (px + 5 - kx) >> 1;
        const int step = (wy * 4 + wx) * 2 + (co >> 5), ln = ((co >> 3) & 3) * 16 + (py * 2 + px) * 3 + c;
        ((elem_t*)Bs)[(step * 64 + ln) * 8 + (co & 7)] = (elem_t)w[i];
    }

    const int lq = lane & 15, lh = lane >> 4;
    // the store's column: lanes 0..11 of every 16 hold (py, px, c); px = 0 and px = 1 of one (py, c) are 3 lanes apart
    const int pyx = lq / 3, oc = lq - 3 * pyx, opy = pyx >> 1, opx = pyx & 1;
    const int partner = (opx ? lane - 3 : lane + 3) & 63;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tx = tile % tiles_x, tr = tile / tiles_x, ty = tr % tiles_y, n = tr / tiles_y;
        const int qy0 = ty * SD_TQ, qx0 = tx * SD_TQ;
        __syncthreads();       // (the B image is complete; the previous tile has been read)
        uint4 v[(SD_A_UNITS + SD_THREADS - 1) / SD_THREADS];
#pragma unroll
        for (int it = 0; it < (SD_A_UNITS + SD_THREADS - 1) / SD_THREADS; ++it) {
            const int u = tid + it * SD_THREADS, P = u >> 3, pr = P / SD_TP, pc = P - pr * SD_TP;
            const int oy = qy0 - 1 + pr, ox = qx0 - 1 + pc;
            v[it] = make_uint4(0u, 0u, 0u, 0u);
            if (u < SD_A_UNITS && (unsigned)oy < (unsigned)QH && (unsigned)ox < (unsigned)QW)
                v[it] = *(const uint4*)(dy + (((size_t)n * QH + oy) * QW + ox) * 64 + (u & 7) * 8);
        }
#pragma unroll
        for (int it = 0; it < (SD_A_UNITS + SD_THREADS - 1) / SD_THREADS; ++it) {
            const int u = tid + it * SD_THREADS;
            if (u < SD_A_UNITS) *(uint4*)(As + sd_a_off(u >> 3, u & 7)) = v[it];
        }
        __syncthreads();

        f32x4 acc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int step = 0; step < 32; ++step) {
            const int wy = step >> 3, wx = (step >> 1) & 3, slot = (step & 1) * 4 + lh;
            const elem8 b = *(const elem8*)(Bs + (step * 64 + lane) * 16);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int P = (wave * 4 + m + wy) * SD_TP + lq + wx;
                const elem8 a = *(const elem8*)(As + sd_a_off(P, slot));
                acc[m] = UDAPOSE_MFMA_16x16x32(a, b, acc[m]);
            }
        }

        // D: column = lane & 15, rows (quads along x) 4*lh .. 4*lh + 3 in the four registers.  The px = 0 lane takes the first two quads
        // of both lanes, the px = 1 lane the last two: each then holds 4 consecutive pixels of one output row
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int qy = qy0 + wave * 4 + m;
            if (qy >= QH) break;        // (wave-uniform)
            const float r0 = __shfl(opx ? acc[m][0] : acc[m][2], partner, 64);
            const float r1 = __shfl(opx ? acc[m][1] : acc[m][3], partner, 64);
            const int qa = qx0 + 4 * lh + 2 * opx;
            if (lq >= 12 || qa >= QW) continue;
            const float o0 = opx ? r0 : acc[m][0], o1 = opx ? acc[m][2] : r0, o2 = opx ? r1 : acc[m][1], o3 = opx ? acc[m][3] : r1;
            float* p = dx + (((size_t)n * 3 + oc) * H + (2 * qy + opy)) * W + 2 * qa;
            const bool two = qa + 1 < QW;
            if (VEC == 4 && two) {
                *(float4*)p = make_float4(o0, o1, o2, o3);
            } else if (VEC >= 2) {
                *(float2*)p = make_float2(o0, o1);
                if (two) *(float2*)(p + 2) = make_float2(o2, o3);
            } else {
                p[0] = o0; p[1] = o1;
                if (two) { p[2] = o2; p[3] = o3; }
            }
        }
    }
}

template <int VEC>
void sd_launch(hipStream_t s, int grid, const elem_t* dy, const float* w, float* dx, int QH, int QW, int tiles_x, int tiles_y, int ntiles) {
    max_dynamic_lds<stem_dgrad_k<VEC>>(SD_A_BYTES + SD_B_BYTES);
    hipLaunchKernelGGL(stem_dgrad_k<VEC>, dim3(grid), dim3(SD_THREADS), SD_A_BYTES + SD_B_BYTES, s, dy, w, dx, QH, QW, tiles_x, tiles_y, ntiles);
}
}  // namespace

int stem_dgrad(hipStream_t s, const elem_t* dy, const float* w, int N, int H, int W, float* dx) {
    if (!dy || !w || !dx || N < 1 || H < 8 || W < 8 || (H & 1) || (W & 1)) return UDAPOSE_ERR_ARG;
    if (((uintptr_t)dy & 15) || ((uintptr_t)w & 3) || ((uintptr_t)dx & 3)) return UDAPOSE_ERR_ARG;
    const int QH = H / 2, QW = W / 2;
    const size_t dy_bytes = (size_t)N * QH * QW * 64 * sizeof(elem_t), dx_bytes = (size_t)N * 3 * H * W * sizeof(float);
    const uintptr_t a = (uintptr_t)dy, b = (uintptr_t)dx;
    if (a < b + dx_bytes && b < a + dy_bytes) return UDAPOSE_ERR_ARG;
    const int tiles_x = (QW + SD_TQ - 1) / SD_TQ, tiles_y = (QH + SD_TQ - 1) / SD_TQ;
    const long long ntiles = (long long)N * tiles_x * tiles_y;
    if (ntiles > 0x7fffffffLL) return UDAPOSE_ERR_UNSUPPORTED;
    const int grid = (int)(ntiles < 512 ? ntiles : 512);      // two work-groups per CU (79 KB of LDS each) walk the tiles
    const int tok = prof_before(s, 1, 2.0 * N * QH * QW * 64 * 49 * 3);
    if (W % 4 == 0 && !(b & 15)) sd_launch<4>(s, grid, dy, w, dx, QH, QW, tiles_x, tiles_y, (int)ntiles);
    else if (!(b & 7)) sd_launch<2>(s, grid, dy, w, dx, QH, QW, tiles_x, tiles_y, (int)ntiles);
    else sd_launch<1>(s, grid, dy, w, dx, QH, QW, tiles_x, tiles_y, (int)ntiles);
    prof_after(s, tok);
    return udapose_check_launch();
}
