// Batched heat-map / image re-warp: the three sequential nearest-neighbour inverse-affine resamplings the reference
// applies per sample with torchvision.transforms.functional.affine (train_human.py:366-368, 421-423), as ONE gather
// kernel driven by a [N][3][6] matrix tensor.  Because every stage is a nearest resample, the composition is evaluated
// as a chain of index maps p3 -> p2 -> p1 -> p0 (NOT as one composed matrix: that would change results).
// Arithmetic follows torchvision/_gen_affine_grid + ATen grid_sampler(nearest, zeros, align_corners=False) in fp32:
// theta / (0.5*[W,H]); base grid at half-integers; ix = ((x+1)*W-1)/2; nearbyint.
// The same chain with bilinear interpolation per stage (affine_warp_chain_bilinear) follows further down.
#include "conv_plan.h"
#include "data.h"
#include "pointwise.h"      // pw_zero

namespace {
constexpr int TPB = 256;

__device__ __forceinline__ bool step(const float* __restrict__ th, int W, int H, int& px, int& py) {
    const float bx = (float)px - 0.5f * (float)W + 0.5f, by = (float)py - 0.5f * (float)H + 0.5f;
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    const float gx = bx * (th[0] / hw) + by * (th[1] / hw) + th[2] / hw;
    const float gy = bx * (th[3] / hh) + by * (th[4] / hh) + th[5] / hh;
    const float ix = ((gx + 1.f) * (float)W - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)H - 1.f) * 0.5f;
    const float rx = nearbyintf(ix), ry = nearbyintf(iy);
    if (!(rx >= 0.f && rx <= (float)(W - 1) && ry >= 0.f && ry <= (float)(H - 1))) return false;
    px = (int)rx; py = (int)ry;
    return true;
}

// MIRRORED VIEWS.  mirror[n] holds two bits per sample: MIRROR_OUT (bit 0) reverses the columns of the chain's OUTPUT,
// MIRROR_IN (bit 1) those of its INPUT; with exactly one of them set and a joint permutation perm [C] given, the source plane of output
// channel c is channel perm[c].  The mirror is an index map at one end of the chain and does no arithmetic: every value is a value of the
// plain chain.  A kernel below takes the two tables as a trailing parameter pack `mir`: none for the plain launch - whose kernel then has the
// parameters and, the bits being the constant 0, the instructions it had before the mirrored forms existed - or one Mirror.
constexpr unsigned MIRROR_OUT = 1, MIRROR_IN = 2;
struct Mirror { const unsigned char* bits; const int* perm; };
__device__ __forceinline__ unsigned mirror_bits(int) { return 0u; }
__device__ __forceinline__ unsigned mirror_bits(int n, const Mirror& mr) { return mr.bits[n] & 3u; }
// the plane the launch reads for channel c of a sample (perm is an involution: the backward reads d(out) from the same plane)
__device__ __forceinline__ int mirror_plane(unsigned, int c) { return c; }
__device__ __forceinline__ int mirror_plane(unsigned m, int c, const Mirror& mr) {
    return mr.perm && (m == MIRROR_OUT || m == MIRROR_IN) ? mr.perm[c] : c;
}
__device__ __forceinline__ int mirror_index(int i, int W) { return i + W - 1 - 2 * (i % W); }      // (y, x) -> (y, W - 1 - x), flat

// nstage sequential warps (1..3); theta: [N][nstage][6] fp32 in application order (stage 0 applied first)
template <bool BWD, class... M>
__global__ void warp_chain_k(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ theta, int N, int C, int H, int W,
                             int nstage, M... mir) {
    const size_t total = (size_t)N * H * W;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB) {
        const int n = (int)(i / ((size_t)H * W));
        const int rem = (int)(i % ((size_t)H * W));
        int py = rem / W, px = rem % W;
        const unsigned m = mirror_bits(n, mir...);
        if (m & MIRROR_OUT) px = W - 1 - px;          // output pixel (y, x) is the chain's (y, W - 1 - x)
        bool ok = true;
        for (int s = nstage - 1; s >= 0 && ok; --s) ok = step(theta + ((size_t)n * nstage + s) * 6, W, H, px, py);
        if (m & MIRROR_IN) px = W - 1 - px;                    // the chain read M(in): its pixel (y, x) is in's (y, W - 1 - x)
        const size_t o = (size_t)n * C * H * W;
        // (blockIdx.y strides the channels: the index map is cheap to recompute and the launch sits, alone on the device, between the
        // forwards and the backward of a step - 16 channel groups took the backward of [32,16,64,64] from 58 us to what one atomic costs)
        if (!BWD) {
            for (int c = blockIdx.y; c < C; c += gridDim.y)
                dst[o + (size_t)c * H * W + rem] = ok ? src[o + (size_t)mirror_plane(m, c, mir...) * H * W + py * W + px] : 0.f;
        } else if (ok) {
            // src = d(out), dst = d(in) (pre-zeroed): several outputs may read the same input pixel
            for (int c = blockIdx.y; c < C; c += gridDim.y)
                atomicAdd(dst + o + (size_t)mirror_plane(m, c, mir...) * H * W + py * W + px, src[o + (size_t)c * H * W + rem]);
        }
    }
}
// Backward of the chain, DETERMINISTIC form (round 6).  d(in)[p] = sum of d(out)[i] over the output pixels i whose chain ends at p; an up-scaling
// chain sends several outputs to one input pixel, and fp32 atomics add them in arrival order (rounds 1-5: the one place outside the weight
// gradients where two runs of a step could differ in the last bit).  Here one work-group owns one (sample, channel) plane: it computes the
// plane's index map into LDS, RANKS the outputs that share a target by ascending output index (round r: every unranked output proposes itself
// with an LDS atomicMin on its target's slot - an integer minimum is order-independent - and the winner takes rank r), and then adds
// rank 0, rank 1, ... into an LDS accumulator with one barrier per rank: every input pixel receives its contributions in ascending output
// index, whatever the scheduling.  A rank is one byte: an epoch ranks at most 254 outputs per target, adds them, retires them, and a collapsing
// map (zoom > ~15, an all-zero theta: up to H*W outputs on one pixel) takes further epochs over the outputs still pending - each epoch ranks
// the smallest pending indices, so the order stays ascending across epochs.  The loop's scales (<= 1 / 0.6 per axis) need one epoch, and
// then the rounds and barriers are those of a single pass.  The plane is stored with plain coalesced stores (no clear of dst beforehand).
// LDS: (int target + int slot + float acc) per pixel + 1 byte rank = 13 bytes per pixel (53 KB for 64x64, 120 KB for 96x96).
// Mirrored (a Mirror in `mir`): i stays the index of the CHAIN'S OWN output pixel, so the ranks - the summation order - are those of the plain launch on the
// un-mirrored gradient; MIRROR_OUT only moves where d(out)[i] is read, MIRROR_IN where the chain's target lies in d(in).
template <class... M>
__global__ __launch_bounds__(TPB) void warp_chain_bwd_det_k(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ theta,
                                                            int C, int H, int W, int nstage, M... mir) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int HW = H * W;
    int* tgt = (int*)smem;
    int* slot = tgt + HW;
    float* acc = (float*)(slot + HW);
    unsigned char* rank = (unsigned char*)(acc + HW);
    const int n = blockIdx.x / C, c = blockIdx.x % C;
    const unsigned m = mirror_bits(n, mir...);
    for (int i = threadIdx.x; i < HW; i += TPB) {
        int py = i / W, px = i % W;
        bool ok = true;
        for (int s = nstage - 1; s >= 0 && ok; --s) ok = step(theta + ((size_t)n * nstage + s) * 6, W, H, px, py);
        if (m & MIRROR_IN) px = W - 1 - px;
        tgt[i] = ok ? py * W + px : -1;
        rank[i] = ok ? 255 : 254;          // 255: not ranked yet; 254: contributes nothing (or already added)
        acc[i] = 0.f;
    }
    __syncthreads();
    const float* sp = src + ((size_t)n * C + mirror_plane(m, c, mir...)) * HW;
    const bool gm = m & MIRROR_OUT;
    for (bool more = true; more;) {
        more = false;
        int nrounds = 0;
        for (int r = 0; r < 254; ++r) {
            for (int i = threadIdx.x; i < HW; i += TPB) slot[i] = 0x7fffffff;
            __syncthreads();
            int pending = 0;
            for (int i = threadIdx.x; i < HW; i += TPB)
                if (rank[i] == 255) { atomicMin(&slot[tgt[i]], i); pending = 1; }
            if (!__syncthreads_or(pending)) break;
            for (int i = threadIdx.x; i < HW; i += TPB)
                if (rank[i] == 255 && slot[tgt[i]] == i) rank[i] = (unsigned char)r;
            nrounds = r + 1;
            more = r == 253;               // (all 254 ranks taken: outputs may still be pending - another epoch finds out)
            __syncthreads();
        }
        for (int r = 0; r < nrounds; ++r) {
            for (int i = threadIdx.x; i < HW; i += TPB)
                if (rank[i] == r) { acc[tgt[i]] += sp[gm ? mirror_index(i, W) : i]; rank[i] = 254; }        // (one writer per target and round)
            __syncthreads();
        }
    }
    float* dp = dst + ((size_t)n * C + c) * HW;
    for (int i = threadIdx.x; i < HW; i += TPB) dp[i] = acc[i];
}
// Occlusion paste (train_human.py:409): img[:, r0:r1, c0:c1] = img[:, rs:rs+(r1-r0), cs:cs+(c1-c0)] for each listed image,
// reading the whole source patch before writing (one block per image; patches are at most 20x20x3 = 1200 values).
__global__ void patch_paste_k(float* __restrict__ img, const int* __restrict__ boxes, int C, int H, int W) {
    __shared__ float buf[4096];
    const int* b = boxes + blockIdx.x * 6;          // r0, r1, c0, c1, rs, cs
    const int r0 = b[0], r1 = b[1], c0 = b[2], c1 = b[3], rs = b[4], cs = b[5];
    const int ph = r1 - r0, pw = c1 - c0, n = C * ph * pw;
    float* base = img + (size_t)blockIdx.x * C * H * W;
    for (int i = threadIdx.x; i < n; i += TPB) {
        const int c = i / (ph * pw), r = (i / pw) % ph, q = i % pw;
        buf[i] = base[((size_t)c * H + rs + r) * W + cs + q];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += TPB) {
        const int c = i / (ph * pw), r = (i / pw) % ph, q = i % pw;
        base[((size_t)c * H + r0 + r) * W + c0 + q] = buf[i];
    }
}
// The occlusion DECISIONS of train_human.py:374-410 on the device, one thread per sample: which samples (any confidence >=
// thresh and a uniform draw <= rate), which confident key point, the box around it in image pixels (rows from y, columns from
// x: the reference's index math) and where the replacement patch comes from.  u[n][0..3] are uniform [0,1) draws supplied by
// the caller: u0 = the rate test, u1 -> np.random.choice among the confident key points, u2 / u3 -> np.random.randint of the
// patch origin.  (The reference consumes its draws only for qualifying samples, from an unseeded global generator; drawing
// all four for every sample gives the same distribution without the read-back that made this step un-capturable.)
// boxes[n] = {r0, r1, c0, c1, rs, cs} (a zero-area box when the sample is not selected), apply[n] = 0 / 1.
__global__ void occlusion_pick_k(const float* __restrict__ conf, const int* __restrict__ idx, const float* __restrict__ u, int N, int K, int w,
                                 double ratio, int image_size, float rate, float thresh, int occ, int* __restrict__ boxes,
                                 unsigned char* __restrict__ apply) {
    const int n = blockIdx.x * TPB + threadIdx.x;
    if (n >= N) return;
    int count = 0;
    for (int k = 0; k < K; ++k) count += conf[n * K + k] >= thresh;
    int* b = boxes + n * 6;
    if (count == 0 || !(u[n * 4] <= rate)) {
        for (int i = 0; i < 6; ++i) b[i] = 0;
        apply[n] = 0;
        return;
    }
    int j = (int)(u[n * 4 + 1] * (float)count);
    if (j > count - 1) j = count - 1;
    int c = 0;
    for (int k = 0; k < K; ++k)
        if (conf[n * K + k] >= thresh) { if (j == 0) { c = k; break; } --j; }
    const int flat = idx[n * K + c];
    const int px = (int)((double)(flat % w) * ratio), py = (int)((double)(flat / w) * ratio);      // (pred_position * ratio).astype(int)
    const int r0 = max(py - occ, 0), r1 = min(py + occ, image_size);
    const int c0 = max(px - occ, 0), c1 = min(px + occ, image_size);
    const int mr = image_size - (r1 - r0) + 1, mc = image_size - (c1 - c0) + 1;
    int rs = (int)(u[n * 4 + 2] * (float)mr), cs = (int)(u[n * 4 + 3] * (float)mc);
    if (rs > mr - 1) rs = mr - 1;
    if (cs > mc - 1) cs = mc - 1;
    b[0] = r0; b[1] = r1; b[2] = c0; b[3] = c1; b[4] = rs; b[5] = cs;
    apply[n] = 1;
}

// dst[n] = flag[n] ? a[n] : b[n] over rows of `row` floats (16-byte vectors): only the selected samples take the occluded image
__global__ void select_rows_k(float* __restrict__ dst, const float* __restrict__ a, const float* __restrict__ b, const unsigned char* __restrict__ flag,
                              size_t row4, size_t total4) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total4; i += (size_t)gridDim.x * TPB) {
        const size_t n = i / row4;
        ((f32x4*)dst)[i] = flag[n] ? ((const f32x4*)a)[i] : ((const f32x4*)b)[i];
    }
}
}  // namespace

int occlusion_pick(hipStream_t s, const float* conf, const int* idx, const float* u, int N, int K, int w, double ratio, int image_size, float rate,
                   float thresh, int occ, int* boxes, unsigned char* apply) {
    if (N <= 0 || K <= 0 || w <= 0 || occ < 0) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(occlusion_pick_k, dim3((N + TPB - 1) / TPB), dim3(TPB), 0, s, conf, idx, u, N, K, w, ratio, image_size, rate, thresh, occ, boxes,
                       apply);
    return udapose_check_launch();
}
int select_rows(hipStream_t s, float* dst, const float* a, const float* b, const unsigned char* flag, int N, size_t row) {
    if (N <= 0 || row % 4) return UDAPOSE_ERR_ARG;
    const size_t total4 = (size_t)N * row / 4;
    size_t blocks = (total4 + TPB - 1) / TPB;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(select_rows_k, dim3((int)blocks), dim3(TPB), 0, s, dst, a, b, flag, row / 4, total4);
    return udapose_check_launch();
}

int patch_paste(hipStream_t s, float* img, const int* boxes, int n, int C, int H, int W, int max_patch_elems) {
    if (n <= 0) return UDAPOSE_OK;
    if (max_patch_elems > 4096) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(patch_paste_k, dim3(n), dim3(TPB), 0, s, img, boxes, C, H, W);
    return udapose_check_launch();
}

// The loop's inverse affine matrices on the device, in double precision (torchvision's _get_inverse_affine_matrix with centre (0,0),
// as warp.inverse_affine_matrix states it): params[n] = (angle, tx, ty, shear_x, shear_y, scale) of the collated aug_param
// (lib/transforms/keypoint_detection.py:139), angles in degrees.
//   fwd[n][3][6]: translate by (tx, ty) / ratio | rotate by angle and scale | shear      (train_human.py:366-368, 421-423)
//   back[n][1][6]: the occlusion path's single warp back (-angle, (-tx, -ty) / ratio, 1 / scale, -shear)   (train_human.py:412)
__device__ __forceinline__ void inv_affine(double angle, double tx, double ty, double scale, double shx, double shy, float* m) {
    const double d2r = 0.017453292519943295;
    const double rot = angle * d2r, sx = shx * d2r, sy = shy * d2r;
    const double a = cos(rot - sy) / cos(sy);
    const double b = -cos(rot - sy) * tan(sx) / cos(sy) - sin(rot);
    const double c = sin(rot - sy) / cos(sy);
    const double d = -sin(rot - sy) * tan(sx) / cos(sy) + cos(rot);
    const double m0 = d / scale, m1 = -b / scale, m3 = -c / scale, m4 = a / scale;
    m[0] = (float)m0; m[1] = (float)m1; m[2] = (float)(m0 * (-tx) + m1 * (-ty));
    m[3] = (float)m3; m[4] = (float)m4; m[5] = (float)(m3 * (-tx) + m4 * (-ty));
}
__global__ void recon_thetas_k(const double* __restrict__ params, int N, double ratio, float* __restrict__ fwd, float* __restrict__ back) {
    const int n = blockIdx.x * TPB + threadIdx.x;
    if (n >= N) return;
    const double* q = params + (size_t)n * 6;
    const double angle = q[0], tx = q[1], ty = q[2], shx = q[3], shy = q[4], scale = q[5];
    if (fwd) {
        float* f = fwd + (size_t)n * 18;
        inv_affine(0.0, tx / ratio, ty / ratio, 1.0, 0.0, 0.0, f);
        inv_affine(angle, 0.0, 0.0, scale, 0.0, 0.0, f + 6);
        inv_affine(0.0, 0.0, 0.0, 1.0, shx, shy, f + 12);
    }
    if (back) inv_affine(-angle, -tx / ratio, -ty / ratio, 1.0 / scale, -shx, -shy, back + (size_t)n * 6);
}
int affine_recon_thetas(hipStream_t s, const double* params, int N, double ratio, float* fwd, float* back) {
    if (N <= 0 || ratio == 0.0) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(recon_thetas_k, dim3((N + TPB - 1) / TPB), dim3(TPB), 0, s, params, N, ratio, fwd, back);
    return udapose_check_launch();
}

// mirror == nullptr: the plain launches; otherwise their mirrored forms under the same dispatch rules
static int warp_chain_dispatch(hipStream_t s, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage, int backward,
                               const unsigned char* mirror, const int* perm) {
    if (nstage < 1 || nstage > 8) return UDAPOSE_ERR_ARG;
    const size_t total = (size_t)N * H * W;
    int blocks = (int)((total + TPB - 1) / TPB);
    if (blocks > 4096) blocks = 4096;
    const int cgroups = C >= 16 ? 16 : (C >= 4 ? 4 : 1);
    const Mirror mir = {mirror, perm};
    if (backward) {
        // deterministic form (one work-group per (sample, channel) plane, ranks in LDS) wherever the plane fits, at any number of outputs per
        // input pixel (more than 254 - a zoom past ~15, a collapsed theta - take further ranking epochs); a plane beyond the LDS budget takes the
        // atomic form
        const size_t lds = (size_t)H * W * 13 + 16;
        if (lds <= 150 * 1024 && (long long)N * C < (1ll << 31)) {
            const unsigned bytes = (unsigned)((lds + 15) & ~(size_t)15);
            if (mirror) {
                max_dynamic_lds<warp_chain_bwd_det_k<Mirror>>(150 * 1024);
                hipLaunchKernelGGL(warp_chain_bwd_det_k<Mirror>, dim3(N * C), dim3(TPB), bytes, s, src, dst, theta, C, H, W, nstage, mir);
            } else {
                max_dynamic_lds<warp_chain_bwd_det_k<>>(150 * 1024);
                hipLaunchKernelGGL(warp_chain_bwd_det_k<>, dim3(N * C), dim3(TPB), bytes, s, src, dst, theta, C, H, W, nstage);
            }
            return udapose_check_launch();
        }
        if (pw_zero(s, dst, (size_t)N * C * H * W * sizeof(float)) != UDAPOSE_OK) return UDAPOSE_ERR_LAUNCH;
        if (mirror) hipLaunchKernelGGL((warp_chain_k<true, Mirror>), dim3(blocks, cgroups), dim3(TPB), 0, s, src, dst, theta, N, C, H, W, nstage, mir);
        else hipLaunchKernelGGL(warp_chain_k<true>, dim3(blocks, cgroups), dim3(TPB), 0, s, src, dst, theta, N, C, H, W, nstage);
    } else if (mirror) {
        hipLaunchKernelGGL((warp_chain_k<false, Mirror>), dim3(blocks, cgroups), dim3(TPB), 0, s, src, dst, theta, N, C, H, W, nstage, mir);
    } else {
        hipLaunchKernelGGL(warp_chain_k<false>, dim3(blocks, cgroups), dim3(TPB), 0, s, src, dst, theta, N, C, H, W, nstage);
    }
    return udapose_check_launch();
}
int affine_warp_chain(hipStream_t s, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage, int backward) {
    return warp_chain_dispatch(s, src, dst, theta, N, C, H, W, nstage, backward, nullptr, nullptr);
}
// src and dst must not overlap (a mirrored or permuted plane is not written where it is read)
int affine_warp_chain_mirror(hipStream_t s, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage, int backward,
                             const unsigned char* mirror, const int* perm) {
    if (!mirror || !src || !dst || !theta || N <= 0 || C <= 0 || H <= 0 || W <= 0) return UDAPOSE_ERR_ARG;
    return warp_chain_dispatch(s, src, dst, theta, N, C, H, W, nstage, backward, mirror, perm);
}

// ---------------------------------------------------------------- BILINEAR chain (tF.affine with InterpolationMode.BILINEAR per stage)
// Per stage: _gen_affine_grid + grid_sample(bilinear, zeros, align_corners=False) - the coordinate expressions of step() above, then floor,
// four taps with weights (x0+1-ix | ix-x0) * (y0+1-iy | iy-y0), a tap outside the plane contributing 0.  Every stage clips against the plane
// on its own (the matrices are NOT composed).  All multiply-adds of the coordinates, the weights and the tap sums are written as explicit
// fmaf, so that forward and backward evaluate one and the same instruction sequence wherever they are inlined: the backward's weights are
// bitwise the forward's.
// Backward = the exact transpose as a GATHER: d_in[r] = sum over the outputs q whose sample point lies in the open 2x2 box around r of
// w(q -> r) * d_out[q], the q visited in raster order by the one thread that owns r - no atomics, no rank limit, the same bits every run.
// In pixel units a stage maps q to ix = t0*bx + t1*by + t2 + (W-1)/2, iy = t3*bx + t4*by + t5 + (H-1)/2 (bx, by = q minus the plane
// centre), so the q that can touch r lie in the image of r's box under the inverse of [[t0,t1],[t3,t4]]: a parallelogram, whose bounding
// box - widened by the forward's fp32 coordinate error and by one output pixel - is enumerated; every candidate's ix, iy, floor and weight
// are recomputed with the forward's expressions, and a candidate that does not touch r adds nothing.  A singular or near-singular matrix
// (an all-zero theta) has no finite box: that stage scans the whole plane - slow, and correct.
namespace {
struct BilinStage { float a, b, c, d, e, f; };
__device__ __forceinline__ BilinStage bilin_stage(const float* __restrict__ th, int W, int H) {
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    return {th[0] / hw, th[1] / hw, th[2] / hw, th[3] / hh, th[4] / hh, th[5] / hh};
}
__device__ __forceinline__ void bilin_coords(const BilinStage& m, int W, int H, int px, int py, float& ix, float& iy) {
    const float bx = (float)px - 0.5f * (float)W + 0.5f, by = (float)py - 0.5f * (float)H + 0.5f;
    const float gx = fmaf(bx, m.a, fmaf(by, m.b, m.c));
    const float gy = fmaf(bx, m.d, fmaf(by, m.e, m.f));
    ix = fmaf(gx + 1.f, (float)W, -1.f) * 0.5f;
    iy = fmaf(gy + 1.f, (float)H, -1.f) * 0.5f;
}
// one output pixel of a stage: p = the stage's input plane
__device__ __forceinline__ float bilin_sample(const float* p, const BilinStage& m, int W, int H, int px, int py) {
    float ix, iy;
    bilin_coords(m, W, H, px, py, ix, iy);
    if (!(ix > -1.f && ix < (float)W && iy > -1.f && iy < (float)H)) return 0.f;        // (all four taps outside; also NaN / infinite coordinates)
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float wx0 = (fx0 + 1.f) - ix, wx1 = ix - fx0, wy0 = (fy0 + 1.f) - iy, wy1 = iy - fy0;
    const bool xl = x0 >= 0, xr = x0 + 1 < W, yt = y0 >= 0, yb = y0 + 1 < H;
    float acc = 0.f;
    if (yt && xl) acc = fmaf(wx0 * wy0, p[y0 * W + x0], acc);
    if (yt && xr) acc = fmaf(wx1 * wy0, p[y0 * W + x0 + 1], acc);
    if (yb && xl) acc = fmaf(wx0 * wy1, p[(y0 + 1) * W + x0], acc);
    if (yb && xr) acc = fmaf(wx1 * wy1, p[(y0 + 1) * W + x0 + 1], acc);
    return acc;
}
// the candidate box of a stage's gather: q = Minv * (r - centre - t) + centre, +- (ex, ey)
struct BilinBox { double i00, i01, i10, i11, tx, ty, ex, ey; int full; };
__device__ __forceinline__ BilinBox bilin_box(const float* __restrict__ th, int W, int H) {
    const double t0 = th[0], t1 = th[1], t2 = th[2], t3 = th[3], t4 = th[4], t5 = th[5];
    const double det = t0 * t4 - t1 * t3, nrm = t0 * t0 + t1 * t1 + t3 * t3 + t4 * t4;
    BilinBox b;
    b.full = !(fabs(det) > 1e-6 * nrm) || !(nrm < 1e30) || !(fabs(t2) < 1e30) || !(fabs(t5) < 1e30);
    if (b.full) { b.i00 = b.i01 = b.i10 = b.i11 = b.tx = b.ty = b.ex = b.ey = 0.0; return b; }
    b.i00 = t4 / det; b.i01 = -t1 / det; b.i10 = -t3 / det; b.i11 = t0 / det;
    b.tx = t2 + 0.5 * (double)(W - 1); b.ty = t5 + 0.5 * (double)(H - 1);
    // half-size of r's box in input pixels: 1, plus a bound on the forward's fp32 error of ix / iy (a few roundings of terms this large)
    const double eps = 16.0 * 5.97e-8;
    const double hx = 1.0 + eps * (fabs(t0) * W + fabs(t1) * H + fabs(t2) + W), hy = 1.0 + eps * (fabs(t3) * W + fabs(t4) * H + fabs(t5) + H);
    b.ex = fabs(b.i00) * hx + fabs(b.i01) * hy + 1.0;
    b.ey = fabs(b.i10) * hx + fabs(b.i11) * hy + 1.0;
    return b;
}
// one input pixel r = (rx, ry) of a stage's backward: g = d(out) of the stage
__device__ __forceinline__ float bilin_gather(const float* g, const BilinStage& m, const BilinBox& b, int W, int H, int rx, int ry) {
    int x_lo = 0, x_hi = W - 1, y_lo = 0, y_hi = H - 1;
    if (!b.full) {
        const double u = (double)rx - b.tx, v = (double)ry - b.ty;
        const double qx = b.i00 * u + b.i01 * v + 0.5 * (double)(W - 1), qy = b.i10 * u + b.i11 * v + 0.5 * (double)(H - 1);
        // (clamped as doubles: a centre far outside the plane must not overflow the conversion; an empty range runs no iteration)
        x_lo = (int)fmax(0.0, fmin((double)W, ceil(qx - b.ex)));
        x_hi = (int)fmin((double)(W - 1), fmax(-1.0, floor(qx + b.ex)));
        y_lo = (int)fmax(0.0, fmin((double)H, ceil(qy - b.ey)));
        y_hi = (int)fmin((double)(H - 1), fmax(-1.0, floor(qy + b.ey)));
    }
    float acc = 0.f;
    for (int qy = y_lo; qy <= y_hi; ++qy)
        for (int qx = x_lo; qx <= x_hi; ++qx) {
            float ix, iy;
            bilin_coords(m, W, H, qx, qy, ix, iy);
            const float fx0 = floorf(ix), fy0 = floorf(iy);
            const float dx = (float)rx - fx0, dy = (float)ry - fy0;         // 0: r is the tap at floor; 1: the tap after it
            if (!((dx == 0.f || dx == 1.f) && (dy == 0.f || dy == 1.f))) continue;
            if (!(ix > -1.f && iy > -1.f)) continue;                        // (the forward's own refusal; r is inside, so < W / < H hold)
            const float wx = dx == 0.f ? (fx0 + 1.f) - ix : ix - fx0, wy = dy == 0.f ? (fy0 + 1.f) - iy : iy - fy0;
            acc = fmaf(wx * wy, g[qy * W + qx], acc);
        }
    return acc;
}
// One work-group owns one (sample, channel) plane: it stages the plane in LDS and runs the stages ping-pong between two LDS planes (the
// backward: the stages in reverse, each as the gather above); the last stage is stored with coalesced stores.  LDS: 2 * H * W * 4 bytes.
// Mirrored (a Mirror in `mir`): the reversed row is taken on the LDS load (the forward's MIRROR_IN, the backward's MIRROR_OUT) or on the final store (the
// other bit of each) - a stride of -1 dword, conflict-free - and the plane staged is channel perm[c]'s; the stages between are the plain ones.
template <bool BWD, class... M>
__global__ __launch_bounds__(TPB) void bilin_chain_lds_k(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ theta,
                                                         int C, int H, int W, int nstage, M... mir) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int HW = H * W;
    float* A = (float*)smem;
    float* B = A + HW;
    const int n = blockIdx.x / C;
    const unsigned mb = mirror_bits(n, mir...);
    const bool m_load = mb & (BWD ? MIRROR_OUT : MIRROR_IN), m_store = mb & (BWD ? MIRROR_IN : MIRROR_OUT);
    const float* sp = src + (sizeof...(M) ? (size_t)n * C + mirror_plane(mb, blockIdx.x % C, mir...) : (size_t)blockIdx.x) * HW;
    float* dp = dst + (size_t)blockIdx.x * HW;
    for (int i = threadIdx.x; i < HW; i += TPB) A[i] = sp[m_load ? mirror_index(i, W) : i];
    __syncthreads();
    for (int k = 0; k < nstage; ++k) {
        const float* th = theta + ((size_t)n * nstage + (BWD ? nstage - 1 - k : k)) * 6;
        const BilinStage m = bilin_stage(th, W, H);
        BilinBox box;
        if (BWD) box = bilin_box(th, W, H);
        const bool last = k == nstage - 1;
        for (int i = threadIdx.x; i < HW; i += TPB) {
            const int py = i / W, px = i % W;
            float v;
            if (BWD) v = bilin_gather(A, m, box, W, H, px, py);
            else v = bilin_sample(A, m, W, H, px, py);
            if (last) dp[m_store ? py * W + (W - 1 - px) : i] = v; else B[i] = v;
        }
        __syncthreads();
        float* t = A; A = B; B = t;
    }
}
// A plane beyond the LDS budget (the 256x256 images warp.affine may be handed): one stage per launch, from and to global memory
template <bool BWD>
__global__ __launch_bounds__(TPB) void bilin_stage_global_k(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ theta,
                                                            int C, int H, int W, int nstage, int s, int tiles) {
    const int HW = H * W;
    const int plane = blockIdx.x / tiles, i = (blockIdx.x % tiles) * TPB + threadIdx.x;
    if (i >= HW) return;
    const float* th = theta + ((size_t)(plane / C) * nstage + s) * 6;
    const BilinStage m = bilin_stage(th, W, H);
    const float* sp = src + (size_t)plane * HW;
    const int py = i / W, px = i % W;
    float v;
    if (BWD) {
        const BilinBox box = bilin_box(th, W, H);
        v = bilin_gather(sp, m, box, W, H, px, py);
    } else {
        v = bilin_sample(sp, m, W, H, px, py);
    }
    dst[(size_t)plane * HW + i] = v;
}
}  // namespace

// src and dst must not overlap.  Planes within the LDS budget (2 * H * W * 4 <= 150 KB: every heat-map size) take one launch and allocate
// nothing.  Larger planes run stage by stage from global memory; with more than one stage they go through one scratch tensor allocated
// and freed in stream order - never inside a stream capture, where such planes are refused (UDAPOSE_ERR_UNSUPPORTED).
static int bilinear_dispatch(hipStream_t s, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage, int backward,
                             const unsigned char* mirror, const int* perm) {
    if (nstage < 1 || nstage > 8 || N <= 0 || C <= 0 || H <= 0 || W <= 0 || !src || !dst || !theta) return UDAPOSE_ERR_ARG;
    if ((long long)H * W > (1ll << 26) || (long long)N * C >= (1ll << 31)) return UDAPOSE_ERR_ARG;
    const int HW = H * W;
    const size_t lds = (size_t)HW * 2 * sizeof(float);
    if (lds <= 150 * 1024) {
        max_dynamic_lds<bilin_chain_lds_k<false>>(150 * 1024);
        max_dynamic_lds<bilin_chain_lds_k<true>>(150 * 1024);
        const unsigned bytes = (unsigned)((lds + 15) & ~(size_t)15);
        if (mirror) {
            const Mirror mir = {mirror, perm};
            max_dynamic_lds<bilin_chain_lds_k<false, Mirror>>(150 * 1024);
            max_dynamic_lds<bilin_chain_lds_k<true, Mirror>>(150 * 1024);
            if (backward) hipLaunchKernelGGL((bilin_chain_lds_k<true, Mirror>), dim3(N * C), dim3(TPB), bytes, s, src, dst, theta, C, H, W, nstage, mir);
            else hipLaunchKernelGGL((bilin_chain_lds_k<false, Mirror>), dim3(N * C), dim3(TPB), bytes, s, src, dst, theta, C, H, W, nstage, mir);
            return udapose_check_launch();
        }
        if (backward) hipLaunchKernelGGL(bilin_chain_lds_k<true>, dim3(N * C), dim3(TPB), bytes, s, src, dst, theta, C, H, W, nstage);
        else hipLaunchKernelGGL(bilin_chain_lds_k<false>, dim3(N * C), dim3(TPB), bytes, s, src, dst, theta, C, H, W, nstage);
        return udapose_check_launch();
    }
    if (mirror) return UDAPOSE_ERR_UNSUPPORTED;        // (the stage-by-stage global form has no mirrored counterpart)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) return UDAPOSE_ERR_LAUNCH;
    if (cap != hipStreamCaptureStatusNone) return UDAPOSE_ERR_UNSUPPORTED;
    const int tiles = (HW + TPB - 1) / TPB;
    if ((long long)N * C * tiles >= (1ll << 31)) return UDAPOSE_ERR_ARG;
    float* scratch = nullptr;
    if (nstage > 1 && hipMallocAsync((void**)&scratch, (size_t)N * C * HW * sizeof(float), s) != hipSuccess) return UDAPOSE_ERR_LAUNCH;
    const float* in = src;
    int rc = UDAPOSE_OK;
    for (int k = 0; k < nstage && rc == UDAPOSE_OK; ++k) {
        float* out = (nstage - 1 - k) % 2 == 0 ? dst : scratch;        // (the stages alternate between the two; the last one writes dst)
        const int st = backward ? nstage - 1 - k : k;
        if (backward) hipLaunchKernelGGL(bilin_stage_global_k<true>, dim3(N * C * tiles), dim3(TPB), 0, s, in, out, theta, C, H, W, nstage, st, tiles);
        else hipLaunchKernelGGL(bilin_stage_global_k<false>, dim3(N * C * tiles), dim3(TPB), 0, s, in, out, theta, C, H, W, nstage, st, tiles);
        rc = udapose_check_launch();
        in = out;
    }
    if (scratch && hipFreeAsync(scratch, s) != hipSuccess && rc == UDAPOSE_OK) rc = UDAPOSE_ERR_LAUNCH;
    return rc;
}
int affine_warp_chain_bilinear(hipStream_t s, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage, int backward) {
    return bilinear_dispatch(s, src, dst, theta, N, C, H, W, nstage, backward, nullptr, nullptr);
}
// planes beyond the LDS budget: UDAPOSE_ERR_UNSUPPORTED
int affine_warp_chain_bilinear_mirror(hipStream_t s, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage,
                                      int backward, const unsigned char* mirror, const int* perm) {
    if (!mirror) return UDAPOSE_ERR_ARG;
    return bilinear_dispatch(s, src, dst, theta, N, C, H, W, nstage, backward, mirror, perm);
}

// mean over k re-warped teacher views (train_human.py:361-372 with --k > 1: `torch.mean(recons, dim=0)`): the k values of an element
// are added in view order in fp32 and divided by k, as ATen's mean over the leading dimension does for a handful of rows
struct ViewPtrs { const float* p[8]; };
__global__ void mean_views_k(ViewPtrs v, int k, float* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float a = v.p[0][i];
        for (int j = 1; j < k; ++j) a += v.p[j][i];
        dst[i] = a / (float)k;
    }
}
int affine_mean_views(hipStream_t s, const float* const* srcs, int k, float* dst, size_t n) {
    if (k < 1 || k > 8 || !srcs || !dst) return UDAPOSE_ERR_ARG;
    ViewPtrs v;
    for (int j = 0; j < 8; ++j) v.p[j] = j < k ? srcs[j] : nullptr;
    for (int j = 0; j < k; ++j) if (!v.p[j]) return UDAPOSE_ERR_ARG;
    size_t g = (n + 255) / 256;
    hipLaunchKernelGGL(mean_views_k, dim3((unsigned)(g > 2048 ? 2048 : (g < 1 ? 1 : g))), dim3(256), 0, s, v, k, dst, n);
    return udapose_check_launch();
}
