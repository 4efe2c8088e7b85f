// Evaluation meter kernels (fp32 coordinates and maps, int64 state: both builds of the library export identical code).
//   pck_accumulate_k          : decoded coordinates [B][K][2] -> hits per threshold, visible count, fixed-point end-point error
//   pck_accumulate_heatmaps_k : the same from the two heat-map tensors, whose arg-max it reduces itself (one launch for two arg-max
//                               sweeps + PCK)
// Both ADD to state [K][T + 3] (columns: include/udapose.h).  Every accumulation is an integer add - private counters, wave shuffles, LDS
// integer atomics, then one 64-bit integer atomic per touched column - so the state after a set is the same bits whatever the batch
// split, the grid shape or the order of arrival.  No floating-point atomics, no scratch, no host synchronisation: capturable.
// The per-pair arithmetic is stated once (pck_pair, pck_first_hit) and never contracted into FMAs: every product, sum, quotient and root
// is one correctly rounded fp32 operation, which tests/helpers/pck_curve_ref.py restates in numpy bit for bit.
#include <math.h>
#include "losses.h"

#pragma clang fp contract(off)

namespace {
constexpr int TPB = 256;
constexpr int MAX_T = UDAPOSE_PCK_MAX_THRESHOLDS;
constexpr float EPE_LIMIT = 70368744177664.f;      // 2^46 px: beyond it (or NaN) the fixed-point value is not taken

struct PckPair {
    float d;             // the normalised distance the thresholds are compared with
    long long q;         // llrintf(e * 65536): the end-point error in 2^-16 px
    int counted;         // the pair is visible
    int nonfinite;       // ... and its e is not finite (q = 0 then)
};

// One (b, k) pair.  Without norm, pck_k's expression (x over the HEIGHT term: the reference's pairing, kept); with norm, the pixel distance
// over the sample's length, and a length that is not finite and > 0 hides the sample's joints.
__device__ __forceinline__ PckPair pck_pair(float px, float py, float tx, float ty, bool visible, const float* __restrict__ norm, size_t b,
                                            float nh, float nw) {
    PckPair r = {0.f, 0, 0, 0};
    const float ex = px - tx, ey = py - ty;
    const float e = sqrtf(ex * ex + ey * ey);
    if (norm) {
        const float n = norm[b];
        if (!(n > 0.f && n < INFINITY)) visible = false;
        r.d = e / n;
    } else {
        const float dx = px / nh - tx / nh, dy = py / nw - ty / nw;
        r.d = sqrtf(dx * dx + dy * dy);
    }
    if (!visible) return r;
    r.counted = 1;
    if (e < EPE_LIMIT) r.q = llrintf(e * (float)UDAPOSE_PCK_EPE_SCALE);      // (a power of two: the product is exact)
    else r.nonfinite = 1;
    return r;
}

// The first threshold hit: the smallest j with d < thr[j], T where there is none (a NaN d hits nothing).  thr ascends strictly, so
// thresholds j >= the result are exactly the ones the T independent compares d < thr[j] would hit.
__device__ __forceinline__ int pck_first_hit(float d, const float* thr, int T) {
    int lo = 0, hi = T;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d < thr[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Block (k, y): joint k, samples b = y * TPB + lane, + gridDim.y * TPB, ...  A lane keeps count / nonfinite / epe_q in registers and drops
// each pair's first hit into an LDS histogram; the waves' sums meet in LDS, column j of row k gets the histogram's prefix sum.
__global__ __launch_bounds__(TPB) void pck_accumulate_k(const float* __restrict__ pred, const float* __restrict__ gt,
                                                        const unsigned char* __restrict__ visible, const float* __restrict__ norm, int B, int K,
                                                        float nh, float nw, const float* __restrict__ thr, int T,
                                                        long long* __restrict__ state) {
    __shared__ float s_thr[MAX_T];
    __shared__ int s_first[MAX_T + 1];
    __shared__ int s_cnt, s_nf;
    __shared__ unsigned long long s_q;
    const int k = blockIdx.x, tid = threadIdx.x;
    if (tid <= T) s_first[tid] = 0;
    if (tid < T) s_thr[tid] = thr[tid];
    if (tid == 0) { s_cnt = 0; s_nf = 0; s_q = 0ull; }
    __syncthreads();
    int cnt = 0, nf = 0;
    long long q = 0;
    for (size_t b = (size_t)blockIdx.y * TPB + tid; b < (size_t)B; b += (size_t)gridDim.y * TPB) {
        const size_t r = b * (size_t)K + (size_t)k;
        const float tx = gt[2 * r], ty = gt[2 * r + 1];
        const bool vis = visible ? visible[r] != 0 : (tx > 1.f && ty > 1.f);
        const PckPair p = pck_pair(pred[2 * r], pred[2 * r + 1], tx, ty, vis, norm, b, nh, nw);
        if (p.counted) {
            ++cnt;
            nf += p.nonfinite;
            q += p.q;
            atomicAdd(&s_first[pck_first_hit(p.d, s_thr, T)], 1);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        nf += __shfl_xor(nf, o, 64);
        q += __shfl_xor(q, o, 64);
    }
    if ((tid & 63) == 0) {
        if (cnt) atomicAdd(&s_cnt, cnt);
        if (nf) atomicAdd(&s_nf, nf);
        if (q) atomicAdd(&s_q, (unsigned long long)q);
    }
    __syncthreads();
    if (tid < T + 3) {
        long long v;
        if (tid < T) {
            int h = 0;
            for (int i = 0; i <= tid; ++i) h += s_first[i];
            v = h;
        } else {
            v = tid == T ? (long long)s_cnt : (tid == T + 1 ? (long long)s_q : (long long)s_nf);
        }
        counter_add(state + (size_t)k * (T + 3) + tid, v);
    }
}

// One work-group per (b, k): both planes are swept once (16-byte loads where the planes allow), each arg-max reduced by hm_block_best;
// every lane then holds the pair, lane j < T adds its own threshold's hit and lanes T .. T+2 the other three columns.
template <bool VEC>
__global__ __launch_bounds__(TPB) void pck_accumulate_heatmaps_k(const float* __restrict__ out, const float* __restrict__ target,
                                                                 const float* __restrict__ norm, int K, int H, int W, float nh, float nw,
                                                                 const float* __restrict__ thr, int T, long long* __restrict__ state,
                                                                 float* __restrict__ preds) {
    __shared__ float sv[TPB / 64];
    __shared__ int si[TPB / 64];
    __shared__ float s_thr[MAX_T];
    const size_t r = blockIdx.x;
    const int tid = threadIdx.x, HW = H * W;
    if (tid < T) s_thr[tid] = thr[tid];           // (published by hm_block_best's barriers)
    const float* po = out + r * (size_t)HW;
    const float* pt = target + r * (size_t)HW;
    float ov = -INFINITY, tv = -INFINITY;
    int oi = 0x7fffffff, ti = 0x7fffffff;
    if (VEC) {
#pragma unroll 2
        for (int i = tid * 4; i < HW; i += TPB * 4) {
            const f32x4 a = *(const f32x4*)(po + i), g = *(const f32x4*)(pt + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (hm_better(a[e], i + e, ov, oi)) { ov = a[e]; oi = i + e; }
                if (hm_better(g[e], i + e, tv, ti)) { tv = g[e]; ti = i + e; }
            }
        }
    } else {
        for (int i = tid; i < HW; i += TPB) {
            const float a = po[i], g = pt[i];
            if (hm_better(a, i, ov, oi)) { ov = a; oi = i; }
            if (hm_better(g, i, tv, ti)) { tv = g; ti = i; }
        }
    }
    hm_block_best<TPB / 64>(ov, oi, sv, si);
    hm_block_best<TPB / 64>(tv, ti, sv, si);
    const bool opos = ov > 0.f, tpos = tv > 0.f;
    const float px = opos ? (float)(oi % W) : 0.f, py = opos ? (float)(oi / W) : 0.f;
    const float tx = tpos ? (float)(ti % W) : 0.f, ty = tpos ? (float)(ti / W) : 0.f;
    if (tid == 0 && preds) { preds[r * 2] = px; preds[r * 2 + 1] = py; }
    const size_t b = r / (size_t)K;
    const int k = (int)(r - b * (size_t)K);
    const PckPair p = pck_pair(px, py, tx, ty, tx > 1.f && ty > 1.f, norm, b, nh, nw);
    if (!p.counted || tid >= T + 3) return;
    long long v;
    if (tid < T) v = tid >= pck_first_hit(p.d, s_thr, T) ? 1 : 0;
    else v = tid == T ? 1 : (tid == T + 1 ? p.q : (long long)p.nonfinite);
    counter_add(state + (size_t)k * (T + 3) + tid, v);
}

int check_sizes(int B, int K, int T) {
    if (B < 1 || K < 1 || T < 1 || T > MAX_T) return UDAPOSE_ERR_ARG;
    if (K > UDAPOSE_PCK_MAX_KEYPOINTS) return UDAPOSE_ERR_UNSUPPORTED;
    if ((long long)B * K > 0x7fffffffLL) return UDAPOSE_ERR_ARG;
    return UDAPOSE_OK;
}
}  // namespace

int pck_accumulate(hipStream_t s, const float* pred, const float* gt, const unsigned char* visible, const float* norm, int B, int K, float nh,
                   float nw, const float* thr, int T, long long* state) {
    if (!pred || !gt || !thr || !state) return UDAPOSE_ERR_ARG;
    if (const int e = check_sizes(B, K, T)) return e;
    int gy = (B + TPB - 1) / TPB;
    if (gy > 32) gy = 32;
    hipLaunchKernelGGL(pck_accumulate_k, dim3((unsigned)K, (unsigned)gy), dim3(TPB), 0, s, pred, gt, visible, norm, B, K, nh, nw, thr, T, state);
    return udapose_check_launch();
}

int pck_accumulate_heatmaps(hipStream_t s, const float* out, const float* target, const float* norm, int B, int K, int H, int W,
                            const float* thr, int T, long long* state, float* preds) {
    if (!out || !target || !thr || !state || H < 1 || W < 1) return UDAPOSE_ERR_ARG;
    if (const int e = check_sizes(B, K, T)) return e;
    if ((long long)H * W > (1LL << 30)) return UDAPOSE_ERR_ARG;      // (the sweep's index stays an int)
    const float nh = (float)(H / 10.0), nw = (float)(W / 10.0);
    const bool vec = (H * W) % 4 == 0 && (((uintptr_t)out | (uintptr_t)target) & 15u) == 0;
    const dim3 grid((unsigned)(B * K));
    if (vec)
        hipLaunchKernelGGL(pck_accumulate_heatmaps_k<true>, grid, dim3(TPB), 0, s, out, target, norm, K, H, W, nh, nw, thr, T, state, preds);
    else
        hipLaunchKernelGGL(pck_accumulate_heatmaps_k<false>, grid, dim3(TPB), 0, s, out, target, norm, K, H, W, nh, nw, thr, T, state, preds);
    return udapose_check_launch();
}
