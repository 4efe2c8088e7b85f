// The instance layer behind predict() (fp32 only: both builds of the library export identical code).
//   pose_rescore_k : a pose's score from its key-point confidences and its box score, its area, whether it is refused, and the walk order
//                    (descending score, ties by ascending index, refused poses last): pose_pair.h's rank by counting, keys staged once in LDS
//   oks_matrix_k   : object-key-point similarity of every pair of a tile, key points staged once in LDS (the per-joint term and the
//                    visibility word are pose_pair.h's, shared with pose_ap.hip); the fp32 matrix (self or rectangular form)
//                    and / or, for the self form, the suppression bit mask, one wave64 __ballot per 64-bit word
//   nms_sweep_k    : the greedy walk by one wave: lane l holds word l of the removed set in a register, membership is a cross-lane read,
//                    the mask rows of the next 2 * SWEEP_GROUP poses of the order are in flight while the walk decides the current one
// No atomics; every sum is added in ascending k: the same bits on every run.  M <= 4096 poses (64 mask words = one per lane), K <= 64.
#include <float.h>
#include "losses.h"
#include "pose_pair.h"
#include "pose_ws.h"

// no FMA contraction: oks(i, j) and oks(j, i) are the same expression tree on swapped operands, and stay the same bits
#pragma clang fp contract(off)

namespace {
constexpr int MAX_M = UDAPOSE_NMS_MAX_POSES;

// ---------------------------------------------------------------------------------------------------------------- rescoring and the order

struct PoseScore { float score, area; bool refused; };

// score = (sum of conf > vis_thr, ascending k) / their count (0 for none) * box_score; refused: status != 0, a non-finite coordinate, area
// or score, area <= 0
__device__ __forceinline__ PoseScore pose_score(int m, const float* __restrict__ kp, const float* __restrict__ conf, const float* __restrict__ boxes,
                                                const unsigned char* __restrict__ status, const float* __restrict__ box_score, float vis_thr, int K) {
    PoseScore r;
    const float* c = conf + (size_t)m * K;
    const float* p = kp + (size_t)m * K * 2;
    float sum = 0.f;
    int n = 0;
    bool bad = false;
    // eight joints' loads in flight at a time (the last stretch re-reads joint K - 1 and drops it); the sum stays in ascending k
    for (int k0 = 0; k0 < K; k0 += 8) {
        float v[8];
        float2 xy[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = min(k0 + e, K - 1);
            v[e] = c[k];
            xy[e] = ((const float2*)p)[k];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (k0 + e < K) {
                if (v[e] > vis_thr) { sum += v[e]; ++n; }
                bad |= !finite_f(xy[e].x) || !finite_f(xy[e].y);
            }
        }
    }
    const float kscore = n ? sum / (float)n : 0.f;
    r.score = kscore * (box_score ? box_score[m] : 1.f);
    r.area = boxes[(size_t)m * 5 + 2] * boxes[(size_t)m * 5 + 3];
    r.refused = bad || (status && status[m] != 0) || !finite_f(r.area) || !(r.area > 0.f) || !finite_f(r.score);
    return r;
}

__global__ __launch_bounds__(RANK_TPB) void pose_rescore_k(const float* __restrict__ kp, const float* __restrict__ conf, const float* __restrict__ boxes,
                                                           const unsigned char* __restrict__ status, const float* __restrict__ box_score,
                                                           const float* __restrict__ vis_thr_dev, int M, int K, float* __restrict__ score,
                                                           int* __restrict__ order, float* __restrict__ area, unsigned char* __restrict__ refused) {
    __shared__ __attribute__((aligned(16))) unsigned int keys[MAX_M];
    __shared__ int part[RANK_PARTS][RANK_ITEMS];
    const int t = threadIdx.x, i0 = blockIdx.x * RANK_ITEMS;
    const float vis_thr = vis_thr_dev[0];
    const int Mpad = rank_padded(M);
    // every block forms all M keys (M K confidences and 2 M K coordinates out of L2); it writes the results of its own poses
    for (int m = t; m < Mpad; m += RANK_TPB) {
        unsigned int key = POSE_KEY_REFUSED;
        if (m < M) {
            const PoseScore r = pose_score(m, kp, conf, boxes, status, box_score, vis_thr, K);
            key = order_key(r.score, r.refused);
            if (m >= i0 && m < i0 + RANK_ITEMS) {
                score[m] = r.score;
                area[m] = r.area;
                refused[m] = r.refused ? 1 : 0;
            }
        }
        keys[m] = key;
    }
    __syncthreads();
    const int p = t & (RANK_ITEMS - 1), q = t / RANK_ITEMS, i = i0 + p;
    const unsigned int ki = i < M ? keys[i] : 0u;
    const int per = Mpad / RANK_PARTS;
    const int rank = rank_finish(part, q, p, rank_count(keys + q * per, per, q * per, ki, i));
    if (q == 0 && i < M) order[rank] = i;
}

// ---------------------------------------------------------------------------------------------------------------- the OKS matrix and the mask
constexpr int OK_TPB = 256, OK_TJ = 64, OK_TI = 32, OK_ROWS = 4;      // a 32 x 64 tile; a wave takes 8 rows, 4 at a time, lane = column
constexpr int OK_WAVE_ROWS = OK_TI / (OK_TPB / 64);

static inline size_t oks_lds_bytes(int K) {
    return (size_t)(OK_TJ + OK_TI) * K * sizeof(float2) + (size_t)K * sizeof(float) + (size_t)OK_TJ * sizeof(u64) +
           (size_t)(OK_TJ + OK_TI) * (2 * sizeof(float) + sizeof(int));
}

// Self form (RECT = false): e_k = d2 / v_k / ((area_i + area_j) * 0.5f + FLT_EPSILON) * 0.5f, oks = sum_k expf(-e_k) / K.
// Rectangular form: A = area_b + FLT_EPSILON, the sum over visible_b > 0 divided by their count (0 for none).
template <bool RECT>
__global__ __launch_bounds__(OK_TPB) void oks_matrix_k(const float* __restrict__ kp_a, const float* __restrict__ area_a, const float* __restrict__ kp_b,
                                                       const float* __restrict__ area_b, const float* __restrict__ visible_b,
                                                       const float* __restrict__ sigmas, const int* __restrict__ frame,
                                                       const unsigned char* __restrict__ refused, const float* __restrict__ oks_thr_dev, int Ma, int Mb,
                                                       int K, int W, float* __restrict__ out, u64* __restrict__ mask) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    float2* tj = (float2*)lds;                         // [K][64]: lane-consecutive
    float2* ti = tj + (size_t)OK_TJ * K;               // [32][K]: a row's key points, read as broadcasts
    u64* vis_j = (u64*)(ti + (size_t)OK_TI * K);       // [64] bit k = joint k of column j counts
    float* vk = (float*)(vis_j + OK_TJ);               // [K] (2 sigma_k)^2
    float* area_j = vk + K;                            // [64]
    float* area_i = area_j + OK_TJ;                    // [32]
    int* frame_j = (int*)(area_i + OK_TI);             // [64]
    int* frame_i = frame_j + OK_TJ;                    // [32]
    float* ok_j = (float*)(frame_i + OK_TI);           // [64] 1 = in range and not refused
    float* ok_i = ok_j + OK_TJ;                        // [32]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int j0 = blockIdx.x * OK_TJ, i0 = blockIdx.y * OK_TI;
    // the tile's key points, once: a pose outside the range is staged as zeros and never written
    for (int e = t; e < OK_TJ * K; e += OK_TPB) {
        const int jj = e / K, k = e - jj * K, j = j0 + jj;
        tj[k * OK_TJ + jj] = j < Mb ? ((const float2*)kp_b)[(size_t)j * K + k] : make_float2(0.f, 0.f);
    }
    for (int e = t; e < OK_TI * K; e += OK_TPB) {
        const int ii = e / K, i = i0 + ii;
        ti[e] = i < Ma ? ((const float2*)kp_a)[(size_t)i * K + (e - ii * K)] : make_float2(0.f, 0.f);
    }
    for (int k = t; k < K; k += OK_TPB) vk[k] = oks_sigma_sq(sigmas[k]);
    if (t < OK_TJ) {
        const int j = j0 + t;
        const bool in = j < Mb;
        area_j[t] = in ? area_b[j] : 1.f;
        frame_j[t] = (in && frame) ? frame[j] : 0;
        ok_j[t] = (in && !(refused && refused[j])) ? 1.f : 0.f;
        vis_j[t] = (RECT && visible_b) ? (in ? visible_bits(visible_b + (size_t)j * K, K) : 0ull) : ~0ull;
    } else if (t < OK_TJ + OK_TI) {
        const int ii = t - OK_TJ, i = i0 + ii;
        const bool in = i < Ma;
        area_i[ii] = (in && area_a) ? area_a[i] : 1.f;
        frame_i[ii] = (in && frame) ? frame[i] : 0;
        ok_i[ii] = (in && !(refused && refused[i])) ? 1.f : 0.f;
    }
    __syncthreads();
    const int j = j0 + lane;
    const float aj = area_j[lane];
    const u64 vb = vis_j[lane];
    const int fj = frame_j[lane];
    const bool okj = ok_j[lane] != 0.f;
    const float thr = mask ? oks_thr_dev[0] : 0.f;
    const int nvis = RECT ? __popcll(vb & full_bits(K)) : K;
#pragma unroll 1
    for (int r0 = wave * OK_WAVE_ROWS; r0 < (wave + 1) * OK_WAVE_ROWS; r0 += OK_ROWS) {
        float A[OK_ROWS], acc[OK_ROWS];
#pragma unroll
        for (int r = 0; r < OK_ROWS; ++r) {
            A[r] = RECT ? oks_rect_area(aj) : (area_i[r0 + r] + aj) * 0.5f + FLT_EPSILON;
            acc[r] = 0.f;
        }
        // (this loop and the staging above are written out here and in ap_match_k: through one shared function of pose_pair.h the self
        // form measured 0.2 to 0.3 us slower at M <= 512, profiles/pose_once.txt; the term itself is the one of pose_pair.h)
        for (int k = 0; k < K; ++k) {
            const float2 pj = tj[k * OK_TJ + lane];
            const float v = vk[k];
            const bool use = !RECT || ((vb >> k) & 1ull);
#pragma unroll
            for (int r = 0; r < OK_ROWS; ++r) {
                const float term = oks_term(ti[(r0 + r) * K + k], pj, v, A[r]);      // (pose_pair.h: the expression pose_ap.hip matches with)
                if (use) acc[r] += term;
            }
        }
#pragma unroll
        for (int r = 0; r < OK_ROWS; ++r) {
            const int i = i0 + r0 + r;
            const float oks = RECT ? oks_rect_mean(acc[r], nvis) : acc[r] / (float)K;
            if (i < Ma) {      // (uniform in the wave: all 64 lanes reach the ballot)
                if (out && j < Mb) out[(size_t)i * Mb + j] = oks;
                if (!RECT && mask) {
                    const bool bit = okj && ok_i[r0 + r] != 0.f && fj == frame_i[r0 + r] && i != j && oks > thr;
                    const u64 word = __ballot(bit);
                    if (lane == 0) mask[(size_t)i * W + blockIdx.x] = word;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the greedy walk
constexpr int SWEEP_GROUP = 16;      // steps between two batches of row loads; a 64-entry stretch of the order is four groups
constexpr int ORD_REFUSED = 0x10000;

// The rows to load are known from `order` before the walk starts: every load is issued 2 * SWEEP_GROUP steps before its row is used,
// without a branch round it (a padded order, clamped lanes), so the walk never waits for a load it has just issued.
template <bool SBY>
__global__ __launch_bounds__(64) void nms_sweep_k(const u64* __restrict__ mask, const int* __restrict__ order, const unsigned char* __restrict__ refused,
                                                  int M, int W, unsigned char* __restrict__ keep, int* __restrict__ n_keep,
                                                  int* __restrict__ suppressed_by) {
    __shared__ int ord[MAX_M + 64];      // pose index | ORD_REFUSED; padded past M with refused entries that name row 0
    __shared__ int sby[SBY ? MAX_M : 1];
    const int lane = threadIdx.x;
    const int Mpad = (M + 63) / 64 * 64 + 64;
    for (int t = lane; t < Mpad; t += 64) {
        int e = ORD_REFUSED;
        if (t < M) {
            int i = order[t];
            const bool bad = (unsigned int)i >= (unsigned int)M;      // (an order that is no permutation of [0, M): the entry is passed over)
            if (bad) i = 0;
            e = i | ((bad || (refused && refused[i])) ? ORD_REFUSED : 0);
            if (SBY) sby[t] = -1;
        }
        ord[t] = e;
    }
    __syncthreads();
    // row `ord[t]` of the mask, word `lane` (a lane past the row's words reads its last word: its bits are never looked at, and are
    // dropped where suppressed_by uses them): the address depends on the order alone, never on the walk
    const unsigned int row_bytes = (unsigned int)W * 8u, word_off = (unsigned int)min(lane, W - 1) * 8u;      // (M W 8 <= 2 MiB)
    const u64 live = lane < W ? ~0ull : 0ull;
    auto row = [&](int e) -> u64 { return *(const u64*)((const char*)mask + ((unsigned int)(e & (ORD_REFUSED - 1)) * row_bytes + word_off)); };
    // the removed set: word `lane`, as two halves.  A step is scalar but for its last two instructions, and has no branch: the entry, the
    // word of the removed set that holds its bit (two cross-lane reads), `gone` = that bit or the refused flag, and the row ANDed in under
    // a mask that is all ones when the pose is kept.  kept = neither removed nor refused, at the end.
    unsigned int rlo = 0u, rhi = 0u;
    // four sets of SWEEP_GROUP rows: group q of a stretch walks set q, and opens by issuing the loads of the group two on into the set
    // the group before it left (a scheduling barrier keeps them there: left alone, the compiler sinks every load to just ahead of the
    // wait for it - and into the next basic block where there is one, so a stretch is walked whole, its padding included, without a
    // branch).  2 * SWEEP_GROUP steps pass before a row is used: more than it takes to arrive.
    u64 buf[4][SWEEP_GROUP];
#pragma unroll
    for (int d = 0; d < 2 * SWEEP_GROUP; ++d) buf[d / SWEEP_GROUP][d % SWEEP_GROUP] = row(ord[d]);      // (in the order of their use)
    int next = ord[lane];
    for (int g = 0; g < M; g += 64) {
        const int mine = next;      // the 64 entries of this stretch, one per lane, and those of the one behind it
        next = ord[g + 64 + lane];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int d = 0; d < SWEEP_GROUP; ++d)
                buf[(q + 2) & 3][d] = row(__builtin_amdgcn_readlane(q < 2 ? mine : next, ((q + 2) * SWEEP_GROUP + d) & 63));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int d = 0; d < SWEEP_GROUP; ++d) {
                const u64 cur = buf[q][d];
                const unsigned int e = (unsigned int)__builtin_amdgcn_readlane(mine, q * SWEEP_GROUP + d);
                const unsigned int wlo = (unsigned int)__builtin_amdgcn_readlane((int)rlo, (int)(e >> 6)),
                                   whi = (unsigned int)__builtin_amdgcn_readlane((int)rhi, (int)(e >> 6));      // (the lane is e's bits 6 .. 11)
                const unsigned int gone = (unsigned int)((((u64)whi << 32) | wlo) >> (e & 63u)) | (e >> 16);
                const unsigned int keeps = 0u - (~gone & 1u);      // (uniform) all ones: kept, it removes what row i names
                if (SBY && keeps) {
                    u64 fresh = cur & live & ~(((u64)rhi << 32) | rlo);
                    while (fresh) {
                        const int b = __ffsll((long long)fresh) - 1;
                        sby[lane * 64 + b] = (int)(e & (ORD_REFUSED - 1));
                        fresh &= fresh - 1ull;
                    }
                }
                rlo |= (unsigned int)cur & keeps;
                rhi |= (unsigned int)(cur >> 32) & keeps;
            }
        }
    }
    __syncthreads();
    int total = 0;
    for (int g = 0; g < M; g += 64) {
        const unsigned int wlo = (unsigned int)__builtin_amdgcn_readlane((int)rlo, g >> 6), whi = (unsigned int)__builtin_amdgcn_readlane((int)rhi, g >> 6);
        const int m = g + lane;
        if (m < M) {
            const bool k = !(((((u64)whi << 32) | wlo) >> lane) & 1ull) && !(refused && refused[m]);
            keep[m] = k ? 1 : 0;
            total += k;
            if (SBY) suppressed_by[m] = sby[m];
        }
    }
    total = wave_sum(total);
    if (lane == 0) n_keep[0] = total;
}

bool bad_sizes(int M, int K) { return bad_poses(M) || bad_keypoints(K); }
}  // namespace

int pose_rescore(hipStream_t s, const float* kp, const float* conf, const float* boxes, const unsigned char* status, const float* box_score,
                 const float* vis_thr, int M, int K, float* score, int* order, float* area, unsigned char* refused) {
    if (!kp || !conf || !boxes || !vis_thr || !score || !order || !area || !refused || bad_sizes(M, K)) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(pose_rescore_k, dim3((M + RANK_ITEMS - 1) / RANK_ITEMS), dim3(RANK_TPB), 0, s, kp, conf, boxes, status, box_score, vis_thr, M, K,
                       score, order, area, refused);
    return udapose_check_launch();
}

int oks_matrix(hipStream_t s, const float* kp_a, const float* area_a, int Ma, const float* kp_b, const float* area_b, const float* visible_b, int Mb,
               int K, const float* sigmas, const int* frame_idx, const unsigned char* refused, const float* oks_thr, float* out,
               unsigned long long* mask) {
    const bool rect = kp_b != nullptr;
    if (!kp_a || (!rect && !area_a) || !sigmas || (!out && !mask) || bad_sizes(Ma, K)) return UDAPOSE_ERR_ARG;
    if (rect ? (!area_b || mask || frame_idx || refused || bad_sizes(Mb, K)) : (area_b || visible_b || Mb != Ma)) return UDAPOSE_ERR_ARG;
    if (mask && !oks_thr) return UDAPOSE_ERR_ARG;
    const dim3 grid((Mb + OK_TJ - 1) / OK_TJ, (Ma + OK_TI - 1) / OK_TI);
    const int W = (Ma + 63) / 64;
    if (rect)
        hipLaunchKernelGGL(oks_matrix_k<true>, grid, dim3(OK_TPB), oks_lds_bytes(K), s, kp_a, area_a, kp_b, area_b, visible_b, sigmas, nullptr, nullptr,
                           nullptr, Ma, Mb, K, W, out, nullptr);
    else
        hipLaunchKernelGGL(oks_matrix_k<false>, grid, dim3(OK_TPB), oks_lds_bytes(K), s, kp_a, area_a, kp_a, area_a, nullptr, sigmas, frame_idx, refused,
                           oks_thr, Ma, Ma, K, W, out, mask);
    return udapose_check_launch();
}

int pose_nms_sweep(hipStream_t s, const unsigned long long* mask, const int* order, const unsigned char* refused, int M, unsigned char* keep,
                   int* n_keep, int* suppressed_by) {
    if (!mask || !order || !keep || !n_keep || bad_poses(M)) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(suppressed_by ? nms_sweep_k<true> : nms_sweep_k<false>, dim3(1), dim3(64), 0, s, mask, order, refused, M, (M + 63) / 64, keep,
                       n_keep, suppressed_by);
    return udapose_check_launch();
}

size_t pose_nms_ws_bytes(int M) { return bad_poses(M) ? 0 : PoseNmsWs(nullptr, M).bytes; }

int pose_nms(hipStream_t s, const float* kp, const float* conf, const float* boxes, const int* frame_idx, const unsigned char* status,
             const float* box_score, const float* sigmas, const float* vis_thr, const float* oks_thr, int M, int K, void* ws, float* score, int* order,
             unsigned char* keep, int* n_keep, int* suppressed_by, float* oks_out) {
    // every check ahead of the first launch: an error leaves nothing written
    if (!kp || !conf || !boxes || !sigmas || !vis_thr || !oks_thr || !ws || !score || !order || !keep || !n_keep || bad_sizes(M, K))
        return UDAPOSE_ERR_ARG;
    if ((uintptr_t)ws & 7u) return UDAPOSE_ERR_ARG;
    const PoseNmsWs w(ws, M);
    int e = pose_rescore(s, kp, conf, boxes, status, box_score, vis_thr, M, K, score, order, w.area, w.refused);
    if (e != UDAPOSE_OK) return e;
    e = oks_matrix(s, kp, w.area, M, nullptr, nullptr, nullptr, M, K, sigmas, frame_idx, w.refused, oks_thr, oks_out, w.mask);
    if (e != UDAPOSE_OK) return e;
    return pose_nms_sweep(s, w.mask, order, w.refused, M, keep, n_keep, suppressed_by);
}
