// What pose_nms.hip and pose_ap.hip share, each piece stated once:
//   the order   order_key, and the rank by counting over keys in LDS (rank_padded, rank_count, rank_finish) of pose_rescore_k, ap_rank_k, ap_sort_k
//   the pair    the per-joint term of object-key-point similarity, the rectangular form's area and mean and the visibility word
//               (visible_bits, full_bits) of oks_matrix_k and ap_match_k: the bits of udapose_oks_matrix are the bits the AP matching
//               compares with its thresholds.  (Each of the two stages its column tile [K][64] and adds its terms itself: the shared
//               form of those loops cost oks_matrix_k's self form 0.2 to 0.3 us, profiles/pose_once.txt)
//   the limits  bad_poses, bad_keypoints, and the finiteness test of the refusals
// What differs stays in the kernels: how a key is formed, which results a rank writes, tile streaming against one-shot staging.
// No FMA contraction inside: every step is one correctly rounded fp32 operation, whatever the including file's own setting.
#pragma once
#include <float.h>
#include "kth_select.h"

typedef unsigned long long u64;
constexpr unsigned int POSE_KEY_REFUSED = 0xffffffffu;

static inline bool bad_poses(int M) { return M < 1 || M > UDAPOSE_NMS_MAX_POSES; }
static inline bool bad_keypoints(int K) { return K < 1 || K > UDAPOSE_NMS_MAX_KEYPOINTS; }
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }

// a key that orders poses as the walks do: smaller = earlier.  Scores descending (-0 = +0); every refused pose shares the last key
__device__ __forceinline__ unsigned int order_key(float score, bool refused) {
    if (refused) return POSE_KEY_REFUSED;
    return ~hm_key_bits(__float_as_uint(score + 0.f));      // (0xffffffff would need the bits 0xffffffff, a NaN: refused)
}

// Rank by counting: a block of RANK_TPB threads ranks RANK_ITEMS items; thread group q = t / RANK_ITEMS counts over its share of the keys
// for item p = t % RANK_ITEMS.  The lanes of a wave read one LDS address (a broadcast).
constexpr int RANK_TPB = 1024, RANK_ITEMS = 256, RANK_PARTS = RANK_TPB / RANK_ITEMS;
// n keys padded with POSE_KEY_REFUSED (never ahead of an item: its index is past every item's) so that every part is a whole number of
// uint4; n <= 4096 stays <= 4096, a multiple of 16
__host__ __device__ constexpr int rank_padded(int n) { return (n + 4 * RANK_PARTS - 1) / (4 * RANK_PARTS) * (4 * RANK_PARTS); }
// #{e < n: (keys[e], base + e) is ahead of (ki, i)}: a smaller key, or an equal one with a smaller index.  keys: LDS, 16-byte aligned; 4 | n
__device__ __forceinline__ int rank_count(const unsigned int* keys, int n, int base, unsigned int ki, int i) {
    int count = 0;
    for (int e = 0; e < n; e += 4) {
        const uint4 kj = *(const uint4*)&keys[e];
        const int j = base + e;
        count += (kj.x < ki || (kj.x == ki && j < i)) + (kj.y < ki || (kj.y == ki && j + 1 < i)) + (kj.z < ki || (kj.z == ki && j + 2 < i)) +
                 (kj.w < ki || (kj.w == ki && j + 3 < i));
    }
    return count;
}
// item p's rank: the sum of its parts' counts (the order is total, so every rank is taken once).  Every thread of the block must reach the call
__device__ __forceinline__ int rank_finish(int (*part)[RANK_ITEMS], int q, int p, int count) {
    part[q][p] = count;
    __syncthreads();
    int rank = 0;
    for (int e = 0; e < RANK_PARTS; ++e) rank += part[e][p];
    return rank;
}

// v_k = (2 sigma_k)^2
__device__ __forceinline__ float oks_sigma_sq(float sigma) {
#pragma clang fp contract(off)
    const float s2 = 2.f * sigma;
    return s2 * s2;
}
// expf(-e_k), e_k = d2 / v_k / A * 0.5f, d2 = dx * dx + dy * dy
__device__ __forceinline__ float oks_term(float2 pi, float2 pj, float v, float A) {
#pragma clang fp contract(off)
    const float dx = pi.x - pj.x, dy = pi.y - pj.y;
    const float d2 = dx * dx + dy * dy;
    const float e = d2 / v / A * 0.5f;
    return expf(-e);
}
// the rectangular form (COCO's convention): the label's area, and the mean over the label's nvis visible joints, 0 for none
__device__ __forceinline__ float oks_rect_area(float area_b) { return area_b + FLT_EPSILON; }
__device__ __forceinline__ float oks_rect_mean(float acc, int nvis) { return nvis ? acc / (float)nvis : 0.f; }

// the low n bits, n in [0, 64]; and bit k = joint k of a pose counts: its visible[k] > 0
__device__ __forceinline__ u64 full_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }
__device__ __forceinline__ u64 visible_bits(const float* __restrict__ visible, int K) {
    u64 bits = 0ull;
    for (int k = 0; k < K; ++k) bits |= (u64)(visible[k] > 0.f) << k;
    return bits;
}
