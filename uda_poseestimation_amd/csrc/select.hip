// Joint selection by an order statistic over [N,K] fp32 rows: top-k (hard / small-loss key-point mining) of the per-(n,k) loss rows
// the sweeps of heatmap.hip produce, per-joint k-th value confidence masks, and a mask against a device-resident threshold.
// Small latency-bound kernels: one launch each, sums in double in a fixed order, no atomics on global memory.
#include "losses.h"
#include "kth_select.h"

namespace {
constexpr int SEL_TPB = 1024;       // topk_select_k: 16 waves, a wave per sample
constexpr int SEL_U = 2;            // ... and two samples of a wave in flight: N = 32 is one round of loads
constexpr int SEL_LDS = 1024;       // ... whose values the ordered sum reads back from LDS (4 KiB)
constexpr int KTH_TPB = 256;        // joint_kth_mask_k: one work-group per joint over n_pool values
constexpr int THR_TPB = 256;

// Per sample n (one wave, lane j = joint j): joint j is BETTER than joint i when key[j] > key[i] (largest; < otherwise) or the keys
// are equal and j < i, keys in hm_key's total order (NaN the largest).  rank(i) = number of candidates better than i; sel = rank < topk.
// A zero-factor row (wfac == 0 or mfac == 0) is no candidate when largest == 0 and is never selected; with largest != 0 it keeps its
// place in the order (its row is 0), so fewer than topk joints may be selected.  The divisor stays topk.
//   sample[n] = (sum of the selected rows, in joint order, in double) / topk;   mean_out = (sum_n sample[n], in sample order, in double) / N
// ONE work-group: wave w takes samples w, w + nwaves, ..., SEL_U of them at a time with every load issued before the first use and
// their loops shared (the kernel's time is one wave's dependent instruction chain: profiles/joint_selection.txt); after a barrier wave 0 adds the samples in order - the first SEL_LDS of them
// from the LDS copy the waves left, the rest from `sample`.
__global__ __launch_bounds__(SEL_TPB) void topk_select_k(const float* __restrict__ rows, const float* __restrict__ wfac,
                                                         const unsigned char* __restrict__ mfac, int N, int K, int topk, int largest,
                                                         unsigned char* __restrict__ sel, float* __restrict__ sample,
                                                         float* __restrict__ mean_out) {
    __shared__ float s_sample[SEL_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const float* __restrict__ wp = wfac ? wfac : rows;
    const unsigned char* __restrict__ mp = mfac ? mfac : (const unsigned char*)rows;
    for (int base = 0; base < N; base += SEL_U * nwaves) {
        float v[SEL_U];
        bool zero[SEL_U];
#pragma unroll
        for (int u = 0; u < SEL_U; ++u) {
            const int n = base + wave + u * nwaves;
            const bool ok = n < N && lane < K;
            // branch-free loads (an absent table reads `rows`, an idle lane element 0; both are discarded) so that all of them are in flight together
            const size_t r = ok ? (size_t)n * K + lane : 0;
            const float x = rows[r], wv = wp[r];
            const unsigned char mv = mp[r];
            v[u] = ok ? x : 0.f;
            zero[u] = !ok || (wfac && wv == 0.f) || (mfac && mv == 0);
        }
        // The order as ONE unsigned compare: c = key' << 6 | (63 - lane), key' = the key (largest) or its complement (smallest), and c = 0 for a
        // lane that is no candidate; then "j is better than i" is c[j] > c[i], and a non-candidate is better than nobody.  j is wave-uniform:
        // v_readlane, not the LDS crossbar; the samples in flight share the loop, so their dependent chains interleave.
        unsigned long long c[SEL_U];
        int rank[SEL_U], pick[SEL_U];
        float out[SEL_U], vm[SEL_U];
        double acc[SEL_U];
#pragma unroll
        for (int u = 0; u < SEL_U; ++u) {
            const unsigned int key = hm_key(v[u]);
            const bool cand = (lane < K) && (largest || !zero[u]);
            c[u] = cand ? ((unsigned long long)(largest ? key : ~key) << 6) | (unsigned long long)(63 - lane) : 0ull;
            rank[u] = 0;
        }
        for (int j = 0; j < K; ++j) {
#pragma unroll
            for (int u = 0; u < SEL_U; ++u) {
                const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)c[u], j);
                const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(c[u] >> 32), j);
                rank[u] += (((unsigned long long)hi << 32) | lo) > c[u];
            }
        }
#pragma unroll
        for (int u = 0; u < SEL_U; ++u) {
            pick[u] = c[u] != 0ull && !zero[u] && rank[u] < topk;
            vm[u] = pick[u] ? v[u] : 0.f;       // (an unselected row adds +0: the sum of the selected rows in joint order)
            acc[u] = 0.0;
        }
        for (int j = 0; j < K; ++j) {
#pragma unroll
            for (int u = 0; u < SEL_U; ++u) acc[u] += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(vm[u]), j));
        }
#pragma unroll
        for (int u = 0; u < SEL_U; ++u) out[u] = (float)(acc[u] / topk);
        // (stores behind the arithmetic of every sample in flight: a load's wait would otherwise wait for them too)
#pragma unroll
        for (int u = 0; u < SEL_U; ++u) {
            const int n = base + wave + u * nwaves;
            if (n < N) {
                if (lane < K) sel[(size_t)n * K + lane] = (unsigned char)pick[u];
                if (lane == 0) {
                    sample[n] = out[u];
                    if (n < SEL_LDS) s_sample[n] = out[u];
                }
            }
        }
    }
    if (!mean_out) return;
    __syncthreads();        // (the samples were written by this work-group: visible to it behind the barrier)
    if (wave == 0) {
        // 64 samples per load, added one by one in sample order
        double t = 0.0;
        for (int base = 0; base < N; base += 64) {
            const int n = base + lane;
            const float x = n < N ? (n < SEL_LDS ? s_sample[n] : sample[n]) : 0.f;
            const int m = N - base < 64 ? N - base : 64;
            for (int j = 0; j < m; ++j) t += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j));
        }
        if (lane == 0) mean_out[0] = (float)(t / N);
    }
}

// block j: thr_out[j] = k-th smallest of pool[i*K + j], i < n_pool; mask[i*K + j] = (tm * act_local)[i*K + j] > thr_out[j], i < n_local
__global__ __launch_bounds__(KTH_TPB) void joint_kth_mask_k(const float* __restrict__ pool, int n_pool, int K, int k,
                                                            const float* __restrict__ tm, const float* __restrict__ act_local, int n_local,
                                                            float* __restrict__ thr_out, unsigned char* __restrict__ mask,
                                                            const int* __restrict__ k_dev) {
    __shared__ unsigned int hist[256];
    __shared__ unsigned int pick[2];
    const int j = blockIdx.x;
    if (k_dev) k = hm_kth_clamp(k_dev[0], n_pool);       // (sel_joint_kth_mask_dev: one uniform load, as in kth_mask_k)
    const float thr = hm_kth_smallest(pool + j, (size_t)K, n_pool, k, hist, pick);
    if (threadIdx.x == 0) thr_out[j] = thr;
    for (int i = threadIdx.x; i < n_local; i += blockDim.x) {
        const size_t e = (size_t)i * K + j;
        mask[e] = ((tm ? tm[e] : 1.f) * act_local[e]) > thr ? 1 : 0;
    }
}

// mask = (tm * act) > thr_dev[0]: the threshold is read on the device (a captured step follows a host change of it)
__global__ void thr_mask_k(const float* __restrict__ act, const float* __restrict__ tm, size_t n, const float* __restrict__ thr_dev,
                           unsigned char* __restrict__ mask) {
    const float thr = thr_dev[0];
    for (size_t i = (size_t)blockIdx.x * THR_TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * THR_TPB)
        mask[i] = ((tm ? tm[i] : 1.f) * act[i]) > thr ? 1 : 0;
}
}  // namespace

int sel_topk(hipStream_t s, const float* rows, const float* wfac, const unsigned char* mfac, int N, int K, int topk, int largest,
             unsigned char* sel, float* sample, float* mean_out) {
    if (K > 64) return UDAPOSE_ERR_UNSUPPORTED;
    if (!rows || !sel || !sample || N < 1 || K < 1 || topk < 1 || topk > K || (long long)N * K > (1ll << 22)) return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(topk_select_k, dim3(1), dim3(SEL_TPB), 0, s, rows, wfac, mfac, N, K, topk, largest ? 1 : 0, sel, sample, mean_out);
    return udapose_check_launch();
}
// da = gscale[0] * half_coef * w[r] * (a - b) / (HW * topk * N) on the selected rows, 0 elsewhere: hm_sqdiff_bwd with mask = sel
int sel_topk_sqdiff_bwd(hipStream_t s, const float* a, const float* b, const float* w, const unsigned char* sel, const float* gscale, int N,
                        int K, int HW, int topk, int half, float* da) {
    if (!a || !b || !sel || !da || N < 1 || K < 1 || HW < 1 || topk < 1 || topk > K || (long long)N * K > (1ll << 22)) return UDAPOSE_ERR_ARG;
    const float coef = (float)((half ? 1.0 : 2.0) / ((double)HW * topk * N));
    return hm_sqdiff_bwd(s, a, b, w, sel, gscale, coef, N * K, HW, da, nullptr, nullptr, 1);
}
// k_dev != NULL: k is read on the device (sel_joint_kth_mask_dev) and the by-value k is not looked at
static int joint_kth_mask(hipStream_t s, const float* pool, int n_pool, int K, int k, const int* k_dev, const float* tm, const float* act_local,
                          int n_local, float* thr_out, unsigned char* mask) {
    if (K < 1 || n_pool < 1 || (!k_dev && (k < 1 || k > n_pool))) return UDAPOSE_ERR_ARG;
    if (!pool || !act_local || !thr_out || !mask || n_local < 0 || (long long)n_pool * K > (1ll << 22) || (long long)n_local * K > (1ll << 22))
        return UDAPOSE_ERR_ARG;
    hipLaunchKernelGGL(joint_kth_mask_k, dim3(K), dim3(KTH_TPB), 0, s, pool, n_pool, K, k, tm, act_local, n_local, thr_out, mask, k_dev);
    return udapose_check_launch();
}
int sel_joint_kth_mask(hipStream_t s, const float* pool, int n_pool, int K, int k, const float* tm, const float* act_local, int n_local,
                       float* thr_out, unsigned char* mask) {
    return joint_kth_mask(s, pool, n_pool, K, k, nullptr, tm, act_local, n_local, thr_out, mask);
}
int sel_joint_kth_mask_dev(hipStream_t s, const float* pool, int n_pool, int K, const int* k_dev, const float* tm, const float* act_local,
                           int n_local, float* thr_out, unsigned char* mask) {
    if (!k_dev) return UDAPOSE_ERR_ARG;
    return joint_kth_mask(s, pool, n_pool, K, 0, k_dev, tm, act_local, n_local, thr_out, mask);
}
int sel_thr_mask(hipStream_t s, const float* act, const float* tm, size_t n, const float* thr_dev, unsigned char* mask) {
    if (!act || !thr_dev || !mask) return UDAPOSE_ERR_ARG;
    if (n == 0) return UDAPOSE_OK;
    size_t blocks = (n + THR_TPB - 1) / THR_TPB;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(thr_mask_k, dim3((int)blocks), dim3(THR_TPB), 0, s, act, tm, n, thr_dev, mask);
    return udapose_check_launch();
}
