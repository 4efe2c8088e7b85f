// Host launchers of the multi-tensor optimizer and gradient-communication kernels (optim.hip), and the job table of the fused tail.
#pragma once
#include "common.h"

// One parameter tensor of the fused optimizer tail (opt_tail).  The executor builds the table: it knows the pack offsets.
struct TailJob {
    float* p; const float* g; float* m; float* v; float* t;   // student parameter, gradient, moments, teacher parameter
    elem_t* sd; elem_t* td; elem_t* sx; elem_t* tx;             // packs: student / teacher same-layout, student / teacher transposed
    int A, T, B, adam;                                          // A == 0: linear job; adam == 0: no gradient (EMA + packs only)
    long long n;
    // a gradient whose pixel reduction was split (net.hip make_partial): `ks` partial tensors in the gradient's own layout, `stride` floats apart,
    // at byte offset part_off of a pass's workspace (ks == 0: not split)
    long long part_off; unsigned stride; int ks;
    int group;                                                  // parameter group: index into opt_tail's states / wds, < TAIL_GROUPS
};
constexpr int TAIL_GROUPS = 8;

int opt_chunk();
// ema_dev (opt_tail, opt_ema): NULL, or the pair {alpha, 1 - alpha} in device memory, read by the kernel in place of the by-value pair
int opt_tail(hipStream_t s, const TailJob* d_jobs, const int* blk_job, const int* blk_sub, int nblocks, int kind, float lr, float beta1, float beta2,
             float eps, int nesterov, int step, float gscale, int ngroups, float* const* states, const float* wds, float alpha, float oma, int do_adam,
             long long grad2_delta, int tick, const void* split_ws1, const void* split_ws2, const float* ema_dev);
int opt_grad_check(hipStream_t s, const long long* g, const long long* sizes, const int* blk_tensor, const long long* blk_off, int nblocks,
                   float* dev_state, long long grad2_delta);
int opt_scaler_update(hipStream_t s, float* dev_state, float growth, float backoff, int interval);
int opt_grad_sumsq(hipStream_t s, const long long* g, const long long* sizes, const int* blk_tensor, const long long* blk_off, int nblocks,
                   long long grad2_delta, float* dev_state, double* partials);
int opt_grad_clip(hipStream_t s, const double* partials, const int* blk_begin, const int* blk_end, int ngroups, float* const* states, float* clip);
int opt_grad_clip_restore(hipStream_t s, int ngroups, float* const* states, const float* clip);
int opt_ema(hipStream_t s, const long long* tgt, const long long* src, const long long* sizes, const int* blk_tensor, const long long* blk_off,
            int nblocks, float alpha, float one_minus_alpha, const float* ema_dev);
int opt_adam(hipStream_t s, const long long* p, const long long* g, const long long* m, const long long* v, const long long* sizes,
             const int* blk_tensor, const long long* blk_off, int nblocks, float lr, float beta1, float beta2, float eps, float wd, int step,
             float gscale, float* dev_state);
int opt_sgd(hipStream_t s, const long long* p, const long long* g, const long long* buf, const long long* sizes, const int* blk_tensor,
            const long long* blk_off, int nblocks, float lr, float momentum, float wd, int nesterov, int first_step, float gscale,
            float* dev_state);
int comm_pack_bf16(hipStream_t s, const float* src, long long n, void* dst, long long npad);
int comm_shard_mean(hipStream_t s, const void* in, int W, long long m, void* out);
int comm_unpack_bf16(hipStream_t s, const void* src, float* dst, long long n);
