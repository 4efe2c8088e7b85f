// The PoseResNet executor's entry points (net.hip; a plan is an opaque void*) and the launch profiler (prof.hip).
#pragma once
#include "conv_plan.h"

// net.hip
void* net_create(const int layers[4], int K, int N, int H, int W, int mode);
void net_destroy(void* h);
void net_set_policy(void* h, const Policy& p);
const Policy& net_get_policy(void* h);
int net_num_params(void* h);
int net_num_buffers(void* h);
long long net_param_numel(void* h, int i);
size_t net_wpack_bytes(void* h);
size_t net_act_bytes(void* h);
size_t net_ws_bytes(void* h);
void net_out_shape(void* h, int* shp);
int net_bind(void* h, const void* const* params, void* const* buffers, void* wpack_);
int net_pack_weights(void* h, hipStream_t s, const void* const* params, void* wpack_, int with_bwd);
int net_forward(void* h, hipStream_t s, const float* x_nchw, const void* const* params, void* const* buffers, const void* wpack_, void* act_, void* ws_,
                float* out_nchw, int training, float momentum);
int net_wgrad_pair(void* h, hipStream_t s, const void* actA, void* wsA, void* const* gradsA, float betaA, const void* actB, void* wsB,
                   void* const* gradsB, float betaB, int part);
int net_wgrad_pair_defer(void* h, hipStream_t s, const void* actA, void* wsA, void* const* gradsA, float betaA, const void* actB, void* wsB,
                         void* const* gradsB, float betaB, int part, int* deferred);
int net_split_sum_flush(void* h, hipStream_t s);
int net_wgrad_deal(const int* nblk, const int* stages, int n_units, int order, int* ent_xcd, int* ent_unit, int* ent_first, int* ent_count, int cap,
                   double* finish_out);
int net_backward(void* h, hipStream_t s, const float* dout_nchw, const void* const* params, const void* wpack_, void* act_, void* ws_,
                 void* const* grads, float beta, int part, int phase);
int net_input_grad(void* h, hipStream_t s, const void* const* params, void* ws_, float* dx);
int net_apply_running(void* h, hipStream_t s, const void* act_, void* const* buffers, float momentum);
int net_bind_grads(void* h, void* const* grads);
long long net_grad_split_param(void* h);
int net_bind_update_groups(void* hs, void* ht, int kind, void* const* params_s, void* const* grads, void* const* h_m, void* const* h_v,
                           void* const* params_t, void* wpack_s_, void* wpack_t_, const int* group_idx);
int net_bind_update(void* hs, void* ht, void* const* params_s, void* const* grads, void* const* h_m, void* const* h_v, void* const* params_t,
                    void* wpack_s_, void* wpack_t_);
int net_fused_update(void* hs, void* ht, hipStream_t s, void* const* params_s, void* const* grads, void* const* h_m, void* const* params_t,
                     void* wpack_s_, void* wpack_t_, float lr, float beta1, float beta2, float eps, float wd, int step, float gscale,
                     float* dev_state, float alpha, float oma, int do_adam, long long grad2_delta, const float* ema_dev);
int net_fused_update_groups(void* hs, void* ht, hipStream_t s, int kind, void* const* params_s, void* const* grads, void* const* h_m,
                            void* const* params_t, void* wpack_s_, void* wpack_t_, float beta1, float beta2, float eps, int nesterov, int ngroups,
                            float* const* states, const float* wds, float alpha, float oma, int do_opt, long long grad2_delta, const float* ema_dev);
// prof.hip
int prof_before(hipStream_t s, int kind, double flops);
void prof_after(hipStream_t s, int token);
void prof_begin();
int prof_end(double* out);
