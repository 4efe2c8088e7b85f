// Host launchers of the memory-bound kernels (pointwise.hip) and the device-table entries their callers fill.
#pragma once
#include "common.h"

// one BN layer of the batched running-statistics update (pw_bn_running_update_multi)
struct BnRunJob { size_t save_off; float* rm; float* rv; long long* nbt; int C, pad; };
// one range of the multi-range clear (pw_zero_multi): byte offset from a base pointer, length in 16-byte units
struct ZeroJob { long long off; long long n16; };
// one layer of the split-sum launch (pw_split_sum): `ks` partial tiles of `n` floats, `stride` floats apart, at byte offset part_off of the pass's
// workspace, are added in split order into the tensor at byte offset dst_off of the gradient base (dst_ws: of the workspace); beta 1 accumulates
#define UDAPOSE_SPLIT_SUM_CHUNK 1024u      // floats of a job one work-group of pw_split_sum adds (one 16-byte column per thread)
struct SumJob { long long part_off; long long dst_off; unsigned n; unsigned stride; int ks; int dst_ws; float beta; int pad; };

// Clears `bytes` (a multiple of 4, 4-byte aligned) at p with a KERNEL.  Every clear on a capturable path goes through this instead of
// hipMemsetAsync: on ROCm 7.2 a hipGraph memset node can be replayed out of order with the kernel node that depends on it (from the
// third replay of a small captured graph on, with the runtime's default DEBUG_CLR_GRAPH_PACKET_CAPTURE=1: the clear lands AFTER the
// scatter that follows it; tools/probe/graph_memset_order.py reproduces it with torch alone).
int pw_zero(hipStream_t s, void* p, size_t bytes);
int pw_split_sum(hipStream_t s, const SumJob* d_jobs, const int* d_blk, int nblk, void* ws, void* grad_base, void* ws2 = nullptr, void* grad_base2 = nullptr);

int pw_nchw_f32_to_nhwc_bf16(hipStream_t s, const float* src, elem_t* dst, int N, int C, int HW, int Cp);
int pw_nchw_f32_to_nhwc_f32(hipStream_t s, const float* src, float* dst, int N, int C, int HW, int Cp);
int pw_nchw_f32_to_nhwc_split(hipStream_t s, const float* src, void* dst, int N, int C, int HW, int Cp, void* dst16 = nullptr);
int pw_nhwc_to_nchw_f32(hipStream_t s, const void* src, int src_is_f32, float* dst, int N, int C, int HW, int Cs, const float* lo, const float* hi);
int pw_cast_f32_bf16(hipStream_t s, const float* src, elem_t* dst, size_t n);
int pw_transpose_cast(hipStream_t s, const float* src, elem_t* dst, int A, int T, int B);
int pw_transpose_f32(hipStream_t s, const float* src, float* dst, int A, int T, int B);
int pw_f32_to_split(hipStream_t s, const float* src, void* dst, size_t n);
int pw_split_to_f32(hipStream_t s, const void* src, float* dst, size_t n);
int pw_transpose_split(hipStream_t s, const float* src, void* dst, int A, int T, int B);
int pw_pack_strided_split(hipStream_t s, const float* src, void* dst, int A, int KH, int KWp, int KW, int Bp, int B, long sa, long skh, long skw, long sb);
int pw_pack_multi(hipStream_t s, const void* jobs, const int* blk_job, const int* blk_sub, int nblocks);
int pw_pack_strided(hipStream_t s, const float* src, elem_t* dst, int A, int KH, int KWp, int KW, int Bp, int B, long sa, long skh, long skw, long sb);
int pw_pack_strided_f32(hipStream_t s, const float* src, float* dst, int A, int KH, int KWp, int KW, int Bp, int B, long sa, long skh, long skw, long sb);
int pw_unpack_strided(hipStream_t s, const float* src, float* dst, int A, int KH, int KWp, int KW, int Bp, int B, long sa, long skh, long skw, long sb, float beta);
int pw_bn_finalize(hipStream_t s, const float* slab, int rows, int C, double count, const float* gamma, const float* beta, float* rm, float* rv,
                   long long* nbt, float momentum, float eps, float* scale, float* shift, float* save_mean, float* save_invstd, const float* pre_bias);
int pw_bn_train_fused(hipStream_t s, const elem_t* y, const elem_t* res, elem_t* z, size_t npix, int C, const float* slab, int rows,
                      const float* gamma, const float* beta, float* rm, float* rv, long long* nbt, float momentum, float eps, float* save,
                      int relu, int enabled, unsigned char* mask);
int pw_bn_train_fused_split(hipStream_t s, const float* y, const void* res, void* z, size_t npix, int C, const float* slab, int rows,
                            const float* gamma, const float* beta, float* rm, float* rv, long long* nbt, float momentum, float eps, float* save,
                            int relu, int enabled, void* y16, void* z16, unsigned char* mask);
int pw_bn_running_update_multi(hipStream_t s, const BnRunJob* d_jobs, int njobs, int maxC, const void* act, float momentum);
int pw_bn_running_update(hipStream_t s, const float* save, int C, float* rm, float* rv, long long* nbt, float momentum);
int pw_zero_multi(hipStream_t s, const ZeroJob* d_jobs, int njobs, void* base);
int pw_axpy(hipStream_t s, float* y, const float* x, size_t n);
int pw_bn_eval_coeff(hipStream_t s, int C, const float* gamma, const float* beta, const float* rm, const float* rv, float eps, float* scale, float* shift);
int pw_bn_apply_xcd_ok(size_t n8, int C);
int pw_bn_apply(hipStream_t s, const elem_t* y, const elem_t* res, elem_t* z, size_t n, int C, const float* scale, const float* shift, int relu,
                unsigned char* mask, int xcd);
int pw_bn_apply_split(hipStream_t s, const float* y, const void* res, void* z, size_t n, int C, const float* scale, const float* shift, int relu,
                      void* y16, void* z16, unsigned char* mask, int xcd);
int pw_bn_apply_f32(hipStream_t s, const float* y, const float* res, float* z, size_t n, int C, const float* scale, const float* shift, int relu);
int pw_bn_bwd_rows(size_t npix);
int pw_bn_bwd_takes_chunked(size_t npix, int C, int chunked);
int pw_bn_bwd_pre_takes_chunked(size_t npix, int C, int rows, int chunked);
int pw_bn_bwd(hipStream_t s, const void* dz, int dz_is_f32, const elem_t* z, const elem_t* y, elem_t* dy, elem_t* gout, size_t npix, int C,
              const float* gamma, const float* mean, const float* invstd, int relu, float* slab, float* coef, float* dgamma, float* dbeta,
              float beta_acc, const float* beta, int chunked);
int pw_bn_bwd_pre(hipStream_t s, const void* g, int g_is_f32, const elem_t* y, elem_t* dy, size_t npix, int C, const float* gamma, const float* mean,
                  const float* invstd, const float* slab, int rows, float* coef, float* dgamma, float* dbeta, float beta_acc, int chunked,
                  int legacy);
int pw_maxpool3x3s2_fwd(hipStream_t s, const elem_t* x, elem_t* y, unsigned char* idx, int N, int H, int W, int C);
int pw_bn_relu_maxpool3x3s2(hipStream_t s, const elem_t* x, elem_t* y, unsigned char* idx, int N, int H, int W, int C, const float* scale,
                            const float* shift);
int pw_bn_bwd_pooled(hipStream_t s, const elem_t* pool_dy, const unsigned char* pool_idx, int H, int W, const elem_t* y, elem_t* dy, size_t npix, int C,
                     const float* gamma, const float* mean, const float* invstd, float* slab, float* coef, float* dgamma, float* dbeta, float beta_acc,
                     const float* beta);
int pw_maxpool3x3s2_fwd_f32(hipStream_t s, const float* x, float* y, unsigned char* idx, int N, int H, int W, int C);
int pw_maxpool3x3s2_fwd_split(hipStream_t s, const void* x, void* y, unsigned char* idx, int N, int H, int W, int C, void* y16);
int pw_maxpool2x2_ceil_split(hipStream_t s, const void* x, void* y, int N, int H, int W, int C);
int pw_maxpool3x3s2_bwd(hipStream_t s, const elem_t* dy, const unsigned char* idx, elem_t* dx, int N, int H, int W, int C);
int pw_maxpool2x2_ceil(hipStream_t s, const elem_t* x, elem_t* y, int N, int H, int W, int C);
int pw_maxpool2x2_ceil_f32(hipStream_t s, const float* x, float* y, int N, int H, int W, int C);
int pw_plane_sum(hipStream_t s, const float* x, float* out, int N, int C, int HW, float beta);
unsigned long long sp_sat_read_pointwise(int reset);
// gradient-direction perturbation inside an l2 / linf ball (perturb.hip): fp32 [N][C][HW]; eps / step device scalars; ws of perturb_ws_bytes
long long perturb_ws_bytes(int N, int C, int HW);
int perturb(hipStream_t s, const float* x, const float* g, const float* x0, int N, int C, int HW, int mode, const float* eps, const float* step,
            const float* lo, const float* hi, void* ws, float* out, float* gnorm);
