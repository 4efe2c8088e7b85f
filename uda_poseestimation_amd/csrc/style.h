// Host launchers of the style bridges: AdaIN, the decoder's training step, Fourier-domain transfer (FDA), and the histogram / colour-statistics
// transfers.
#pragma once
#include "conv_plan.h"

// adain.hip
int adain_launch(hipStream_t s, const elem_t* content, const elem_t* style, elem_t* out, int N, int HWc, int HWs, int C, float eps, float alpha,
                 const float* alpha_dev, float* stats_out);
int adain_launch_f32(hipStream_t s, const float* content, const float* style, float* out, int N, int HWc, int HWs, int C, float eps, float alpha,
                     const float* alpha_dev, float* stats_out);
int adain_launch_split(hipStream_t s, const void* content, const void* style, void* out, int N, int HWc, int HWs, int C, float eps, float alpha,
                       const float* alpha_dev, float* stats_out);
unsigned long long sp_sat_read_adain(int reset);
// adain_train.hip
size_t conv_bwd_ws_bytes(const ConvGeom& g);
int conv_bwd_prepare(const ConvGeom& g);
int conv_dgrad_reflect_padded(hipStream_t s, const ConvGeom& g, const elem_t* dy, const elem_t* w_bwd, elem_t* dP);
int reflect_fold(hipStream_t s, const elem_t* dP, int up, const elem_t* x, int mask, const float* stats, const float* gs_s, const elem_t* t,
                 const float* gs_c, float c_scale, const float* add_nchw, int add_c, elem_t* dx, int N, int H, int W, int C, float term_scale);
int conv_dgrad_reflect(hipStream_t s, const ConvGeom& g, const elem_t* dy, const elem_t* w_bwd, elem_t* dx, const elem_t* mask_src, void* ws);
int conv_wgrad_reflect(hipStream_t s, const ConvGeom& g, const elem_t* dy, const elem_t* x, float* dw, int co_valid, void* ws, float out_scale);
int maxpool2x2_ceil_bwd(hipStream_t s, const elem_t* x, const elem_t* dy, elem_t* dx, int N, int H, int W, int C, int mask);
size_t bias_grad_ws_bytes(long long M, int C);
int bias_grad(hipStream_t s, const elem_t* dy, float* db, long long M, int C, int c_valid, void* ws, float out_scale);
size_t feat_mse_ws_bytes();
int feat_mse_fwd(hipStream_t s, const elem_t* a, const elem_t* b, long long n, float* out, void* ws);
int style_stat_loss(hipStream_t s, const float* stats, int R, float* out, int accumulate);
// fda.hip
long long fda_ws_bytes(int planes, int H, int W, int b);
int fda_spectrum(hipStream_t s, const float* x, int planes, int H, int W, int b, void* ws, float* spec);
int fda_apply(hipStream_t s, const float* content, const float* spec_c, const float* spec_s, float* out, int planes, int C, int H, int W, int b, float alpha,
              const float* alpha_dev, const float* lo, const float* hi, const float* mean, const float* stdv);
// pixel_style.hip
long long pixel_summary_bytes(int N, int C);
int pixel_summary(hipStream_t s, const float* x, int N, int C, int H, int W, const float* mean, const float* stdv, void* summary);
int pixel_transfer(hipStream_t s, const float* content, const void* sum_c, const void* sum_s, float* out, int N, int C, int H, int W, int mode, double eps,
                   float alpha, const float* alpha_dev, const float* lo, const float* hi, const float* mean, const float* stdv);
