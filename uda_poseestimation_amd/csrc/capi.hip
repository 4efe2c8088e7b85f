// extern "C" surface of libudapose_hip.so (declared in include/udapose.h).
#include <cstdio>
#include "net.h"
#include "pointwise.h"
#include "losses.h"
#include "optim.h"
#include "style.h"
#include "data.h"
#include "../../include/udapose.h"

// a caller's policy as the library's: a whole-struct copy, plus the one normalisation (wgrad_stages <= 0 means the default)
static Policy from_c(const udapose_policy& c) {
    Policy p;
    static_cast<udapose_policy&>(p) = c;
    if (p.wgrad_stages <= 0) p.wgrad_stages = 128;
    return p;
}
static void to_c(const Policy& p, udapose_policy* c) { *c = p; }
// a convolution descriptor and the policy it names, as the host-side geometry (the policy lives as long as this object)
struct Geom {
    Policy pol;
    ConvGeom g;
    explicit Geom(const udapose_conv_desc* d)
        : g{d->N, d->Hi, d->Wi, d->Ci, d->Co, d->KH, d->KW, d->stride, d->pad, d->transposed, d->reflect, d->upsample} {
        if (d->policy) { pol = from_c(*d->policy); g.pol = &pol; }
    }
};
#define S(x) ((hipStream_t)(x))
#define B16(x) ((elem_t*)(x))
#define CB16(x) ((const elem_t*)(x))

extern "C" {

int udapose_version(void) { return 200; }
int udapose_elem_kind(void) { return UDAPOSE_ELEM_KIND; }      // 0: this build stores / multiplies bf16, 1: fp16

void udapose_policy_default(udapose_policy* p) { if (p) to_c(default_policy(), p); }
void udapose_conv_out_hw(const udapose_conv_desc* d, int* Ho, int* Wo) { Geom G(d); *Ho = G.g.Ho(); *Wo = G.g.Wo(); }
int udapose_conv_stat_rows(const udapose_conv_desc* d) { Geom G(d); return conv_stat_rows(G.g); }
int udapose_conv_prepare(const udapose_conv_desc* d) { if (!d) return UDAPOSE_ERR_ARG; Geom G(d); return conv_prepare(G.g); }
int udapose_conv2d_fwd(void* stream, const udapose_conv_desc* d, const void* x, const void* w_fwd, void* y, const void* res, const float* bias,
                       float* stats, int flags) {
    if (!d || !x || !w_fwd || !y) return UDAPOSE_ERR_ARG;
    ConvEpilogue e;
    e.res = CB16(res); e.bias = bias; e.stats = stats; e.relu = (flags & UDAPOSE_EPI_RELU) != 0; e.out_f32 = (flags & UDAPOSE_EPI_OUT_F32) != 0; e.f32 = (flags & UDAPOSE_EPI_F32) != 0;
    e.split = (flags & UDAPOSE_EPI_SPLIT) != 0;
    if (e.split && e.f32) return UDAPOSE_ERR_ARG;
    Geom G(d);
    return conv_fprop(S(stream), G.g, CB16(x), CB16(w_fwd), y, e);
}
int udapose_conv2d_bwd_data(void* stream, const udapose_conv_desc* d, const void* dy, const void* w_bwd, void* dx, const void* res, int out_f32) {
    if (!d || !dy || !w_bwd || !dx) return UDAPOSE_ERR_ARG;
    Geom G(d);
    return conv_dgrad(S(stream), G.g, CB16(dy), CB16(w_bwd), dx, CB16(res), out_f32);
}
int udapose_conv_bwd_stat_rows(const udapose_conv_desc* d) { if (!d) return UDAPOSE_ERR_ARG; Geom G(d); return conv_dgrad_stat_rows(G.g); }
int udapose_conv2d_bwd_data_bn(void* stream, const udapose_conv_desc* d, const void* dy, const void* w_bwd, void* dx, const void* res, int out_f32,
                               const void* bn_y, const void* bn_z, const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                               const float* bn_beta, float* slab) {
    if (!d || !dy || !w_bwd || !dx || !bn_y || !bn_mean || !bn_invstd || !slab) return UDAPOSE_ERR_ARG;
    DgradBnStat st;
    st.y = CB16(bn_y); st.z = CB16(bn_z); st.mean = bn_mean; st.invstd = bn_invstd; st.gamma = bn_gamma; st.beta = bn_beta; st.slab = slab;
    Geom G(d);
    return conv_dgrad(S(stream), G.g, CB16(dy), CB16(w_bwd), dx, CB16(res), out_f32, &st);
}
int udapose_conv2d_bwd_weight(void* stream, const udapose_conv_desc* d, const void* dy, const void* x, float* dw, int accumulate) {
    if (!d || !dy || !x || !dw) return UDAPOSE_ERR_ARG;
    Geom G(d);
    return conv_wgrad(S(stream), G.g, CB16(dy), CB16(x), dw, accumulate, -1);
}
int udapose_cast_f32_bf16(void* stream, const float* src, void* dst, size_t n) { return pw_cast_f32_bf16(S(stream), src, B16(dst), n); }
int udapose_transpose_cast(void* stream, const float* src, void* dst, int A, int T, int B) { return pw_transpose_cast(S(stream), src, B16(dst), A, T, B); }
int udapose_pack_strided(void* stream, const float* src, void* dst, int A, int KH, int KWp, int KW, int Bp, int B, long sa, long skh, long skw, long sb) {
    return pw_pack_strided(S(stream), src, B16(dst), A, KH, KWp, KW, Bp, B, sa, skh, skw, sb);
}
int udapose_nchw_f32_to_nhwc_bf16(void* stream, const float* src, void* dst, int N, int C, int HW, int Cpad) {
    return pw_nchw_f32_to_nhwc_bf16(S(stream), src, B16(dst), N, C, HW, Cpad);
}
int udapose_nhwc_to_nchw_f32(void* stream, const void* src, int src_is_f32, float* dst, int N, int C, int HW, int Cs, const float* lo, const float* hi) {
    return pw_nhwc_to_nchw_f32(S(stream), src, src_is_f32, dst, N, C, HW, Cs, lo, hi);
}
int udapose_bn_finalize(void* stream, const float* stats, int rows, int C, double count, const float* gamma, const float* beta, float* rm, float* rv,
                        long long* nbt, float momentum, float eps, float* scale, float* shift, float* save_mean, float* save_invstd) {
    return pw_bn_finalize(S(stream), stats, rows, C, count, gamma, beta, rm, rv, nbt, momentum, eps, scale, shift, save_mean, save_invstd, nullptr);
}
int udapose_bn_eval_coeff(void* stream, int C, const float* gamma, const float* beta, const float* rm, const float* rv, float eps, float* scale,
                          float* shift) {
    return pw_bn_eval_coeff(S(stream), C, gamma, beta, rm, rv, eps, scale, shift);
}
int udapose_bn_apply(void* stream, const void* y, const void* res, void* z, size_t numel, int C, const float* scale, const float* shift, int relu) {
    return pw_bn_apply(S(stream), CB16(y), CB16(res), B16(z), numel, C, scale, shift, relu, nullptr, default_policy().bn_xcd_rows >= 2);
}
int udapose_bn_bwd_rows(size_t npix) { return pw_bn_bwd_rows(npix); }
int udapose_bn_bwd(void* stream, const void* dz, int dz_is_f32, const void* z, const void* y, void* dy, void* gout, size_t npix, int C,
                   const float* gamma, const float* mean, const float* invstd, int relu, float* slab, float* coef, float* dgamma, float* dbeta,
                   float beta_acc, const float* beta) {
    return pw_bn_bwd(S(stream), dz, dz_is_f32, CB16(z), CB16(y), B16(dy), B16(gout), npix, C, gamma, mean, invstd, relu, slab, coef, dgamma, dbeta,
                     beta_acc, beta, default_policy().bn_bwd_chunked);
}
int udapose_bn_bwd_pre(void* stream, const void* g, int g_is_f32, const void* y, void* dy, size_t npix, int C, const float* gamma, const float* mean,
                       const float* invstd, const float* slab, int rows, float* coef, float* dgamma, float* dbeta, float beta_acc) {
    if (!g || !y || !dy || !gamma || !mean || !invstd || !slab || !coef) return UDAPOSE_ERR_ARG;
    return pw_bn_bwd_pre(S(stream), g, g_is_f32, CB16(y), B16(dy), npix, C, gamma, mean, invstd, slab, rows, coef, dgamma, dbeta, beta_acc,
                         default_policy().bn_bwd_chunked, default_policy().bn_bwd_pre_legacy);
}
// ---- every BatchNorm / pooling form by explicit selectors (what the executor picks from its policy): each returns a form code >= 0
// (bit 0: the channel-chunked form took the layer, bit 1: the XCD row mapping was engaged) or a negative error
int udapose_bn_train_fwd_ex(void* stream, int kind, const void* y, const void* res, void* z, size_t npix, int C, const float* slab, int rows,
                            const float* gamma, const float* beta, const float* pre_bias, float* running_mean, float* running_var,
                            long long* num_batches_tracked, float momentum, float eps, float* scale, float* shift, float* save, int relu,
                            int fwd_chunked, int xcd_rows, unsigned char* mask, void* y16, void* z16) {
    if (!y || !z || !slab || !gamma || !beta || !scale || !shift || !save || npix < 1 || rows < 1 || C < 8 || C % 8 || kind < 0 || kind > 3)
        return UDAPOSE_ERR_ARG;
    if ((kind == 3) != (y16 != nullptr) || (kind == 3) != (z16 != nullptr) || (mask && (kind == 1 || kind == 2))) return UDAPOSE_ERR_ARG;
    if (kind == 3 && UDAPOSE_ELEM_KIND != 1) return UDAPOSE_ERR_UNSUPPORTED;      // (the shadows are the fp16 build's backward operands)
    const int chunked = fwd_chunked | (xcd_rows ? (1 << 30) : 0);
    int took = 0;
    if (kind == 0 && !pre_bias)
        took = pw_bn_train_fused(S(stream), CB16(y), CB16(res), B16(z), npix, C, slab, rows, gamma, beta, running_mean, running_var,
                                 num_batches_tracked, momentum, eps, save, relu, chunked, mask);
    else if (kind >= 2 && !pre_bias)
        took = pw_bn_train_fused_split(S(stream), (const float*)y, res, z, npix, C, slab, rows, gamma, beta, running_mean, running_var,
                                       num_batches_tracked, momentum, eps, save, relu, chunked, y16, z16, mask);
    if (took < 0) return took;
    if (took) return 1 | (xcd_rows ? 2 : 0);
    int rc = pw_bn_finalize(S(stream), slab, rows, C, (double)npix, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, scale,
                            shift, save, save + C, pre_bias);
    if (rc != UDAPOSE_OK) return rc;
    const int xcd = xcd_rows >= 2;
    if (kind == 0) rc = pw_bn_apply(S(stream), CB16(y), CB16(res), B16(z), npix * C, C, scale, shift, relu, mask, xcd);
    else if (kind == 1) rc = pw_bn_apply_f32(S(stream), (const float*)y, (const float*)res, (float*)z, npix * C, C, scale, shift, relu);
    else rc = pw_bn_apply_split(S(stream), (const float*)y, res, z, npix * C, C, scale, shift, relu, y16, z16, mask, xcd);
    if (rc != UDAPOSE_OK) return rc;
    return (xcd && (kind == 0 || kind == 3) && pw_bn_apply_xcd_ok(npix * (C / 8), C)) ? 2 : 0;
}
int udapose_bn_bwd_ex(void* stream, const void* dz, int dz_is_f32, const void* z, const void* y, void* dy, void* gout, size_t npix, int C,
                      const float* gamma, const float* mean, const float* invstd, int relu, float* slab, float* coef, float* dgamma, float* dbeta,
                      float beta_acc, const float* beta, int chunked) {
    if (!dz || !y || !dy || !gamma || !mean || !invstd || !slab || !coef || npix < 1 || C < 8) return UDAPOSE_ERR_ARG;
    const int rc = pw_bn_bwd(S(stream), dz, dz_is_f32, CB16(z), CB16(y), B16(dy), B16(gout), npix, C, gamma, mean, invstd, relu, slab, coef, dgamma,
                             dbeta, beta_acc, beta, chunked);
    return rc != UDAPOSE_OK ? rc : pw_bn_bwd_takes_chunked(npix, C, chunked);
}
int udapose_bn_bwd_pre_ex(void* stream, const void* g, int g_is_f32, const void* y, void* dy, size_t npix, int C, const float* gamma,
                          const float* mean, const float* invstd, const float* slab, int rows, float* coef, float* dgamma, float* dbeta,
                          float beta_acc, int chunked, int legacy) {
    if (!g || !y || !dy || !gamma || !mean || !invstd || !slab || !coef || npix < 1 || C < 8) return UDAPOSE_ERR_ARG;
    const int rc = pw_bn_bwd_pre(S(stream), g, g_is_f32, CB16(y), B16(dy), npix, C, gamma, mean, invstd, slab, rows, coef, dgamma, dbeta, beta_acc,
                                 chunked, legacy);
    if (rc != UDAPOSE_OK) return rc;
    if (pw_bn_bwd_pre_takes_chunked(npix, C, rows, chunked)) return 1 | (((chunked >> 30) & 1) ? 2 : 0);
    return (!legacy && ((chunked >> 29) & 1) && pw_bn_apply_xcd_ok(npix * (C / 8), C)) ? 2 : 0;
}
int udapose_bn_relu_maxpool3x3s2(void* stream, const void* x, void* y, unsigned char* idx, int N, int H, int W, int C, const float* scale,
                                 const float* shift) {
    if (!x || !y || !scale || !shift || N < 1 || H < 1 || W < 1 || C < 8) return UDAPOSE_ERR_ARG;
    return pw_bn_relu_maxpool3x3s2(S(stream), CB16(x), B16(y), idx, N, H, W, C, scale, shift);
}
int udapose_bn_bwd_pooled(void* stream, const void* pool_dy, const unsigned char* pool_idx, int H, int W, const void* y, void* dy, size_t npix, int C,
                          const float* gamma, const float* mean, const float* invstd, float* slab, float* coef, float* dgamma, float* dbeta,
                          float beta_acc, const float* beta) {
    if (!pool_dy || !pool_idx || !y || !dy || !gamma || !mean || !invstd || !slab || !coef || H < 1 || W < 1 || npix < 1 || C < 8) return UDAPOSE_ERR_ARG;
    return pw_bn_bwd_pooled(S(stream), CB16(pool_dy), pool_idx, H, W, CB16(y), B16(dy), npix, C, gamma, mean, invstd, slab, coef, dgamma, dbeta,
                            beta_acc, beta);
}
int udapose_bn_running_update(void* stream, const float* save, int C, float* running_mean, float* running_var, long long* num_batches_tracked,
                              float momentum) {
    if (!save || !running_mean || !running_var || C < 1) return UDAPOSE_ERR_ARG;
    return pw_bn_running_update(S(stream), save, C, running_mean, running_var, num_batches_tracked, momentum);
}
int udapose_bn_running_update_multi(void* stream, const void* d_jobs, int njobs, int max_c, const void* act, float momentum) {
    if (!d_jobs || !act || njobs < 1 || max_c < 1) return UDAPOSE_ERR_ARG;
    return pw_bn_running_update_multi(S(stream), (const BnRunJob*)d_jobs, njobs, max_c, act, momentum);
}
int udapose_maxpool3x3s2_fwd_ex(void* stream, int kind, const void* x, void* y, unsigned char* idx, int N, int H, int W, int C, void* y16) {
    if (!x || !y || N < 1 || H < 1 || W < 1 || C < 8 || C % 8 || kind < 0 || kind > 3 || (kind == 3) != (y16 != nullptr)) return UDAPOSE_ERR_ARG;
    if (kind == 3 && UDAPOSE_ELEM_KIND != 1) return UDAPOSE_ERR_UNSUPPORTED;
    if (kind == 0) return pw_maxpool3x3s2_fwd(S(stream), CB16(x), B16(y), idx, N, H, W, C);
    if (kind == 1) return pw_maxpool3x3s2_fwd_f32(S(stream), (const float*)x, (float*)y, idx, N, H, W, C);
    return pw_maxpool3x3s2_fwd_split(S(stream), x, y, idx, N, H, W, C, y16);
}
int udapose_maxpool3x3s2_fwd(void* stream, const void* x, void* y, unsigned char* idx, int N, int H, int W, int C) {
    return pw_maxpool3x3s2_fwd(S(stream), CB16(x), B16(y), idx, N, H, W, C);
}
int udapose_maxpool3x3s2_bwd(void* stream, const void* dy, const unsigned char* idx, void* dx, int N, int H, int W, int C) {
    return pw_maxpool3x3s2_bwd(S(stream), CB16(dy), idx, B16(dx), N, H, W, C);
}
int udapose_maxpool2x2_ceil(void* stream, const void* x, void* y, int N, int H, int W, int C) {
    return pw_maxpool2x2_ceil(S(stream), CB16(x), B16(y), N, H, W, C);
}
int udapose_maxpool2x2_ceil_f32(void* stream, const float* x, float* y, int N, int H, int W, int C) {
    return pw_maxpool2x2_ceil_f32(S(stream), x, y, N, H, W, C);
}
int udapose_nchw_f32_to_nhwc_f32(void* stream, const float* src, float* dst, int N, int C, int HW, int Cpad) {
    return pw_nchw_f32_to_nhwc_f32(S(stream), src, dst, N, C, HW, Cpad);
}
int udapose_nchw_f32_to_nhwc_split(void* stream, const float* src, void* dst, int N, int C, int HW, int Cpad) {
    if (!src || !dst) return UDAPOSE_ERR_ARG;
    return pw_nchw_f32_to_nhwc_split(S(stream), src, dst, N, C, HW, Cpad);
}
int udapose_f32_to_split(void* stream, const float* src, void* dst, size_t n) {
    if (!src || !dst) return UDAPOSE_ERR_ARG;
    return pw_f32_to_split(S(stream), src, dst, n);
}
int udapose_split_to_f32(void* stream, const void* src, float* dst, size_t n) {
    if (!src || !dst) return UDAPOSE_ERR_ARG;
    return pw_split_to_f32(S(stream), src, dst, n);
}
int udapose_maxpool2x2_ceil_split(void* stream, const void* x, void* y, int N, int H, int W, int C) {
    if (!x || !y) return UDAPOSE_ERR_ARG;
    return pw_maxpool2x2_ceil_split(S(stream), x, y, N, H, W, C);
}

int udapose_net_create(const int layers[4], int K, int N, int H, int W, int fp32, udapose_net_t* out) {
    if (!out) return UDAPOSE_ERR_ARG;
    *out = net_create(layers, K, N, H, W, fp32);
    return *out ? UDAPOSE_OK : UDAPOSE_ERR_ARG;
}
void udapose_net_destroy(udapose_net_t n) { net_destroy(n); }
int udapose_net_set_policy(udapose_net_t n, const udapose_policy* p) {
    if (!n || !p) return UDAPOSE_ERR_ARG;
    net_set_policy(n, from_c(*p));
    return UDAPOSE_OK;
}
int udapose_net_get_policy(udapose_net_t n, udapose_policy* p) {
    if (!n || !p) return UDAPOSE_ERR_ARG;
    to_c(net_get_policy(n), p);
    return UDAPOSE_OK;
}
int udapose_net_bind(udapose_net_t n, const void* const* params, void* const* buffers, void* wpack) {
    if (!n || !params || !wpack) return UDAPOSE_ERR_ARG;
    return net_bind(n, params, buffers, wpack);
}
int udapose_net_bind_grads(udapose_net_t n, void* const* grads) {
    if (!n || !grads) return UDAPOSE_ERR_ARG;
    return net_bind_grads(n, grads);
}
int udapose_net_num_params(udapose_net_t n) { return net_num_params(n); }
int udapose_net_num_buffers(udapose_net_t n) { return net_num_buffers(n); }
long long udapose_net_param_numel(udapose_net_t n, int i) { return net_param_numel(n, i); }
size_t udapose_net_wpack_bytes(udapose_net_t n) { return net_wpack_bytes(n); }
size_t udapose_net_act_bytes(udapose_net_t n) { return net_act_bytes(n); }
size_t udapose_net_ws_bytes(udapose_net_t n) { return net_ws_bytes(n); }
void udapose_net_out_shape(udapose_net_t n, int shape[4]) { net_out_shape(n, shape); }
int udapose_net_pack_weights(udapose_net_t n, void* stream, const void* const* params, void* wpack, int with_bwd) {
    return net_pack_weights(n, S(stream), params, wpack, with_bwd);
}
int udapose_net_forward(udapose_net_t n, void* stream, const float* x, const void* const* params, void* const* buffers, const void* wpack, void* act,
                        void* ws, float* out, int training, float momentum) {
    return net_forward(n, S(stream), x, params, buffers, wpack, act, ws, out, training, momentum);
}
int udapose_net_apply_running(udapose_net_t n, void* stream, const void* act, void* const* buffers, float momentum) {
    return net_apply_running(n, S(stream), act, buffers, momentum);
}
int udapose_axpy_f32(void* stream, float* y, const float* x, size_t n) { return pw_axpy(S(stream), y, x, n); }
int udapose_net_backward(udapose_net_t n, void* stream, const float* dout, const void* const* params, const void* wpack, void* act, void* ws,
                         void* const* grads, float beta) {
    return net_backward(n, S(stream), dout, params, wpack, act, ws, grads, beta, 0, 0);
}
int udapose_net_backward_part(udapose_net_t n, void* stream, const float* dout, const void* const* params, const void* wpack, void* act,
                              void* ws, void* const* grads, float beta, int part) {
    if (part != 1 && part != 2) return UDAPOSE_ERR_ARG;
    return net_backward(n, S(stream), dout, params, wpack, act, ws, grads, beta, part, 0);
}
int udapose_net_wgrad_pair(udapose_net_t n, void* stream, const void* act_a, void* ws_a, void* const* grads_a, float beta_a, const void* act_b,
                           void* ws_b, void* const* grads_b, float beta_b, int part) {
    if (!n || !act_a || !ws_a || !grads_a || !act_b || !ws_b || !grads_b) return UDAPOSE_ERR_ARG;
    return net_wgrad_pair(n, S(stream), act_a, ws_a, grads_a, beta_a, act_b, ws_b, grads_b, beta_b, part);
}
int udapose_net_wgrad_pair_defer(udapose_net_t n, void* stream, const void* act_a, void* ws_a, void* const* grads_a, float beta_a, const void* act_b,
                                 void* ws_b, void* const* grads_b, float beta_b, int part, int* deferred) {
    if (!n || !act_a || !ws_a || !grads_a || !act_b || !ws_b || !grads_b) return UDAPOSE_ERR_ARG;
    return net_wgrad_pair_defer(n, S(stream), act_a, ws_a, grads_a, beta_a, act_b, ws_b, grads_b, beta_b, part, deferred);
}
int udapose_net_split_sum_flush(udapose_net_t n, void* stream) { return n ? net_split_sum_flush(n, S(stream)) : UDAPOSE_ERR_ARG; }
int udapose_wgrad_deal(const int* nblk, const int* stages, int n_units, int order, int* ent_xcd, int* ent_unit, int* ent_first, int* ent_count, int cap,
                       double* finish_out) {
    return net_wgrad_deal(nblk, stages, n_units, order, ent_xcd, ent_unit, ent_first, ent_count, cap, finish_out);
}
int udapose_net_backward_phase(udapose_net_t n, void* stream, const float* dout, const void* const* params, const void* wpack, void* act,
                               void* ws, void* const* grads, float beta, int part, int phase) {
    if (!n) return UDAPOSE_ERR_ARG;
    return net_backward(n, S(stream), dout, params, wpack, act, ws, grads, beta, part, phase);
}
int udapose_stem_dgrad(void* stream, const void* dy, const float* w, int N, int H, int W, float* dx) {
    return stem_dgrad(S(stream), (const elem_t*)dy, w, N, H, W, dx);
}
int udapose_net_input_grad(udapose_net_t n, void* stream, const void* const* params, void* ws, float* dx) {
    if (!n || !params || !ws || !dx) return UDAPOSE_ERR_ARG;
    return net_input_grad(n, S(stream), params, ws, dx);
}
long long udapose_perturb_ws_bytes(int N, int C, int HW) { return perturb_ws_bytes(N, C, HW); }
int udapose_perturb(void* stream, const float* x, const float* g, const float* x0, int N, int C, int HW, int mode, const float* eps_dev,
                    const float* step_dev, const float* lo, const float* hi, void* ws, float* out, float* gnorm) {
    return perturb(S(stream), x, g, x0, N, C, HW, mode, eps_dev, step_dev, lo, hi, ws, out, gnorm);
}
long long udapose_net_grad_split_param(udapose_net_t n) { return net_grad_split_param(n); }
int udapose_net_bind_update(udapose_net_t student, udapose_net_t teacher, void* const* params_s, void* const* grads, void* const* exp_avg,
                            void* const* exp_avg_sq, void* const* params_t, void* wpack_s, void* wpack_t) {
    if (!student || !teacher || !params_s || !grads || !exp_avg || !exp_avg_sq || !params_t || !wpack_s || !wpack_t) return UDAPOSE_ERR_ARG;
    return net_bind_update(student, teacher, params_s, grads, exp_avg, exp_avg_sq, params_t, wpack_s, wpack_t);
}
int udapose_net_fused_update(udapose_net_t student, udapose_net_t teacher, void* stream, void* const* params_s, void* const* grads,
                             void* const* exp_avg, void* const* params_t, void* wpack_s, void* wpack_t, float lr, float beta1, float beta2,
                             float eps, float weight_decay, int step, float grad_scale, float* dev_state, float alpha, float one_minus_alpha,
                             int do_adam, long long grad2_delta_bytes) {
    if (!student || !teacher) return UDAPOSE_ERR_ARG;
    return net_fused_update(student, teacher, S(stream), params_s, grads, exp_avg, params_t, wpack_s, wpack_t, lr, beta1, beta2, eps, weight_decay,
                            step, grad_scale, dev_state, alpha, one_minus_alpha, do_adam, grad2_delta_bytes, nullptr);
}
int udapose_net_fused_update_dev(udapose_net_t student, udapose_net_t teacher, void* stream, void* const* params_s, void* const* grads,
                                 void* const* exp_avg, void* const* params_t, void* wpack_s, void* wpack_t, float lr, float beta1, float beta2,
                                 float eps, float weight_decay, int step, float grad_scale, float* dev_state, const float* ema_dev, int do_adam,
                                 long long grad2_delta_bytes) {
    if (!student || !teacher || !ema_dev) return UDAPOSE_ERR_ARG;
    return net_fused_update(student, teacher, S(stream), params_s, grads, exp_avg, params_t, wpack_s, wpack_t, lr, beta1, beta2, eps, weight_decay,
                            step, grad_scale, dev_state, 0.f, 0.f, do_adam, grad2_delta_bytes, ema_dev);
}
int udapose_net_bind_update_groups(udapose_net_t student, udapose_net_t teacher, int kind, void* const* params_s, void* const* grads,
                                   void* const* state1, void* const* state2, void* const* params_t, void* wpack_s, void* wpack_t,
                                   const int* group_idx) {
    if (!student || !teacher || !params_s || !grads || !state1 || (kind == UDAPOSE_OPT_ADAM && !state2) || !params_t || !wpack_s || !wpack_t)
        return UDAPOSE_ERR_ARG;
    return net_bind_update_groups(student, teacher, kind, params_s, grads, state1, state2, params_t, wpack_s, wpack_t, group_idx);
}
int udapose_net_fused_update_groups(udapose_net_t student, udapose_net_t teacher, void* stream, int kind, void* const* params_s,
                                    void* const* grads, void* const* state1, void* const* params_t, void* wpack_s, void* wpack_t, float beta1,
                                    float beta2, float eps, int nesterov, int n_groups, float* const* dev_states, const float* weight_decays,
                                    float alpha, float one_minus_alpha, int do_opt, long long grad2_delta_bytes) {
    if (!student || !teacher || !params_s || !grads || !state1 || !params_t) return UDAPOSE_ERR_ARG;
    return net_fused_update_groups(student, teacher, S(stream), kind, params_s, grads, state1, params_t, wpack_s, wpack_t, beta1, beta2, eps, nesterov,
                                   n_groups, dev_states, weight_decays, alpha, one_minus_alpha, do_opt, grad2_delta_bytes, nullptr);
}
int udapose_net_fused_update_groups_dev(udapose_net_t student, udapose_net_t teacher, void* stream, int kind, void* const* params_s,
                                        void* const* grads, void* const* state1, void* const* params_t, void* wpack_s, void* wpack_t,
                                        float beta1, float beta2, float eps, int nesterov, int n_groups, float* const* dev_states,
                                        const float* weight_decays, const float* ema_dev, int do_opt, long long grad2_delta_bytes) {
    if (!student || !teacher || !params_s || !grads || !state1 || !params_t || !ema_dev) return UDAPOSE_ERR_ARG;
    return net_fused_update_groups(student, teacher, S(stream), kind, params_s, grads, state1, params_t, wpack_s, wpack_t, beta1, beta2, eps, nesterov,
                                   n_groups, dev_states, weight_decays, 0.f, 0.f, do_opt, grad2_delta_bytes, ema_dev);
}

int udapose_joints_mse_fwd(void* stream, const float* pred, const float* gt, const float* w, int R, int HW, float* rows, float* mean_out) {
    return hm_sqdiff_rows(S(stream), pred, gt, w, nullptr, R, HW, 0.5f, rows, mean_out, nullptr, nullptr, 1);
}
int udapose_joints_mse_bwd(void* stream, const float* pred, const float* gt, const float* w, const float* gscale, int R, int HW, float* dpred) {
    return hm_sqdiff_bwd(S(stream), pred, gt, w, nullptr, gscale, (float)(1.0 / ((double)R * HW)), R, HW, dpred, nullptr, nullptr, 1);
}
int udapose_cons_loss_fwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, int R, int HW, float* rows, float* mean_out) {
    return hm_sqdiff_rows(S(stream), stu, tea, nullptr, mask, R, HW, 1.0f, rows, mean_out, nullptr, nullptr, 1);
}
int udapose_cons_loss_bwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const float* gscale, int R, int HW, float* dstu) {
    return hm_sqdiff_bwd(S(stream), stu, tea, nullptr, mask, gscale, (float)(2.0 / ((double)R * HW)), R, HW, dstu, nullptr, nullptr, 1);
}
int udapose_mask_count(void* stream, const unsigned char* mask, size_t n, float* count) {
    if (!mask || !count) return UDAPOSE_ERR_ARG;
    return hm_mask_count(S(stream), mask, n, count);
}
int udapose_cons_loss_valid_fwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const unsigned char* valid,
                                const float* valid_count, int R, int K, int HW, float* rows, float* mean_out) {
    if (!valid || !valid_count) return UDAPOSE_ERR_ARG;
    return hm_sqdiff_rows(S(stream), stu, tea, nullptr, mask, R, HW, 1.0f, rows, mean_out, valid, valid_count, K);
}
int udapose_cons_loss_valid_bwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const unsigned char* valid,
                                const float* valid_count, const float* gscale, int R, int K, int HW, float* dstu) {
    if (!valid || !valid_count) return UDAPOSE_ERR_ARG;
    return hm_sqdiff_bwd(S(stream), stu, tea, nullptr, mask, gscale, (float)(2.0 / ((double)R * HW)), R, HW, dstu, valid, valid_count, K);
}
int udapose_joints_kl_fwd(void* stream, const float* pred, const float* gt, const float* w, float epsilon, int R, int group, int HW, float* rows,
                          float* stats, float* out) {
    return sml_kl_fwd(S(stream), pred, gt, w, epsilon, R, group, HW, rows, stats, out);
}
int udapose_joints_kl_bwd(void* stream, const float* pred, const float* gt, const float* w, float epsilon, const float* stats,
                          const float* gscale, int R, int HW, float* dpred) {
    return sml_kl_bwd(S(stream), pred, gt, w, epsilon, stats, gscale, R, HW, dpred);
}
int udapose_entropy_loss_fwd(void* stream, const float* x, int R, int group, int HW, float threshold, float* rows, float* stats, float* out,
                             float* count) {
    return sml_ent_fwd(S(stream), x, R, group, HW, threshold, rows, stats, out, count);
}
int udapose_entropy_loss_bwd(void* stream, const float* x, const float* rows, const float* stats, const float* count, const float* gscale,
                             float threshold, int R, int HW, float* dx) {
    return sml_ent_bwd(S(stream), x, rows, stats, count, gscale, threshold, R, HW, dx);
}
int udapose_cons_softmax_fwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const unsigned char* valid,
                             const float* valid_count, int R, int K, int HW, float* rows, float* stats, float* out) {
    return sml_cons_fwd(S(stream), 0, stu, tea, mask, valid, valid_count, R, K, HW, rows, stats, out);
}
int udapose_cons_softmax_bwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const unsigned char* valid,
                             const float* valid_count, const float* stats, const float* gscale, int R, int K, int HW, float* dstu) {
    return sml_cons_bwd(S(stream), 0, stu, tea, mask, valid, valid_count, stats, gscale, R, K, HW, dstu);
}
int udapose_cons_kl_fwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const unsigned char* valid,
                        const float* valid_count, int log_target, int R, int K, int HW, float* rows, float* stats, float* out) {
    return sml_cons_fwd(S(stream), log_target ? 1 : 2, stu, tea, mask, valid, valid_count, R, K, HW, rows, stats, out);
}
int udapose_cons_kl_bwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const unsigned char* valid,
                        const float* valid_count, int log_target, const float* stats, const float* gscale, int R, int K, int HW, float* dstu) {
    return sml_cons_bwd(S(stream), log_target ? 1 : 2, stu, tea, mask, valid, valid_count, stats, gscale, R, K, HW, dstu);
}
long long udapose_coral_ws_bytes(int N, int K, int H, int W, int down) { return coral_ws_bytes(N, K, H, W, down); }
int udapose_coral_fwd(void* stream, const float* src, const float* tgt, int N, int K, int H, int W, int down, void* ws, float* coef, float* loss) {
    return coral_fwd(S(stream), src, tgt, N, K, H, W, down, ws, coef, loss);
}
int udapose_coral_bwd(void* stream, const float* src, const float* tgt, const float* coef, const float* gscale, int N, int K, int H, int W,
                      int down, float* dsrc, float* dtgt) {
    return coral_bwd(S(stream), src, tgt, coef, gscale, N, K, H, W, down, dsrc, dtgt);
}
int udapose_soft_argmax_fwd(void* stream, const float* hm, int R, int H, int W, float beta, int window, float* coords, float* maxvals,
                            int* flat_idx, float* stats) {
    return sa_fwd(S(stream), hm, R, H, W, beta, window, coords, maxvals, flat_idx, stats);
}
int udapose_soft_argmax_bwd(void* stream, const float* hm, const float* dcoords, const int* flat_idx, const float* stats, int R, int H, int W,
                            float beta, int window, float* dhm) {
    return sa_bwd(S(stream), hm, dcoords, flat_idx, stats, R, H, W, beta, window, dhm);
}
int udapose_coord_loss_fwd(void* stream, const float* hm, const float* target, const float* weight, const unsigned char* mask, int R, int group,
                           int H, int W, float beta, int window, int norm, float* rows, int* flat_idx, float* stats, float* out) {
    return sa_coord_fwd(S(stream), hm, target, weight, mask, R, group, H, W, beta, window, norm, rows, flat_idx, stats, out);
}
int udapose_coord_loss_bwd(void* stream, const float* hm, const float* target, const float* weight, const unsigned char* mask, const int* flat_idx,
                           const float* stats, const float* gscale, int R, int H, int W, float beta, int window, int norm, float* dhm) {
    return sa_coord_bwd(S(stream), hm, target, weight, mask, flat_idx, stats, gscale, R, H, W, beta, window, norm, dhm);
}
int udapose_heatmap_argmax(void* stream, const float* hm, int R, int H, int W, float* maxvals, int* flat_idx, float* preds, float* rect,
                           const float* patch, int rad) {
    if (rect && !patch) return UDAPOSE_ERR_ARG;
    return hm_argmax_rectify(S(stream), hm, R, H, W, maxvals, flat_idx, preds, rect, patch, rad);
}
int udapose_prior_weights(void* stream, const float* std_table, int K, float gamma, float epsilon, int v3, float* w) {
    return pm_weights(S(stream), std_table, K, gamma, epsilon, v3, w);
}
int udapose_prior_map(void* stream, const float* coords, const float* conf, const float* mean, const float* w, const float* hm, int B, int K, int H,
                      int W, float sigma, int v3, float* out) {
    return pm_map(S(stream), coords, conf, mean, w, hm, B, K, H, W, sigma, v3, out);
}
int udapose_pair_dist_accumulate(void* stream, const float* coords, const unsigned char* visible, int M, int K, double* acc) {
    return pm_pair_accumulate(S(stream), coords, visible, M, K, acc);
}
int udapose_pair_dist_finish(void* stream, const double* acc, int K, float* mean, float* std_table) {
    return pm_pair_finish(S(stream), acc, K, mean, std_table);
}
int udapose_hflip_batch(void* stream, const float* src, float* dst, int N, size_t rows_per_image, int W, int keep_original) {
    return flip_hbatch(S(stream), src, dst, N, rows_per_image, W, keep_original);
}
int udapose_flip_merge(void* stream, const float* a, const float* f, const int* perm, int N, int K, int H, int W, int shift, int mode, float* out,
                       float* maxvals, int* flat_idx, float* preds_xy) {
    return flip_merge(S(stream), a, f, perm, N, K, H, W, shift, mode, out, maxvals, flat_idx, preds_xy);
}
int udapose_box_crop(void* stream, const unsigned char* frames_u8, int F, int Hs, int Ws, const int* frame_idx, const float* boxes, int M, int Ho,
                     int Wo, const float* mean3, const float* std3, int mirror, float* out_f32, unsigned char* out_u8, unsigned char* status) {
    return box_crop(S(stream), frames_u8, F, Hs, Ws, frame_idx, boxes, M, Ho, Wo, mean3, std3, mirror, out_f32, out_u8, status);
}
int udapose_coords_to_image(void* stream, const float* coords, const float* boxes, int M, int K, float stride_x, float stride_y, int Ho, int Wo,
                            float* out) {
    return box_coords_to_image(S(stream), coords, boxes, M, K, stride_x, stride_y, Ho, Wo, out);
}
int udapose_pose_rescore(void* stream, const float* kp, const float* conf, const float* boxes, const unsigned char* status, const float* box_score,
                         const float* vis_thr, int M, int K, float* score, int* order, float* area, unsigned char* refused) {
    return pose_rescore(S(stream), kp, conf, boxes, status, box_score, vis_thr, M, K, score, order, area, refused);
}
int udapose_oks_matrix(void* stream, const float* kp_a, const float* area_a, int Ma, const float* kp_b, const float* area_b, const float* visible_b,
                       int Mb, int K, const float* sigmas, const int* frame_idx, const unsigned char* refused, const float* oks_thr, float* out,
                       unsigned long long* mask) {
    return oks_matrix(S(stream), kp_a, area_a, Ma, kp_b, area_b, visible_b, Mb, K, sigmas, frame_idx, refused, oks_thr, out, mask);
}
int udapose_pose_nms_sweep(void* stream, const unsigned long long* mask, const int* order, const unsigned char* refused, int M, unsigned char* keep,
                           int* n_keep, int* suppressed_by) {
    return pose_nms_sweep(S(stream), mask, order, refused, M, keep, n_keep, suppressed_by);
}
long long udapose_ap_match_ws_bytes(int M, int G, int F) { return (long long)ap_match_ws_bytes(M, G, F); }
int udapose_ap_match(void* stream, const float* kp, const float* score, const int* frame_idx, const unsigned char* valid, const float* area, int M,
                     const float* gt_kp, const float* gt_visible, const float* gt_area, const int* gt_frame, const unsigned char* gt_ignore, int G,
                     int K, int F, const float* sigmas, const float* thresholds, int T, const float* ranges, int A, int max_dets, void* ws,
                     float* rec_score, unsigned long long* rec_matched, unsigned long long* rec_ignored, int capacity, long long* counters) {
    return ap_match(S(stream), kp, score, frame_idx, valid, area, M, gt_kp, gt_visible, gt_area, gt_frame, gt_ignore, G, K, F, sigmas, thresholds, T,
                    ranges, A, max_dets, ws, rec_score, rec_matched, rec_ignored, capacity, counters);
}
long long udapose_ap_curve_ws_bytes(int capacity, int T, int A) { return (long long)ap_curve_ws_bytes(capacity, T, A); }
int udapose_ap_curve(void* stream, const float* rec_score, const unsigned long long* rec_matched, const unsigned long long* rec_ignored,
                     int capacity, const long long* counters, int T, int A, const double* recall_points, int R, void* ws, double* precision,
                     float* scores, double* recall) {
    return ap_curve(S(stream), rec_score, rec_matched, rec_ignored, capacity, counters, T, A, recall_points, R, ws, precision, scores, recall);
}
long long udapose_pose_nms_ws_bytes(int M) { return (long long)pose_nms_ws_bytes(M); }
int udapose_pose_nms(void* stream, const float* kp, const float* conf, const float* boxes, const int* frame_idx, const unsigned char* status,
                     const float* box_score, const float* sigmas, const float* vis_thr, const float* oks_thr, int M, int K, void* ws, float* score,
                     int* order, unsigned char* keep, int* n_keep, int* suppressed_by, float* oks_out) {
    return pose_nms(S(stream), kp, conf, boxes, frame_idx, status, box_score, sigmas, vis_thr, oks_thr, M, K, ws, score, order, keep, n_keep,
                    suppressed_by, oks_out);
}
int udapose_refine_decode(void* stream, const float* hm, int R, int H, int W, int mode, int kernel, float sigma, float* coords, float* maxvals,
                          int* flat_idx) {
    return refine_decode(S(stream), hm, R, H, W, mode, kernel, sigma, coords, maxvals, flat_idx);
}
int udapose_kth_mask(void* stream, const float* act, const float* tm, int n, int k, float* thr_out, unsigned char* mask, const float* act_local,
                     int n_local) {
    return hm_kth_mask(S(stream), act, tm, n, k, thr_out, mask, act_local, n_local);
}
int udapose_kth_mask_dev(void* stream, const float* act, const float* tm, int n, const int* k_dev, float* thr_out, unsigned char* mask,
                         const float* act_local, int n_local) {
    return hm_kth_mask_dev(S(stream), act, tm, n, k_dev, thr_out, mask, act_local, n_local);
}
int udapose_topk_select(void* stream, const float* rows, const float* wfac, const unsigned char* mfac, int N, int K, int topk, int largest,
                        unsigned char* sel, float* sample, float* mean_out) {
    return sel_topk(S(stream), rows, wfac, mfac, N, K, topk, largest, sel, sample, mean_out);
}
int udapose_topk_sqdiff_bwd(void* stream, const float* a, const float* b, const float* w, const unsigned char* sel, const float* gscale, int N,
                            int K, int HW, int topk, int half, float* da) {
    return sel_topk_sqdiff_bwd(S(stream), a, b, w, sel, gscale, N, K, HW, topk, half, da);
}
int udapose_joint_kth_mask(void* stream, const float* pool, int n_pool, int K, int k, const float* tm, const float* act_local, int n_local,
                           float* thr_out, unsigned char* mask) {
    return sel_joint_kth_mask(S(stream), pool, n_pool, K, k, tm, act_local, n_local, thr_out, mask);
}
int udapose_joint_kth_mask_dev(void* stream, const float* pool, int n_pool, int K, const int* k_dev, const float* tm, const float* act_local,
                               int n_local, float* thr_out, unsigned char* mask) {
    return sel_joint_kth_mask_dev(S(stream), pool, n_pool, K, k_dev, tm, act_local, n_local, thr_out, mask);
}
int udapose_thr_mask(void* stream, const float* act, const float* tm, size_t n, const float* thr_dev, unsigned char* mask) {
    return sel_thr_mask(S(stream), act, tm, n, thr_dev, mask);
}
int udapose_pck(void* stream, const float* pred, const float* gt, int B, int K, float nx, float ny, float thr, float* acc, float* avg_cnt) {
    return hm_pck(S(stream), pred, gt, B, K, nx, ny, thr, acc, avg_cnt);
}
int udapose_pck_accumulate(void* stream, const float* pred_xy, const float* gt_xy, const unsigned char* visible, const float* norm, int B, int K,
                           float nh, float nw, const float* thr, int T, long long* state) {
    return pck_accumulate(S(stream), pred_xy, gt_xy, visible, norm, B, K, nh, nw, thr, T, state);
}
int udapose_pck_accumulate_heatmaps(void* stream, const float* out, const float* target, const float* norm, int B, int K, int H, int W,
                                    const float* thr, int T, long long* state, float* preds_xy) {
    return pck_accumulate_heatmaps(S(stream), out, target, norm, B, K, H, W, thr, T, state, preds_xy);
}
int udapose_multi_chunk(void) { return opt_chunk(); }
int udapose_ema_multi(void* stream, const long long* t, const long long* s, const long long* sizes, const int* bt, const long long* bo, int nb,
                      float alpha, float oma) {
    return opt_ema(S(stream), t, s, sizes, bt, bo, nb, alpha, oma, nullptr);
}
int udapose_ema_multi_dev(void* stream, const long long* t, const long long* s, const long long* sizes, const int* bt, const long long* bo, int nb,
                          const float* ema_dev) {
    if (!ema_dev) return UDAPOSE_ERR_ARG;
    return opt_ema(S(stream), t, s, sizes, bt, bo, nb, 0.f, 0.f, ema_dev);
}
int udapose_adam_multi(void* stream, const long long* p, const long long* g, const long long* m, const long long* v, const long long* sizes,
                       const int* bt, const long long* bo, int nb, float lr, float b1, float b2, float eps, float wd, int step, float gscale,
                       float* dev_state) {
    return opt_adam(S(stream), p, g, m, v, sizes, bt, bo, nb, lr, b1, b2, eps, wd, step, gscale, dev_state);
}
int udapose_sgd_multi(void* stream, const long long* p, const long long* g, const long long* buf, const long long* sizes, const int* bt,
                      const long long* bo, int nb, float lr, float mom, float wd, int nesterov, int first, float gscale, float* dev_state) {
    return opt_sgd(S(stream), p, g, buf, sizes, bt, bo, nb, lr, mom, wd, nesterov, first, gscale, dev_state);
}
int udapose_grad_scaler_check(void* stream, const long long* g, const long long* sizes, const int* bt, const long long* bo, int nb, float* dev_state) {
    return opt_grad_check(S(stream), g, sizes, bt, bo, nb, dev_state, 0);
}
int udapose_grad_scaler_check2(void* stream, const long long* g, const long long* sizes, const int* bt, const long long* bo, int nb, float* dev_state,
                               long long grad2_delta_bytes) {
    return opt_grad_check(S(stream), g, sizes, bt, bo, nb, dev_state, grad2_delta_bytes);
}
int udapose_grad_scaler_update(void* stream, float* dev_state, float growth, float backoff, int interval) {
    return opt_scaler_update(S(stream), dev_state, growth, backoff, interval);
}
int udapose_grad_sumsq(void* stream, const long long* g, const long long* sizes, const int* bt, const long long* bo, int nb,
                       long long grad2_delta_bytes, float* dev_state, double* partials) {
    return opt_grad_sumsq(S(stream), g, sizes, bt, bo, nb, grad2_delta_bytes, dev_state, partials);
}
int udapose_grad_clip(void* stream, const double* partials, const int* blk_begin, const int* blk_end, int n_groups, float* const* dev_states,
                      float* clip) {
    return opt_grad_clip(S(stream), partials, blk_begin, blk_end, n_groups, dev_states, clip);
}
int udapose_grad_clip_restore(void* stream, int n_groups, float* const* dev_states, const float* clip) {
    return opt_grad_clip_restore(S(stream), n_groups, dev_states, clip);
}
int udapose_comm_pack_bf16(void* stream, const float* src, long long n, void* dst_bf16, long long n_padded) {
    if (!src || !dst_bf16) return UDAPOSE_ERR_ARG;
    return comm_pack_bf16(S(stream), src, n, dst_bf16, n_padded);
}
int udapose_comm_shard_mean(void* stream, const void* shards_bf16, int world, long long m, void* out_bf16) {
    if (!shards_bf16 || !out_bf16) return UDAPOSE_ERR_ARG;
    return comm_shard_mean(S(stream), shards_bf16, world, m, out_bf16);
}
int udapose_comm_unpack_bf16(void* stream, const void* src_bf16, float* dst, long long n) {
    if (!src_bf16 || !dst) return UDAPOSE_ERR_ARG;
    return comm_unpack_bf16(S(stream), src_bf16, dst, n);
}
int udapose_adain(void* stream, const void* c, const void* s, void* out, int N, int HWc, int HWs, int C, float eps, float alpha, float* stats_out) {
    return adain_launch(S(stream), CB16(c), CB16(s), B16(out), N, HWc, HWs, C, eps, alpha, nullptr, stats_out);
}
int udapose_adain_alpha_dev(void* stream, const void* c, const void* s, void* out, int N, int HWc, int HWs, int C, float eps, const float* alpha_dev,
                            float* stats_out, int is_f32) {
    if (!alpha_dev) return UDAPOSE_ERR_ARG;
    if (is_f32) return adain_launch_f32(S(stream), (const float*)c, (const float*)s, (float*)out, N, HWc, HWs, C, eps, 1.f, alpha_dev, stats_out);
    return adain_launch(S(stream), CB16(c), CB16(s), B16(out), N, HWc, HWs, C, eps, 1.f, alpha_dev, stats_out);
}
long long udapose_fda_ws_bytes(int planes, int H, int W, int b) { return fda_ws_bytes(planes, H, W, b); }
int udapose_fda_spectrum(void* stream, const float* x, int planes, int H, int W, int b, void* ws, float* spec) {
    return fda_spectrum(S(stream), x, planes, H, W, b, ws, spec);
}
int udapose_fda_apply(void* stream, const float* content, const float* spec_c, const float* spec_s, float* out, int planes, int C, int H, int W, int b,
                      float alpha, const float* alpha_dev, const float* lo, const float* hi, const float* mean, const float* std) {
    return fda_apply(S(stream), content, spec_c, spec_s, out, planes, C, H, W, b, alpha, alpha_dev, lo, hi, mean, std);
}
long long udapose_pixel_summary_bytes(int N, int C) { return pixel_summary_bytes(N, C); }
int udapose_pixel_summary(void* stream, const float* x, int N, int C, int H, int W, const float* mean, const float* std, void* summary) {
    return pixel_summary(S(stream), x, N, C, H, W, mean, std, summary);
}
int udapose_pixel_transfer(void* stream, const float* content, const void* sum_c, const void* sum_s, float* out, int N, int C, int H, int W, int mode,
                           double eps, float alpha, const float* alpha_dev, const float* lo, const float* hi, const float* mean, const float* std) {
    return pixel_transfer(S(stream), content, sum_c, sum_s, out, N, C, H, W, mode, eps, alpha, alpha_dev, lo, hi, mean, std);
}
int udapose_adain_f32(void* stream, const float* c, const float* s, float* out, int N, int HWc, int HWs, int C, float eps, float alpha,
                      float* stats_out) {
    return adain_launch_f32(S(stream), c, s, out, N, HWc, HWs, C, eps, alpha, nullptr, stats_out);
}
int udapose_adain_split(void* stream, const void* c, const void* s, void* out, int N, int HWc, int HWs, int C, float eps, float alpha,
                        const float* alpha_dev, float* stats_out) {
    if (!c || !s) return UDAPOSE_ERR_ARG;
    return adain_launch_split(S(stream), c, s, out, N, HWc, HWs, C, eps, alpha, alpha_dev, stats_out);
}

int udapose_patch_paste(void* stream, float* img, const int* boxes, int n, int C, int H, int W, int max_patch_elems) {
    return patch_paste(S(stream), img, boxes, n, C, H, W, max_patch_elems);
}
int udapose_occlusion_pick(void* stream, const float* conf, const int* flat_idx, const float* u, int N, int K, int w, double ratio, int image_size,
                           float rate, float thresh, int occlude_size, int* boxes, unsigned char* apply) {
    if (!conf || !flat_idx || !u || !boxes || !apply) return UDAPOSE_ERR_ARG;
    return occlusion_pick(S(stream), conf, flat_idx, u, N, K, w, ratio, image_size, rate, thresh, occlude_size, boxes, apply);
}
int udapose_select_rows(void* stream, float* dst, const float* a, const float* b, const unsigned char* flag, int N, size_t row_elems) {
    if (!dst || !a || !b || !flag) return UDAPOSE_ERR_ARG;
    return select_rows(S(stream), dst, a, b, flag, N, row_elems);
}
int udapose_recon_thetas(void* stream, const double* params, int N, double ratio, float* theta_fwd, float* theta_back) {
    if (!params || (!theta_fwd && !theta_back)) return UDAPOSE_ERR_ARG;
    return affine_recon_thetas(S(stream), params, N, ratio, theta_fwd, theta_back);
}
int udapose_split_saturations(int reset, unsigned long long* count) {
    if (!count) return UDAPOSE_ERR_ARG;
    unsigned long long t = 0;
    for (unsigned long long v : {sp_sat_read_adain(reset), sp_sat_read_igemm(reset), sp_sat_read_patchconv(reset), sp_sat_read_pointwise(reset)}) {
        if (v == ~0ull) return UDAPOSE_ERR_LAUNCH;
        t += v;
    }
    *count = t;
    return UDAPOSE_OK;
}
int udapose_mean_views(void* stream, const float* const* h_views, int k, float* dst, size_t n) {
    return affine_mean_views(S(stream), h_views, k, dst, n);
}
int udapose_view_merge(void* stream, const float* const* h_views, int k, int R, int H, int W, int mode, const float* radius_dev, int min_views,
                       float* mean, int* peaks, float* maxvals, int* inliers, int* n_inliers, int* spread2, float* agree, float* energy) {
    return affine_view_merge(S(stream), h_views, k, R, H, W, mode, radius_dev, min_views, mean, peaks, maxvals, inliers, n_inliers, spread2, agree,
                             energy);
}
int udapose_affine_nearest(void* stream, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage, int backward) {
    return affine_warp_chain(S(stream), src, dst, theta, N, C, H, W, nstage, backward);
}
int udapose_affine_bilinear(void* stream, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage, int backward) {
    return affine_warp_chain_bilinear(S(stream), src, dst, theta, N, C, H, W, nstage, backward);
}
int udapose_affine_nearest_mirror(void* stream, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage, int backward,
                                  const unsigned char* mirror, const int* perm) {
    return affine_warp_chain_mirror(S(stream), src, dst, theta, N, C, H, W, nstage, backward, mirror, perm);
}
int udapose_affine_bilinear_mirror(void* stream, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage, int backward,
                                   const unsigned char* mirror, const int* perm) {
    return affine_warp_chain_bilinear_mirror(S(stream), src, dst, theta, N, C, H, W, nstage, backward, mirror, perm);
}
int udapose_aug_hflip_u8(void* stream, const unsigned char* src, unsigned char* dst, const unsigned char* flag, int N, int H, int W) {
    return aug_hflip_u8(S(stream), src, dst, flag, N, H, W);
}

int udapose_aug_affine_u8(void* stream, const unsigned char* src, unsigned char* dst, const long long* coef, int N, int H, int W) {
    if (!src || !dst || !coef) return UDAPOSE_ERR_ARG;
    return aug_affine_u8(S(stream), src, dst, coef, N, H, W);
}
int udapose_aug_color_op(void* stream, unsigned char* img, const int* op, const float* factor, int* mean_scratch, int N, int HW) {
    if (!img || !op || !factor || !mean_scratch) return UDAPOSE_ERR_ARG;
    return aug_color_op(S(stream), img, op, factor, mean_scratch, N, HW);
}
int udapose_aug_gaussian_blur_u8(void* stream, unsigned char* img, unsigned char* tmp, const unsigned int* prm, int N, int H, int W) {
    if (!img || !tmp || !prm) return UDAPOSE_ERR_ARG;
    return aug_gaussian_blur_u8(S(stream), img, tmp, prm, N, H, W);
}
int udapose_aug_point_op(void* stream, unsigned char* img, const int* op, const int* param, const double* inv_scale, unsigned char* lut_scratch,
                         int N, int HW) {
    if (!img || !op || !param || !inv_scale || !lut_scratch) return UDAPOSE_ERR_ARG;
    return aug_point_op(S(stream), img, op, param, inv_scale, lut_scratch, N, HW);
}
int udapose_aug_sharpness_u8(void* stream, unsigned char* img, unsigned char* tmp, const int* op, const float* factor, int N, int H, int W) {
    if (!img || !tmp || !op || !factor) return UDAPOSE_ERR_ARG;
    return aug_sharpness_u8(S(stream), img, tmp, op, factor, N, H, W);
}
int udapose_aug_erase_f32(void* stream, float* x, const int* boxes, float v0, float v1, float v2, int N, int H, int W) {
    if (!x || !boxes) return UDAPOSE_ERR_ARG;
    return aug_erase_f32(S(stream), x, boxes, v0, v1, v2, N, H, W);
}
int udapose_aug_resized_crop_u8(void* stream, const unsigned char* src, unsigned char* dst, unsigned char* tmp, const int* box, const int* bounds,
                                const int* coef, int N, int Hs, int Ws, int S, int ksize) {
    if (!src || !dst || !tmp || !box || !bounds || !coef) return UDAPOSE_ERR_ARG;
    return aug_resized_crop_u8(S(stream), src, dst, tmp, box, bounds, coef, N, Hs, Ws, S, ksize);
}
int udapose_aug_to_tensor(void* stream, const unsigned char* img, float* out, int N, int HW, const float* mean3, const float* std3) {
    if (!img || !out || !mean3 || !std3) return UDAPOSE_ERR_ARG;
    return aug_to_tensor(S(stream), img, out, N, HW, mean3, std3);
}
int udapose_gaussian_labels(void* stream, const double* kp, const float* vis, float* target, float* weight, int R, int Hh, int Wh,
                            double stride_x, double stride_y, const float* patch, int rad) {
    if (!kp || !vis || !target || !weight) return UDAPOSE_ERR_ARG;
    return aug_gaussian_labels(S(stream), kp, vis, target, weight, R, Hh, Wh, stride_x, stride_y, patch, rad);
}
int udapose_gaussian_labels_subpixel(void* stream, const double* kp, const float* vis, float* target, float* weight, int R, int Hh, int Wh,
                                     double stride_x, double stride_y, double sigma, int rad) {
    if (!kp || !vis || !target || !weight) return UDAPOSE_ERR_ARG;
    return aug_gaussian_labels_subpixel(S(stream), kp, vis, target, weight, R, Hh, Wh, stride_x, stride_y, sigma, rad);
}
int udapose_draw_labelmap_ori(void* stream, const float* pt, const float* vis, const unsigned char* gate, float* target, float* weight, int R,
                              int Hh, int Wh, float r3, const float* patch, int psize) {
    if (!target || !weight) return UDAPOSE_ERR_ARG;
    return aug_draw_labelmap_ori(S(stream), pt, vis, gate, target, weight, R, Hh, Wh, r3, patch, psize);
}
void udapose_prof_begin(void) { prof_begin(); }
int udapose_prof_end(double* h_out9) { return prof_end(h_out9); }

long long udapose_conv_bwd_ws_bytes(const udapose_conv_desc* d) {
    if (!d) return UDAPOSE_ERR_ARG;
    Geom G(d);
    const size_t b = conv_bwd_ws_bytes(G.g);
    return b ? (long long)b : UDAPOSE_ERR_UNSUPPORTED;
}
int udapose_conv_bwd_prepare(const udapose_conv_desc* d) { if (!d) return UDAPOSE_ERR_ARG; Geom G(d); return conv_bwd_prepare(G.g); }
int udapose_conv2d_bwd_data_reflect_padded(void* stream, const udapose_conv_desc* d, const void* dy, const void* w_bwd, void* dP) {
    if (!d) return UDAPOSE_ERR_ARG;
    Geom G(d);
    return conv_dgrad_reflect_padded(S(stream), G.g, CB16(dy), CB16(w_bwd), B16(dP));
}
int udapose_reflect_fold(void* stream, const void* dP, int upsample, const void* x, int relu_mask, const float* stats, const float* gscale_s,
                         const void* t, const float* gscale_c, float c_scale, const float* add_nchw, int add_c, void* dx, int N, int H, int W, int C,
                         float term_scale) {
    return reflect_fold(S(stream), CB16(dP), upsample ? 1 : 0, CB16(x), relu_mask, stats, gscale_s, CB16(t), gscale_c, c_scale, add_nchw, add_c,
                        B16(dx), N, H, W, C, term_scale);
}
int udapose_conv2d_bwd_data_reflect(void* stream, const udapose_conv_desc* d, const void* dy, const void* w_bwd, void* dx, const void* relu_src,
                                    void* ws) {
    if (!d || !dx) return UDAPOSE_ERR_ARG;
    Geom G(d);
    return conv_dgrad_reflect(S(stream), G.g, CB16(dy), CB16(w_bwd), B16(dx), CB16(relu_src), ws);
}
int udapose_conv2d_bwd_weight_reflect(void* stream, const udapose_conv_desc* d, const void* dy, const void* x, float* dw, int co_valid, void* ws,
                                      float out_scale) {
    if (!d) return UDAPOSE_ERR_ARG;
    Geom G(d);
    return conv_wgrad_reflect(S(stream), G.g, CB16(dy), CB16(x), dw, co_valid, ws, out_scale);
}
int udapose_maxpool2x2_ceil_bwd(void* stream, const void* x, const void* dy, void* dx, int N, int H, int W, int C, int relu_mask) {
    return maxpool2x2_ceil_bwd(S(stream), CB16(x), CB16(dy), B16(dx), N, H, W, C, relu_mask);
}
long long udapose_bias_grad_ws_bytes(long long M, int C) { return (long long)bias_grad_ws_bytes(M, C); }
int udapose_bias_grad(void* stream, const void* dy, float* db, long long M, int C, int c_valid, void* ws, float out_scale) {
    return bias_grad(S(stream), CB16(dy), db, M, C, c_valid, ws, out_scale);
}
long long udapose_feat_mse_ws_bytes(void) { return (long long)feat_mse_ws_bytes(); }
int udapose_feat_mse_fwd(void* stream, const void* a, const void* b, long long n, float* out, void* ws) {
    return feat_mse_fwd(S(stream), CB16(a), CB16(b), n, out, ws);
}
int udapose_style_stat_loss(void* stream, const float* stats, int R, float* out, int accumulate) {
    return style_stat_loss(S(stream), stats, R, out, accumulate);
}

}  // extern "C"
