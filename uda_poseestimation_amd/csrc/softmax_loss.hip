// Soft-max heat-map losses (fp32 NCHW rows [R = B*K][HW]): JointsKLLoss, EntLoss, ConsSoftmaxLoss, ConsKLLoss of the reference's
// lib/models/loss.py:52-173, forward and backward.  Same conventions as heatmap.hip: one 256-thread block per (b,k) row, operands
// read as f32x4 where HW % 4 == 0 (element by element otherwise), sums carried in double, no atomics (two runs give the same bits),
// a tiny second launch for the reduction over rows.
// Forward: p = exp(s - max) / sum exp(s - max), log p = (s - max) - log(sum): the max shift keeps logits of any finite magnitude finite,
// and the soft-max is carried as the triple (max, 1 / sum, log sum) rather than as one lse = max + log(sum), whose fp32 rounding would
// tilt every probability of a row by the same 1e-6.  A row of up to 4096 floats is read ONCE and stays in registers (16 floats per
// thread and operand) across the max / sum / loss passes; longer or ragged rows are re-read (L2-resident).  The forward stores per row
// what the backward needs (the triple of each operand and one or two scalars), so the backward is one sweep.
#include "softmax_rows.h"      // Row / each2 / row_map, the block reductions, reduce_rows_k
#include "losses.h"

namespace {
// The soft-max of one row: p_i = exp(x_i - mx) * inv, log p_i = (x_i - mx) - lsum.  Kept per row in `stats` as three floats.
struct Sm {
    float mx, inv, lsum;
    __device__ __forceinline__ Sm() {}
    __device__ __forceinline__ Sm(float m, double sum) : mx(m), inv((float)(1.0 / sum)), lsum((float)log(sum)) {}
    __device__ __forceinline__ Sm(const float* st, size_t R, size_t r) : mx(st[r]), inv(st[R + r]), lsum(st[2 * R + r]) {}
    __device__ __forceinline__ void store(float* st, size_t R, size_t r) const { st[r] = mx; st[R + r] = inv; st[2 * R + r] = lsum; }
    __device__ __forceinline__ float p(float x) const { return expf(x - mx) * inv; }
    __device__ __forceinline__ float lp(float x) const { return (x - mx) - lsum; }
};
// soft-max triples of two rows (b may be the same row as a)
__device__ __forceinline__ void softmax2(const Row& a, const Row& b, Sm& sa_, Sm& sb_, double* red, float* redf) {
    float ma = -INFINITY, mb = -INFINITY;
    each2(a, b, [&](int, float x, float y) { ma = fmaxf(ma, x); mb = fmaxf(mb, y); });
    block_max2_f(ma, mb, redf);
    double sa = 0.0, sb = 0.0;
    each2(a, b, [&](int, float x, float y) { sa += (double)expf(x - ma); sb += (double)expf(y - mb); });
    block_sum2_d(sa, sb, red);
    sa_ = Sm(ma, sa);
    sb_ = Sm(mb, sb);
}

// JointsKLLoss (loss.py:82-95): q = (g + eps) / sum(g + eps); rows[r] = w[r] * sum_i (xlogy(q_i, q_i) - q_i * log p_i)
// stats [5][R]: the soft-max triple, sum(g + eps), sum_i q_i
__global__ __launch_bounds__(TPB) void kl_fwd_k(const float* __restrict__ s, const float* __restrict__ g, const float* __restrict__ w, float eps,
                                                int R, int HW, float* __restrict__ rows, float* __restrict__ stats) {
    __shared__ double red[2 * TPB / 64];
    __shared__ float redf[2 * TPB / 64];
    const size_t r = blockIdx.x;
    const Row S(s + r * HW, HW), G(g + r * HW, HW);
    float mx = -INFINITY, unused = -INFINITY;
    each2(S, S, [&](int, float x, float) { mx = fmaxf(mx, x); });
    block_max2_f(mx, unused, redf);
    double se = 0.0, sg = 0.0;
    each2(S, G, [&](int, float x, float y) { se += (double)expf(x - mx); sg += (double)(y + eps); });
    block_sum2_d(se, sg, red);
    const Sm sm(mx, se);
    const float gs = (float)sg;
    const double lsum = log(se);
    double l = 0.0, sq = 0.0;
    // the value's terms in double (q log q and q log p cancel to about half their size: the device library's logf, good to an ulp, left the
    // mean over 512 rows an fp32 ulp off); sum_i q_i of the fp32 q_i that the backward forms
    each2(S, G, [&](int, float x, float y) {
        const double q = ((double)y + (double)eps) / sg;        // (0 / 0 = NaN for an all-zero row with eps = 0, as in torch)
        const double xl = q == 0.0 ? 0.0 : q * log(q);          // torch.xlogy: 0 where q == 0
        l += xl - q * (((double)x - (double)mx) - lsum);
        sq += (double)((y + eps) / gs);
    });
    block_sum2_d(l, sq, red);
    if (threadIdx.x == 0) {
        rows[r] = w ? (float)l * w[r] : (float)l;
        sm.store(stats, R, r);
        stats[3 * (size_t)R + r] = gs; stats[4 * (size_t)R + r] = (float)sq;
    }
}
// EntLoss (loss.py:103-117): rows[r] = -sum p log p / log(HW); stats [4][R]: the soft-max triple, H_r = -sum p log p
__global__ __launch_bounds__(TPB) void ent_fwd_k(const float* __restrict__ s, int R, int HW, double log_hw, float* __restrict__ rows,
                                                 float* __restrict__ stats) {
    __shared__ double red[2 * TPB / 64];
    __shared__ float redf[2 * TPB / 64];
    const size_t r = blockIdx.x;
    const Row S(s + r * HW, HW);
    float mx = -INFINITY, unused = -INFINITY;
    each2(S, S, [&](int, float x, float) { mx = fmaxf(mx, x); });
    block_max2_f(mx, unused, redf);
    double se = 0.0, z = 0.0;
    each2(S, S, [&](int, float x, float) { se += (double)expf(x - mx); });
    block_sum2_d(se, z, red);
    const Sm sm(mx, se);
    double h = 0.0;
    each2(S, S, [&](int, float x, float) { h -= (double)(sm.p(x) * sm.lp(x)); });
    block_sum2_d(h, z, red);
    if (threadIdx.x == 0) { rows[r] = (float)(h / log_hw); sm.store(stats, R, r); stats[3 * (size_t)R + r] = (float)h; }
}
// The consistency losses on probabilities.  mode 0, ConsSoftmaxLoss (loss.py:139-152): e_i = (p_i - pt_i)^2, scalar sum_j v_j p_j (p_j - pt_j);
// mode 1, ConsKLLoss(log_target=True): e_i = pt_i (log pt_i - log p_i), scalar sum_j v_j pt_j; mode 2, ConsKLLoss as the reference
// evaluates it (loss.py:160-173, KLDivLoss given LOG-probabilities as its target): t = log pt_i, e_i = xlogy(t, t) - t log p_i - NaN
// wherever t < 0 - scalar sum_j v_j t_j.  rows[r] = m_r * sum_i v_i e_i; stats [7][R]: the student's triple, the teacher's, the scalar.
// valid: optional per-pixel selection [R/Kc][HW] (a selection, not a factor: an unselected NaN stays out).
template <int MODE>
__global__ __launch_bounds__(TPB) void cons_fwd_k(const float* __restrict__ s, const float* __restrict__ t, const unsigned char* __restrict__ mask,
                                                  const unsigned char* __restrict__ valid, int Kc, int R, int HW, float* __restrict__ rows,
                                                  float* __restrict__ stats) {
    __shared__ double red[2 * TPB / 64];
    __shared__ float redf[2 * TPB / 64];
    const size_t r = blockIdx.x;
    const Row S(s + r * HW, HW), T(t + r * HW, HW);
    const unsigned char* pv = valid ? valid + (r / Kc) * HW : nullptr;
    Sm ss, st;
    softmax2(S, T, ss, st, red, redf);
    double l = 0.0, a = 0.0;
    each2(S, T, [&](int i, float x, float y) {
        if (pv && !pv[i]) return;
        if (MODE == 0) {
            const float p = ss.p(x), d = p - st.p(y);
            l += (double)(d * d);
            a += (double)(p * d);
        } else if (MODE == 1) {
            const float q = st.p(y);
            l += (double)(q * (st.lp(y) - ss.lp(x)));
            a += (double)q;
        } else {
            const float lq = st.lp(y);
            l += (double)((lq == 0.f ? 0.f : lq * logf(lq)) - lq * ss.lp(x));
            a += (double)lq;
        }
    });
    block_sum2_d(l, a, red);
    if (threadIdx.x == 0) {
        rows[r] = mask ? (float)l * (mask[r] ? 1.f : 0.f) : (float)l;
        ss.store(stats, R, r);
        st.store(stats + 3 * (size_t)R, R, r);
        stats[6 * (size_t)R + r] = (float)a;
    }
}

// ds_i = gscale / R * w_r * (p_i * sum_j q_j - q_i)
__global__ __launch_bounds__(TPB) void kl_bwd_k(const float* __restrict__ s, const float* __restrict__ g, const float* __restrict__ w, float eps,
                                                const float* __restrict__ stats, const float* __restrict__ gscale, int R, int HW,
                                                float* __restrict__ ds) {
    const size_t r = blockIdx.x;
    const Sm sm(stats, R, r);
    const float gs = stats[3 * (size_t)R + r], sq = stats[4 * (size_t)R + r];
    const float c = (gscale ? gscale[0] : 1.f) / (float)R * (w ? w[r] : 1.f);
    row_map(s + r * HW, g + r * HW, ds + r * HW, HW, [&](int, float x, float y) { return c * (sm.p(x) * sq - (y + eps) / gs); });
}
// ds_i = -gscale / count * sel_r * p_i * (log p_i + H_r) / log(HW)
__global__ __launch_bounds__(TPB) void ent_bwd_k(const float* __restrict__ s, const float* __restrict__ rows, const float* __restrict__ stats,
                                                 const float* __restrict__ count, const float* __restrict__ gscale, float thr, int R, int HW,
                                                 double log_hw, float* __restrict__ ds) {
    const size_t r = blockIdx.x;
    const Sm sm(stats, R, r);
    const float h = stats[3 * (size_t)R + r];
    const bool sel = !(thr > 0.f) || rows[r] < thr;
    const float c = sel ? -(float)((double)(gscale ? gscale[0] : 1.f) / ((double)count[0] * log_hw)) : 0.f;
    row_map(s + r * HW, nullptr, ds + r * HW, HW, [&](int, float x, float) { return c * sm.p(x) * (sm.lp(x) + h); });
}
// mode 0: ds_i = 2 c m_r p_i (v_i (p_i - pt_i) - A_r); modes 1 / 2: ds_i = c m_r (p_i A_r - v_i u_i), u = pt (1) or log pt (2);
// c = gscale / (R * HW), or gscale / (Kc * count) with a valid_mask
template <int MODE>
__global__ __launch_bounds__(TPB) void cons_bwd_k(const float* __restrict__ s, const float* __restrict__ t, const unsigned char* __restrict__ mask,
                                                  const unsigned char* __restrict__ valid, const float* __restrict__ count, int Kc,
                                                  const float* __restrict__ stats, const float* __restrict__ gscale, int R, int HW,
                                                  float* __restrict__ ds) {
    const size_t r = blockIdx.x;
    const Sm ss(stats, R, r), st(stats + 3 * (size_t)R, R, r);
    const float a = stats[6 * (size_t)R + r];
    const unsigned char* pv = valid ? valid + (r / Kc) * HW : nullptr;
    const double den = valid ? (double)Kc * (double)count[0] : (double)R * (double)HW;
    const float c = (float)((double)(gscale ? gscale[0] : 1.f) / den) * (mask ? (mask[r] ? 1.f : 0.f) : 1.f);
    row_map(s + r * HW, t + r * HW, ds + r * HW, HW, [&](int i, float x, float y) {
        const float p = ss.p(x);
        const bool v = !pv || pv[i];
        if (MODE == 0) return 2.f * c * p * ((v ? p - st.p(y) : 0.f) - a);
        return c * (p * a - (v ? (MODE == 1 ? st.p(y) : st.lp(y)) : 0.f));
    });
}
}  // namespace

#define SML_ARGS(cond) if (R <= 0 || HW <= 0 || (cond)) return UDAPOSE_ERR_ARG

// group: rows per output value (R for reduction='mean', K for the reference's 'none' = loss.mean(dim=-1) of the [B,K] rows)
int sml_kl_fwd(hipStream_t st, const float* s, const float* g, const float* w, float eps, int R, int group, int HW, float* rows, float* stats,
               float* out) {
    SML_ARGS(!s || !g || !rows || !stats || !out || group < 1 || R % group);
    hipLaunchKernelGGL(kl_fwd_k, dim3(R), dim3(TPB), 0, st, s, g, w, eps, R, HW, rows, stats);
    hipLaunchKernelGGL(reduce_rows_k, dim3(R / group), dim3(TPB), 0, st, rows, group, 0.f, (double)group, nullptr, 1, out, nullptr);
    return udapose_check_launch();
}
int sml_kl_bwd(hipStream_t st, const float* s, const float* g, const float* w, float eps, const float* stats, const float* gscale, int R, int HW,
               float* ds) {
    SML_ARGS(!s || !g || !stats || !ds);
    hipLaunchKernelGGL(kl_bwd_k, dim3(R), dim3(TPB), 0, st, s, g, w, eps, stats, gscale, R, HW, ds);
    return udapose_check_launch();
}
int sml_ent_fwd(hipStream_t st, const float* s, int R, int group, int HW, float thr, float* rows, float* stats, float* out, float* count) {
    SML_ARGS(!s || !rows || !stats || !out || !count || group < 1 || R % group || (thr > 0.f && group != R));
    hipLaunchKernelGGL(ent_fwd_k, dim3(R), dim3(TPB), 0, st, s, R, HW, log((double)HW), rows, stats);
    hipLaunchKernelGGL(reduce_rows_k, dim3(R / group), dim3(TPB), 0, st, rows, group, thr, (double)group, nullptr, 1, out, count);
    return udapose_check_launch();
}
int sml_ent_bwd(hipStream_t st, const float* s, const float* rows, const float* stats, const float* count, const float* gscale, float thr, int R,
                int HW, float* ds) {
    SML_ARGS(!s || !rows || !stats || !count || !ds);
    hipLaunchKernelGGL(ent_bwd_k, dim3(R), dim3(TPB), 0, st, s, rows, stats, count, gscale, thr, R, HW, log((double)HW), ds);
    return udapose_check_launch();
}
int sml_cons_fwd(hipStream_t st, int mode, const float* s, const float* t, const unsigned char* mask, const unsigned char* valid,
                 const float* count, int R, int Kc, int HW, float* rows, float* stats, float* out) {
    SML_ARGS(!s || !t || !rows || !stats || !out || (valid && (!count || Kc < 1 || R % Kc)));
    if (!valid) Kc = 1;
    if (mode == 0) hipLaunchKernelGGL(cons_fwd_k<0>, dim3(R), dim3(TPB), 0, st, s, t, mask, valid, Kc, R, HW, rows, stats);
    else if (mode == 1) hipLaunchKernelGGL(cons_fwd_k<1>, dim3(R), dim3(TPB), 0, st, s, t, mask, valid, Kc, R, HW, rows, stats);
    else hipLaunchKernelGGL(cons_fwd_k<2>, dim3(R), dim3(TPB), 0, st, s, t, mask, valid, Kc, R, HW, rows, stats);
    hipLaunchKernelGGL(reduce_rows_k, dim3(1), dim3(TPB), 0, st, rows, R, 0.f, (double)R * (double)HW, valid ? count : nullptr, Kc, out, nullptr);
    return udapose_check_launch();
}
int sml_cons_bwd(hipStream_t st, int mode, const float* s, const float* t, const unsigned char* mask, const unsigned char* valid,
                 const float* count, const float* stats, const float* gscale, int R, int Kc, int HW, float* ds) {
    SML_ARGS(!s || !t || !stats || !ds || (valid && (!count || Kc < 1 || R % Kc)));
    if (!valid) Kc = 1;
    if (mode == 0) hipLaunchKernelGGL(cons_bwd_k<0>, dim3(R), dim3(TPB), 0, st, s, t, mask, valid, count, Kc, stats, gscale, R, HW, ds);
    else if (mode == 1) hipLaunchKernelGGL(cons_bwd_k<1>, dim3(R), dim3(TPB), 0, st, s, t, mask, valid, count, Kc, stats, gscale, R, HW, ds);
    else hipLaunchKernelGGL(cons_bwd_k<2>, dim3(R), dim3(TPB), 0, st, s, t, mask, valid, count, Kc, stats, gscale, R, HW, ds);
    return udapose_check_launch();
}
