// Host-side description of one convolution and the tap plans (fprop / dgrad / wgrad) the igemm kernels execute.
#pragma once
#include <atomic>
#include <mutex>
#include <vector>
#include "igemm.h"

// The dispatch policy inside the library: the public udapose_policy (every field is documented there, once) constructed with the
// measured production defaults.  A network plan owns a copy, a convolution call names one through ConvGeom::pol.
struct Policy : udapose_policy {
    Policy() : udapose_policy{} {
        igemm_tile = -1; igemm_h3 = 1; igemm_lean = 1; igemm_short_lds = 1; igemm_tap0 = 1;
        wgrad_tile = -1; wgrad_ksplit = -1; wgrad_fastgeo = 2;
        wgrad_group = 1; wgrad_stages = 128; wgrad_group_stem = 1;
        bn_bwd_fused = 1; bn_fwd_chunked = 1; bn_bwd_chunked = 1; bn_bwd_pre_legacy = 0;
        igemm_wg_min = 512; wgrad_row3 = 1; bn3_mask = 1; stem_fused = 1; debug_sync = 0;
        igemm_big_min = 0; patch_conv = 2; eval_fold = 1; bn_xcd_rows = 1; wgrad_det = 1; igemm_ns3_k = 0;
        timeline = nullptr; wgrad_order = 1; wgrad_fastgeo_strided = 1;
    }
};
inline const Policy& default_policy() { static const Policy p; return p; }

// Allow `Kernel` `bytes` of dynamic LDS.  hipFuncSetAttribute is a per-DEVICE property of a kernel: set once per (kernel, device ordinal).
template <auto Kernel>
inline void max_dynamic_lds(int bytes) {
    static std::atomic<unsigned long long> done{0};
    static std::mutex mu;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return;
    std::lock_guard<std::mutex> lk(mu);
    if (done.load(std::memory_order_relaxed) & bit) return;
    (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    done.fetch_or(bit, std::memory_order_release);
}

struct ConvGeom {
    int N, Hi, Wi, Ci;      // logical input (for transposed: the small side)
    int Co, KH, KW, stride, pad;
    int transposed;         // 1 = ConvTranspose2d(k, stride, pad, output_padding = 0)
    int reflect;            // reflection padding (style net)
    int upsample;           // nearest x2 upsample folded into the loader (style decoder); Hi/Wi are the PHYSICAL dims
    const Policy* pol = nullptr;   // dispatch policy of this call (null: the default = production policy)
    const Policy& policy() const { return pol ? *pol : default_policy(); }
    int Ho() const { return transposed ? (Hi - 1) * stride - 2 * pad + KH : (((Hi << upsample) + 2 * pad - KH) / stride + 1); }
    int Wo() const { return transposed ? (Wi - 1) * stride - 2 * pad + KW : (((Wi << upsample) + 2 * pad - KW) / stride + 1); }
    bool smallc() const { return Ci == 8; }
    int KWp() const { return smallc() ? ((KW + 7) & ~7) : KW; }   // taps padded so that 8 taps fill a 64-wide K step
    int wtaps() const { return KH * KWp(); }
};

struct TapPlan {
    std::vector<IgTap> taps;
    int nclass = 1;
    IgClass cls[4];
    const IgTap* d_taps = nullptr;   // device copy (owned by the plan cache)
};

// direction 0: fprop (also the plan wgrad walks), 1: dgrad, 2: row-tap wgrad of a Ci == 8 conv.  Plans (a few hundred bytes of
// device memory each) are cached per (device, geometry class); building one allocates and copies synchronously, so a plan
// that is missing while `stream` is being captured is NOT built: the call returns null (UDAPOSE_ERR_NOT_PREPARED at the ABI).
// conv_prepare builds the plans of a geometry up front (udapose_conv_prepare / udapose_net_bind).
const TapPlan* get_tap_plan(const ConvGeom& g, int direction, hipStream_t stream = nullptr);
int conv_prepare(const ConvGeom& g);

int igemm_pick_tile(int M, int Co, int nclass, int K, int h3_ok, const Policy& pol);   // h3_ok: 3x3 stride-1 pad-1 same-size conv (conv_h3_ok)
int conv_h3_ok(const ConvGeom& g);
int igemm_stat_rows(int M, int Co, int nclass, int tile);
int igemm_launch(IgParams& p, int tile, hipStream_t stream, const Policy& pol);
int wgrad_pick_tile(int Rdim, int Cdim, int smallc, const Policy& pol);
int wgrad_launch(WgParams& p, int tile, int accumulate, hipStream_t stream, const Policy& pol);
// bit-reproducible per-layer form: split bz of the pixel reduction stores its partial tile at bz * Co*wtaps*Ci floats of `parts`
// (wgrad_parts_plan: the split count and tile of a problem; the caller adds the splits in split order)
int wgrad_parts_plan(int M, int Ci, int Co, int total_taps, int* tile_out);
int wgrad_launch_parts(WgParams& p, float* parts, hipStream_t stream);
// Grouped wgrad (many layers, one launch per tile class).  wgrad_group_plan completes p for the group kernels and returns
// the tile class (0 = 128x128, 1 = 64x64) or < 0 when the layer needs its own launch; stages_per_block bounds a work-group's
// pixel range (longer reductions are split and accumulated with fp32 atomics into a zeroed dW).
#define WG_STAMP_BLOCKS (1 << 17)   // work-groups of one plan's grouped launches (both classes, both passes) a Policy::timeline buffer must hold
#define WG_CLASSES 2      // tile classes of a grouped launch: 0 = 128x128, 1 = 64x64 (+ filter-row form)
int wgrad_group_plan(WgParams& p, int accumulate, int stages_per_block, const Policy& pol);
// the x / dy / dw fields of the table entries are byte offsets from the three bases
int wgrad_group_launch(hipStream_t stream, int tile, const WgParams* d_tab, const WgGroupBlk* d_blk, int per_xcd, const void* x_base,
                       const void* dy_base, void* dw_base, const WgParams* d_tab2 = nullptr, const WgGroupBlk* d_blk2 = nullptr,
                       const void* x_base2 = nullptr, const void* dy_base2 = nullptr, void* dw_base2 = nullptr,
                       unsigned long long* stamps = nullptr);     // stamps: [work-groups][8] timeline stamps (tuning), normally null

struct ConvEpilogue {
    const elem_t* res = nullptr;
    const float* bias = nullptr;
    const float* scale = nullptr;   // per-channel factor applied to the fp32 result before the bias (igemm path only; eval-mode BN folding)
    float* stats = nullptr;
    int relu = 0;
    int out_f32 = 0;
    int f32 = 0;            // x, w, res, y are fp32 (exact fp32 MFMA path; forward only)
    int split = 0;          // x, w, res (and y unless out_f32) are f16x2 split tensors: the fp32-grade mode (forward only)
};
// y = conv(x, w_fwd[Co][wtaps][Ci])
int conv_fprop(hipStream_t s, const ConvGeom& g, const elem_t* x, const elem_t* w_fwd, void* y, const ConvEpilogue& e);
// patch-staged forms of the style network's end layers (patchconv.hip); conv_fprop routes to them when patch_conv_ok
int patch_conv_ok(const ConvGeom& g, const ConvEpilogue& e);
int patch_conv_fprop(hipStream_t s, const ConvGeom& g, const void* x, const void* w_fwd, void* y, const ConvEpilogue& e);
// The BatchNorm whose backward consumes a dgrad's output (IgParams::bs_*): the dgrad epilogue masks dx with that BN's ReLU
// and leaves the partial sums of g and g * xhat in slab[rows][2][C]; `rows` is set by conv_dgrad.
struct DgradBnStat {
    const elem_t* y = nullptr;      // the BN's input (pre-BN conv output)
    const elem_t* z = nullptr;      // mask source (BN + residual + ReLU output) or null: mask recomputed from y
    const unsigned char* mask = nullptr;   // ... or the ReLU bit mask the forward saved (bit e of byte i: channel 8i+e of the flat NHWC tensor is > 0): 1/16 of z's bytes
    const float* mean = nullptr; const float* invstd = nullptr; const float* gamma = nullptr; const float* beta = nullptr;
    float* slab = nullptr;
    int rows = 0;
};
// dx = conv^T(dy, w_bwd[Ci][wtaps][Co]) (+ res)
int conv_dgrad(hipStream_t s, const ConvGeom& g, const elem_t* dy, const elem_t* w_bwd, void* dx, const elem_t* res, int out_f32,
               DgradBnStat* bs = nullptr);
// the stem's data gradient (stem_dgrad.hip): dx fp32 NCHW [N][3][H][W] = conv^T(dy NHWC [N][H/2][W/2][64], fp32 w [64][7][7][3] rounded to elem_t)
int stem_dgrad(hipStream_t s, const elem_t* dy, const float* w, int N, int H, int W, float* dx);
// dw (fp32, [Co][wtaps][Ci]; transposed: [Ci][wtaps][Co]) (+)= ...;  rows_valid < 0 -> all rows
int conv_wgrad(hipStream_t s, const ConvGeom& g, const elem_t* dy, const elem_t* x, float* dw, int accumulate, int rows_valid);
// the same problem as a parameter block (for the grouped launch); returns the layer's algorithmic FLOPs in *flops
int conv_wgrad_params(const ConvGeom& g, const elem_t* dy, const elem_t* x, float* dw, int rows_valid, WgParams* out, double* flops);
int conv_prof_before(hipStream_t s, int kind, double flops);
void conv_prof_after(hipStream_t s, int token);
int conv_stat_rows(const ConvGeom& g);
int conv_dgrad_stat_rows(const ConvGeom& g);   // rows of a DgradBnStat slab for this layer's dgrad
// saturation counters of the f16x2 stores in igemm.hip / patchconv.hip (common.h UDAPOSE_SP_SAT_READER)
unsigned long long sp_sat_read_igemm(int reset);
unsigned long long sp_sat_read_patchconv(int reset);
