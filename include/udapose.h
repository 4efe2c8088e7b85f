/* udapose.h - C ABI of libudapose_hip.so: the MI355X (gfx950) kernels behind the mean-teacher UDA pose-estimation
 * hot path of VisionLearningGroup/UDA_PoseEstimation.
 *
 * The reference has no FFI layer: its hot path is reached through Python modules (lib.models.pose_resnet*,
 * lib.models.loss, lib.models.Style_net, lib.keypoint_detection, utils).  Each entry point below names the reference
 * interface (file:line under the reference tree) whose device work it replaces; the Python shells in
 * uda_poseestimation_amd/ bind them with ctypes.
 *
 * Conventions: extern "C"; plain pointers and sizes; every pointer is a DEVICE pointer unless its name starts with
 * h_ (host) or the comment says "host array"; `stream` is a hipStream_t passed as void*; return 0 on success,
 * negative UDAPOSE_ERR_* otherwise.
 *
 * State and re-entrancy.  No entry point reads an environment variable or a mutable global to decide what it runs: the
 * dispatch policy is an explicit value (udapose_policy: per network plan, or named by a convolution descriptor; a
 * default-initialised one is the measured production policy).  Device-side tables are built only by the explicit
 * preparation calls - udapose_net_create / udapose_net_bind / udapose_net_bind_grads for a network plan,
 * udapose_conv_prepare for a single geometry - which allocate and copy synchronously and therefore must run outside stream
 * capture; every compute call (udapose_conv2d_*, udapose_net_forward / backward / pack_weights / apply_running, all the
 * element-wise and loss kernels) then neither allocates nor synchronises, and returns UDAPOSE_ERR_NOT_PREPARED instead of
 * building a missing table (a per-op convolution call on an unprepared geometry outside capture prepares it itself, once per
 * device, under a lock).  Distinct network plans may be driven concurrently from different host threads on different
 * streams; ONE plan is not re-entrant (its scratch workspace belongs to one call at a time).  Kernel attributes are set
 * once per device, so one process may drive several GPUs.
 * Activations are NHWC bf16 (fp16 in the fp16 build) unless stated; heat-maps are NCHW fp32.
 */
#ifndef UDAPOSE_H
#define UDAPOSE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define UDAPOSE_OK 0
#define UDAPOSE_ERR_ARG (-1)
#define UDAPOSE_ERR_LAUNCH (-2)
#define UDAPOSE_ERR_UNSUPPORTED (-3)
#define UDAPOSE_ERR_NOT_PREPARED (-4)   /* a device table this call needs was not built (udapose_net_bind*, udapose_conv_prepare) */

int udapose_version(void);
/* element type this build stores and multiplies: 0 = bf16 (libudapose_hip.so), 1 = fp16 (libudapose_hip_f16.so: the same
 * sources with -DUDAPOSE_ELEM_F16; every `void*` activation / packed-weight pointer below is then fp16) */
int udapose_elem_kind(void);

/* ---------------------------------------------------------------- convolution family
 * Replaces torch.nn.Conv2d / ConvTranspose2d as used by torchvision Bottleneck (lib/models/resnet.py:8-10,25-40),
 * Upsampling (lib/models/pose_resnet.py:33-43), the head (pose_resnet.py:74) and the VGG encoder / decoder
 * (lib/models/Style_net.py:32-118). */
/* Explicit dispatch policy.  The production policy - every default named below, what udapose_policy_default fills in - IS the measured one;
 * nothing in the library reads an environment variable or a mutable global to choose a kernel.  A network plan owns a copy
 * (udapose_net_set_policy), a single convolution call names one through its descriptor (udapose_conv_desc.policy, NULL = production).
 * The other values exist for tests (force a code path) and tuning (A/B runs through bench.py's flags).  One field per line: this list is
 * the one statement of the fields, and of their order, that the library and its ctypes binding are checked against. */
typedef struct {
    int igemm_tile;        /* default -1: the tile heuristics of the implicit GEMM; >= 0 forces that tile configuration id */
    int igemm_h3;          /* run-staged 3x3 form: 0 off, 1 (default) the measured per-shape policy, 2 / 3 force the 64- / 128-row form */
    int igemm_lean;        /* 1 (default): the lean 1x1 form (saddr LDS-DMA loads) where eligible */
    int igemm_short_lds;   /* 1 (default): one-stage LDS request for launches whose K loop is one stage */
    int igemm_tap0;        /* 1 (default): 1x1 kernels skip the tap-table read */
    int wgrad_tile;        /* default -1: heuristics; >= 0 forces that weight-gradient tile id */
    int wgrad_ksplit;      /* default -1: heuristics; > 0 forces the pixel-split count of a per-layer weight-gradient launch */
    int wgrad_fastgeo;     /* weight-gradient loader on power-of-two maps: 0 general, 1 bit-field pixel coordinates (pointer selects), 2 (default, the
                            * production form) the same through buffer loads to LDS with out-of-range zero fill and an unrolled ring (wgrad_fast2_body) */
    int wgrad_group;       /* 1 (default): udapose_net_backward runs one grouped weight-gradient launch per tile class; 0: layer by layer */
    int wgrad_stages;      /* default 128 (also what a value <= 0 means): 64-pixel stages a work-group of a grouped launch reduces before a layer's
                            * pixel range is split */
    int wgrad_group_stem;  /* 1 (default): the Ci == 8 stem joins the 64x64 group in its row-tap form */
    int bn_bwd_fused;      /* 1 (default): in the network backward, dgrad epilogues mask for the consumer BatchNorm and reduce its backward sums */
    int bn_fwd_chunked;    /* BatchNorm forward, finalize + apply of the wide, small-spatial layers in one channel-chunked launch where it pays: 0 off,
                            * 1 (default) on, > 1 on with that target work-group count instead of 1024 */
    int bn_bwd_chunked;    /* BatchNorm backward, channel-chunked forms without a finalize launch: 0 off, 1 (default) on, > 1 as bn_fwd_chunked's */
    int bn_bwd_pre_legacy; /* 0 (default); 1: BatchNorm backward from pre-reduced sums through the generic apply kernel (A/B) */
    int igemm_wg_min;      /* default 512: 128x64 tiles as soon as they give this many work-groups, else 64x64 (2 per CU measured best in-step) */
    int wgrad_row3;        /* 1 (default): weight gradients of 3x3 stride-1 convolutions with one work-group per (64x64 tile, filter row) - the row's
                            * three taps share one staged dy tile and one x window (a third of the LDS fill per FLOP, which is what bounds these
                            * kernels).  As fast as the 128x128 one-tap form alone; in the grouped launch with the 64x64 kernel at four work-groups
                            * per CU: 1366 vs 1387 us per pass alone, -0.10 ms per step */
    int bn3_mask;          /* 1 (default): block outputs save a ReLU bit mask in the forward that the masking data gradients read instead of z; 0: read z */
    int stem_fused;        /* stem: 0 separate launches, 1 (default) BN apply + ReLU + max-pool in one sweep, 2 = also the max-pool backward gathered
                            * inside the BN backward's two sweeps (0.2 GB less traffic, but 99 + 87 us against 55 + 30 + 48 us for the three separate
                            * launches: neutral in the step) */
    int debug_sync;        /* 0 (default); 1: network calls synchronise after every stage and report the first failing source line */
    int igemm_big_min;     /* > 0: 128x128 tiles (2-stage ring) for single-class launches with Co % 128 == 0 whose 128x64 grid has at least this
                            * many work-groups - the style network's large maps, run on one stream (+13-18 % there); 0 (default): never */
    int patch_conv;        /* reflection-padded 3x3 stride-1 convolutions (the style network) through the patch-staged kernels (input patch staged once,
                            * not once per tap): 0 never (the implicit GEMM for every layer), 1 the 64 -> 3 and 3 -> 64 end layers, 2 (default)
                            * the trunk layers too (128 pixels x 64 channels per work-group), 3 = 2 with 128 output channels per work-group in the
                            * 16-bit form where Co % 128 == 0 (measured equal to 2) */
    int eval_fold;         /* 1 (default): eval-mode network forwards (validate(), train_human.py:461-500) apply BatchNorm's running-statistics scale /
                            * shift, the residual and the ReLU in the convolution's epilogue: no BN-apply launch, no pre-BN tensor; 0: conv + apply */
    int bn_xcd_rows;       /* 1 (default): the BatchNorm apply kernels (forward and backward, chunked and streaming forms) give XCD k the k-th eighth of
                            * the pixel rows - what the implicit GEMMs' work-groups on XCD k wrote and will read (each XCD owns a contiguous range of
                            * m-tiles there) - so activations cross the conv <-> BatchNorm kernel boundaries through one L2
                            * (tools/probe/l2_handoff.hip: 17.9 against 6.7 TB/s); bit-identical results, -0.06..-0.15 ms per step
                            * (r4_ab_runs.txt); 0: interleaved */
    int wgrad_det;         /* 1 (default, round 6): split weight-gradient reductions of the grouped launches store per-split partial tiles into the pass's
                            * workspace and ONE launch adds them in split order (bit-reproducible gradients; the `loss.backward()` of
                            * train_human.py:436 run twice gives the same bits); 0: fp32 atomics into cleared tensors, arrival order (rounds 1-5) */
    int igemm_ns3_k;       /* 64x64 implicit-GEMM tiles take the 3-stage LDS ring from this reduction length on (K = taps x Ci), the 2-stage ring
                            * below it; 0 = the default, 2048 */
    void* timeline;        /* NULL (default), or a device buffer of uint64 [work-groups][8] for timeline stamps (tuning).  The grouped weight-gradient launches
                            * of a plan stamp {start, end (100 MHz), XCD, table slot, problem, stages | form bits (from bit 32: filter-row form, stem row-tap form, strided
                            * bit-field loader, transposed, stride 2), pass, tile rows} per work-group, the 128x128
                            * class first, the 64x64 class behind it: the buffer must hold 1 << 17 work-groups (8 MiB); a plan with more refuses */
    int wgrad_order;       /* grouped weight gradients, the deal of work-groups to the XCDs' lists (net.hip wg_deal): 1 (default) = layers cut into runs of 32 work-groups, the runs
                            * with the most stages per work-group first, so every list ends with its share of the short work-groups; 0 = whole
                            * (layer, split) units in deal order by unit load (rounds 1-6).  Same work into the same places either way: bit-identical gradients */
    int wgrad_fastgeo_strided; /* 1 (default): the weight-gradient layers that wgrad_fastgeo's loaders do not take although every map is a power of two - stride-2
                            * convolutions, stride-2 transposed convolutions (four sub-pixel classes), the stem's row-tap form - load through a bit-field
                            * geometry of their own (shifts for the two strides, 32-bit offsets, no divisions) instead of the general loader;
                            * 0: the general loader (exact divisions, 64-bit addresses).  No effect with wgrad_fastgeo = 0 or on other maps (384x384
                            * inputs: 96 / 48 / 24 wide).  Address generation only: bit-identical gradients.  Honoured by the grouped launches' plan and
                            * by the per-layer launch; like every field it takes effect when a plan's tables are built (udapose_net_bind_grads) */
} udapose_policy;
void udapose_policy_default(udapose_policy* p);

typedef struct {
    int N, Hi, Wi, Ci;   /* input NHWC (Ci multiple of 32, or exactly 8 for 3-channel images padded to 8) */
    int Co, KH, KW, stride, pad;
    int transposed;      /* 1: ConvTranspose2d(k, stride, pad), output_padding 0 */
    int reflect;         /* 1: ReflectionPad2d(pad) instead of zero padding */
    int upsample;        /* 1: input is read through nn.Upsample(scale_factor=2, mode='nearest') */
    const udapose_policy* policy;   /* host pointer, NULL = production policy */
} udapose_conv_desc;
/* builds (once per device) the small tap tables the three directions of this geometry use: the only allocation a convolution
 * ever needs; call it before capturing a stream that will run udapose_conv2d_* on the geometry */
int udapose_conv_prepare(const udapose_conv_desc* d);

#define UDAPOSE_EPI_RELU 1
#define UDAPOSE_EPI_OUT_F32 2
#define UDAPOSE_EPI_F32 4   /* x, w_fwd ([Co][taps][Ci] fp32), res and y are fp32: exact fp32 MFMA path (Ci multiple of 32 or 8) */
/* x, w_fwd, res - and y unless UDAPOSE_EPI_OUT_F32 - are "f16x2" split tensors: the FAST fp32-grade mode (forward only).  A split
 * tensor has the byte footprint and addressing of the fp32 tensor of the same shape; every group of 8 consecutive channels
 * (32 bytes) holds [8 x h fp16][8 x l fp16] with value = h + l * 2^-11, |value| <= 65504 (udapose_f32_to_split /
 * udapose_split_to_f32 convert).  The kernel multiplies with three v_mfma_f32_16x16x32_f16 per 32-deep K step (h.h, h.l, l.h; fp32
 * accumulation): products carry ~2^-22 relative error against the fp32 the reference computes the teacher, validate() and the
 * style network in (train_human.py:346-358,461-500), at 3/16 of the exact-fp32 MFMA's cost. */
#define UDAPOSE_EPI_SPLIT 8
void udapose_conv_out_hw(const udapose_conv_desc* d, int* Ho, int* Wo);
int udapose_conv_stat_rows(const udapose_conv_desc* d);
/* y[N,Ho,Wo,Co] = conv(x, w_fwd) (+bias[Co]) (+res) (ReLU); stats (optional): [stat_rows][2][Co] fp32 partial
 * (sum, sum of squares) of the fp32 result before bias/res - the BatchNorm batch statistics.  w_fwd: bf16 [Co][KH*KWp][Ci]. */
int udapose_conv2d_fwd(void* stream, const udapose_conv_desc* d, const void* x, const void* w_fwd, void* y, const void* res,
                       const float* bias, float* stats, int epilogue_flags);
/* dx[N,Hi,Wi,Ci] = conv^T(dy, w_bwd) (+res);  w_bwd: bf16 [Ci][KH*KW][Co]; out_f32: dx stored as fp32 (gradients that
 * feed a BatchNorm backward close to the loss, where the BN projection cancels most of the gradient) */
int udapose_conv2d_bwd_data(void* stream, const udapose_conv_desc* d, const void* dy, const void* w_bwd, void* dx, const void* res,
                            int out_f32);
/* The same dgrad when dx is the gradient dz entering a training-mode BatchNorm (+ReLU) whose input was bn_y [N,Hi,Wi,Ci] bf16:
 * the epilogue writes g = dz * mask to dx (mask: bn_z > 0 when bn_z is given - BN + residual + ReLU -, else
 * bn_y*gamma*invstd + (beta - mean*gamma*invstd) > 0, the forward's own expression) and one partial row per m-tile of
 * (sum g, sum g * (bn_y - mean) * invstd) to slab[rows][2][Ci] fp32, rows = the return value of udapose_conv_bwd_stat_rows.
 * That BatchNorm's backward then needs no reduction pass (reference: torch autograd of lib/models/resnet.py's
 * conv-bn-relu chains, train_human.py:338-444). */
int udapose_conv_bwd_stat_rows(const udapose_conv_desc* d);
int udapose_conv2d_bwd_data_bn(void* stream, const udapose_conv_desc* d, const void* dy, const void* w_bwd, void* dx, const void* res,
                               int out_f32, const void* bn_y, const void* bn_z, const float* bn_mean, const float* bn_invstd,
                               const float* bn_gamma, const float* bn_beta, float* slab);
/* dw fp32 [Co][KH*KWp][Ci] (transposed: [Ci][KH*KW][Co]) = (accumulate ? dw : 0) + sum_pixels dy * x.  This per-layer call splits long pixel
 * reductions over work-groups that add with fp32 atomics (arrival order: last-bit differences between runs; policy wgrad_ksplit = 1 forbids the
 * split); the network plans' grouped launches (udapose_net_backward*, udapose_net_wgrad_pair) are bit-reproducible (udapose_policy.wgrad_det). */
int udapose_conv2d_bwd_weight(void* stream, const udapose_conv_desc* d, const void* dy, const void* x, float* dw, int accumulate);
/* weight packing from fp32: cast (n % 8 == 0); per-tap transpose [A][T][B] -> [B][T][A]; strided gather with zero padding */
int udapose_cast_f32_bf16(void* stream, const float* src, void* dst, size_t n);
int udapose_transpose_cast(void* stream, const float* src, void* dst, int A, int T, int B);
int udapose_pack_strided(void* stream, const float* src, void* dst, int A, int KH, int KWp, int KW, int Bp, int B, long sa, long skh,
                         long skw, long sb);

/* ---------------------------------------------------------------- layout conversion at the NCHW fp32 boundary */
int udapose_nchw_f32_to_nhwc_bf16(void* stream, const float* src, void* dst, int N, int C, int HW, int Cpad);
/* the same into fp32 NHWC (style path at the reference's precision: it runs outside autocast, train_human.py:347-356) */
int udapose_nchw_f32_to_nhwc_f32(void* stream, const float* src, float* dst, int N, int C, int HW, int Cpad);
/* the same into an f16x2 split NHWC tensor (UDAPOSE_EPI_SPLIT), and the element-wise conversions fp32 <-> split (n % 8 == 0;
 * udapose_f32_to_split may run in place) */
int udapose_nchw_f32_to_nhwc_split(void* stream, const float* src, void* dst, int N, int C, int HW, int Cpad);
int udapose_f32_to_split(void* stream, const float* src, void* dst, size_t n);
int udapose_split_to_f32(void* stream, const void* src, float* dst, size_t n);
/* optional per-channel clamp lo/hi[C] = the "recover" clamp of train_human.py:32-33,276,351,356 */
/* src_is_f32: 0 = the library's 16-bit element type, 1 = fp32, 2 = f16x2 split */
int udapose_nhwc_to_nchw_f32(void* stream, const void* src, int src_is_f32, float* dst, int N, int C, int HW, int Cstride,
                             const float* lo, const float* hi);

/* ---------------------------------------------------------------- BatchNorm2d, training mode (torch.nn.BatchNorm2d in
 * .train(): 107 layers of the pose net, train_human.py:320-321) */
int udapose_bn_finalize(void* stream, const float* stats, int stat_rows, int C, double count, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps,
                        float* scale, float* shift, float* save_mean, float* save_invstd);
int udapose_bn_eval_coeff(void* stream, int C, const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, float eps, float* scale, float* shift);
int udapose_bn_apply(void* stream, const void* y, const void* res, void* z, size_t numel, int C, const float* scale, const float* shift,
                     int relu);
int udapose_bn_bwd_rows(size_t npix);
/* dz (bf16, or fp32 when dz_is_f32) -> dy (+ masked g); slab: [bn_bwd_rows][2][C] fp32 scratch, coef: [3][C] fp32 scratch.
 * relu: 0 = none; 1 = ReLU mask from the saved output z (z > 0); 2 = mask recomputed from y as y*gamma*invstd +
 * (beta - mean*gamma*invstd) > 0, the forward's own expression: z is not read (valid when the BN output had no residual
 * added before its ReLU); beta = the BN bias parameter, needed for relu == 2 only. */
int udapose_bn_bwd(void* stream, const void* dz, int dz_is_f32, const void* z, const void* y, void* dy, void* gout, size_t npix, int C,
                   const float* gamma, const float* save_mean, const float* save_invstd, int relu, float* slab, float* coef,
                   float* dgamma, float* dbeta, float beta_acc, const float* beta);
/* The same backward when the dgrad that produced the gradient already applied the ReLU mask and reduced it
 * (udapose_conv2d_bwd_data_bn): g (bf16, or fp32 when g_is_f32) and slab[rows][2][C] -> dgamma, dbeta (beta_acc*old + new) and
 * dy = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)); coef: [3][C] fp32 scratch.  No reduction pass over the activations. */
int udapose_bn_bwd_pre(void* stream, const void* g, int g_is_f32, const void* y, void* dy, size_t npix, int C, const float* gamma,
                       const float* save_mean, const float* save_invstd, const float* slab, int rows, float* coef, float* dgamma,
                       float* dbeta, float beta_acc);

/* Every BatchNorm form by explicit selectors instead of the default policy (what the executor picks from its plan's policy).  Each
 * returns a form code >= 0 - bit 0: the channel-chunked form took the layer, bit 1: the XCD row mapping was engaged - or a negative
 * error.
 * udapose_bn_train_fwd_ex: finalize + apply of one training-mode layer from the convolution's statistics slab[rows][2][C]; count = npix.
 * kind 0: y, res, z 16-bit; 1: fp32; 2: y fp32, res / z f16x2 split; 3: kind 2 plus the 'strict' shadows y16 = fp16(y), z16 = the
 * h half of z and, when mask is given, the ReLU bit mask of z16 (fp16 build only: UDAPOSE_ERR_UNSUPPORTED otherwise).  pre_bias: a
 * per-channel bias the producer added after its statistics (streaming form only).  fwd_chunked / xcd_rows: the policy fields
 * bn_fwd_chunked / bn_xcd_rows.  mask (kinds 0 and 3): one byte per 8 channels, bit e = stored z > 0.  scale, shift: [C] scratch of the
 * streaming form; save: [3][C] = mean, invstd, unbiased variance. */
int udapose_bn_train_fwd_ex(void* stream, int kind, const void* y, const void* res, void* z, size_t npix, int C, const float* slab, int rows,
                            const float* gamma, const float* beta, const float* pre_bias, float* running_mean, float* running_var,
                            long long* num_batches_tracked, float momentum, float eps, float* scale, float* shift, float* save, int relu,
                            int fwd_chunked, int xcd_rows, unsigned char* mask, void* y16, void* z16);
/* udapose_bn_bwd / udapose_bn_bwd_pre with the policy fields as arguments: chunked = bn_bwd_chunked (udapose_bn_bwd_pre_ex: | 1 << 30 for
 * XCD-aligned pixel ranges in the chunked form, | 1 << 29 in the streaming form), legacy = bn_bwd_pre_legacy. */
int udapose_bn_bwd_ex(void* stream, const void* dz, int dz_is_f32, const void* z, const void* y, void* dy, void* gout, size_t npix, int C,
                      const float* gamma, const float* save_mean, const float* save_invstd, int relu, float* slab, float* coef,
                      float* dgamma, float* dbeta, float beta_acc, const float* beta, int chunked);
int udapose_bn_bwd_pre_ex(void* stream, const void* g, int g_is_f32, const void* y, void* dy, size_t npix, int C, const float* gamma,
                          const float* save_mean, const float* save_invstd, const float* slab, int rows, float* coef, float* dgamma,
                          float* dbeta, float beta_acc, int chunked, int legacy);
/* The stem's fused forms (16-bit): y = maxpool3x3s2(relu(x*scale + shift)) with the winning taps, z never written; and the BatchNorm
 * backward (ReLU mask recomputed from y) whose incoming gradient is the max-pool backward of (pool_dy, pool_idx), gathered on the fly.
 * H x W: the pool's input size; npix = N*H*W; slab: [bn_bwd_rows(npix)][2][C]. */
int udapose_bn_relu_maxpool3x3s2(void* stream, const void* x, void* y, unsigned char* idx, int N, int H, int W, int C, const float* scale,
                                 const float* shift);
int udapose_bn_bwd_pooled(void* stream, const void* pool_dy, const unsigned char* pool_idx, int H, int W, const void* y, void* dy, size_t npix,
                          int C, const float* gamma, const float* save_mean, const float* save_invstd, float* slab, float* coef,
                          float* dgamma, float* dbeta, float beta_acc, const float* beta);
/* The deferred running-statistics update on its own: running = (1 - momentum) * running + momentum * saved, counter += 1, from the
 * statistics save[3][C] (mean, invstd, unbiased variance) a forward left.  _multi: njobs layers in one launch, as
 * udapose_net_apply_running does; d_jobs is a device table of njobs records { size_t save_off; float* running_mean; float* running_var;
 * long long* num_batches_tracked; int C; int pad; } whose save is at act + save_off; max_c >= every record's C. */
int udapose_bn_running_update(void* stream, const float* save, int C, float* running_mean, float* running_var,
                              long long* num_batches_tracked, float momentum);
int udapose_bn_running_update_multi(void* stream, const void* d_jobs, int njobs, int max_c, const void* act, float momentum);

/* ---------------------------------------------------------------- pooling (ResNet stem maxpool 3x3 s2 p1, resnet.py:30;
 * VGG MaxPool2d(2,2,ceil_mode=True), Style_net.py:72) */
int udapose_maxpool3x3s2_fwd(void* stream, const void* x, void* y, unsigned char* idx, int N, int H, int W, int C);
/* kind 0: 16-bit; 1: fp32; 2: f16x2 split; 3: split plus y16 = the pooled fp16 map (fp16 build only) */
int udapose_maxpool3x3s2_fwd_ex(void* stream, int kind, const void* x, void* y, unsigned char* idx, int N, int H, int W, int C, void* y16);
int udapose_maxpool3x3s2_bwd(void* stream, const void* dy, const unsigned char* idx, void* dx, int N, int H, int W, int C);
int udapose_maxpool2x2_ceil(void* stream, const void* x, void* y, int N, int H, int W, int C);
int udapose_maxpool2x2_ceil_f32(void* stream, const float* x, float* y, int N, int H, int W, int C);   /* fp32 NHWC (Style_net.py:72) */
int udapose_maxpool2x2_ceil_split(void* stream, const void* x, void* y, int N, int H, int W, int C);   /* f16x2 split NHWC */

/* ---------------------------------------------------------------- whole pose network (lib/models/pose_resnet.py:59-126:
 * PoseResNet.forward = head(upsampling(backbone(x)))), parameters by index in .parameters() order (host arrays of
 * device pointers), buffers in .buffers() order.  4-D weights are fp32 in channels_last physical layout. */
typedef void* udapose_net_t;
/* fp32 == 1: fp32 activations and exact fp32 MFMA, FORWARD ONLY (the reference runs the teacher and validate() in fp32,
 * train_human.py:347-358,461-500); fp32 == 2: the fast fp32-grade form of the same (f16x2 split activations and weight packs,
 * UDAPOSE_EPI_SPLIT; pre-BatchNorm conv outputs and statistics in fp32), FORWARD ONLY; fp32 == 0: the library's 16-bit
 * element type with fp32 accumulation, forward and backward.
 * fp32 == 3 ('strict', the fp16 build only; not with bit 9): a DIFFERENTIABLE plan with the fp32-grade forward of fp32 == 2 and the
 * 16-bit backward of fp32 == 0.  Its forward's outputs and BatchNorm statistics are bit for bit those of fp32 == 2; its BN apply,
 * max-pool and image conversion launches also write, in the same pass, the fp16 tensors the 16-bit backward reads (pre-BN y rounded
 * from the fp32 y, post-BN z = the h half of the split z, the block outputs' ReLU bit mask, the pooled map and its taps, the 8-channel
 * image) at the offsets of the fp32 == 0 layout, so udapose_net_backward* run unchanged.  The backward is therefore NOT fp32-grade:
 * its gradients are those of the fp16 backward evaluated at fp32-grade activations, and need loss scaling as in fp32 == 0.  The
 * forward's split / fp32 tensors live in one set of scratch slots inside the plan's own arena (udapose_net_act_bytes: the 16-bit
 * arena + ~0.6 GB at N = 32, 256x256).  Weight packs: split forward packs and 16-bit data-gradient packs; udapose_net_fused_update
 * writes the latter in its sweep and refreshes the former with one pack launch after it (same job table as udapose_net_pack_weights). */
/* bit 8 of `fp32` (value | 0x100): the three deconvolutions carry a bias parameter (`deconv_with_bias=True`, lib/models/pose_resnet.py:
 * 15,41,96) - parameter order weight, bias, then the BatchNorm's, as in the reference's Upsampling. */
/* bit 9 of `fp32` (value | 0x200): a FORWARD-ONLY plan (the teacher's forwards under torch.no_grad(), train_human.py:346-372, and
 * validate(), :461-500): nothing is kept for a backward, so the pre- and post-BatchNorm tensors of all layers rotate through five
 * scratch buffers laid out by liveness (udapose_net_act_bytes: ~0.3 GB instead of 2.8 GB at N = 32, 256x256) and stay resident
 * in the L2s / the Infinity Cache; udapose_net_backward* and udapose_net_bind_grads return UDAPOSE_ERR_UNSUPPORTED on such a plan. */
int udapose_net_create(const int layers[4], int num_keypoints, int N, int H, int W, int fp32, udapose_net_t* out);
void udapose_net_destroy(udapose_net_t net);
int udapose_net_num_params(udapose_net_t net);
int udapose_net_num_buffers(udapose_net_t net);
long long udapose_net_param_numel(udapose_net_t net, int i);
size_t udapose_net_wpack_bytes(udapose_net_t net);
size_t udapose_net_act_bytes(udapose_net_t net);
size_t udapose_net_ws_bytes(udapose_net_t net);
void udapose_net_out_shape(udapose_net_t net, int shape[4]);
/* the plan's dispatch policy (set it before udapose_net_bind_grads: the grouped weight-gradient tables depend on it).  Tables keep
 * the policy they were built under (split form wgrad_det, split length wgrad_stages, wgrad_group_stem): after a change of these,
 * the backward returns UDAPOSE_ERR_NOT_PREPARED until udapose_net_ws_bytes has been asked again (size `ws` by its new answer) and
 * udapose_net_bind_grads has run for each gradient placement; it then equals a plan created with the new policy. */
int udapose_net_set_policy(udapose_net_t net, const udapose_policy* p);
int udapose_net_get_policy(udapose_net_t net, udapose_policy* p);
/* Preparation (allocates + copies synchronously; outside stream capture; repeat when a pointer changes):
 *   bind:        tap tables of every layer geometry, the weight-packing job tables for (h_params, wpack), the
 *                running-statistics job table for h_buffers (may be NULL for a plan that never defers them);
 *   bind_grads:  the grouped weight-gradient tables for this placement of the gradient tensors (they hold offsets relative
 *                to h_grads[0]: any other set of buffers with the same relative placement reuses them).
 * pack_weights / forward / apply_running / backward return UDAPOSE_ERR_NOT_PREPARED if what they are given was not bound. */
int udapose_net_bind(udapose_net_t net, const void* const* h_params, void* const* h_buffers, void* wpack);
int udapose_net_bind_grads(udapose_net_t net, void* const* h_grads);
int udapose_net_pack_weights(udapose_net_t net, void* stream, const void* const* h_params, void* wpack, int with_bwd);
int udapose_net_forward(udapose_net_t net, void* stream, const float* x_nchw, const void* const* h_params, void* const* h_buffers,
                        const void* wpack, void* act, void* ws, float* out_nchw, int training, float momentum);
/* training: bit 0 = batch statistics (train mode), bit 1 = do NOT update the running statistics in this call; apply them
 * later, in program order, with udapose_net_apply_running (two forwards of one module running on different streams). */
int udapose_net_apply_running(udapose_net_t net, void* stream, const void* act, void* const* h_buffers, float momentum);
/* y += x over n fp32 values (y, x 16-byte aligned): sum of per-pass gradient buffers */
int udapose_axpy_f32(void* stream, float* y, const float* x, size_t n);
int udapose_net_backward(udapose_net_t net, void* stream, const float* dout_nchw, const void* const* h_params, const void* wpack,
                         void* act, void* ws, void* const* h_grads, float beta);
/* The same backward in two calls, cut after the first block of layer3, for a data-parallel step that overlaps the gradient
 * all-reduce with the backward (replaces nn.DataParallel's reduce, train_human.py:145-148,436): part 1 = head, deconvs,
 * layer4, layer3 and the weight gradients of those layers - a contiguous suffix of .parameters() starting at
 * udapose_net_grad_split_param(), final when part 1 has run; part 2 = layer2, layer1, stem and theirs, continuing from the
 * gradient part 1 left in `ws` (same act / ws / grads / beta as part 1; dout is ignored). */
int udapose_net_backward_part(udapose_net_t net, void* stream, const float* dout_nchw, const void* const* h_params, const void* wpack,
                              void* act, void* ws, void* const* h_grads, float beta, int part);
/* The same with the two halves of a part separable: phase 0 = the gradient chain of `part` followed by its grouped weight-gradient
 * launches (= udapose_net_backward_part; part 0 = the whole backward); phase 1 = the chain only; phase 2 = the grouped
 * weight-gradient launches of `part` only, on ANY stream that has waited for the chain (every layer owns its dy buffer in `ws`):
 * one device: the weight gradients of part 1 run under the gradient chain of part 2. */
int udapose_net_backward_phase(udapose_net_t net, void* stream, const float* dout_nchw, const void* const* h_params, const void* wpack,
                               void* act, void* ws, void* const* h_grads, float beta, int part, int phase);
/* The grouped weight-gradient launches (phase 2) of TWO passes of one plan whose gradient chains (phase 1) have run - each with its
 * own act / ws arenas, gradient tensors and beta - as ONE launch per tile class: the two student passes of a mean-teacher step end
 * together and their weight gradients are exposed there; one grid of twice the size has half the tail.  The result always equals the two
 * udapose_net_backward_phase(..., phase 2) calls A then B: when the two passes' gradient tensors share any byte (h_grads_a == h_grads_b,
 * B accumulating onto A), or their tables differ, the call issues exactly those two launches in that order.
 * Determinism (round 6, udapose_policy.wgrad_det = 1, the default): a layer whose pixel range is split over several work-groups (layer1 / layer2,
 * the last deconvolution, the head, the stem) has every split store its partial tile into `ws`; one launch then adds the splits in split order
 * into the gradient tensor.  Two runs of a backward on the same inputs give the same bits (rounds 1-5 accumulated the splits with fp32
 * atomics in arrival order).  `ws` must have the size udapose_net_ws_bytes returns AFTER udapose_net_set_policy. */
int udapose_net_wgrad_pair(udapose_net_t net, void* stream, const void* act_a, void* ws_a, void* const* h_grads_a, float beta_a,
                           const void* act_b, void* ws_b, void* const* h_grads_b, float beta_b, int part);
/* udapose_net_wgrad_pair that MAY leave the split sums of the gradient tensors to the optimizer sweep: when both passes overwrite (beta 0),
 * share one table, cover the whole backward (part 0) and udapose_net_bind_update has bound an update table for h_grads_a's tensors after
 * udapose_net_bind_grads, the launch that adds the partial tiles is left out, *deferred = 1, and the NEXT udapose_net_fused_update - which must
 * be given h_grads_a and grad2_delta_bytes = the distance to h_grads_b's buffer - adds the partial tiles inside its sweep, in the same order, to
 * the same bits (one launch and the write + re-read of the split layers' sums less).  Until then the split layers' gradient TENSORS hold stale
 * values: a caller that wants them, or whose update does not run, calls udapose_net_split_sum_flush (the sums as their own launch; no-op
 * without a pending sum).  Any other weight-gradient call on the plan while a sum is pending fails with UDAPOSE_ERR_NOT_PREPARED.
 * Otherwise (*deferred = 0) it is udapose_net_wgrad_pair. */
int udapose_net_wgrad_pair_defer(udapose_net_t net, void* stream, const void* act_a, void* ws_a, void* const* h_grads_a, float beta_a,
                                 const void* act_b, void* ws_b, void* const* h_grads_b, float beta_b, int part, int* deferred);
int udapose_net_split_sum_flush(udapose_net_t net, void* stream);
/* Data gradient of the stem convolution (Conv2d(3, 64, 7, stride 2, pad 3, bias=False), resnet.py's conv1): the gradient of a loss with
 * respect to the network's INPUT.
 *   dx[n][c][iy][ix] = sum over co, ky, kx with 2*oy + ky - 3 == iy and 2*ox + kx - 3 == ix of dy[n][oy][ox][co] * w[co][c][ky][kx]
 * dy: NHWC [N][H/2][W/2][64] in the element type (16-byte aligned); w: the fp32 master weight in its channels-last memory layout
 * [64][7][7][3], rounded to the element type by the kernel (every data gradient of a plan reads element-type weights); dx: fp32 NCHW
 * [N][3][H][W], every element written (no prior clear), fp32 accumulation in one fixed order: no atomics, no workspace, no allocation,
 * capturable, and two calls give the same bits.  UDAPOSE_ERR_ARG: a null pointer, N < 1, H or W odd or below 8, dy not 16-byte aligned, dx
 * overlapping dy; nothing is launched then. */
int udapose_stem_dgrad(void* stream, const void* dy, const float* w, int N, int H, int W, float* dx);
/* The same launch on a plan's own tensors: dy = the stem's output gradient of the pass whose workspace is `ws`, w = h_params[stem weight].
 * Contract: valid once the gradient chain that holds the stem has been enqueued on `stream` (or on a stream `stream` waits for) with this
 * `ws` - udapose_net_backward, udapose_net_backward_part(part 2), or phase 0 / phase 1 of either through udapose_net_backward_phase - and
 * before `ws` is given to another pass; the stem's dy stays in `ws` for the grouped weight-gradient launch, so the call may come before or
 * after phase 2.  Stateless: the pass is named by `ws` alone, so two passes of one plan on two streams each hand in their own workspace.  dx
 * (fp32 NCHW [N][3][H][W] of the plan) carries the loss scale the backward's dout carried.  UDAPOSE_ERR_UNSUPPORTED: forward-only plans and
 * the fp32 / f16x2 modes (they keep nothing for a backward); 'strict' plans are supported (their backward is the fp16 one). */
int udapose_net_input_grad(udapose_net_t net, void* stream, const void* const* h_params, void* ws, float* dx);
/* Gradient-direction perturbation of an image batch inside a norm ball (csrc/perturb.hip).  x, g, out (and x0, the centre of
 * the ball; NULL: x0 = x): fp32 [N][C][HW] contiguous.  eps_dev, step_dev: DEVICE fp32 scalars, read by the launches (a captured launch follows
 * a host change of them); step_dev NULL: step = eps.  lo, hi: per-channel fp32 [C] clamp of the result (both or neither).
 *   mode UDAPOSE_PERTURB_L2, per sample:    u = g / ||g||_2; d = (x - x0) + step * u; if ||d||_2 > eps: d *= eps / ||d||_2; out = clamp(x0 + d)
 *                                          (x0 NULL and step_dev NULL: the one-step form x + eps * u, which runs no second norm)
 *   mode UDAPOSE_PERTURB_LINF, per element: d = clip((x - x0) + step * sign(g), -eps, eps); out = clamp(x0 + d); sign(0) = sign(NaN) = 0
 * A sample whose sum of squares of g is zero, infinite or NaN (g == 0, a non-finite element, or squares that overflow) gets
 * out = clamp(x) - x bit for bit without a clamp - and gnorm 0; the other samples are unaffected.  The sum of squares is formed in l2 always
 * and in linf when gnorm is given; linf without gnorm is ONE launch with no reduction and handles a non-finite g per element (sign).
 * gnorm [N] (may be NULL): ||g[n]||_2.  ws: udapose_perturb_ws_bytes(N, C, HW) bytes (4-byte aligned; may be NULL in linf without gnorm),
 * per-(sample, work-group) partial sums that every consumer adds in index order: no atomics, no allocation, capturable, two calls give the
 * same bits, and g scaled by 2^k gives the same out bits (range of k: perturb.hip).  16-byte accesses where HW % 4 == 0 and x, g, x0, out are
 * 16-byte aligned, 4-byte accesses otherwise.  out == x (in place) is allowed.  UDAPOSE_ERR_ARG, nothing launched: a null x, g, eps_dev or
 * out; a null ws where it is needed; N < 1; C * HW < 1; an unknown mode; one of lo / hi alone; out overlapping g.  UDAPOSE_ERR_UNSUPPORTED:
 * C * HW >= 2^31 - 1024. */
#define UDAPOSE_PERTURB_L2 0
#define UDAPOSE_PERTURB_LINF 1
long long udapose_perturb_ws_bytes(int N, int C, int HW);
int udapose_perturb(void* stream, const float* x, const float* g, const float* x0, int N, int C, int HW, int mode, const float* eps_dev,
                    const float* step_dev, const float* lo, const float* hi, void* ws, float* out, float* gnorm);
/* The deal of a grouped weight-gradient launch, as a pure host function (no device): unit i = nblk[i] work-groups of stages[i] 64-pixel stages.
 * Writes the runs of the eight XCD lists, XCD by XCD in list order, as entries (ent_xcd, ent_unit, ent_first = first work-group of the unit,
 * ent_count), at most `cap` of them, and returns how many entries there are (< 0: an error code); finish_out[8]: modelled finish time of each
 * list (128 resident work-groups per XCD, a work-group takes stages + 4).  order: udapose_policy.wgrad_order.  Outputs may be NULL. */
int udapose_wgrad_deal(const int* nblk, const int* stages, int n_units, int order, int* ent_xcd, int* ent_unit, int* ent_first, int* ent_count, int cap,
                       double* finish_out);
long long udapose_net_grad_split_param(udapose_net_t net);

/* ---------------------------------------------------------------- heat-map losses and decode (fp32 NCHW rows [R=B*K][HW]) */
/* JointsMSELoss (lib/models/loss.py:39-49): rows[r] = 0.5*w[r]*mean_hw((p-g)^2); mean_out = mean_r rows (reduction='mean') */
int udapose_joints_mse_fwd(void* stream, const float* pred, const float* gt, const float* w, int R, int HW, float* rows, float* mean_out);
/* d pred = gscale[0] * w[r] * (p-g) / (R*HW) */
int udapose_joints_mse_bwd(void* stream, const float* pred, const float* gt, const float* w, const float* gscale, int R, int HW,
                           float* dpred);
/* ConsLoss (lib/models/loss.py:124-132): mean_out = sum(mask*(s-t)^2)/(R*HW) */
int udapose_cons_loss_fwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, int R, int HW, float* rows,
                          float* mean_out);
int udapose_cons_loss_bwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const float* gscale, int R,
                          int HW, float* dstu);
/* ConsLoss(valid_mask=) (lib/models/loss.py:129-130: loss_map[valid_mask].mean()): `valid` [R/K][HW] selects (b,h,w) positions of
 * loss_map = mean over the K channels; valid_count = number of selected positions, on the device (udapose_mask_count):
 * mean_out = sum over selected of mask*(s-t)^2 / (K * valid_count) */
int udapose_mask_count(void* stream, const unsigned char* mask, size_t n, float* count);
int udapose_cons_loss_valid_fwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const unsigned char* valid,
                                const float* valid_count, int R, int K, int HW, float* rows, float* mean_out);
int udapose_cons_loss_valid_bwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const unsigned char* valid,
                                const float* valid_count, const float* gscale, int R, int K, int HW, float* dstu);
/* ---- soft-max losses (lib/models/loss.py:52-173).  Per row r: p_i = exp(s_i - max) / sum_j exp(s_j - max), log p_i = (s_i - max) - log sum.
 * Every forward writes rows[R] (the per-row loss) and stats (per-row scalars of the backward, layout [n][R]; a row's soft-max is the
 * triple max, 1 / sum, log sum) and then reduces rows into `out`; every backward is one sweep that needs the forward's stats.  gscale: device scalar (NULL = 1).  No atomics: results are bit-reproducible.
 * All return UDAPOSE_ERR_ARG for R <= 0, HW <= 0 or a null operand.
 * JointsKLLoss (loss.py:82-95): q = (g + eps) / sum(g + eps); rows[r] = w[r] * sum_i (xlogy(q_i, q_i) - q_i * log p_i), w optional.
 * out[R/group] = means over `group` consecutive rows: group = R is reduction='mean', group = K the reference's 'none'
 * (loss.mean(dim=-1) of the [B,K] rows).  stats [5][R]: the triple, sum(g + eps), sum_i q_i. */
int udapose_joints_kl_fwd(void* stream, const float* pred, const float* gt, const float* w, float epsilon, int R, int group, int HW, float* rows,
                          float* stats, float* out);
/* d pred_i = gscale[0] / R * w[r] * (p_i * sum_j q_j - q_i)   (reduction='mean') */
int udapose_joints_kl_bwd(void* stream, const float* pred, const float* gt, const float* w, float epsilon, const float* stats,
                          const float* gscale, int R, int HW, float* dpred);
/* EntLoss (loss.py:103-117): rows[r] = H_r / log(HW), H_r = -sum_i p_i log p_i.  threshold > 0 selects the rows below it (loss.py:111-112):
 * out[0] = their mean, count[0] = their number (0 selected: NaN); it needs group = R.  Otherwise out[R/group] = group means and
 * count[0] = group.  stats [4][R]: the triple, H_r. */
int udapose_entropy_loss_fwd(void* stream, const float* x, int R, int group, int HW, float threshold, float* rows, float* stats, float* out,
                             float* count);
/* dx_i = -gscale[0] / count[0] * sel_r * p_i * (log p_i + H_r) / log(HW), sel_r from rows[r] < threshold */
int udapose_entropy_loss_bwd(void* stream, const float* x, const float* rows, const float* stats, const float* count, const float* gscale,
                             float threshold, int R, int HW, float* dx);
/* ConsSoftmaxLoss (loss.py:139-152): ConsLoss on the two soft-maxes: out[0] = sum_r mask[r] sum_i (p_i - pt_i)^2 / (R*HW); with `valid`
 * ([R/K][HW], valid_count from udapose_mask_count) only the selected (b,h,w) positions, divided by K * valid_count (loss.py:149-150).
 * mask, valid optional.  stats [7][R]: the student's triple, the teacher's, A_r = sum_j v_j p_j (p_j - pt_j). */
int udapose_cons_softmax_fwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const unsigned char* valid,
                             const float* valid_count, int R, int K, int HW, float* rows, float* stats, float* out);
/* d stu_i = 2 c mask[r] p_i (v_i (p_i - pt_i) - A_r), c = gscale[0] / (R*HW) or gscale[0] / (K * valid_count) */
int udapose_cons_softmax_bwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const unsigned char* valid,
                             const float* valid_count, const float* stats, const float* gscale, int R, int K, int HW, float* dstu);
/* ConsKLLoss (loss.py:160-173), reduced like ConsSoftmaxLoss.  log_target = 0 is the reference as written: KLDivLoss(log_target=False) is
 * handed the teacher's LOG-probabilities t_i = log pt_i as its target and evaluates xlogy(t_i, t_i) - t_i * log p_i, NaN wherever
 * t_i < 0 (every map of more than one pixel).  log_target = 1 (an extension) is the divergence itself, pt_i * (log pt_i - log p_i).
 * stats [7][R]: the student's triple, the teacher's, S_r = sum_j v_j u_j with u = pt (log_target) or log pt. */
int udapose_cons_kl_fwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const unsigned char* valid,
                        const float* valid_count, int log_target, int R, int K, int HW, float* rows, float* stats, float* out);
/* d stu_i = c mask[r] (p_i S_r - v_i u_i) */
int udapose_cons_kl_bwd(void* stream, const float* stu, const float* tea, const unsigned char* mask, const unsigned char* valid,
                        const float* valid_count, int log_target, const float* stats, const float* gscale, int R, int K, int HW, float* dstu);
/* CORAL through n x n Gram matrices (GramCoralLoss; the reference's CoralLoss, lib/models/loss.py:176-208, without its D x D covariances).
 * src, tgt: fp32 NCHW [N][K][H][W].  down >= 1 is the reference's coral_downsample folded into the loads: maps of floor(H/down) x floor(W/down),
 * each element the mean of the central 2x2 pixels of its down x down block (even down) or the centre pixel (odd down).  D = K * floor(H/down) *
 * floor(W/down), Xc the batch-centred N x D data, Gab = Xa_c Xb_c^T, S = sum(Gss^2 + Gtt^2 - 2 Gst^2) / (N-1)^2 (clamped at 0):
 * loss[0] = sqrt(S) / (4 D^2).  The Gram matrices are accumulated by exact-fp32 MFMA in chains of 16 products that are added in fp64, one fp64
 * partial per work-group, added in fp64 in work-group order (a fixed association) and finished in fp64: no atomics, two runs agree to the bit.
 * coef: [MP][MP] floats, MP = 2N rounded up to a multiple of 32, written by the forward and read by the backward: k [Gss, -Gst; -Gst^T, Gtt],
 * k = 1 / (2 D^2 sqrt(S) (N-1)^2), and all zero where S == 0 (a zero gradient where torch's autograd gives NaN).
 * ws: udapose_coral_ws_bytes bytes, 8-byte aligned.
 * All three return UDAPOSE_ERR_ARG for a null pointer, N < 2, N > 64, down < 1, or a down-sampled map with no pixels. */
long long udapose_coral_ws_bytes(int N, int K, int H, int W, int down);
int udapose_coral_fwd(void* stream, const float* src, const float* tgt, int N, int K, int H, int W, int down, void* ws, float* coef, float* loss);
/* dsrc, dtgt [N][K][H][W]: gscale[0] (device scalar, NULL = 1) * d loss / d src, d tgt.  Every pixel is written (explicit zeros off the
 * down-sampling footprints): no prior clear. */
int udapose_coral_bwd(void* stream, const float* src, const float* tgt, const float* coef, const float* gscale, int N, int K, int H, int W,
                      int down, float* dsrc, float* dtgt);
/* Soft-argmax decode (no counterpart in the reference: lib.keypoint_detection.soft_argmax).  Per row h_i of hm [R][H*W], i = y*W + x:
 * (x*, y*) = the first flat arg-max in udapose_heatmap_argmax's order (NaN is the largest value), m = h_i*; O = the whole map
 * (window < 0) or {|x - x*| <= window, |y - y*| <= window} clipped to the map (window 0: the arg-max itself);
 * p_i = exp(beta (h_i - m)) / Z over O; coords[r] = (cx, cy) = (sum p_i x_i, sum p_i y_i) in pixel-index units, NOT zeroed where the
 * maximum is <= 0; maxvals[r] = m, the number udapose_heatmap_argmax returns.  A row whose maximum is NaN or +-inf gives NaN
 * coordinates.  beta must be finite and > 0 (UDAPOSE_ERR_ARG otherwise).  flat_idx [R] and stats [4][R] = (m, 1/Z, cx, cy) are what
 * the backward reads.  One block per row, sums in double, no atomics. */
int udapose_soft_argmax_fwd(void* stream, const float* hm, int R, int H, int W, float beta, int window, float* coords, float* maxvals,
                            int* flat_idx, float* stats);
/* d hm_i = beta p_i ((x_i - cx) dcoords[r][0] + (y_i - cy) dcoords[r][1]) in O, 0 outside (the full row is written); the arg-max
 * selection is a constant: nothing flows through the choice of window. */
int udapose_soft_argmax_bwd(void* stream, const float* hm, const float* dcoords, const int* flat_idx, const float* stats, int R, int H, int W,
                            float beta, int window, float* dhm);
/* Coordinate loss on the soft-argmax of hm (JointsSoftArgmaxLoss / ConsSoftArgmaxLoss): target [R][2] (x, y) in heat-map pixels,
 * rows[r] = f_r (l((cx - tx_r) / W) + l((cy - ty_r) / H)), l(d) = |d| (norm 0, "l1") or 0.5 d^2 (norm 1, "l2"),
 * f_r = weight[r] (float, may be NULL) * (mask[r] != 0) (bytes, may be NULL); out[g] = sum of the `group` rows of g / group
 * (group = R: the mean; group = K: per-sample means).  flat_idx [R] and stats [4][R] as above. */
int udapose_coord_loss_fwd(void* stream, const float* hm, const float* target, const float* weight, const unsigned char* mask, int R, int group,
                           int H, int W, float beta, int window, int norm, float* rows, int* flat_idx, float* stats, float* out);
/* d hm of the mean (group = R): the sweep of udapose_soft_argmax_bwd with dcoords[r] = gscale[0] / R * f_r *
 * (l'((cx - tx_r) / W) / W, l'((cy - ty_r) / H) / H); gscale is a device scalar (NULL: 1), so nothing is read back. */
int udapose_coord_loss_bwd(void* stream, const float* hm, const float* target, const float* weight, const unsigned char* mask, const int* flat_idx,
                           const float* stats, const float* gscale, int R, int H, int W, float beta, int window, int norm, float* dhm);
/* get_max_preds(_torch) (lib/keypoint_detection.py:9-37, utils.py:54-75) and rectify (utils.py:77-109): any output may
 * be NULL.  patch: [(2*rad+1)^2] fp32 Gaussian table built by the caller exactly as utils.py:93-98 does. */
int udapose_heatmap_argmax(void* stream, const float* hm, int R, int H, int W, float* maxvals, int* flat_idx, float* preds_xy,
                           float* rectified, const float* patch, int rad);
/* Skeleton-prior maps: generate_prior_map (utils.py:111-145) without its [B][K][K][H][W] tensors.  Every joint i decoded from a heat-map casts a
 * ring of radius mean[i][j] round itself for every joint j: t_ij(x, y) = exp(-(d_i - mean[i][j])^2 / (2 sigma^2)), d_i = |(x, y) - (cx_i, cy_i)|
 * (x pairs with preds_xy[..][0], y with [..][1]), and out[b][j] = sum_i f[i][j] t_ij.
 * udapose_prior_weights writes the [K][K] table w in one small launch.  Default mode (v3 = 0, utils.py:139-141): the soft-max over i of
 * -std[i][j] / gamma with the diagonal set to epsilon first, max subtracted: std = +inf weighs exactly 0, and so does the diagonal for K > 1
 * with the reference's epsilon = -10e10 (at K = 1 it weighs 1).  v3 = 1 (utils.py:132): 1 / (1 + std[i][j]), diagonal included; gamma and
 * epsilon are not read.  UDAPOSE_ERR_ARG: a null pointer, K < 1, gamma 0 or not finite, epsilon NaN; UDAPOSE_ERR_UNSUPPORTED: K > 64. */
int udapose_prior_weights(void* stream, const float* std_table, int K, float gamma, float epsilon, int v3, float* w);
/* coords [B][K][2], conf [B][K]: preds_xy and maxvals of udapose_heatmap_argmax (a row with a maximum <= 0 casts its rings from (0, 0), as in the
 * reference).  f = w (v3 = 0; conf may be NULL) or conf[b][i] * w[i][j] (v3 = 1, utils.py:133-136: negative and NaN confidences pass through).
 * out [B][K][H][W]; with hm [B][K][H][W] given, out = hm * map (one fp32 multiply; the reference's "multiplier for the original prediction map").
 * One work-group per image and run of 256 pixels; coordinates and tables staged in LDS ((2 K ceil8(K) + 2 K) * 4 bytes), d_i once per pixel and
 * pass of 8 outputs, one hardware exponential per term with log2(e) / (2 sigma^2) folded in.  Every element of out is written; no atomics, no
 * scratch, no allocation (capturable).  UDAPOSE_ERR_ARG: a null pointer (hm may be NULL), B, K, H or W < 1, sigma not finite or <= 0;
 * UDAPOSE_ERR_UNSUPPORTED: K > 64, H * W > 2^30.  Nothing is launched on an error. */
int udapose_prior_map(void* stream, const float* coords, const float* conf, const float* mean, const float* w, const float* hm, int B, int K, int H,
                      int W, float sigma, int v3, float* out);
/* The tables of a prior (the reference builds none: `prior` of utils.py:111 arrives from nowhere).  coords [M][K][2] fp32, visible [M][K] bytes
 * (non-zero = visible); acc fp64 [3][K][K] = (count, sum d, sum d^2) per pair (i, j) over the samples where both joints are visible, d in fp64
 * from the fp32 coordinates; the call ADDS to acc (the caller clears it once).  One work-group per pair, a fixed-order tree, one thread adds the
 * partial into acc: the same batches in the same order give the same bits.  UDAPOSE_ERR_ARG: a null pointer, M < 1, K < 1;
 * UDAPOSE_ERR_UNSUPPORTED: K > 64. */
int udapose_pair_dist_accumulate(void* stream, const float* coords, const unsigned char* visible, int M, int K, double* acc);
/* mean [K][K], std_table [K][K] fp32: sum d / n and the population standard deviation sqrt(max(sum d^2 / n - mean^2, 0)), computed in fp64
 * and rounded once.  A pair never seen: mean 0, std +inf, which weighs 0 in both modes of udapose_prior_weights. */
int udapose_pair_dist_finish(void* stream, const double* acc, int K, float* mean, float* std_table);
/* Flip test (the -f/--flip evaluation of the reference's animal scripts, train_animal.py:556; pairing tables lib/datasets/util.py:186-224):
 * the image side.  src [N][rows_per_image][W] fp32 (an NCHW image batch: rows_per_image = 3*H).  keep_original = 1: dst [2N][rows][W],
 * dst[0:N] = src and dst[N:2N][r][x] = src[r][W-1-x] - the batch and its mirror image in one launch; keep_original = 0: dst [N][rows][W]
 * holds the mirrored rows only.  16-byte accesses when W % 4 == 0 and both pointers are 16-byte aligned, element by element otherwise.
 * dst must not overlap src (UDAPOSE_ERR_ARG). */
int udapose_hflip_batch(void* stream, const float* src, float* dst, int N, size_t rows_per_image, int W, int keep_original);
/* Flip test: the heat-map side.  a, f, out [N][K][H][W] fp32; perm [K] a device table of partner joints (NULL: no pairs), an entry outside
 * [0, K) counts as k itself, so nothing outside f is ever read.  fb[n][k][y][x] = f[n][perm[k]][y][W-1-x] (flip back + channel swap);
 * s = fb (shift 0), or s[..][x] = fb[..][x-1] for x >= 1 and s[..][0] = fb[..][0] (shift 1: the one-pixel shift Simple Baselines gives the
 * flipped output).  mode 0: out = s (a may be NULL); mode 1: out = (a + s) * 0.5f, in fp32 in that order.  out may BE a (same thread, same
 * element); it must not overlap f, nor a partially (UDAPOSE_ERR_ARG).  maxvals [N*K], flat_idx [N*K], preds_xy [N*K][2] (each may be NULL)
 * are what udapose_heatmap_argmax returns for out, bit for bit, reduced in the same pass from the values just written: first flat index on
 * ties, NaN as the maximum, coordinates zeroed where the maximum is <= 0.  One work-group per (n, k) plane, no atomics, no scratch. */
int udapose_flip_merge(void* stream, const float* a, const float* f, const int* perm, int N, int K, int H, int W, int shift, int mode,
                       float* out, float* maxvals, int* flat_idx, float* preds_xy);
/* Sub-pixel decodes of hm [R][H*W] fp32 (no counterpart in the reference; the two decodes published with Simple Baselines and DARK,
 * "Distribution-Aware Coordinate Representation for Human Pose Estimation").  (x*, y*), m = maxvals[r] and flat_idx[r] are exactly what
 * udapose_heatmap_argmax returns for the row (first flat index on ties, NaN as the largest value; maxvals and flat_idx may be NULL).
 * Where m > 0 is false coords[r] = (0, 0), as get_max_preds gives, and nothing is refined; otherwise coords[r] = (x*, y*) + offset:
 * mode 0 (quarter): if 1 < x* < W-1 and 1 < y* < H-1 (both), offset = 0.25 * (sign(h[y*][x*+1] - h[y*][x*-1]),
 *   sign(h[y*+1][x*] - h[y*-1][x*])) with sign(0) = 0 and a NaN difference adding nothing.  Nothing is staged; kernel and sigma are ignored.
 * mode 1 (DARK): kernel odd, 3 <= kernel <= 31; sigma <= 0 selects 0.3 * ((kernel - 1) / 2 - 1) + 0.8 (2.0 at 11).  Taps
 *   t_i = exp(-(i - c)^2 / 2 sigma^2) / sum, c = (kernel - 1) / 2, computed in double and rounded to fp32.  g = the separable blur of the map
 *   (rows, then columns; zero padding of c on every side; taps added in ascending order), g *= m / max(g), g = log(max(g, 1e-10)).
 *   If 1 < x* < W-2 and 1 < y* < H-2, with the central differences at (x*, y*)
 *     dx = (g[y][x+1] - g[y][x-1]) / 2, dy likewise, dxx = (g[y][x+2] - 2 g[y][x] + g[y][x-2]) / 4, dyy likewise,
 *     dxy = (g[y+1][x+1] - g[y-1][x+1] - g[y+1][x-1] + g[y-1][x-1]) / 4,
 *   offset = -Hess^-1 (dx, dy)^T, Hess = [[dxx, dxy], [dxy, dyy]].  Three guards leave (x*, y*) unrefined where the published code divides
 *   regardless: max(g) > 0 is false (a positive peak in a negative surround: the scale m / max(g) has no meaning), det Hess == 0 (a flat or
 *   clamped neighbourhood), and an offset that is not finite (inf or NaN in the map).
 * One launch, one work-group per map.  Mode 1 stages the map in LDS and blurs it there (2 * H * W * 4 bytes: the map, then g, and the
 * row-blurred map), so g never reaches memory; it takes H * W <= UDAPOSE_REFINE_MAX_PIXELS (every kernel size; 64x64 and 96x96 fit) and
 * returns UDAPOSE_ERR_ARG beyond it, as for a null hm or coords, R, H or W < 1, a mode other than 0 or 1, a bad kernel or a sigma that is
 * NaN or +inf, with nothing launched.  No atomics, no scratch, fixed summation order: capturable, and two calls give the same bits. */
#define UDAPOSE_REFINE_MAX_PIXELS 19200
int udapose_refine_decode(void* stream, const float* hm, int R, int H, int W, int mode, int kernel, float sigma, float* coords, float* maxvals,
                          int* flat_idx);
/* Top-down inference, the image side: box crops (the reference's crop + Resize, lib/datasets/util.py:87-123, and crop_ori, util.py:235-287,
 * on the device).  frames [F][Hs][Ws][3] uint8; frame_idx [M] int32 (several boxes may name one frame); boxes [M][5] fp32 =
 * (cx, cy, bw, bh, rot_deg); mean3, std3 [3] fp32; all four are read from device memory, so a captured launch follows new boxes.
 * out_f32 [M or 2M][3][Ho][Wo] fp32 normalised (udapose_aug_to_tensor's expression; may be NULL, mean3 / std3 may be NULL then),
 * out_u8 [M or 2M][Ho][Wo][3] uint8 = min(255, floor(value + 0.5)) (may be NULL; not both); status [M] bytes.
 * Pixel i covers [i, i + 1).  sx = bw / Wo, sy = bh / Ho, (c, s) = (cos, sin)(rot) - exact for multiples of 90 degrees, else the fp64 value
 * rounded to fp32; tx = clamp(ceil(sx), 1, 8), ty likewise.  Output pixel (u, v) is the mean of tx * ty bilinear samples at
 *   dx = ((u + (i + 0.5) / tx) - Wo / 2) * sx, dy = ((v + (j + 0.5) / ty) - Ho / 2) * sy, X = cx + c dx - s dy, Y = cy + s dx + c dy,
 * each reading x0 = floor(X - 0.5) with weight X - 0.5 - x0 on x0 + 1 (the same in y); a tap outside the frame contributes 0 (zero padding
 * in pixel values, ahead of the normalisation); samples are added j-major, then divided by tx * ty: no atomics, the same bits every time.
 * A box more than 8 times the output size is under-sampled (the tap cap).  Exact in fp32 when sx, sy are in {1/2, 1, 2, 4, 8}, cx, cy are
 * multiples of 1/8 and rot is a multiple of 90.  mirror = 1: images M .. 2M-1 are the column-reversed crops, from the same reads.
 * status[m] = 1 and a crop of zero pixel values, with nothing of the frames read, for a box with a non-finite field, bw <= 0 or bh <= 0,
 * or a frame index outside [0, F); 0 otherwise.  UDAPOSE_ERR_ARG (nothing launched): a null required pointer or both outputs null,
 * F < 1, M < 1 or M > 65535, Ho or Wo outside [1, 1024], Hs or Ws outside [1, 8192], mirror other than 0 / 1. */
int udapose_box_crop(void* stream, const unsigned char* frames_u8, int F, int Hs, int Ws, const int* frame_idx, const float* boxes, int M,
                     int Ho, int Wo, const float* mean3, const float* std3, int mirror, float* out_f32, unsigned char* out_u8,
                     unsigned char* status);
/* The way back: coords [M][K][2] fp32 (x, y) in heat-map pixels of crop m (index i stands for input coordinate i * stride, generate_target's
 * convention) -> out [M][K][2] in pixels of the frame: (cx, cy) + R(rot) (((x stride_x, y stride_y) - (Wo / 2, Ho / 2)) * (sx, sy)), with
 * udapose_box_crop's sx, sy, c, s.  A refused box gives what its fields give (NaN for NaN).  UDAPOSE_ERR_ARG: a null pointer, M, K, Ho or
 * Wo < 1. */
int udapose_coords_to_image(void* stream, const float* coords, const float* boxes, int M, int K, float stride_x, float stride_y, int Ho, int Wo,
                            float* out);
/* Top-down inference, the instance layer: one pose per box -> distinct, scored poses (Simple Baselines' rescoring and greedy OKS-NMS; none in the
 * reference; csrc/pose_nms.hip).  No atomics, the same bits on every run.  Everywhere: 1 <= M <= UDAPOSE_NMS_MAX_POSES,
 * 1 <= K <= UDAPOSE_NMS_MAX_KEYPOINTS, else UDAPOSE_ERR_ARG with nothing launched, as for a null required pointer.
 * kp [M][K][2] fp32 (x, y) in frame pixels (8-byte aligned); conf [M][K]; boxes [M][5] = udapose_box_crop's; status [M] bytes (may be NULL: all
 * 0); box_score [M] (may be NULL: all 1); vis_thr, oks_thr [1] fp32 and sigmas [K] fp32 in device memory: a captured launch follows new values.
 * udapose_pose_rescore:
 *   score[m] = kscore * box_score[m], kscore = (sum of conf[m][k] over k with conf[m][k] > vis_thr, ascending k, fp32) / their count, 0 for none;
 *   area[m] = bw * bh (the fp32 product); refused[m] = 1 when status[m] != 0, a coordinate of kp[m], area[m] or score[m] is not finite, or
 *   area[m] <= 0; 0 otherwise.  order [M] int32: the poses by descending score (-0 = +0), equal scores by ascending index; refused poses last,
 *   by ascending index, whatever their scores.  order[rank] = m with rank = the number of poses ahead of m, counted over keys in LDS.
 *   All four outputs are required. */
#define UDAPOSE_NMS_MAX_POSES 4096
#define UDAPOSE_NMS_MAX_KEYPOINTS 64
int udapose_pose_rescore(void* stream, const float* kp, const float* conf, const float* boxes, const unsigned char* status, const float* box_score,
                         const float* vis_thr, int M, int K, float* score, int* order, float* area, unsigned char* refused);
/* Object-key-point similarity.  v_k = (2 sigmas[k])^2, d2_k = (x_i - x_j)^2 + (y_i - y_j)^2, e_k = d2_k / v_k / A * 0.5f, every step fp32 without
 * contraction, sums in ascending k.
 * Self form (kp_b, area_b, visible_b NULL, Mb = Ma): A = (area_i + area_j) * 0.5f + FLT_EPSILON, oks = (sum_k expf(-e_k)) / K; oks(i, j) and
 *   oks(j, i) are the same bits.  out [Ma][Ma] fp32 (may be NULL).  mask [Ma][ceil(Ma / 64)] 64-bit words (may be NULL; needs oks_thr): bit
 *   (j & 63) of word (j >> 6) of row i is set when i != j, frame_idx[i] == frame_idx[j] (frame_idx [Ma] int32, may be NULL: one frame),
 *   neither pose is refused (refused [Ma] bytes, may be NULL: none) and oks(i, j) > oks_thr; the bits past Ma are clear.
 * Rectangular form (kp_b [Mb][K][2], area_b [Mb] given; mask, frame_idx, refused NULL): predictions a against labelled poses b, COCO's
 *   convention: A = area_b[j] + FLT_EPSILON, oks = (sum of expf(-e_k) over k with visible_b[j][k] > 0) / their count, 0 for none
 *   (visible_b [Mb][K] fp32, may be NULL: every joint counts).  out [Ma][Mb] fp32.  area_a is not used and may be NULL.
 * A non-finite operand gives what the expressions give.  UDAPOSE_ERR_ARG as well when both outputs are NULL. */
int udapose_oks_matrix(void* stream, const float* kp_a, const float* area_a, int Ma, const float* kp_b, const float* area_b, const float* visible_b,
                       int Mb, int K, const float* sigmas, const int* frame_idx, const unsigned char* refused, const float* oks_thr, float* out,
                       unsigned long long* mask);
/* Greedy NMS over the self form's mask, by one wave: walk order[0 .. M); a pose that is not refused (refused may be NULL: none) and has not been
 * removed is kept, and removes every pose whose bit is set in its mask row.  (The mask holds same-frame pairs only, so one walk is per-frame
 * NMS.)  keep [M] bytes 0 / 1; n_keep [1] int32 = their sum; suppressed_by [M] int32 (may be NULL): the kept pose that removed m, -1 for a
 * kept and for a refused pose.  An entry of order outside [0, M) is passed over. */
int udapose_pose_nms_sweep(void* stream, const unsigned long long* mask, const int* order, const unsigned char* refused, int M, unsigned char* keep,
                           int* n_keep, int* suppressed_by);
/* The three launches behind one entry: rescore, the self form's mask (and the matrix into oks_out [M][M], may be NULL), the walk.  ws: device
 * memory of udapose_pose_nms_ws_bytes(M) bytes, 8-byte aligned (the mask, the areas, the refused flags; 0 bytes for an M out of range).
 * score, order, keep, n_keep are required, suppressed_by may be NULL.  Every argument is checked before the first launch: an error leaves
 * nothing written. */
long long udapose_pose_nms_ws_bytes(int M);
int udapose_pose_nms(void* stream, const float* kp, const float* conf, const float* boxes, const int* frame_idx, const unsigned char* status,
                     const float* box_score, const float* sigmas, const float* vis_thr, const float* oks_thr, int M, int K, void* ws, float* score,
                     int* order, unsigned char* keep, int* n_keep, int* suppressed_by, float* oks_out);
/* Key-point AP under OKS, COCO-style (cocoapi's evaluateImg + accumulate for key points; csrc/pose_ap.hip).  Detections
 * against labelled poses per frame -> records on the device -> precision / recall tables.  Integer atomics on the int64 counters only, no
 * floating-point atomics, nothing read back: every launch can be captured, and a replay appends again.
 * udapose_ap_match, one update.  Detections: kp [M][K][2] fp32 (8-byte aligned), score [M], frame_idx [M] int32, valid [M] bytes (may be
 *   NULL: all valid), area [M] (may be NULL: (max_k x - min_k x) * (max_k y - min_k y) in fp32).  Labels: gt_kp [G][K][2], gt_visible [G][K]
 *   fp32, > 0 counts (may be NULL: every joint), gt_area [G], gt_frame [G] int32, gt_ignore [G] bytes (may be NULL: none).  Frame ids are in
 *   [0, F).  sigmas [K], thresholds [T] (strictly ascending, the CALLER's duty) and ranges [A][2] = (lo, hi) are fp32 in device memory.
 *   Refused (counted, never in a curve): valid == 0, a score, coordinate or given area that is not finite, a frame outside [0, F).  A label on
 *   a frame outside [0, F) is dropped and counted.  Per frame the non-refused detections in descending score (-0 = +0), equal scores by
 *   ascending index; the first max_dets take part, the rest count in `cut`; a frame with more than UDAPOSE_AP_MAX_LABELS_PER_FRAME labels is
 *   left out whole (its labels and detections count nowhere but in `overflow_frames`).  oks(d, g): the bits of udapose_oks_matrix's
 *   rectangular form.  Per (t, a): label g is ignored when gt_ignore[g] != 0, it has no visible joint, gt_area[g] < lo or > hi; a detection
 *   starts with best = thresholds[t] and takes, over the not yet matched labels, counted ones first by ascending index and ignored ones only
 *   when no counted one was taken, every label whose oks is not < best (best = oks; among equal values the later label); matched, it takes
 *   its label's ignore flag; unmatched, it is ignored when its area is < lo or > hi.
 *   A record per detection that took part: rec_score, and bit a * T + t of rec_matched / rec_ignored.  Records are appended at
 *   counters[0] in ascending frame id, then in-frame order; those at or beyond `capacity` are dropped and counted.
 *   counters: int64 [UDAPOSE_AP_COUNTERS + A] = records, dropped, refused, cut, overflow_frames, bad_labels, then npig[a] (the counted labels
 *   of range a over all counted frames); the caller zeroes them once, a call adds.
 *   ws: udapose_ap_match_ws_bytes(M, G, F) bytes, 8-byte aligned (0 for sizes out of range).
 *   UDAPOSE_ERR_ARG, every check ahead of the first launch and nothing written: a null required pointer, M, G outside
 *   [1, UDAPOSE_NMS_MAX_POSES], F outside [1, UDAPOSE_AP_MAX_FRAMES], K outside [1, UDAPOSE_NMS_MAX_KEYPOINTS], T or A < 1 or
 *   T * A > UDAPOSE_AP_MAX_COMBOS, max_dets outside [1, UDAPOSE_AP_MAX_DETS], capacity outside [1, UDAPOSE_AP_MAX_CAPACITY].
 * udapose_ap_curve, the tables of the N = counters[0] records: sorted by descending score, equal scores by sequence number (stable); per
 *   (t, a) in fp64: tp = cumsum(matched & ~ignored), fp = cumsum(~matched & ~ignored), rc = tp / npig[a], pr = tp / (fp + tp + DBL_EPSILON),
 *   pr[i] = max(pr[i:]); per recall point r the first index q with rc[q] >= recall_points[r]: precision [T][R][A] fp64 = pr[q],
 *   scores [T][R][A] fp32 = the score of record q, both 0 without such an index; recall [T][A] fp64 = rc[N - 1], 0 for N = 0.  Where
 *   npig[a] == 0 all three are -1.  recall_points [R] fp64 in device memory, R <= UDAPOSE_AP_MAX_RECALL_POINTS.
 *   ws: udapose_ap_curve_ws_bytes(capacity, T, A) bytes, 8-byte aligned.  The records are not changed: more updates may follow. */
#define UDAPOSE_AP_MAX_FRAMES 4096
#define UDAPOSE_AP_MAX_LABELS_PER_FRAME 64
#define UDAPOSE_AP_MAX_DETS 64
#define UDAPOSE_AP_MAX_COMBOS 64
#define UDAPOSE_AP_MAX_RECALL_POINTS 128
#define UDAPOSE_AP_MAX_CAPACITY 262144
#define UDAPOSE_AP_COUNTERS 6
long long udapose_ap_match_ws_bytes(int M, int G, int F);
int udapose_ap_match(void* stream, const float* kp, const float* score, const int* frame_idx, const unsigned char* valid, const float* area, int M,
                     const float* gt_kp, const float* gt_visible, const float* gt_area, const int* gt_frame, const unsigned char* gt_ignore, int G,
                     int K, int F, const float* sigmas, const float* thresholds, int T, const float* ranges, int A, int max_dets, void* ws,
                     float* rec_score, unsigned long long* rec_matched, unsigned long long* rec_ignored, int capacity, long long* counters);
long long udapose_ap_curve_ws_bytes(int capacity, int T, int A);
int udapose_ap_curve(void* stream, const float* rec_score, const unsigned long long* rec_matched, const unsigned long long* rec_ignored,
                     int capacity, const long long* counters, int T, int A, const double* recall_points, int R, void* ws, double* precision,
                     float* scores, double* recall);
/* confidence mask (train_human.py:427-430): thr = k-th smallest of act[n]; mask[i] = (tea_mask[i]*act_local[i]) > thr */
int udapose_kth_mask(void* stream, const float* act, const float* tea_mask, int n, int k, float* thr_out, unsigned char* mask,
                     const float* act_local, int n_local);
/* The same launch with k read on the device: k_dev[0] is one int32 in device memory, loaded once at kernel entry and held inside 1 ... n, so
 * that a captured launch follows a ramped mask_ratio through a 4-byte copy.  For the same k the same kernel body gives the same bits.
 * UDAPOSE_ERR_ARG: a null act, k_dev or mask, n < 1 or n > 1 << 22. */
int udapose_kth_mask_dev(void* stream, const float* act, const float* tea_mask, int n, const int* k_dev, float* thr_out, unsigned char* mask,
                         const float* act_local, int n_local);
/* ---- joint selection by an order statistic over [N,K] rows (csrc/select.hip).  One launch each, sums in double in a fixed order, no
 * atomics on global memory: capturable, and two calls give the same bits.
 * udapose_topk_select: top-k mining over the per-(n,k) loss rows of udapose_joints_mse_fwd (null mean_out) or udapose_cons_loss_fwd.
 *   Per sample, joint j is BETTER than joint i when rows[j] > rows[i] (largest != 0; < otherwise) or the two are equal and j < i; values
 *   order as torch.kthvalue orders them (NaN is the largest).  rank(i) = the number of candidates better than i, sel[n*K+i] = rank < topk.
 *   A row whose factor is zero (wfac[r] == 0 or mfac[r] == 0; either table may be null) is no candidate when largest == 0 and always gets
 *   sel = 0, in either direction: with largest != 0 it keeps its place in the order, so fewer than topk joints may be selected.  The
 *   divisor stays topk:  sample[n] = (sum of the selected rows, in joint order, in double) / topk;
 *                        mean_out[0] = (sum_n sample[n], in sample order, in double) / N   (null: not written).
 *   K > 64: UDAPOSE_ERR_UNSUPPORTED (a wave holds a sample, a lane a joint).  topk outside 1 ... K, N < 1, N*K > 1 << 22 or a null rows /
 *   sel / sample: UDAPOSE_ERR_ARG.  On any refusal nothing is launched and nothing is written.
 * udapose_topk_sqdiff_bwd: da = gscale[0] * c * w[r] * (a - b) / (HW * topk * N) on the rows with sel != 0 and 0 elsewhere; c = 1 for the
 *   0.5 * square rows of JointsMSE (half != 0), 2 for the plain squares of ConsLoss (half == 0); w may be null.  The sweep of
 *   udapose_joints_mse_bwd with sel as its mask.
 * udapose_joint_kth_mask: for every joint j, thr_out[j] = the k-th smallest (1-indexed) of the n_pool values pool[i*K + j], and
 *   mask[i*K + j] = (tea_mask * act_local)[i*K + j] > thr_out[j] for the n_local rows of act_local (tea_mask may be null).  One work-group per
 *   joint, the radix select of udapose_kth_mask; NaN as there.  k < 1, k > n_pool, K < 1, a null pointer or more than 1 << 22 values:
 *   UDAPOSE_ERR_ARG.
 * udapose_joint_kth_mask_dev: the same launch with k read on the device (k_dev[0], one int32, held inside 1 ... n_pool), as
 *   udapose_kth_mask_dev; a null k_dev: UDAPOSE_ERR_ARG.
 * udapose_thr_mask: mask[i] = (tea_mask[i] * act[i]) > thr_dev[0], i < n; the threshold is read on the device. */
int udapose_topk_select(void* stream, const float* rows, const float* wfac, const unsigned char* mfac, int N, int K, int topk, int largest,
                        unsigned char* sel, float* sample, float* mean_out);
int udapose_topk_sqdiff_bwd(void* stream, const float* a, const float* b, const float* w, const unsigned char* sel, const float* gscale, int N,
                            int K, int HW, int topk, int half, float* da);
int udapose_joint_kth_mask(void* stream, const float* pool, int n_pool, int K, int k, const float* tea_mask, const float* act_local,
                           int n_local, float* thr_out, unsigned char* mask);
int udapose_joint_kth_mask_dev(void* stream, const float* pool, int n_pool, int K, const int* k_dev, const float* tea_mask, const float* act_local,
                               int n_local, float* thr_out, unsigned char* mask);
int udapose_thr_mask(void* stream, const float* act, const float* tea_mask, size_t n, const float* thr_dev, unsigned char* mask);
/* PCK (lib/keypoint_detection.py:40-94) from decoded coordinates [B,K,2]; acc[K], avg_cnt[2] = (avg_acc, cnt) */
int udapose_pck(void* stream, const float* pred_xy, const float* gt_xy, int B, int K, float norm_x, float norm_y, float thr, float* acc,
                float* avg_cnt);
/* ---- evaluation meter (csrc/pck_curve.hip): a PCK curve, the visible count and the end-point error of a whole set, kept on the device as
 * integers.  state is an int64 array [K][T + 3]; row k belongs to joint k and its columns are
 *     0 .. T-1 : hits[j], the visible (sample, joint) pairs with d < thr[j]
 *     T        : count, the visible pairs
 *     T + 1    : epe_q, the sum over the visible pairs with a finite error of llrintf(e * UDAPOSE_PCK_EPE_SCALE)
 *     T + 2    : nonfinite, the visible pairs whose e is NaN, infinite or >= 2^46 px (they add nothing to epe_q)
 * The caller zeroes state once; a call only ADDS, with integer adds alone (registers, wave shuffles, LDS integer atomics, one 64-bit
 * integer atomic per touched column), so the state after a set is the same bits whatever the batch split, the grid or the order of
 * arrival; no floating-point atomics, no scratch, no host synchronisation: capturable.
 * Per visible pair (b, k), prediction (px, py), target (tx, ty), every operation one correctly rounded fp32 operation (no FMA):
 *     e = sqrtf((px-tx)*(px-tx) + (py-ty)*(py-ty))                                    heat-map pixels
 *     norm == NULL: dx = px / nh - tx / nh, dy = py / nw - ty / nw, d = sqrtf(dx*dx + dy*dy)   (udapose_pck's expression: x over the
 *                   HEIGHT term nh = H / 10, y over nw = W / 10, the reference's pairing)
 *     norm [B]    : d = e / norm[b]; a norm[b] that is not finite and > 0 makes the sample's joints count as not visible
 *     threshold j is hit iff d < thr[j] (strict; a NaN d hits nothing and is still counted)
 * thr [T] fp32 on the device, strictly ascending (the CALLER's duty: it lives on the device, the first hit is found by bisection and the
 * columns equal the T independent compares only for an ascending table), 1 <= T <= UDAPOSE_PCK_MAX_THRESHOLDS.
 * udapose_pck_accumulate: pred_xy, gt_xy [B][K][2].  Visible: visible[b*K + k] != 0, or with a NULL visible the reference's rule on the
 *   target, tx > 1 && ty > 1.  One work-group per (joint, 256 samples), a lane per sample.
 * udapose_pck_accumulate_heatmaps: out, target [B][K][H][W]; one work-group per (b, k) reduces both planes (16-byte loads when H*W % 4 == 0
 *   and both pointers are 16-byte aligned) in udapose_heatmap_argmax's order, bit for bit: first flat index on ties, NaN as the largest
 *   value, (0, 0) where the maximum is <= 0.  nh = H / 10, nw = W / 10; visible by tx > 1 && ty > 1 on the target's arg-max.  preds_xy
 *   [B][K][2] (may be NULL) receives exactly what udapose_heatmap_argmax returns for out.  H * W <= 1 << 30.
 * UDAPOSE_ERR_ARG: a null required pointer (everything but visible, norm, preds_xy), B, K, T (H, W) < 1, T > UDAPOSE_PCK_MAX_THRESHOLDS,
 * B * K > INT_MAX.  UDAPOSE_ERR_UNSUPPORTED: K > UDAPOSE_PCK_MAX_KEYPOINTS.  On a refusal nothing is launched. */
#define UDAPOSE_PCK_MAX_THRESHOLDS 64
#define UDAPOSE_PCK_MAX_KEYPOINTS 256
#define UDAPOSE_PCK_EPE_SCALE 65536
int udapose_pck_accumulate(void* stream, const float* pred_xy, const float* gt_xy, const unsigned char* visible, const float* norm, int B, int K,
                           float nh, float nw, const float* thr, int T, long long* state);
int udapose_pck_accumulate_heatmaps(void* stream, const float* out, const float* target, const float* norm, int B, int K, int H, int W,
                                    const float* thr, int T, long long* state, float* preds_xy);

/* ---------------------------------------------------------------- optimizer sweeps over many tensors (device tables) */
int udapose_multi_chunk(void);
/* OldWeightEMA.step (utils.py:21-25): t = fl(fl(t*alpha) + fl(s*one_minus_alpha)), bit-exact two-rounding form */
int udapose_ema_multi(void* stream, const long long* tgt_ptrs, const long long* src_ptrs, const long long* sizes, const int* blk_tensor,
                      const long long* blk_off, int nblocks, float alpha, float one_minus_alpha);
/* The same sweep with the pair read on the device: ema_dev[0] = alpha, ema_dev[1] = one_minus_alpha, two fp32 values in device memory that
 * the host rounded exactly as it rounds the by-value pair (1 - alpha in double, each then to fp32).  The same two values enter the same
 * two-rounding expression: the same bits, and a captured launch follows a ramped teacher_alpha through an 8-byte copy. */
int udapose_ema_multi_dev(void* stream, const long long* tgt_ptrs, const long long* src_ptrs, const long long* sizes, const int* blk_tensor,
                          const long long* blk_off, int nblocks, const float* ema_dev);
/* torch.optim.Adam.step (train_human.py:139,286).  dev_state (optional, 8 floats: [step, 1-b1^step, sqrt(1-b2^step), lr,
 * grad_scale, -, -, -]): the step counter and bias corrections are advanced by the call itself on the device, and lr /
 * grad_scale are READ from it instead of the by-value arguments, so that a captured call follows an lr scheduler
 * (MultiStepLR, train_human.py:143,202) through an 8-byte copy; if NULL, `step`, `lr`, `grad_scale` are the host's. */
int udapose_adam_multi(void* stream, const long long* p, const long long* g, const long long* m, const long long* v,
                       const long long* sizes, const int* blk_tensor, const long long* blk_off, int nblocks, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int step, float grad_scale, float* dev_state);
/* torch.optim.SGD(momentum, nesterov) (train_human.py:137); dev_state as for Adam ([0] = step counter, [3] = lr,
 * [4] = grad_scale; first_step is then `step == 1` on the device) */
int udapose_sgd_multi(void* stream, const long long* p, const long long* g, const long long* buf, const long long* sizes,
                      const int* blk_tensor, const long long* blk_off, int nblocks, float lr, float momentum, float weight_decay,
                      int nesterov, int first_step, float grad_scale, float* dev_state);

/* The whole tail of a mean-teacher step in ONE sweep over the parameters: torch.optim.Adam.step on the student
 * (train_human.py:437), OldWeightEMA.step into the teacher (utils.py:21-25, train_human.py:438) and the element-type weight
 * packs that the next forwards of both networks' plans need (what udapose_net_pack_weights would re-read the masters for):
 * 46 bytes per parameter instead of 58, four launches fewer.  Arithmetic identical to udapose_adam_multi followed by
 * udapose_ema_multi (bit for bit); parameters by index in .parameters() order (host arrays of device pointers); exp_avg /
 * exp_avg_sq entries are NULL for parameters without gradient (backbone.fc: EMA only).  bind_update builds the device job
 * table (allocates: outside capture; again when a pointer changes); dev_state as for udapose_adam_multi; do_adam = 0: EMA
 * and packs only. */
int udapose_net_bind_update(udapose_net_t student, udapose_net_t teacher, void* const* h_params_s, void* const* h_grads,
                            void* const* h_exp_avg, void* const* h_exp_avg_sq, void* const* h_params_t, void* wpack_s, void* wpack_t);
int udapose_net_fused_update(udapose_net_t student, udapose_net_t teacher, void* stream, void* const* h_params_s, void* const* h_grads,
                             void* const* h_exp_avg, void* const* h_params_t, void* wpack_s, void* wpack_t, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int step, float grad_scale, float* dev_state, float alpha,
                             float one_minus_alpha, int do_adam, long long grad2_delta_bytes);
/* grad2_delta_bytes != 0: the gradient is h_grads[i] + the tensor grad2_delta_bytes behind it (the second per-pass gradient buffer
 * of a step whose two backward passes ran on different streams; a multiple of 16): the sum udapose_axpy_f32 would have written
 * first, taken in the same sweep.  h_grads itself is left holding the first pass's share. */

/* The same sweep for either optimizer and for parameter groups (PoseResNet.get_parameters(lr): the backbone at a tenth of the rate).
 * kind: UDAPOSE_OPT_ADAM - h_state1 / h_state2 = exp_avg / exp_avg_sq, (beta1, beta2, eps) - or UDAPOSE_OPT_SGD = torch.optim.SGD with
 * momentum (train_human.py:136-137) - h_state1 = the momentum buffers, h_state2 is not read (may be NULL), beta1 is the momentum, nesterov
 * 0 / 1; arithmetic identical to udapose_sgd_multi followed by udapose_ema_multi (bit for bit): 38 bytes per parameter instead of 62
 * (axpy 12, SGD 20, EMA 12, packs 18).  group_idx[i] (NULL: one group) is the parameter group of parameter i, at most 8 groups
 * (UDAPOSE_ERR_UNSUPPORTED beyond).  dev_states[g] / weight_decays[g], g < n_groups: every group's 8-float device state (required: lr,
 * grad_scale, the step counter and found_inf are read from it - for SGD the first step is `counter == 1` after the tick, as in
 * udapose_sgd_multi) and its weight decay, read when the call is made.  ONE tick launch advances every group's counter.  A found_inf
 * step neither ticks nor updates; the EMA and the packs still run.  A table bound for SGD never takes over split sums
 * (udapose_net_wgrad_pair_defer then defers nothing).  Contract as above: bind allocates (outside capture), the update only launches
 * and returns UDAPOSE_ERR_NOT_PREPARED when the table is stale or was bound for another kind or group count.  One Adam group through
 * these gives the bits of udapose_net_fused_update. */
#define UDAPOSE_OPT_ADAM 0
#define UDAPOSE_OPT_SGD 1
int udapose_net_bind_update_groups(udapose_net_t student, udapose_net_t teacher, int kind, void* const* h_params_s, void* const* h_grads,
                                   void* const* h_state1, void* const* h_state2, void* const* h_params_t, void* wpack_s, void* wpack_t,
                                   const int* group_idx);
int udapose_net_fused_update_groups(udapose_net_t student, udapose_net_t teacher, void* stream, int kind, void* const* h_params_s,
                                    void* const* h_grads, void* const* h_state1, void* const* h_params_t, void* wpack_s, void* wpack_t,
                                    float beta1, float beta2, float eps, int nesterov, int n_groups, float* const* dev_states,
                                    const float* weight_decays, float alpha, float one_minus_alpha, int do_opt, long long grad2_delta_bytes);
/* Both sweeps with the EMA pair read on the device (ema_dev: {alpha, one_minus_alpha} as for udapose_ema_multi_dev, loaded once at kernel
 * entry in place of the by-value pair; null: UDAPOSE_ERR_ARG).  Everything else as the call of the same name without _dev, bit for bit. */
int udapose_net_fused_update_dev(udapose_net_t student, udapose_net_t teacher, void* stream, void* const* h_params_s, void* const* h_grads,
                                 void* const* h_exp_avg, void* const* h_params_t, void* wpack_s, void* wpack_t, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, int step, float grad_scale, float* dev_state,
                                 const float* ema_dev, int do_adam, long long grad2_delta_bytes);
int udapose_net_fused_update_groups_dev(udapose_net_t student, udapose_net_t teacher, void* stream, int kind, void* const* h_params_s,
                                        void* const* h_grads, void* const* h_state1, void* const* h_params_t, void* wpack_s, void* wpack_t,
                                        float beta1, float beta2, float eps, int nesterov, int n_groups, float* const* dev_states,
                                        const float* weight_decays, const float* ema_dev, int do_opt, long long grad2_delta_bytes);

/* Dynamic loss scaling = torch.cuda.amp.GradScaler (train_human.py:260,285-287,324,436-440) on the device, for the fp16 build.
 * dev_state is the optimizer's 8-float state: [5] = found_inf, [6] = loss scale S, [7] = growth tracker, [4] = 1/S.
 * check: raises found_inf if any gradient is inf / nan (then adam_multi / sgd_multi skip the step, counter included);
 * update: S *= backoff on found_inf, S *= growth after `interval` clean steps; clears found_inf, refreshes 1/S. */
int udapose_grad_scaler_check(void* stream, const long long* g, const long long* sizes, const int* blk_tensor, const long long* blk_off,
                              int nblocks, float* dev_state);
/* the same check over g + g2, g2 = the second per-pass gradient buffer at grad2_delta_bytes from the first (the sum the fused optimizer tail
 * forms itself, udapose_net_fused_update's grad2_delta_bytes): no separate axpy in front of the check (round 4) */
int udapose_grad_scaler_check2(void* stream, const long long* g, const long long* sizes, const int* blk_tensor, const long long* blk_off,
                               int nblocks, float* dev_state, long long grad2_delta_bytes);
int udapose_grad_scaler_update(void* stream, float* dev_state, float growth, float backoff, int interval);

/* Gradient clipping by global norm (torch.nn.utils.clip_grad_norm_, norm_type 2) without rewriting a gradient: the norm is formed on the
 * device and the clip coefficient is multiplied into every group's dev_state[4] (grad_scale), which the sweeps above read at run time.
 *   x_i   = fl32(g_i + g2_i)                       (g2: the second per-pass buffer grad2_delta_bytes behind g, a multiple of 4; 0: none)
 *   S_g   = sum_i x_i^2 in double, fixed order     (udapose_grad_sumsq: partials[block], one block per udapose_multi_chunk() elements)
 *   total = sum_g (double)state_g[4]^2 * S_g       (the UNSCALED gradient: state[4] is 1/S under the loss scaler), groups in order
 *   norm  = (float)sqrt(total)                     (before clipping, as clip_grad_norm_ returns it; +inf beyond fp32's range)
 *   coef  = (float)min(1.0, (double)max_norm / ((double)norm + 1e-6))   from the STORED norm; NaN stays NaN; max_norm = +inf gives 1.0f
 *   state_g[4] *= coef for every group, its old value saved - unless some state_g[5] (found_inf) is up: then nothing is scaled.
 * sumsq: one launch per table, writing partials[0 .. nblocks); dev_state (optional) also raises dev_state[5] on a non-finite x exactly as
 * udapose_grad_scaler_check2 does, in the same read.  clip: one work-group; group g owns partials[blk_begin[g] .. blk_end[g]); dev_states is
 * a HOST array of n_groups (1 .. 8) device pointers, read when the call is made.  restore: dev_state_g[4] = the saved value (issue it behind
 * the sweeps and in front of udapose_grad_scaler_update, which then refreshes 1/S as before).
 * clip: UDAPOSE_CLIP_FLOATS device floats owned by the caller: [UDAPOSE_CLIP_MAX_NORM] is READ on the device (a captured call follows a host
 * change through a 4-byte copy), [UDAPOSE_CLIP_NORM] and [UDAPOSE_CLIP_COEF] are written, [UDAPOSE_CLIP_SAVED + g] holds group g's saved
 * state[4].  No atomics, no allocation, fixed summation order: capturable, and two calls on the same gradients give the same bits.
 * UDAPOSE_ERR_ARG: a null table / partials / clip / state pointer, n_groups outside 1 .. 8, a negative or reversed block range, a
 * grad2_delta_bytes that is no multiple of 4; nothing is launched then. */
#define UDAPOSE_CLIP_MAX_NORM 0
#define UDAPOSE_CLIP_NORM 1
#define UDAPOSE_CLIP_COEF 2
#define UDAPOSE_CLIP_SAVED 4
#define UDAPOSE_CLIP_FLOATS 12
int udapose_grad_sumsq(void* stream, const long long* g, const long long* sizes, const int* blk_tensor, const long long* blk_off, int nblocks,
                       long long grad2_delta_bytes, float* dev_state, double* partials);
int udapose_grad_clip(void* stream, const double* partials, const int* blk_begin, const int* blk_end, int n_groups, float* const* dev_states,
                      float* clip);
int udapose_grad_clip_restore(void* stream, int n_groups, float* const* dev_states, const float* clip);

/* ---------------------------------------------------------------- gradient all-reduce in bf16 on the wire (data parallel,
 * the 212 MB fp32 student-gradient buffer): pack = one rounding of the fp32 bucket to bf16 (zero padded to n_padded, a
 * multiple of the world size); after an all-to-all every rank holds the W ranks' copies of its shard: shard_mean adds them in fp32
 * (rank order), multiplies by 1/W and ROUNDS THE MEAN to bf16 for the all-gather - an averaged element therefore carries two bf16
 * roundings, one per contribution and one of the mean (all-gathering the mean in fp32 would cost 6 instead of 4 bytes per element and rank
 * on the wire); unpack widens the bucket back to fp32.  tests/test_gpu_hotpath.py emulates W = 2, 3, 8 ranks on one GPU. */
int udapose_comm_pack_bf16(void* stream, const float* src, long long n, void* dst_bf16, long long n_padded);
int udapose_comm_shard_mean(void* stream, const void* shards_bf16, int world, long long m, void* out_bf16);
int udapose_comm_unpack_bf16(void* stream, const void* src_bf16, float* dst, long long n);

/* ---------------------------------------------------------------- AdaIN (lib/models/Style_net.py:4-29,167-168), NHWC bf16
 * out = alpha*adain(content, style) + (1-alpha)*content; stats_out (optional) [N][C][4] = (mean_c, std_c, mean_s, std_s) */
int udapose_adain(void* stream, const void* content, const void* style, void* out, int N, int HWc, int HWs, int C, float eps,
                  float alpha, float* stats_out);
/* the same on fp32 NHWC features (the reference's precision); out may be NULL: statistics only (calc_mean_std) */
int udapose_adain_f32(void* stream, const float* content, const float* style, float* out, int N, int HWc, int HWs, int C, float eps,
                      float alpha, float* stats_out);
/* the same on f16x2 split NHWC features (UDAPOSE_EPI_SPLIT): statistics and blend in fp32, out (may be NULL) split;
 * alpha_dev != NULL: the blend factor is read from device memory at run time */
int udapose_adain_split(void* stream, const void* content, const void* style, void* out, int N, int HWc, int HWs, int C, float eps,
                        float alpha, const float* alpha_dev, float* stats_out);
/* the same with the blend factor read from device memory at run time (one float): a launch captured in a hipGraph then follows
 * the step's draw of alpha.  is_f32 selects the fp32 form (content / style / out are float*), else the library's element type. */
int udapose_adain_alpha_dev(void* stream, const void* content, const void* style, void* out, int N, int HWc, int HWs, int C, float eps,
                            const float* alpha_dev, float* stats_out, int is_f32);

/* ---------------------------------------------------------------- Fourier-domain style transfer (FDA, Yang & Soatto, CVPR 2020)
 * A style bridge without weights: the content image keeps its phase and takes the style image's amplitude on the lowest spatial frequencies,
 * |u|, |v| <= b.  fp32 throughout, identical in both builds.  A plane is one (n, c) channel of a contiguous NCHW fp32 tensor.
 * udapose_fda_spectrum: spec [planes][2b+1][b+1][2] = (re, im) of G[u, v] = sum_y sum_x x[y, x] exp(-2 pi i (u y / H + v x / W)), row u + b,
 * u = -b .. b, v = 0 .. b (real input: the other half is the conjugate).  Phases are reduced exactly in integers and looked up in tables that
 * are rounded once from fp64; sums run in a fixed order without atomics (two runs agree to the bit; a plane's result does not depend on the
 * other planes of the call).  ws: udapose_fda_ws_bytes(planes, H, W, b) bytes, 8-byte aligned (< 0: these sizes are refused).
 * udapose_fda_apply: out = content + IDFT2(dF), dF[u, v] = alpha (|Gs| - |Gc|) Gc / |Gc| on the window (Gc = spec_c, Gs = spec_s; Gc == 0: the
 * phase is 1 + 0i), then the optional per-channel clamp max(min(out, hi[c]), lo[c]) (lo, hi [C]: both or neither), c = plane % C.  alpha_dev
 * (one float on the device) overrides alpha when non-null.  alpha == 0, or spec_s bit-equal to spec_c: out is the clamped content bit for bit.
 * mean, std [C] (both or neither): the planes hold (raw - mean[c]) / std[c]; the DC coefficient's amplitude and phase are then those of the raw
 * image, std[c] G[0, 0] + mean[c] H W, and its dF is divided by std[c] - FDA of the raw images, in normalised units.
 * Refused before any launch, nothing written: UDAPOSE_ERR_ARG for a null pointer, planes, C, H or W <= 0, planes % C != 0, b < 0 or
 * 2b + 1 > min(H, W) (the window would reach the Nyquist row); UDAPOSE_ERR_UNSUPPORTED for b > UDAPOSE_FDA_MAX_B or H or W >
 * UDAPOSE_FDA_MAX_DIM (the window, a work-group's 32 rows of row coefficients and both phase tables live in 150 KiB of LDS). */
#define UDAPOSE_FDA_MAX_B 63
#define UDAPOSE_FDA_MAX_DIM 4096
long long udapose_fda_ws_bytes(int planes, int H, int W, int b);
int udapose_fda_spectrum(void* stream, const float* x, int planes, int H, int W, int b, void* ws, float* spec);
int udapose_fda_apply(void* stream, const float* content, const float* spec_c, const float* spec_s, float* out, int planes, int C, int H, int W, int b,
                      float alpha, const float* alpha_dev, const float* lo, const float* hi, const float* mean, const float* std);

/* ---------------------------------------------------------------- Histogram matching and colour-statistics style transfer
 * Two more style bridges without weights (with FDA, the classical pixel-level three).  fp32 NCHW throughout, identical in both builds.
 * LEVEL of a pixel of channel c: l = (int) min(max(rint(fmaf(x, std[c], mean[c]) * 255), 0), 255), in fp32 as written (mean, std [C], both or
 * neither; without them std = 1, mean = 0: raw images in [0, 1]).  The clamp comes before the cast: out-of-range, infinite and NaN pixels
 * land on a bound.  For images that came from bytes through that normalisation the level is the byte; for other floats it is a quantisation.
 * SUMMARY: udapose_pixel_summary_bytes(N, C) bytes (< 0: refused), 8-byte aligned, int32 words; sample n owns the row of
 * R = C * 256 + (C == 3 ? 8 : 0) words at n * R:
 *   word c * 256 + k             uint32, the number of pixels of channel c at level k
 *   words 768 .. 773 (C == 3)    three uint64, low word first: sum l_0 l_1, sum l_0 l_2, sum l_1 l_2 over the pixels; words 774, 775 are zero
 * Exact integers (a kernel clears the buffer, integer atomics add): two runs agree to the bit, a sample's row does not depend on the batch.
 * TRANSFER: out = x + alpha (T - l) / (255 std[c]), then the optional clamp max(min(out, hi[c]), lo[c]) (lo, hi [C]: both or neither); T is
 * the target level from the content's and the style's summary (same N, C, H, W; sample n pairs with sample n).  alpha_dev (one float on the
 * device) overrides alpha when non-null.  alpha == 0 returns the (clamped) content bit for bit.  Per plane or sample everything is derived
 * in fp64 from the integers and rounded once to fp32; the per-pixel work is fp32.
 *   UDAPOSE_PIXEL_HIST      per channel, scikit-image's match_histograms on integer cumulative counts Cc, Cs: q = Cc[l]; v_0 < v_1 < .. the
 *                           occupied style levels; T = v_0 for q < Cs[v_0], v_last for q >= Cs[v_last], else with j the last index such that
 *                           Cs[v_j] <= q:  T = v_j + (q - Cs[v_j]) / (Cs[v_j+1] - Cs[v_j]) (v_j+1 - v_j).  sum_s bit-equal to sum_c: out == content.
 *   UDAPOSE_PIXEL_MEANSTD   per channel, AdaIN on pixels: T / 255 = (l / 255 - mu_c) sqrt(var_s + eps) / sqrt(var_c + eps) + mu_s, unbiased
 *                           variances of l / 255.  H W >= 2.
 *   UDAPOSE_PIXEL_CHOLESKY  C == 3: T / 255 = L_s L_c^-1 (l / 255 - mu_c) + mu_s, L = chol(Sigma + eps I), Sigma the unbiased 3 x 3
 *                           covariance of l / 255 (closed-form Cholesky and triangular inverse).  H W >= 2.
 * Refused before any launch, nothing written: UDAPOSE_ERR_ARG for a null or misaligned pointer, N, C, H or W <= 0, an unknown mode, CHOLESKY
 * with C != 3, H W < 2 or eps <= 0 in the two variance modes, one of lo / hi or of mean / std alone; UDAPOSE_ERR_UNSUPPORTED for
 * H W > UDAPOSE_PIXEL_MAX_HW (the counts are uint32 and the exact variance numerator n sum l^2 - (sum l)^2 stays below 2^64).
 * A work-group of either kernel covers UDAPOSE_PIXEL_SHARE pixels of a plane. */
#define UDAPOSE_PIXEL_HIST 0
#define UDAPOSE_PIXEL_MEANSTD 1
#define UDAPOSE_PIXEL_CHOLESKY 2
#define UDAPOSE_PIXEL_MAX_HW 16777216
#define UDAPOSE_PIXEL_SHARE 4096
long long udapose_pixel_summary_bytes(int N, int C);
int udapose_pixel_summary(void* stream, const float* x, int N, int C, int H, int W, const float* mean, const float* std, void* summary);
int udapose_pixel_transfer(void* stream, const float* content, const void* sum_c, const void* sum_s, float* out, int N, int C, int H, int W, int mode,
                           double eps, float alpha, const float* alpha_dev, const float* lo, const float* hi, const float* mean, const float* std);

/* ---------------------------------------------------------------- AdaIN decoder training (reference adain/net.py:102-162, adain/train/)
 * The backward of the style network's step on NHWC tensors of the library's element type, fp32 accumulation.  Reflection-padded 3x3
 * stride-1 convolutions (desc: reflect = 1, pad = 1, K = 3, optional upsample; Ci and Co multiples of 64 - zero-pad the 3-channel end
 * layers) run their backward on the padded (Hl+2) x (Wl+2) grid, Hl = Hi << upsample.  Every reduction is bit-reproducible.
 * Workspace: udapose_conv_bwd_ws_bytes(desc) bytes (< 0: geometry unsupported); compute calls never allocate.
 * udapose_conv_bwd_prepare builds the device tables these calls use (outside stream capture). */
long long udapose_conv_bwd_ws_bytes(const udapose_conv_desc* d);
int udapose_conv_bwd_prepare(const udapose_conv_desc* d);
/* dP [N][Hl+2][Wl+2][Ci] = data gradient of the conv on the padded grid (w_bwd: [Ci][9][Co] as for udapose_conv2d_bwd_data) */
int udapose_conv2d_bwd_data_reflect_padded(void* stream, const udapose_conv_desc* d, const void* dy, const void* w_bwd, void* dP);
/* dx [N][H][W][C] = mask * (fold(dP) + style term + content term + add), each optional (NULL):
 *   fold: reflection adjoint of dP [N][Hl+2][Wl+2][C] then, with upsample, the sum of each 2x2 block;
 *   style term (mean/std loss): gscale_s[0] * 2/(N*C) * [(m - m_t)/HW + (sd - sd_t) * (x - m) / ((HW - 1) * sd)] with
 *     stats [N][C][4] = (m, sd, m_t, sd_t) of x and of the target (udapose_adain's statistics output);
 *   content term: gscale_c[0] * c_scale * (x - t);  add: fp32 NCHW [N][add_c][H][W] added to channels < add_c;
 *   relu_mask != 0: multiplied by (x > 0).  gscale_* are device scalars (no host synchronisation).  term_scale multiplies the style,
 *   content and add terms: a constant gradient scale that keeps 16-bit (fp16) gradients out of the subnormal range; the weight and
 *   bias gradient calls take its inverse as out_scale. */
int udapose_reflect_fold(void* stream, const void* dP, int upsample, const void* x, int relu_mask, const float* stats, const float* gscale_s,
                         const void* t, const float* gscale_c, float c_scale, const float* add_nchw, int add_c, void* dx, int N, int H, int W, int C,
                         float term_scale);
/* dx [N][Hi][Wi][Ci] = padded dgrad + fold, masked by relu_src > 0 when relu_src != NULL */
int udapose_conv2d_bwd_data_reflect(void* stream, const udapose_conv_desc* d, const void* dy, const void* w_bwd, void* dx, const void* relu_src,
                                    void* ws);
/* dw fp32 [co_valid][Ci][3][3] (torch Conv2d layout) = out_scale * sum over pixels of dy x the reflect/upsample-gathered input x */
int udapose_conv2d_bwd_weight_reflect(void* stream, const udapose_conv_desc* d, const void* dy, const void* x, float* dw, int co_valid, void* ws,
                                      float out_scale);
/* MaxPool2d(2, 2, ceil_mode=True) backward from the saved input x [N][H][W][C]: each output gradient goes to the first maximum of its
 * window in scan order (torch's tie rule); relu_mask != 0 also applies (x > 0) */
int udapose_maxpool2x2_ceil_bwd(void* stream, const void* x, const void* dy, void* dx, int N, int H, int W, int C, int relu_mask);
/* db[c] = out_scale * sum over the M rows of dy [M][C] (C <= 2048), c < c_valid; ws: udapose_bias_grad_ws_bytes(M, C) bytes */
long long udapose_bias_grad_ws_bytes(long long M, int C);
int udapose_bias_grad(void* stream, const void* dy, float* db, long long M, int C, int c_valid, void* ws, float out_scale);
/* out[0] = mean((a - b)^2) over n elements (n % 8 == 0); ws: udapose_feat_mse_ws_bytes() bytes */
long long udapose_feat_mse_ws_bytes(void);
int udapose_feat_mse_fwd(void* stream, const void* a, const void* b, long long n, float* out, void* ws);
/* out[0] (+)= (sum_r (m - m_t)^2 + (sd - sd_t)^2) / R over stats [R][4] (the mean/std style-loss term) */
int udapose_style_stat_loss(void* stream, const float* stats, int R, float* out, int accumulate);

/* ---------------------------------------------------------------- batched nearest inverse-affine re-warp
 * (torchvision.transforms.functional.affine x3 per sample, train_human.py:366-368,388-390,412,421-423): NCHW fp32;
 * theta [N][nstage][6] = the inverse affine matrices in application order; backward != 0: src = d(out), dst = d(in). */
int udapose_affine_nearest(void* stream, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage,
                           int backward);
/* the same chain with InterpolationMode.BILINEAR per stage (grid_sample bilinear, zeros, align_corners=False; every stage clips against
 * the plane on its own), same theta tensor, nstage 1..8; src and dst must not overlap.  backward != 0: the exact transpose of the forward's
 * weights as a gather - no float atomics, a fixed summation order, no limit on the outputs per input pixel: bit-reproducible.
 * Planes with 2 * H * W * 4 <= 150 KB (every heat-map size) take one launch and allocate nothing.  Larger planes run stage by stage from
 * global memory and, for nstage > 1, allocate one scratch tensor in stream order: inside a stream capture they are refused
 * (UDAPOSE_ERR_UNSUPPORTED). */
int udapose_affine_bilinear(void* stream, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage,
                            int backward);
/* MIRRORED VIEWS: the two chains above for views that are A(M(base)), M = the reversal of the columns.  mirror [N] holds two
 * bits per sample: UDAPOSE_MIRROR_OUT - dst[n][c][y][x] = chain(src[n][p(c)])[y][W-1-x], the mirror after the chain (a heat-map re-warp back to
 * the base frame); UDAPOSE_MIRROR_IN - dst = chain(M(src[n][p(c)])), the mirror ahead of the chain (the way back to the view).  perm [C] int
 * (may be NULL: p = identity) is the joint permutation of the flip, an INVOLUTION with values in [0, C) - the caller checks it; it is applied
 * to a sample when exactly one of the two bits is set.  The mirror is an index map and does no arithmetic: forward and backward give the bits
 * of the composition of the plain entry point with the column reversal and the channel selection, a sample whose byte is 0 the bits of the
 * plain launch.  backward != 0: the exact transpose (src = d(out), dst = d(in)); the deterministic nearest form still adds in ascending index
 * of the chain's own output pixel, the bilinear gather in the raster order of the chain's own output.  src and dst must not overlap.
 * mirror == NULL: UDAPOSE_ERR_ARG.  Dispatch as for the plain entry points, except that a bilinear plane beyond the LDS budget
 * (2 * H * W * 4 > 150 KB) is refused with UDAPOSE_ERR_UNSUPPORTED. */
#define UDAPOSE_MIRROR_OUT 1
#define UDAPOSE_MIRROR_IN 2
int udapose_affine_nearest_mirror(void* stream, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage,
                                  int backward, const unsigned char* mirror, const int* perm);
int udapose_affine_bilinear_mirror(void* stream, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage,
                                   int backward, const unsigned char* mirror, const int* perm);
/* f16x2 (UDAPOSE_EPI_SPLIT / split tensors) range check: the number of split STORES, since the last reset, of a value outside fp16's range
 * (|v| > 65504, which the format saturates, or NaN) by any kernel of THIS library on the current device.  Synchronous (reads device
 * counters): call it at an evaluation boundary - engine.validate() does and warns - never inside a stream capture. */
int udapose_split_saturations(int reset, unsigned long long* count);
/* mean of k re-warped teacher heat-map tensors (train_human.py:361-372 with `--k` > 1: `torch.mean(recons, dim=0)` per sample): h_views = HOST
 * array of k (1..8) device pointers to fp32 tensors of n elements; dst[i] = (v0[i] + v1[i] + ...) / k, added in view order in fp32. */
int udapose_mean_views(void* stream, const float* const* h_views, int k, float* dst, size_t n);
/* Merge of the k re-warped teacher views BY AGREEMENT, one launch in place of udapose_mean_views.  h_views = HOST array of
 * k (1..8) device pointers to contiguous fp32 tensors of R = B*K planes of H x W.  Per plane r and view v:
 *   peak p_v = (idx % W, idx / W), idx = the first flat index of the plane's maximum (udapose_heatmap_argmax's order), maxval_v = that
 *     maximum; view v is VALID on the plane iff maxval_v > 0.  d2(u, v) = the integer squared distance of p_u and p_v.
 *   medoid = the valid view with the smallest sum of d2 to the other valid views, the lowest view index on a tie; none without a valid view.
 *   inliers = the valid views with (float)d2(v, medoid) <= r * r, r = radius_dev[0] read on the device (fp32 product; inf admits every valid
 *     view): inliers[r] holds bit v, n_inliers[r] their number - both 0 without a valid view.
 *   spread2[r] = the largest d2 over pairs of valid views (0 with fewer than two).  agree[r] = 1.f iff n_inliers >= min_views (1..k), else 0.f.
 *   mean, mode UDAPOSE_MERGE_MEAN: ((v0 + v1) + ...) / (float)k per pixel in fp32, in view order - the bits of udapose_mean_views;
 *     mode UDAPOSE_MERGE_TRIMMED: the same over the inlier views only, in view order, divided by (float)n_inliers; a plane without an inlier
 *     gets the MEAN value (its agree is 0).
 *   energy[r] (optional) = the mean over pixels of sum_v (v - m)^2 / k, m = the MEAN value of the pixel, over ALL views in either mode;
 *     the pixels are added in a fixed order (double precision): the same bits on every run.
 * peaks [k][R][2] int (x, y), maxvals [k][R], inliers / n_inliers / spread2 [R] int, agree / energy [R] float: every output but mean may be NULL.
 * No atomics.  16-byte accesses when H * W % 4 == 0 and every tensor is 16-byte aligned, element by element otherwise (the same bits).
 * UDAPOSE_ERR_ARG, before any launch and with nothing written: k outside 1..8, a NULL view / mean / radius_dev, min_views outside 1..k,
 * R, H or W < 1, H or W > 2048, an unknown mode. */
#define UDAPOSE_MERGE_MEAN 0
#define UDAPOSE_MERGE_TRIMMED 1
int udapose_view_merge(void* stream, const float* const* h_views, int k, int R, int H, int W, int mode, const float* radius_dev, int min_views,
                       float* mean, int* peaks, float* maxvals, int* inliers, int* n_inliers, int* spread2, float* agree, float* energy);
/* the loop's matrices on the device, in double precision, from the collated aug_param of lib/transforms/keypoint_detection.py:139:
 * params[n] = (angle, tx, ty, shear_x, shear_y, scale), angles in degrees (6 doubles per sample).  theta_fwd [N][3][6] (may be NULL):
 * translate by (tx, ty) / ratio | rotate by angle and scale | shear - the three warps of train_human.py:366-368,421-423;
 * theta_back [N][1][6] (may be NULL): the occlusion path's warp back (train_human.py:412).  A captured step computes its matrices
 * with this launch from a static parameter buffer: the host only copies 48 bytes per sample. */
int udapose_recon_thetas(void* stream, const double* params, int N, double ratio, float* theta_fwd, float* theta_back);

/* occlusion paste (train_human.py:399-409): for image i of img[n][C][H][W] (fp32) and boxes[i] = (r0,r1,c0,c1,rs,cs):
 * img[i][:, r0:r1, c0:c1] = img[i][:, rs:rs+(r1-r0), cs:cs+(c1-c0)] (source read completely before the write). */
int udapose_patch_paste(void* stream, float* img, const int* boxes, int n, int C, int H, int W, int max_patch_elems);
/* The occlusion DECISIONS (train_human.py:374-410) on the device, so that the step needs no read-back and can be captured:
 * conf / flat_idx [N][K] from udapose_heatmap_argmax of the teacher's re-warped heat-maps, u [N][4] uniform [0,1) draws (rate
 * test, key-point choice, patch row / column origin) -> boxes [N][6] for udapose_patch_paste (zero area when not selected) and
 * apply [N]; udapose_select_rows then keeps the occluded image for the selected samples only: dst[n] = apply[n] ? a[n] : b[n]. */
int udapose_occlusion_pick(void* stream, const float* conf, const int* flat_idx, const float* u, int N, int K, int w, double ratio,
                           int image_size, float rate, float thresh, int occlude_size, int* boxes, unsigned char* apply);
int udapose_select_rows(void* stream, float* dst, const float* a, const float* b, const unsigned char* flag, int N, size_t row_elems);

/* ---------------------------------------------------------------- per-launch timing of the MFMA kernels (bench.py roofline)
 * HIP events are recorded on the launch stream around every convolution launch between begin and end.
 * h_out9 (host): for kind in (fprop, dgrad, wgrad): launches, total milliseconds, total algorithmic FLOPs. */
/* ---------------------------------------------------------------- device-side data pipeline of the target views (the work
 * of the reference's DataLoader workers for the `_mt` datasets, lib/datasets/human36m_mt.py:76-161): images are uint8 NHWC
 * [N][H][W][3] as PIL arrays are; results are bit-exact with PIL's own arithmetic.
 * aug_affine_u8: torchvision F.affine on a PIL image = Image.transform(AFFINE, NEAREST) (lib/transforms/keypoint_detection.py:138):
 *   coef [N][6] int64 = PIL's 16.16 fixed-point coefficients (FIX(a0), FIX(a1), FIX(a2 + a0/2 + a1/2), FIX(a3), FIX(a4),
 *   FIX(a5 + a3/2 + a4/2)) of the inverse affine matrix (a0..a5), prepared on the host in double.
 * aug_color_op: one PIL.ImageEnhance step per image, in place (ColorJitter, train_human.py:68): op[n] 0 none, 1 brightness,
 *   2 contrast, 3 saturation; factor[n]; mean_scratch [N] int (the contrast step's rounded L mean).
 * aug_to_tensor: ToTensor + Normalize -> NCHW fp32.
 * gaussian_labels: generate_target (lib/datasets/util.py:12-70): kp [R][2] double pixels, vis [R] -> target [R][Hh][Wh],
 *   weight [R]; patch = the (2*rad+1)^2 Gaussian built by the caller as the reference builds it. */
int udapose_aug_affine_u8(void* stream, const unsigned char* src, unsigned char* dst, const long long* coef, int N, int H, int W);
/* the mirrored base crop of a flipped view, out of place: dst[n][y][x] = src[n][y][flag[n] ? W - 1 - x : x] (flag [N] bytes); aug_affine_u8 of
 * the result is, byte for byte, aug_affine_u8 of the image reversed along its columns */
int udapose_aug_hflip_u8(void* stream, const unsigned char* src, unsigned char* dst, const unsigned char* flag, int N, int H, int W);
int udapose_aug_color_op(void* stream, unsigned char* img, const int* op, const float* factor, int* mean_scratch, int N, int HW);
/* PIL.ImageFilter.GaussianBlur (T.GaussianBlur, lib/transforms/keypoint_detection.py:216-225) in place on img [N][H][W][3] uint8 through
 * the scratch buffer tmp (same size): three box-blur passes per direction in PIL's 8.24 fixed point, bit-exact.  prm[n] = (r, ww, fw)
 * as uint32 (box radius integer part, centre and far weights: data_gpu.pil_box_blur_params), r = 0xffffffff: sample n is left as is. */
int udapose_aug_gaussian_blur_u8(void* stream, unsigned char* img, unsigned char* tmp, const unsigned int* prm, int N, int H, int W);
/* The strong student view (FixMatch / RandAugment colour ops; no counterpart in the reference, whose student view is ColorJitter), in place
 * on img [N][HW][3] uint8, byte for byte PIL's results.  op [N] continues aug_color_op's codes, one per image: 4 ImageOps.autocontrast
 * (cutoff 0), 5 ImageOps.equalize, 6 ImageOps.posterize(bits = param[n], 1..8), 7 ImageOps.solarize (param[n] = the integer cut
 * ceil(threshold) in [0, 256]: a pixel below it is kept, any other becomes 255 - i); an image with any other code is left alone.
 * Two launches, no read-back: a per-image, per-channel 256-entry table into lut_scratch [N][768] bytes (ops 4 and 5 from the image's own
 * histograms, counted on the device), then the look-up.  inv_scale [255] double on the device, inv_scale[d - 1] = 255.0 / d computed by
 * the host (autocontrast's scale: the table is formed in fp64 with separately rounded product and sum, no fp64 divide on the device).
 * param [N] int is read for ops 6 and 7 only.  The histograms count in 32 bits: UDAPOSE_ERR_UNSUPPORTED above HW = UDAPOSE_AUG_MAX_HW
 * (2^30: equalize's running sum step / 2 + HW stays below 2^31).  UDAPOSE_ERR_ARG: a null pointer, N or HW < 1. */
#define UDAPOSE_AUG_MAX_HW (1 << 30)
int udapose_aug_point_op(void* stream, unsigned char* img, const int* op, const int* param, const double* inv_scale, unsigned char* lut_scratch,
                         int N, int HW);
/* op code 8, ImageEnhance.Sharpness(img).enhance(factor[n]) = Image.blend(img.filter(SMOOTH), img, factor), in place on img [N][H][W][3]
 * uint8 through the scratch buffer tmp (same size; the images with op[n] == 8 are copied there and the stencil reads the copy).  SMOOTH is
 * the 3x3 kernel (1,1,1,1,5,1,1,1,1) / 13 in float32 exactly as libImaging sums it (coefficients float32(k / 13), start 0.5f, rows top
 * down, no fused multiply-add), the one-pixel border keeps its bytes; the blend is aug_color_op's.  H < 3 or W < 3: nothing is launched
 * (PIL returns the image).  An image with any other code is left alone.  UDAPOSE_ERR_ARG: a null pointer, N, H or W < 1;
 * UDAPOSE_ERR_UNSUPPORTED: H * W above UDAPOSE_AUG_MAX_HW. */
int udapose_aug_sharpness_u8(void* stream, unsigned char* img, unsigned char* tmp, const int* op, const float* factor, int N, int H, int W);
/* RandomErasing's write (lib/transforms/__init__.py:171-174) on x [N][3][H][W] fp32, in place: x[n][c][top : top + h, left : left + w] = v_c
 * with boxes[n] = (top, left, h, w) int32 on the device.  A box with h or w < 1 erases nothing; so does one that leaves the image.
 * Everything outside the box keeps its bits.  UDAPOSE_ERR_ARG: a null pointer, N, H or W < 1; UDAPOSE_ERR_UNSUPPORTED: H * W above
 * UDAPOSE_AUG_MAX_HW. */
int udapose_aug_erase_f32(void* stream, float* x, const int* boxes, float v0, float v1, float v2, int N, int H, int W);
/* T.RandomResizedCrop's image side (lib/transforms/keypoint_detection.py:456-521 -> resized_crop :66-88 = F.crop + F.resize(BILINEAR) on a
 * PIL image): src [N][Hs][Ws][3] uint8 -> dst [N][S][S][3] uint8, sample n's crop box[n] = (top, left, h, w) resampled to S x S with PIL's
 * two-pass 8-bit resampler (libImaging Resample.c: horizontal pass into the uint8 intermediate tmp [N][Hs][S][3], then vertical; 22-bit
 * fixed-point coefficients), bit-exact.  bounds [N][2][S][2] int32 = (first source index, tap count) per output column (axis 0) / row
 * (axis 1), coef [N][2][S][ksize] int32: prepared on the host in double as PIL does (data_gpu.pil_resample_coeffs). */
int udapose_aug_resized_crop_u8(void* stream, const unsigned char* src, unsigned char* dst, unsigned char* tmp, const int* box, const int* bounds,
                                const int* coef, int N, int Hs, int Ws, int S, int ksize);
int udapose_aug_to_tensor(void* stream, const unsigned char* img, float* out, int N, int HW, const float* mean3, const float* std3);
int udapose_gaussian_labels(void* stream, const double* kp, const float* vis, float* target, float* weight, int R, int Hh, int Wh,
                            double stride_x, double stride_y, const float* patch, int rad);
/* The un-quantised label encoding (DARK's second half; no counterpart in the reference).  Centre c = int(kp / stride + 0.5) and weight
 * exactly as udapose_gaussian_labels finds them (weight = vis, 0 when c is outside the map); target[y][x] =
 * exp(-((x - mx)^2 + (y - my)^2) / (2 sigma^2)) with m = kp / stride NOT rounded, computed in double and rounded to fp32, where
 * |x - cx| <= rad, |y - cy| <= rad and weight > 0.5; 0 elsewhere.  Every element of target and weight is written.
 * UDAPOSE_ERR_ARG: a null pointer, R, Hh or Wh < 1, rad < 0, sigma not finite or <= 0. */
int udapose_gaussian_labels_subpixel(void* stream, const double* kp, const float* vis, float* target, float* weight, int R, int Hh, int Wh,
                                     double stride_x, double stride_y, double sigma, int rad);
/* draw_labelmap_ori (lib/datasets/util.py:326-363), the animal pipelines' label generator as their datasets call it
 * (lib/datasets/real_animal_all_mt.py:274-283, animal_pose_mt.py:169-177,200-205; BASELINE.json configs[4]): pt [R][2] float32 = the 0-based
 * centres the datasets pass (`tpts[i] - 1`), truncated to int32 inside; vis [R] = pts[:, 2]; gate [R] uint8 = the datasets' `tpts[i, 1] > 0`
 * test (0: the row keeps vis and an empty map) -> target [R][Hh][Wh] fp32, weight [R] = vis * (whole stamp inside the map) where the
 * gate is open.  r3 = float32(3 * sigma); patch = the reference's (6 sigma + 1)^2 float64 stamp, 'Gaussian' or 'Cauchy', rounded to
 * float32 by the caller (psize = its side). */
int udapose_draw_labelmap_ori(void* stream, const float* pt, const float* vis, const unsigned char* gate, float* target, float* weight, int R,
                              int Hh, int Wh, float r3, const float* patch, int psize);

/* measurement: HIP events around every conv launch between begin and end (process-wide recorder, mutex-guarded) */
void udapose_prof_begin(void);
int udapose_prof_end(double* h_out9);

#ifdef __cplusplus
}
#endif
#endif
