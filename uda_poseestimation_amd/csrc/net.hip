// PoseResNet executor: the whole forward / backward of the reference's pose network
// (lib/models/pose_resnet.py:59-91 over the torchvision ResNet-v1.5 trunk, lib/models/resnet.py:25-40) as one C++ plan
// that enqueues hand-written gfx950 kernels on a HIP stream.  No allocation, no synchronisation, no host round trip
// inside forward/backward (graph-capturable after one warm-up call that fills the tap-plan cache).
//
// Data layout in HBM: activations NHWC bf16 (pre-BN conv output y and post-BN/ReLU z both kept for backward), weights
// bf16 packed [Co][taps][Ci] (fprop) and [Ci][taps][Co] (dgrad) from the fp32 channels_last master copies, BN statistics
// fp32.  Parameters are addressed by index in torch `.parameters()` order, buffers in `.buffers()` order.
// 'strict' plans (mode 3) run the f16x2 forward and the 16-bit backward: every offset below that the backward reads (y_off, z_off,
// in_off, mask_off, pool_off, poolidx_off, x8_off, save_off) holds the fp16 tensor of the 16-bit layout, written by the forward's own
// apply / pool / conversion launches next to the fp32-grade tensor; the fp32-grade tensors (the f* offsets) live only in the forward.
#include <algorithm>
#include <deque>
#include <functional>
#include <queue>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>
#include "net.h"
#include "pointwise.h"
#include "optim.h"

namespace {

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
// Policy::debug_sync: synchronise after every enqueued stage and report the source line of the first failure (set for the
// duration of a net_* call on the calling thread; never on by default)
static thread_local int t_dbg_sync = 0;
struct DbgSyncScope { int prev; explicit DbgSyncScope(int on) : prev(t_dbg_sync) { t_dbg_sync = on; } ~DbgSyncScope() { t_dbg_sync = prev; } };
#define CK(expr) do { int _e = (expr); \
    if (t_dbg_sync) { fprintf(stderr, "[udapose] net.hip:%d %s\n", __LINE__, #expr); fflush(stderr); \
        if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "[udapose] FAILED at net.hip:%d\n", __LINE__); return UDAPOSE_ERR_LAUNCH; } } \
    if (_e != UDAPOSE_OK) return _e; } while (0)

struct ConvL {
    ConvGeom g;
    int w_idx = -1;         // parameter index of the weight
    int bias_idx = -1;
    size_t wf_off = 0, wb_off = 0;   // bf16 packs inside wpack (bytes)
    size_t in_off = 0;      // activation arena offset of the input (bytes)
    size_t y_off = 0;       // pre-BN output
    size_t fin_off = 0, fy_off = 0;     // what the FORWARD reads / writes: in_off / y_off, except in 'strict' plans (split input, fp32 y)
    size_t dy_off = 0;      // workspace offset of this layer's own dy buffer (backward)
};
struct BnL {
    int C = 0;
    int g_idx = -1, b_idx = -1;             // parameter indices
    int rm_idx = -1, rv_idx = -1, nbt_idx = -1;   // buffer indices
    size_t save_off = 0;    // fp32 [3][C] saved mean / invstd / unbiased var in the arena
    size_t z_off = 0;       // post-BN(-ReLU) output
    size_t mask_off = 0;    // bn3 of a block: ReLU bit mask of z (one byte per 8 channels), what the data gradients read instead of z
    size_t fz_off = 0;      // what the forward writes: z_off, except in 'strict' plans (split z)
    size_t npix = 0;
};
struct Block {
    ConvL c1, c2, c3, cd;
    BnL b1, b2, b3, bd;
    bool has_ds = false;
    size_t in_off = 0, zd_off = 0;
    size_t fin_off = 0, fzd_off = 0;    // (the forward's residual inputs, as ConvL::fin_off)
    size_t npix_in = 0;
};

// A device table its holder owns: upload replaces what it holds (allocation + synchronous copy: never inside a stream capture), the
// destructor frees it.  After a failed upload it holds nothing.  The only device allocation, copy and free of this file.
template <class T> struct DevTable {
    T* d = nullptr; size_t n = 0;
    DevTable() = default;
    DevTable(DevTable&& o) noexcept : d(o.d), n(o.n) { o.d = nullptr; o.n = 0; }
    DevTable& operator=(DevTable&& o) noexcept { if (this != &o) { reset(); d = o.d; n = o.n; o.d = nullptr; o.n = 0; } return *this; }
    ~DevTable() { reset(); }
    void reset() { if (d) (void)hipFree(d); d = nullptr; n = 0; }
    int upload(const std::vector<T>& v) {
        reset();
        if (hipMalloc((void**)&d, v.size() * sizeof(T)) != hipSuccess) { d = nullptr; return UDAPOSE_ERR_LAUNCH; }
        if (hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { reset(); return UDAPOSE_ERR_LAUNCH; }
        n = v.size();
        return UDAPOSE_OK;
    }
};
// the job table of a multi-job launch with its work-group -> (job, sub-block) maps: all three live, or none
template <class J> struct JobTab {
    DevTable<J> jobs; DevTable<int> blk_job, blk_sub;
    int nblocks() const { return (int)blk_job.n; }
    void reset() { jobs.reset(); blk_job.reset(); blk_sub.reset(); }
    int upload(const std::vector<J>& j, const std::vector<int>& bj, const std::vector<int>& bs) {
        if (jobs.upload(j) == UDAPOSE_OK && blk_job.upload(bj) == UDAPOSE_OK && blk_sub.upload(bs) == UDAPOSE_OK) return UDAPOSE_OK;
        reset();
        return UDAPOSE_ERR_LAUNCH;
    }
};
struct PackJobH { const float* src; elem_t* dst; int A, T, B, kind; long long n; };

struct Net {
    int layers[4], K, N, H, W;
    int split_dz_idx = -1;  // pool buffer holding the gradient that net_backward part 1 hands to part 2 (a function of the plan)
    Policy policy;          // dispatch policy of this plan (udapose_net_set_policy); every ConvGeom below points at it
    int f32 = 0;            // 1: fp32 storage + exact fp32 MFMA (forward only: the reference's teacher / validate() precision)
                            // 2: f16x2 split storage (common.h), three fp16 MFMAs per K step: the FAST fp32-grade mode (forward only);
                            //    conv inputs (z, pooled map, image) and weight packs are split tensors, pre-BN conv outputs y are fp32
    int strict = 0;         // mode 3 ('strict', f32 == 2 as well): the f16x2 forward of a differentiable plan whose backward is the 16-bit one.
                            // The 16-bit layout is bump-allocated as in mode 0; the forward's split / fp32 tensors (f* offsets) are mapped onto
                            // the six scratch slots of the forward-only plans (inside this plan's arena), since nothing reads them after the forward
    int fwd_only = 0;       // forward-only plan (mode bit 9; the teacher's no-grad forwards, validate()): nothing is kept for a backward, so the
                            // pre-BN outputs y and the post-BN outputs z of all layers rotate through SIX scratch buffers (y | block input | block
                            // output | bn1 output | bn2 output | downsample output) instead of a bump-allocated arena - layer after layer rewrites the same
                            // few MB, which stay resident in the L2s / the Infinity Cache (round 5; the arena form streams 2.8 GB per forward to HBM)
    struct Scratch { size_t need[6] = {0, 0, 0, 0, 0, 0}, off[6] = {0, 0, 0, 0, 0, 0}; bool sizing = false; } sc;     // (forward-only plans: build())
    int deconv_bias = 0;    // Upsampling(bias=True) (pose_resnet.py:15,41,96 `deconv_with_bias`): every ConvTranspose2d has a bias parameter
    size_t es = 2;          // bytes per activation element
    int n_params = 0, n_buffers = 0;
    std::vector<long long> param_numel;
    // stem
    ConvL stem; BnL stem_bn;
    size_t x8_off = 0, pool_off = 0, poolidx_off = 0;
    size_t fx8_off = 0, fpool_off = 0;    // (the forward's image / pooled map: x8_off / pool_off, except in 'strict' plans)
    int Hs = 0, Ws = 0, Hp = 0, Wp = 0;
    std::vector<Block> blocks;
    ConvL up[3]; BnL up_bn[3];
    ConvL head;
    size_t head_out_off = 0;          // fp32 NHWC [N,Ho,Wo,K]
    int fc_w_idx = -1, fc_b_idx = -1;
    size_t act_bytes = 0, wpack_bytes = 0, ws_bytes = 0;
    // workspace carve (bytes)
    size_t ws_slab = 0, ws_slabf = 0, ws_coef = 0, ws_gbuf[6] = {0, 0, 0, 0, 0, 0}, ws_dyhead = 0, ws_dwtmp = 0, ws_headbwd = 0;
    size_t ws_wgpart = 0, ws_wgpart_bytes = 0;      // partial tiles of the split weight-gradient reductions (sized by net_ws_bytes from the policy of that moment)
    size_t gbuf_bytes = 0;
    int Hout = 0, Wout = 0;
    // batched weight packing: device job tables, rebuilt when the parameter / pack pointers change
    struct PackTab : JobTab<PackJobH> { const void* key0 = nullptr; const void* key1 = nullptr; const void* keyw = nullptr; };
    PackTab pack_fwd, pack_all;
    // grouped weight-gradient launch of one backward pass: device tables, rebuilt when the buffers change
    struct WgGroup {
        float k_beta = -1.f; int k_stages = 0; int k_part = 0;     // part: 0 all layers, 1 upper (head..layer3), 2 lower (layer2..stem)
        // the policy the tables were built under: the form of the split reductions (1: partial tiles + split sums, 0: atomics into cleared
        // tensors) and whether they hold the stem.  A later udapose_net_set_policy does not change what a bound table does: find_wg_group
        // no longer finds it, and the backward returns UDAPOSE_ERR_NOT_PREPARED until udapose_net_bind_grads builds tables for the new policy.
        bool k_det = false, k_stem = false; int k_order = 0, k_geo_s = 0;      // (k_order: the work order of the lists, policy wgrad_order)
        size_t part_bytes = 0;                           // workspace bytes of partial tiles the split sums read (k_det)
        std::vector<std::pair<int, ptrdiff_t>> rel;      // (parameter index, byte offset of its gradient from grads[0]) the table assumes
        std::vector<size_t> rel_bytes;                   // bytes of rel[i]'s gradient tensor (what the launch writes there)
        std::vector<int> rel_cls;                        // tile class of the launch that computes rel[i]'s gradient
        // tile classes of the grouped launch: 0 = 128x128, 1 = 64x64 (and the filter-row form), 2 = 256x128 (128x64 per wave)
        DevTable<WgParams> d_tab[WG_CLASSES]; DevTable<WgGroupBlk> d_blk[WG_CLASSES]; int per_xcd[WG_CLASSES] = {};
        double flops[WG_CLASSES] = {};
        std::vector<std::pair<ptrdiff_t, size_t>> zero;  // dW ranges (offset from grads[0], bytes) cleared first (split reductions, when overwriting)
        DevTable<ZeroJob> d_zero;                        // the same ranges as a device job table, when all are 16-byte granular
        // Deterministic split reductions (round 6): a layer whose pixel range is split over several work-groups (layer1 / layer2, the last
        // deconvolution, head, stem) has every split store its PARTIAL tile into the pass's workspace (ws_wgpart); one launch then adds the
        // splits of all such layers in split order into the gradient tensors (pw_split_sum): no atomics, no clears, bit-reproducible
        DevTable<SumJob> d_sum; DevTable<int> d_sum_blk; int n_sum_blk = 0;
        // (the blocks of the jobs that sum into the workspace - the stem's row-tap scratch - are the LAST n_sum_ws_blk of d_sum_blk: a pair call that
        // leaves the sums of the gradient TENSORS to the optimizer sweep still runs those; h_sum: the jobs, for net_bind_update)
        int n_sum_ws_blk = 0;
        std::vector<SumJob> h_sum;
        unsigned long long last_use = 0;
    };
    std::deque<WgGroup> wg_groups;       // (stable addresses, never evicted: a captured hipGraph may reference any table built so far)
    // fused optimizer tail (Adam + EMA + weight packs of student and teacher in one sweep): device job table
    struct UpdTab : JobTab<TailJob> {
                    const void* k_ps = nullptr; const void* k_pt = nullptr; const void* k_g = nullptr; const void* k_m = nullptr;
                    const void* k_ws = nullptr; const void* k_wt = nullptr;
                    int kind = 0, ngroups = 1; };       // (optimizer the table was bound for: 0 Adam, 1 SGD; number of parameter groups)
    UpdTab upd;
    // Split sums left to the optimizer sweep (udapose_net_wgrad_pair_defer): the pair call records the two passes' workspaces and gradient bases
    // here, the next udapose_net_fused_update consumes and clears the mark (its sweep adds the partial tiles itself), udapose_net_split_sum_flush
    // runs the sums as their own launch instead.  Any other weight-gradient call while the mark stands is refused.
    struct Deferred { const WgGroup* G = nullptr; char* wsA = nullptr; char* wsB = nullptr; char* gA = nullptr; char* gB = nullptr; } deferred;
    const WgGroup* upd_sum_group = nullptr;     // the table whose split jobs the bound update's job table carries (null: none)
    // batched deferred running-statistics update: device job table, rebuilt when the buffer pointers change
    DevTable<BnRunJob> d_runjobs; const void* runjobs_key = nullptr;
    unsigned long long wg_tick = 0;
};

// The plan's layers in .parameters() order: stem; per block c1 / b1, c2 / b2, c3 / b3 and, with a downsample branch, cd / bd; up[i] / up_bn[i].
// fn returns void, or an int status: the walk stops at the first that is not UDAPOSE_OK and returns it.  The head is not part of the walks:
// every site treats it apart (output channels padded to 64, no BatchNorm, fp32 output).
template <class F, class... A> int walk_rc(F& fn, A&... a) {
    if constexpr (std::is_void_v<decltype(fn(a...))>) { fn(a...); return UDAPOSE_OK; }
    else return fn(a...);
}
template <class N, class F> int for_each_layer(N& n, F fn) {
    int rc = walk_rc(fn, n.stem, n.stem_bn);
    for (size_t i = 0; rc == UDAPOSE_OK && i < n.blocks.size(); ++i) {
        auto& b = n.blocks[i];
        if ((rc = walk_rc(fn, b.c1, b.b1)) == UDAPOSE_OK && (rc = walk_rc(fn, b.c2, b.b2)) == UDAPOSE_OK && (rc = walk_rc(fn, b.c3, b.b3)) == UDAPOSE_OK && b.has_ds)
            rc = walk_rc(fn, b.cd, b.bd);
    }
    for (int i = 0; rc == UDAPOSE_OK && i < 3; ++i) rc = walk_rc(fn, n.up[i], n.up_bn[i]);
    return rc;
}
template <class N, class F> int for_each_conv(N& n, F fn) { return for_each_layer(n, [&](auto& c, auto&) { return walk_rc(fn, c); }); }
template <class N, class F> int for_each_bn(N& n, F fn) { return for_each_layer(n, [&](auto&, auto& b) { return walk_rc(fn, b); }); }

size_t act_alloc(Net& n, size_t bytes) { size_t o = n.act_bytes; n.act_bytes = align_up(o + bytes); return o; }
size_t wp_alloc(Net& n, size_t bytes) { size_t o = n.wpack_bytes; n.wpack_bytes = align_up(o + bytes); return o; }

// forward-only plans: named scratch slots, each as large as its largest tenant (sized in a dry pass of the layout)
enum { SC_Y = 0, SC_A, SC_B, SC_MID, SC_MID2, SC_DS, SC_COUNT };
size_t sc_take(Net& n, int slot, size_t bytes) {
    if (n.sc.sizing) { n.sc.need[slot] = std::max(n.sc.need[slot], align_up(bytes)); return 0; }
    return n.sc.off[slot];
}
// (in_off / fin_off: the input the backward / the forward reads, the same offset outside 'strict' plans)
void add_conv(Net& n, ConvL& c, int Hi, int Wi, int Ci, int Co, int K, int stride, int pad, int transposed, size_t in_off, size_t fin_off, bool need_bwd_pack,
              int y_slot = -1) {
    c.g = ConvGeom{n.N, Hi, Wi, Ci, Co, K, K, stride, pad, transposed, 0, 0};
    c.w_idx = n.n_params++;
    n.param_numel.push_back((long long)Co * (Ci == 8 ? 3 : Ci) * K * K);
    c.in_off = in_off;
    c.fin_off = fin_off;
    const size_t welems = (size_t)Co * c.g.wtaps() * Ci;
    // fp32 mode reads plain-conv weights straight from the fp32 master ([Co][taps][Ci] is its physical layout)
    if (n.f32 != 1 || c.g.smallc() || transposed) c.wf_off = wp_alloc(n, welems * (n.f32 ? 4 : 2));
    if (need_bwd_pack && (!n.f32 || n.strict)) c.wb_off = wp_alloc(n, welems * 2);
    const size_t ybytes = (size_t)n.N * c.g.Ho() * c.g.Wo() * Co * n.es;
    c.y_off = (n.fwd_only && y_slot >= 0) ? sc_take(n, y_slot, ybytes) : act_alloc(n, ybytes);
    c.fy_off = n.strict ? sc_take(n, y_slot, (size_t)n.N * c.g.Ho() * c.g.Wo() * Co * 4) : c.y_off;
}
void add_bn(Net& n, BnL& b, int C, size_t npix, bool alloc_z = true, int z_slot = -1) {
    b.C = C;
    b.g_idx = n.n_params++; n.param_numel.push_back(C);
    b.b_idx = n.n_params++; n.param_numel.push_back(C);
    b.rm_idx = n.n_buffers++; b.rv_idx = n.n_buffers++; b.nbt_idx = n.n_buffers++;
    b.save_off = act_alloc(n, (size_t)3 * C * 4);
    b.npix = npix;
    if (alloc_z) {
        b.z_off = (n.fwd_only && z_slot >= 0) ? sc_take(n, z_slot, npix * C * n.es) : act_alloc(n, npix * C * n.es);
        b.fz_off = n.strict ? sc_take(n, z_slot, npix * C * 4) : b.z_off;
    }
}

Net* build(const int layers[4], int K, int N, int H, int W, int mode) {
    Net* np = new Net();
    Net& n = *np;
    const int f32 = mode & 0xff;          // (mode: low byte = precision 0 / 1 / 2 / 3, bit 8 = the deconvolutions carry a bias, bit 9 = forward-only plan)
    n.deconv_bias = (mode >> 8) & 1;
    n.strict = f32 == 3;
    n.f32 = f32 >= 2 ? 2 : (f32 ? 1 : 0);
    n.es = (f32 && !n.strict) ? 4 : 2;    // (bytes per element of the tensors at the backward's offsets; a strict plan's are fp16)
    for (int i = 0; i < 4; ++i) n.layers[i] = layers[i];
    n.K = K; n.N = N; n.H = H; n.W = W;
    n.fwd_only = (mode >> 9) & 1;
    // The arena layout.  Differentiable plans: every tensor its own range (the backward reads them all).  Forward-only plans: the
    // SAME walk with the y / z tensors mapped onto six scratch slots by liveness - one live pre-BN output at a time (SC_Y), the
    // block's input and output ping-pong between SC_A and SC_B (the input is the residual: live until bn3), bn1 / bn2 outputs
    // in SC_MID / SC_MID2, the downsample branch's output waits in SC_DS for bn3.  The walk runs twice:
    // a dry pass sizes each slot by its largest tenant and is rewound, the second assigns the offsets.
    auto layout = [&](Net& n) {
    const bool fo = n.fwd_only != 0;
    n.x8_off = fo ? sc_take(n, SC_DS, (size_t)N * H * W * 8 * n.es) : act_alloc(n, (size_t)N * H * W * 8 * n.es);
    n.fx8_off = n.strict ? sc_take(n, SC_DS, (size_t)N * H * W * 8 * 4) : n.x8_off;
    // stem: conv 7x7 s2 p3 (3 -> padded 8 input channels), bn, relu, maxpool 3x3 s2 p1
    add_conv(n, n.stem, H, W, 8, 64, 7, 2, 3, 0, n.x8_off, n.fx8_off, false, SC_Y);
    n.Hs = n.stem.g.Ho(); n.Ws = n.stem.g.Wo();
    add_bn(n, n.stem_bn, 64, (size_t)N * n.Hs * n.Ws, true, SC_B);
    n.Hp = (n.Hs + 2 - 3) / 2 + 1; n.Wp = (n.Ws + 2 - 3) / 2 + 1;
    n.pool_off = fo ? sc_take(n, SC_A, (size_t)N * n.Hp * n.Wp * 64 * n.es) : act_alloc(n, (size_t)N * n.Hp * n.Wp * 64 * n.es);
    n.poolidx_off = fo ? sc_take(n, SC_MID, (size_t)N * n.Hp * n.Wp * 64) : act_alloc(n, (size_t)N * n.Hp * n.Wp * 64);      // (written, never read, by a forward-only plan)
    n.fpool_off = n.strict ? sc_take(n, SC_A, (size_t)N * n.Hp * n.Wp * 64 * 4) : n.pool_off;
    size_t cur = n.pool_off, fcur = n.fpool_off;
    int cur_slot = SC_A;
    int Hc = n.Hp, Wc = n.Wp, Cc = 64;
    const int planes[4] = {64, 128, 256, 512};
    for (int L = 0; L < 4; ++L)
        for (int bi = 0; bi < layers[L]; ++bi) {
            n.blocks.emplace_back();
            Block& b = n.blocks.back();
            const int P = planes[L], stride = (bi == 0 && L > 0) ? 2 : 1;
            const int out_slot = cur_slot == SC_A ? SC_B : SC_A;
            b.in_off = cur;
            b.fin_off = fcur;
            b.npix_in = (size_t)N * Hc * Wc;
            b.has_ds = (bi == 0);
            // parameter order follows torchvision Bottleneck: conv1,bn1,conv2,bn2,conv3,bn3,(downsample.0, downsample.1)
            add_conv(n, b.c1, Hc, Wc, Cc, P, 1, 1, 0, 0, cur, fcur, true, SC_Y);
            add_bn(n, b.b1, P, (size_t)N * Hc * Wc, true, SC_MID);
            add_conv(n, b.c2, Hc, Wc, P, P, 3, stride, 1, 0, b.b1.z_off, b.b1.fz_off, true, SC_Y);
            const int Ho = b.c2.g.Ho(), Wo = b.c2.g.Wo();
            add_bn(n, b.b2, P, (size_t)N * Ho * Wo, true, SC_MID2);     // (its own slot: with eval_fold conv2 reads z1 and writes z2 in one launch)
            add_conv(n, b.c3, Ho, Wo, P, P * 4, 1, 1, 0, 0, b.b2.z_off, b.b2.fz_off, true, SC_Y);
            add_bn(n, b.b3, P * 4, (size_t)N * Ho * Wo, true, out_slot);
            if ((!n.f32 || n.strict) && !fo) b.b3.mask_off = act_alloc(n, (size_t)N * Ho * Wo * (P * 4) / 8);     // (the ReLU bit mask is the backward's)
            if (b.has_ds) {
                add_conv(n, b.cd, Hc, Wc, Cc, P * 4, 1, stride, 0, 0, cur, fcur, true, SC_Y);
                add_bn(n, b.bd, P * 4, (size_t)N * Ho * Wo, true, SC_DS);
                b.zd_off = b.bd.z_off;
                b.fzd_off = b.bd.fz_off;
            }
            cur = b.b3.z_off; fcur = b.b3.fz_off; cur_slot = out_slot; Hc = Ho; Wc = Wo; Cc = P * 4;
        }
    n.fc_w_idx = n.n_params++; n.param_numel.push_back(1000LL * 2048);
    n.fc_b_idx = n.n_params++; n.param_numel.push_back(1000);
    for (int i = 0; i < 3; ++i) {
        add_conv(n, n.up[i], Hc, Wc, Cc, 256, 4, 2, 1, 1, cur, fcur, true, SC_Y);
        if (n.deconv_bias) { n.up[i].bias_idx = n.n_params++; n.param_numel.push_back(256); }      // (.parameters() order: weight, bias, then the BN)
        Hc = n.up[i].g.Ho(); Wc = n.up[i].g.Wo(); Cc = 256;
        cur_slot = cur_slot == SC_A ? SC_B : SC_A;
        add_bn(n, n.up_bn[i], 256, (size_t)N * Hc * Wc, true, cur_slot);
        cur = n.up_bn[i].z_off;
        fcur = n.up_bn[i].fz_off;
    }
    // head: 1x1 conv with bias -> fp32
    n.head.g = ConvGeom{N, Hc, Wc, 256, K, 1, 1, 1, 0, 0, 0, 0};
    n.head.w_idx = n.n_params++; n.param_numel.push_back((long long)K * 256);
    n.head.bias_idx = n.n_params++; n.param_numel.push_back(K);
    n.head.in_off = cur;
    n.head.fin_off = fcur;
    n.head.wf_off = wp_alloc(n, (size_t)K * 256 * (n.f32 ? 4 : 2));
    n.head.wb_off = wp_alloc(n, (size_t)256 * 64 * 2);      // [256][1][64] zero-padded for dgrad
    n.head_out_off = fo ? sc_take(n, SC_Y, (size_t)N * Hc * Wc * K * 4) : act_alloc(n, (size_t)N * Hc * Wc * K * 4);
    n.Hout = Hc; n.Wout = Wc;
    return Hc * 65536 + Wc;
    };
    if (n.fwd_only || n.strict) {
        n.sc.sizing = true;
        (void)layout(n);
        n.sc.sizing = false;
        // (rewind what the dry pass advanced; every offset it assigned is assigned again below)
        n.act_bytes = n.wpack_bytes = 0; n.n_params = n.n_buffers = 0; n.param_numel.clear(); n.blocks.clear();
        for (int k = 0; k < SC_COUNT; ++k) n.sc.off[k] = act_alloc(n, n.sc.need[k]);
    }
    const int hw_out = layout(n);
    const int Hc = hw_out >> 16, Wc = hw_out & 0xffff;

    // transient workspace: BN stat slabs, coefficient vectors, gradient ping-pong buffers
    size_t max_slab = 0, max_act = 0;
    auto upd = [&](const ConvL& c) {
        const size_t rows = (size_t)conv_stat_rows(c.g);
        max_slab = std::max(max_slab, rows * 2 * c.g.Co * 4);
        max_act = std::max(max_act, (size_t)n.N * c.g.Ho() * c.g.Wo() * c.g.Co * 2);
        max_act = std::max(max_act, (size_t)n.N * c.g.Hi * c.g.Wi * c.g.Ci * 2);
    };
    for_each_conv(n, upd);
    max_slab = std::max(max_slab, (size_t)1024 * 2 * 2048 * 4);   // bn backward partials: <=1024 rows x 2 x C
    size_t o = 0;
    n.ws_slab = o; o = align_up(o + max_slab);
    n.ws_slabf = o; o = align_up(o + max_slab);     // partial sums written by dgrad epilogues (the downsample BN keeps ws_slab)
    n.ws_coef = o; o = align_up(o + (size_t)3 * 2048 * 4 + 2 * 2048 * 4);
    // every convolution of the plan dispatches with the plan's policy
    // (the walk skips the unused `cd` of blocks without a downsample branch: its default geometry keeps pol == nullptr and is never dispatched)
    for_each_conv(n, [&](ConvL& c) { c.g.pol = &n.policy; });
    n.head.g.pol = &n.policy;
    if (n.fwd_only) {           // (no backward: statistics slabs and coefficient vectors only)
        n.ws_bytes = o;
        return np;
    }
    n.gbuf_bytes = align_up(2 * max_act);   // x2: the deconv-stage gradients are fp32
    for (int i = 0; i < 6; ++i) { n.ws_gbuf[i] = o; o += n.gbuf_bytes; }
    n.ws_dyhead = o; o = align_up(o + (size_t)N * Hc * Wc * 64 * 2);
    n.ws_dwtmp = o; o = align_up(o + std::max((size_t)64 * 56 * 8 * 4, (size_t)64 * 256 * 4));
    // every conv layer owns its dy buffer: the weight gradients of the whole pass are computed by ONE grouped launch after
    // the dgrad / BN-backward chain, so every dy must still be there
    auto dyb = [&](ConvL& c) { c.dy_off = o; o = align_up(o + (size_t)n.N * c.g.Ho() * c.g.Wo() * c.g.Co * 2); };
    for_each_conv(n, dyb);
    n.ws_wgpart = o;          // (last: its size follows the policy's split length, net_ws_bytes)
    n.ws_bytes = o;
    return np;
}

struct Pool {
    char* base; size_t off[6]; bool used[6] = {false, false, false, false, false, false};
    elem_t* get() { for (int i = 0; i < 6; ++i) if (!used[i]) { used[i] = true; return (elem_t*)(base + off[i]); } return nullptr; }
    void put(const void* p) { for (int i = 0; i < 6; ++i) if ((char*)p == base + off[i]) used[i] = false; }
};

// The weight packs that are not jobs of the plan's pack table (pw_pack_multi) or of the optimizer sweep: the stem's 3 -> 8 channel gather in
// every mode and, in the exact-fp32 mode, the deconvolutions' transposes (plain convolutions and the head read their fp32 masters there)
int pack_conv(hipStream_t s, const Net& n, const ConvL& c, const void* const* params, char* wpack) {
    const float* w = (const float*)params[c.w_idx];
    const ConvGeom& g = c.g;
    if (g.smallc()) {
        // master: [Co][KH][KW][3] (channels_last of [Co,3,KH,KW]) -> [Co][KH][KWp][8]; f16x2: every group of 8 values split into [8 h][8 l]
        if (n.f32 == 2) return pw_pack_strided_split(s, w, wpack + c.wf_off, g.Co, g.KH, g.KWp(), g.KW, 8, 3, (long)g.KH * g.KW * 3, (long)g.KW * 3, 3, 1);
        if (n.f32) return pw_pack_strided_f32(s, w, (float*)(wpack + c.wf_off), g.Co, g.KH, g.KWp(), g.KW, 8, 3, (long)g.KH * g.KW * 3, (long)g.KW * 3, 3, 1);
        return pw_pack_strided(s, w, (elem_t*)(wpack + c.wf_off), g.Co, g.KH, g.KWp(), g.KW, 8, 3, (long)g.KH * g.KW * 3, (long)g.KW * 3, 3, 1);
    }
    if (n.f32 != 1) return UDAPOSE_ERR_UNSUPPORTED;       // (16-bit and f16x2 packs of every other layer are table jobs)
    return g.transposed ? pw_transpose_f32(s, w, (float*)(wpack + c.wf_off), g.Ci, g.KH * g.KW, g.Co) : UDAPOSE_OK;
}

int conv_bn_fwd(hipStream_t s, const Net& n, const ConvL& c, const BnL& b, const void* const* params, void* const* buffers, const char* wpack,
                char* act, char* ws, int training, float momentum, const elem_t* res, int relu, bool upd, bool no_apply = false) {
    ConvEpilogue e;
    float* slab = (float*)(ws + n.ws_slab);
    float* scale = (float*)(ws + n.ws_coef);
    float* shift = scale + 2048;
    float* save = (float*)(act + b.save_off);
    e.stats = training ? slab : nullptr;
    e.f32 = n.f32 != 0;
    e.split = n.f32 == 2;
    e.out_f32 = n.f32 == 2;       // (f16x2: the pre-BN output stays fp32; the BN apply writes the split z)
    // a bias in front of the BatchNorm (deconv_with_bias): added to the stored output; the statistics epilogue sees the raw
    // accumulators, so the finalize launch shifts the mean by it
    const float* pre_bias = c.bias_idx >= 0 ? (const float*)params[c.bias_idx] : nullptr;
    e.bias = pre_bias;
    // block outputs: the apply also saves the ReLU bit mask of z (1/16 of z's bytes) for the data gradients that mask with it
    unsigned char* mask = (b.mask_off && n.policy.bn3_mask && relu) ? (unsigned char*)(act + b.mask_off) : nullptr;
    // 'strict' training forwards: the split apply also writes the fp16 y, z (and mask) of the 16-bit layout for the backward
    const bool sh = n.strict && training;
    void* y16 = sh ? (void*)(act + c.y_off) : nullptr;
    void* z16 = sh ? (void*)(act + b.z_off) : nullptr;
    const void* wptr = (n.f32 == 1 && !c.g.smallc() && !c.g.transposed) ? params[c.w_idx] : (const void*)(wpack + c.wf_off);
    const float* gamma = (const float*)params[b.g_idx];
    const float* beta = (const float*)params[b.b_idx];
    // (the running statistics a training forward updates, unless the update is deferred; the chunking word of the one-launch finalize + apply)
    float* rm = upd ? (float*)buffers[b.rm_idx] : nullptr;
    float* rv = upd ? (float*)buffers[b.rv_idx] : nullptr;
    long long* nbt = upd ? (long long*)buffers[b.nbt_idx] : nullptr;
    const int chunked = n.policy.bn_fwd_chunked | (n.policy.bn_xcd_rows ? (1 << 30) : 0);
    if (!training && !no_apply && !pre_bias && n.policy.eval_fold) {
        // Eval mode (validate(), train_human.py:461-500): the BatchNorm is a per-channel affine map known BEFORE the convolution, so the
        // conv's epilogue applies it from the fp32 accumulators - z = relu(conv * scale + shift (+ residual)) is written by the conv
        // itself: no apply launch, no pre-BN tensor, one rounding less than conv -> y -> apply
        CK(pw_bn_eval_coeff(s, b.C, gamma, beta, (const float*)buffers[b.rm_idx], (const float*)buffers[b.rv_idx], 1e-5f, scale, shift));
        e.stats = nullptr;
        e.scale = scale; e.bias = shift; e.relu = relu;
        e.res = res;
        e.out_f32 = 0;                    // (z has the plan's storage type: 16-bit, fp32, or the f16x2 split form)
        return conv_fprop(s, c.g, (const elem_t*)(act + c.fin_off), (const elem_t*)wptr, act + b.fz_off, e);
    }
    CK(conv_fprop(s, c.g, (const elem_t*)(act + c.fin_off), (const elem_t*)wptr, act + c.fy_off, e));
    if (training && !n.f32 && !no_apply && !pre_bias) {
        // wide, small-spatial layers: finalize + apply in ONE launch (channel-chunked work-groups, pointwise.hip)
        const int took = pw_bn_train_fused(s, (const elem_t*)(act + c.y_off), res, (elem_t*)(act + b.z_off), b.npix, b.C, slab, conv_stat_rows(c.g), gamma,
                                           beta, rm, rv, nbt, momentum, 1e-5f, save, relu, chunked, mask);
        if (took < 0) return took;
        if (took) return UDAPOSE_OK;
    }
    if (training && n.f32 == 2 && !no_apply && !pre_bias) {
        const int took = pw_bn_train_fused_split(s, (const float*)(act + c.fy_off), res, act + b.fz_off, b.npix, b.C, slab, conv_stat_rows(c.g), gamma, beta,
                                                 rm, rv, nbt, momentum, 1e-5f, save, relu, chunked, y16, z16, sh ? mask : nullptr);
        if (took < 0) return took;
        if (took) return UDAPOSE_OK;
    }
    if (training)
        CK(pw_bn_finalize(s, slab, conv_stat_rows(c.g), b.C, (double)b.npix, gamma, beta, rm, rv, nbt, momentum, 1e-5f, scale, shift, save,
                          save + b.C, pre_bias));
    else
        CK(pw_bn_eval_coeff(s, b.C, gamma, beta, (const float*)buffers[b.rm_idx], (const float*)buffers[b.rv_idx], 1e-5f, scale, shift));
    if (no_apply) return UDAPOSE_OK;      // (the caller's next launch applies scale / shift itself: the stem's fused pool)
    if (n.f32 == 2)
        return pw_bn_apply_split(s, (const float*)(act + c.fy_off), res, act + b.fz_off, b.npix * b.C, b.C, scale, shift, relu, y16, z16, sh ? mask : nullptr,
                                 n.policy.bn_xcd_rows >= 2);
    if (n.f32)
        return pw_bn_apply_f32(s, (const float*)(act + c.y_off), (const float*)res, (float*)(act + b.z_off), b.npix * b.C, b.C, scale, shift, relu);
    return pw_bn_apply(s, (const elem_t*)(act + c.y_off), res, (elem_t*)(act + b.z_off), b.npix * b.C, b.C, scale, shift, relu, mask, n.policy.bn_xcd_rows >= 2);
}

}  // namespace

// ============================================================================ public (C++) entry points
void* net_create(const int layers[4], int K, int N, int H, int W, int mode) {
    if (K < 1 || K > 64 || N < 1 || H % 32 || W % 32 || (mode & 0xff) > 3 || (mode >> 10)) return nullptr;
    // 'strict' (3): differentiable by definition (not with the forward-only bit), and its backward is the fp16 build's (the shadows are fp16)
    if ((mode & 0xff) == 3 && ((mode >> 9) & 1 || UDAPOSE_ELEM_KIND != 1)) return nullptr;
    return build(layers, K, N, H, W, mode);
}
void net_destroy(void* h) {
    delete (Net*)h;       // (every device table goes with its holder)
}
void net_set_policy(void* h, const Policy& p) { ((Net*)h)->policy = p; }
const Policy& net_get_policy(void* h) { return ((Net*)h)->policy; }
int net_num_params(void* h) { return ((Net*)h)->n_params; }
int net_num_buffers(void* h) { return ((Net*)h)->n_buffers; }
long long net_param_numel(void* h, int i) { return ((Net*)h)->param_numel[i]; }
size_t net_wpack_bytes(void* h) { return ((Net*)h)->wpack_bytes; }
size_t net_act_bytes(void* h) { return ((Net*)h)->act_bytes; }
namespace { size_t wg_partial_bytes(Net& n); }
size_t net_ws_bytes(void* h) {
    // the partial tiles of the split weight-gradient reductions (policy wgrad_det) close the workspace: their size follows the policy's
    // split length, which udapose_net_set_policy may have changed since the plan was created - sized here, when the caller asks
    Net& n = *(Net*)h;
    if ((n.f32 && !n.strict) || n.fwd_only || !n.policy.wgrad_group || !n.policy.wgrad_det) { n.ws_wgpart_bytes = 0; return n.ws_bytes; }
    n.ws_wgpart_bytes = wg_partial_bytes(n);
    return n.ws_bytes + n.ws_wgpart_bytes;
}
void net_out_shape(void* h, int* shp) { Net& n = *(Net*)h; shp[0] = n.N; shp[1] = n.K; shp[2] = n.Hout; shp[3] = n.Wout; }

namespace {
void add_pack_jobs(const Net& n, const ConvL& c, const void* const* params, char* wpack, bool with_bwd, std::vector<PackJobH>& jobs) {
    const ConvGeom& g = c.g;
    if (g.smallc()) return;                       // stem: strided gather, launched separately
    const float* w = (const float*)params[c.w_idx];
    const int T = g.KH * g.KW;
    elem_t* wf = (elem_t*)(wpack + c.wf_off);
    elem_t* wb = (elem_t*)(wpack + c.wb_off);
    const int sp = n.f32 == 2 ? 2 : 0;          // (kind bit 1: f16x2 split output, forward packs only)
    if (sp && !n.strict) with_bwd = false;     // ('strict': split forward packs, 16-bit data-gradient packs)
    if (!g.transposed) {
        jobs.push_back(PackJobH{w, wf, 0, 0, 0, sp, (long long)g.Co * T * g.Ci});
        if (with_bwd) jobs.push_back(PackJobH{w, wb, g.Co, T, g.Ci, 1, 0});
    } else {
        jobs.push_back(PackJobH{w, wf, g.Ci, T, g.Co, 1 | sp, 0});
        if (with_bwd) jobs.push_back(PackJobH{w, wb, 0, 0, 0, 0, (long long)g.Ci * T * g.Co});
    }
}
int build_pack_table(Net& n, Net::PackTab& tab, const void* const* params, char* wpack, bool with_bwd) {
    std::vector<PackJobH> jobs;
    for_each_conv(n, [&](const ConvL& c) { add_pack_jobs(n, c, params, wpack, with_bwd, jobs); });
    jobs.push_back(PackJobH{(const float*)params[n.head.w_idx], (elem_t*)(wpack + n.head.wf_off), 0, 0, 0, n.f32 == 2 ? 2 : 0, (long long)n.K * 256});
    std::vector<int> bj, bs;
    for (size_t j = 0; j < jobs.size(); ++j) {
        const PackJobH& q = jobs[j];
        const long nb = (q.kind & 1) == 0 ? (long)((q.n + 8191) / 8192) : (long)((q.A + 31) / 32) * ((q.B + 31) / 32) * q.T;
        for (long k = 0; k < nb; ++k) { bj.push_back((int)j); bs.push_back((int)k); }
    }
    CK(tab.upload(jobs, bj, bs));
    tab.key0 = params[0]; tab.key1 = params[n.n_params - 1]; tab.keyw = wpack;
    return UDAPOSE_OK;
}
int build_run_jobs(Net& n, void* const* buffers) {
    std::vector<BnRunJob> jobs;
    for_each_bn(n, [&](const BnL& b) {
        jobs.push_back(BnRunJob{b.save_off, (float*)buffers[b.rm_idx], (float*)buffers[b.rv_idx], (long long*)buffers[b.nbt_idx], b.C, 0});
    });
    CK(n.d_runjobs.upload(jobs));
    n.runjobs_key = buffers[0];
    return UDAPOSE_OK;
}
}  // namespace

// Builds every device table the plan's calls need for THESE parameter / buffer / pack pointers (pack job tables, the
// running-statistics job table, the tap plans of all layer geometries): the only place where net_pack_weights, net_forward and
// net_apply_running's tables are allocated and uploaded (synchronously: call it outside stream capture, again whenever a
// pointer changes).  Those calls return UDAPOSE_ERR_NOT_PREPARED when their table does not match the pointers they are given.
int net_bind(void* h, const void* const* params, void* const* buffers, void* wpack_) {
    Net& n = *(Net*)h;
    char* wpack = (char*)wpack_;
    CK(for_each_conv(n, [](const ConvL& c) { return conv_prepare(c.g); }));
    { ConvGeom hg = n.head.g; CK(conv_prepare(hg)); hg.Co = 64; CK(conv_prepare(hg)); }
    if (n.f32 != 1) {
        CK(build_pack_table(n, n.pack_fwd, params, wpack, false));
        CK(build_pack_table(n, n.pack_all, params, wpack, n.f32 == 0 || n.strict));
    }
    if (buffers) CK(build_run_jobs(n, buffers));
    return UDAPOSE_OK;
}

int net_pack_weights(void* h, hipStream_t s, const void* const* params, void* wpack_, int with_bwd) {
    Net& n = *(Net*)h;
    DbgSyncScope dbg(n.policy.debug_sync);
    char* wpack = (char*)wpack_;
    if (n.f32 != 1) {
        // ONE launch casts / transposes every weight through the job table net_bind built for these pointers
        if (n.f32 == 2 && !n.strict) with_bwd = 0;
        Net::PackTab& tab = with_bwd ? n.pack_all : n.pack_fwd;
        if (!tab.jobs.d || tab.key0 != params[0] || tab.key1 != params[n.n_params - 1] || tab.keyw != (const void*)wpack)
            return UDAPOSE_ERR_NOT_PREPARED;
        CK(pack_conv(s, n, n.stem, params, wpack));
        CK(pw_pack_multi(s, tab.jobs.d, tab.blk_job.d, tab.blk_sub.d, tab.nblocks()));
        if (with_bwd)   // head dgrad pack [256][1][64]: wb[ci][k] = w[k][ci], zero for k >= K
            CK(pw_pack_strided(s, (const float*)params[n.head.w_idx], (elem_t*)(wpack + n.head.wb_off), 256, 1, 1, 1, 64, n.K, 1, 0, 0, 256));
        return UDAPOSE_OK;
    }
    // exact fp32: the stem's gather and the deconvolutions' transposes, layer by layer; plain convolutions and the head read their fp32
    // masters directly, and there is no backward to pack for
    // (CK inside the walk: with debug_sync every layer's launch is synchronised and reported under this line)
    return for_each_conv(n, [&](const ConvL& c) -> int { CK(pack_conv(s, n, c, params, wpack)); return UDAPOSE_OK; });
}

int net_forward(void* h, hipStream_t s, const float* x_nchw, const void* const* params, void* const* buffers, const void* wpack_, void* act_, void* ws_,
                float* out_nchw, int training, float momentum) {
    const Net& n = *(const Net*)h;
    DbgSyncScope dbg(n.policy.debug_sync);
    const bool upd = !(training & 2);               // bit 1 of `training`: defer the running-statistics update
    training &= 1;
    const char* wpack = (const char*)wpack_;
    char* act = (char*)act_;
    char* ws = (char*)ws_;
    // ('strict' training forwards: the conversion, the stem's max-pool and every BN apply also write the fp16 tensors of the 16-bit layout)
    const bool sh = n.strict && training;
    if (n.f32 == 2) CK(pw_nchw_f32_to_nhwc_split(s, x_nchw, act + n.fx8_off, n.N, 3, n.H * n.W, 8, sh ? act + n.x8_off : nullptr));
    else if (n.f32) CK(pw_nchw_f32_to_nhwc_f32(s, x_nchw, (float*)(act + n.x8_off), n.N, 3, n.H * n.W, 8));
    else CK(pw_nchw_f32_to_nhwc_bf16(s, x_nchw, (elem_t*)(act + n.x8_off), n.N, 3, n.H * n.W, 8));
    const bool stem_fused = n.policy.stem_fused && !n.f32;
    CK(conv_bn_fwd(s, n, n.stem, n.stem_bn, params, buffers, wpack, act, ws, training, momentum, nullptr, 1, upd, stem_fused));
    if (stem_fused)     // BN apply + ReLU + max-pool in one sweep; z of the stem is never materialised (the backward masks from y)
        CK(pw_bn_relu_maxpool3x3s2(s, (const elem_t*)(act + n.stem.y_off), (elem_t*)(act + n.pool_off), (unsigned char*)(act + n.poolidx_off), n.N,
                                   n.Hs, n.Ws, 64, (const float*)(ws + n.ws_coef), (const float*)(ws + n.ws_coef) + 2048));
    else if (n.f32 == 2)
        CK(pw_maxpool3x3s2_fwd_split(s, act + n.stem_bn.fz_off, act + n.fpool_off, (unsigned char*)(act + n.poolidx_off), n.N, n.Hs, n.Ws, 64,
                                     sh ? act + n.pool_off : nullptr));
    else if (n.f32)
        CK(pw_maxpool3x3s2_fwd_f32(s, (const float*)(act + n.stem_bn.z_off), (float*)(act + n.pool_off), (unsigned char*)(act + n.poolidx_off), n.N,
                                   n.Hs, n.Ws, 64));
    else
        CK(pw_maxpool3x3s2_fwd(s, (const elem_t*)(act + n.stem_bn.z_off), (elem_t*)(act + n.pool_off), (unsigned char*)(act + n.poolidx_off), n.N,
                               n.Hs, n.Ws, 64));
    for (auto& b : n.blocks) {
        CK(conv_bn_fwd(s, n, b.c1, b.b1, params, buffers, wpack, act, ws, training, momentum, nullptr, 1, upd));
        CK(conv_bn_fwd(s, n, b.c2, b.b2, params, buffers, wpack, act, ws, training, momentum, nullptr, 1, upd));
        const elem_t* res = (const elem_t*)(act + b.fin_off);
        if (b.has_ds) {
            CK(conv_bn_fwd(s, n, b.cd, b.bd, params, buffers, wpack, act, ws, training, momentum, nullptr, 0, upd));
            res = (const elem_t*)(act + b.fzd_off);
        }
        CK(conv_bn_fwd(s, n, b.c3, b.b3, params, buffers, wpack, act, ws, training, momentum, res, 1, upd));
    }
    for (int i = 0; i < 3; ++i) CK(conv_bn_fwd(s, n, n.up[i], n.up_bn[i], params, buffers, wpack, act, ws, training, momentum, nullptr, 1, upd));
    ConvEpilogue e;
    e.bias = (const float*)params[n.head.bias_idx];
    e.out_f32 = 1;
    e.f32 = n.f32 != 0;
    e.split = n.f32 == 2;
    const void* hwp = n.f32 == 1 ? params[n.head.w_idx] : (const void*)(wpack + n.head.wf_off);
    CK(conv_fprop(s, n.head.g, (const elem_t*)(act + n.head.fin_off), (const elem_t*)hwp, act + n.head_out_off, e));
    return pw_nhwc_to_nchw_f32(s, act + n.head_out_off, 1, out_nchw, n.N, n.K, n.Hout * n.Wout, n.K, nullptr, nullptr);
}

namespace {
// backward of conv+bn(+relu): dz (grad wrt z) -> parameter grads, returns dx of the conv input in a pool buffer
// relu: 0 none, 1 mask from the saved z (bn3: z includes the residual), 2 mask recomputed from y (z is not read)
// pre:  the dgrad that produced dz already applied this BN's mask and left the partial sums in pre->slab (dz is g)
// next: the BN that consumes dx; this layer's dgrad masks dx for it and reduces its sums (filled by bn_stat_of)
int conv_bn_bwd(hipStream_t s, const Net& n, const ConvL& c, const BnL& b, const void* const* params, const char* wpack, char* act, char* ws,
                void* const* grads, float beta, Pool& pool, const void* dz, int dz_f32, elem_t* gout, int relu, const elem_t* dx_res,
                elem_t** dx_out, bool need_dx, int dx_f32, bool grouped_wgrad, const DgradBnStat* pre = nullptr, DgradBnStat* next = nullptr) {
    float* slab = (float*)(ws + n.ws_slab);
    float* coef = (float*)(ws + n.ws_coef) + 4096;
    const float* save = (const float*)(act + b.save_off);
    elem_t* dy = (elem_t*)(ws + c.dy_off);
    if (pre)
        CK(pw_bn_bwd_pre(s, dz, dz_f32, (const elem_t*)(act + c.y_off), dy, b.npix, b.C, (const float*)params[b.g_idx], save, save + b.C, pre->slab,
                         pre->rows, coef, (float*)grads[b.g_idx], (float*)grads[b.b_idx], beta, n.policy.bn_bwd_chunked | (n.policy.bn_xcd_rows ? (1 << 30) : 0) | (n.policy.bn_xcd_rows >= 2 ? (1 << 29) : 0),
                         n.policy.bn_bwd_pre_legacy));
    else
        CK(pw_bn_bwd(s, dz, dz_f32, (const elem_t*)(act + b.z_off), (const elem_t*)(act + c.y_off), dy, gout, b.npix, b.C, (const float*)params[b.g_idx],
                     save, save + b.C, relu, slab, coef, (float*)grads[b.g_idx], (float*)grads[b.b_idx], beta, (const float*)params[b.b_idx],
                     n.policy.bn_bwd_chunked));
    const elem_t* xin = (const elem_t*)(act + c.in_off);
    if (c.bias_idx >= 0 && beta == 0.f) {
        // bias in front of a training-mode BatchNorm: its gradient is the pixel sum of dy = gamma * invstd * (g - mean(g) - xhat * mean(g xhat)),
        // which is zero identically (autograd returns rounding noise around 0 there)
        if (pw_zero(s, grads[c.bias_idx], (size_t)c.g.Co * sizeof(float)) != UDAPOSE_OK) return UDAPOSE_ERR_LAUNCH;
    }
    if (c.g.smallc() && grouped_wgrad && n.policy.wgrad_group_stem) {
        // (the stem's weight gradient joins the grouped launch in its row-tap form, run_wg_group)
    } else if (c.g.smallc()) {
        float* tmp = (float*)(ws + n.ws_dwtmp);
        CK(conv_wgrad(s, c.g, dy, xin, tmp, 0, -1));
        CK(pw_unpack_strided(s, tmp, (float*)grads[c.w_idx], c.g.Co, c.g.KH, c.g.KWp(), c.g.KW, 8, 3, (long)c.g.KH * c.g.KW * 3, (long)c.g.KW * 3, 3, 1,
                             beta));
    } else if (!grouped_wgrad) {
        CK(conv_wgrad(s, c.g, dy, xin, (float*)grads[c.w_idx], beta != 0.f, -1));
    }
    if (need_dx) {
        elem_t* dx = pool.get();
        if (!dx) return UDAPOSE_ERR_ARG;
        CK(conv_dgrad(s, c.g, dy, (const elem_t*)(wpack + c.wb_off), dx, dx_res, dx_f32, next));
        *dx_out = dx;
    }
    return UDAPOSE_OK;
}

// the consumer-BN description a dgrad epilogue needs: relu 1 = mask from the saved z, 2 = mask recomputed from y
DgradBnStat bn_stat_of(const Net& n, const ConvL& c, const BnL& b, const void* const* params, char* act, char* ws, int relu) {
    DgradBnStat st;
    const float* save = (const float*)(act + b.save_off);
    st.y = (const elem_t*)(act + c.y_off);
    st.z = relu == 1 ? (const elem_t*)(act + b.z_off) : nullptr;
    st.mask = (relu == 1 && b.mask_off && n.policy.bn3_mask) ? (const unsigned char*)(act + b.mask_off) : nullptr;
    st.mean = save; st.invstd = save + b.C;
    st.gamma = (const float*)params[b.g_idx]; st.beta = (const float*)params[b.b_idx];
    st.slab = (float*)(ws + n.ws_slabf);
    return st;
}

// ---- grouped weight gradients ------------------------------------------------------------------------------------------
// The weight gradient of a layer needs only that layer's dy and saved input, and nobody reads it before the optimizer.
// Launched layer by layer, most of these GEMMs are too small for the chip (a layer3 1x1: 4 GFLOP, 16 tiles of 128x128) and
// had to split their pixel reduction 8-64 ways to fill it (fp32 atomics into a zeroed dW: ~1.3 TB/s chip-wide).  One
// launch over ALL layers has thousands of tiles: most layers reduce all their pixels inside one work-group (plain stores,
// deterministic, no memset), take 128x128 tiles, and only the large-image layers are still split.

// first block of layer3: the backward of a data-parallel step is cut there (net_backward part 1 / part 2), because the
// gradients of everything above it - 94 % of the parameters - are complete at that point and their all-reduce can run under
// the rest of the backward
inline int split_block(const Net& n) { return n.layers[0] + n.layers[1]; }

// which layers a `part` of the grouped weight gradients covers: 0 all, 1 / 2 the data-parallel cut
struct PartSel { bool head_up; int hi, lo; bool stem; };
PartSel part_sel(const Net& n, int part) {
    const int nb = (int)n.blocks.size(), split = split_block(n);
    if (part == 1) return PartSel{true, nb - 1, split, false};
    if (part == 2) return PartSel{false, split - 1, 0, true};
    return PartSel{true, nb - 1, 0, true};
}
// the convolutions of a part in the order of the grouped table's entries (after the head and the stem, which every site treats apart):
// up[2..0], then the blocks from last to first, each as c3, c2, cd, c1.  fn as in the walks above: void, or an int status that stops the walk.
template <class N, class F> int for_each_conv_wgrad(N& n, const PartSel& sel, F fn) {
    int rc = UDAPOSE_OK;
    for (int i = 2; sel.head_up && rc == UDAPOSE_OK && i >= 0; --i) rc = walk_rc(fn, n.up[i]);
    for (int bi = sel.hi; rc == UDAPOSE_OK && bi >= sel.lo; --bi) {
        auto& b = n.blocks[bi];
        if ((rc = walk_rc(fn, b.c3)) == UDAPOSE_OK && (rc = walk_rc(fn, b.c2)) == UDAPOSE_OK && (!b.has_ds || (rc = walk_rc(fn, b.cd)) == UDAPOSE_OK))
            rc = walk_rc(fn, b.c1);
    }
    return rc;
}

// ---- the deal of a grouped launch: which XCD runs which work-groups, and in which order ----------------------------------------
// A unit is one (layer, split): `nblk` work-groups (local indices base .. base + nblk - 1) of `st` 64-pixel stages each (+ 4: prologue,
// epilogue and stores, in stage units).  The hardware starts an XCD's list in list order on its 128 resident slots (32 CUs x 4).
// order 0 (rounds 1-6): whole units sorted by unit load nblk * (st + 4), each dealt to the least loaded XCD, lists kept in deal order.
//   Measured on the benched plan (profiles/tail_timeline.txt): nearly every work-group of both classes has 128 stages (~300 / ~170 us of
//   lifetime), the few 32-stage layers (layer4) sit on ONE XCD each in the middle of its list, every list ends with 128-stage work-groups
//   and the launches drain for 260 / 160 us; what a stage costs depends on what else is resident on the XCD (1.7 - 3.1 us for the same
//   tile), so lists levelled by st + 4 still finish up to 200 us apart.
// order 1: units are cut into runs of at most WG_DEAL_RUN consecutive work-groups (neighbouring tiles of one tap: they still share their
//   operands in that XCD's L2; a layer that is cut re-reads its dy / x once per XCD it lands on - the short layers this matters for hold
//   2048 pixels), the runs are sorted by stages per work-group, longest first (ties: larger run first), and dealt in that order to the
//   least loaded XCD.  Every list is then longest-first by construction and ends with its share of the SHORT work-groups, which level
//   the lists; and because every XCD gets the same mix of layers, a stage's true cost need not be known for the lists to finish together.
// The model (wg_model_finish): work-groups start in list order, each on the slot that frees first, and run st + 4 time units.
#define WG_DEAL_RUN 32
struct WgUnit { int prob, base, nblk, st; long load; };
double wg_model_finish(const std::vector<WgUnit>& runs, const std::vector<int>& lst, int slots = 128) {
    std::priority_queue<double, std::vector<double>, std::greater<double>> free_at;
    for (int i = 0; i < slots; ++i) free_at.push(0.0);
    double end = 0.0;
    for (int ui : lst)
        for (int l = 0; l < runs[ui].nblk; ++l) {
            const double t = free_at.top() + runs[ui].st + 4;
            free_at.pop();
            free_at.push(t);
            end = std::max(end, t);
        }
    return end;
}
// units -> runs (order 0: the units themselves) and the list of run indices of each XCD
void wg_deal(const std::vector<WgUnit>& units, int order, std::vector<WgUnit>& runs, std::vector<int> lst[8]) {
    runs.clear();
    for (const WgUnit& u : units) {
        const int step = order == 0 ? u.nblk : WG_DEAL_RUN;
        for (int l0 = 0; l0 < u.nblk; l0 += step) {
            const int cnt = std::min(step, u.nblk - l0);
            runs.push_back(WgUnit{u.prob, u.base + l0, cnt, u.st, (long)cnt * (u.st + 4)});
        }
    }
    std::vector<int> idx(runs.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int)i;
    if (order == 0) std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return runs[a].load > runs[b].load; });
    else std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return runs[a].st != runs[b].st ? runs[a].st > runs[b].st : runs[a].load > runs[b].load; });
    long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 8; ++k) lst[k].clear();
    for (int ui : idx) {
        int x = 0;
        for (int k = 1; k < 8; ++k) if (load[k] < load[x]) x = k;
        load[x] += runs[ui].load;
        lst[x].push_back(ui);
    }
}

// (sizing = true: a dry walk that only adds up the bytes of partial tiles the part's split reductions need, into *need)
int build_wg_group(Net& n, Net::WgGroup& G, void* const* grads, float beta, int part, bool sizing = false, size_t* need = nullptr) {
    const PartSel sel = part_sel(n, part);
    const bool upper = sel.head_up, lower = sel.stem;
    std::vector<WgParams> tab[WG_CLASSES];
    std::vector<WgUnit> units[WG_CLASSES];
    G.zero.clear();
    G.rel.clear();
    G.rel_bytes.clear();
    G.rel_cls.clear();
    for (int t = 0; t < WG_CLASSES; ++t) G.flops[t] = 0.0;
    // Split reductions: every non-empty split z of a layer stores its partial tile at ws_wgpart + part_cur + z * span (plain stores,
    // WG_FLAG_DW_WS addressing); SumJob (part, dst, span, splits) lets pw_split_sum add them in split order into the gradient tensor
    // (dst = beta * dst + sum) - or, for the stem's row-tap form, into its padded scratch, from which the unpack launch goes on.
    std::vector<SumJob> sums;
    size_t part_cur = 0;
    const bool det = n.policy.wgrad_det && n.policy.wgrad_group;      // (the same condition sizes the workspace: net_ws_bytes)
    auto make_partial = [&](WgParams& p, long long dst_off, int dst_ws, int Cdim) -> int {
        const int ms_total = (p.M + 63) / 64, per = (ms_total + p.ksplit - 1) / p.ksplit;
        const int ks_eff = (ms_total + per - 1) / per;                      // splits that own at least one stage (the others have no unit)
        const size_t span = (size_t)p.rows_valid * p.wtaps * Cdim;
        if (span >= (1ull << 31) || (span & 3)) return UDAPOSE_ERR_UNSUPPORTED;
        p.flags = (p.flags & ~WG_FLAG_ATOMIC) | WG_FLAG_DW_WS;
        p.dw = (float*)(n.ws_wgpart + part_cur);
        p.part_stride = (unsigned)span;
        sums.push_back(SumJob{(long long)(n.ws_wgpart + part_cur), dst_off, (unsigned)span, (unsigned)span, ks_eff, dst_ws, dst_ws ? 0.f : beta, 0});
        part_cur = align_up(part_cur + (size_t)ks_eff * span * sizeof(float));
        return UDAPOSE_OK;
    };
    // one table entry of class t: the layer's parameters, its flops, and one unit per split that owns at least one stage
    auto emit = [&](int t, const WgParams& p, double fl) {
        const int prob = (int)tab[t].size();
        tab[t].push_back(p);
        G.flops[t] += fl;
        const int nblk = p.r_tiles * p.c_tiles * p.total_taps;
        const int ms_total = (p.M + 63) / 64, per = (ms_total + p.ksplit - 1) / p.ksplit;
        for (int z = 0; z < p.ksplit; ++z) {
            const int st = std::min(per, ms_total - z * per);
            if (st > 0) units[t].push_back(WgUnit{prob, z * nblk, nblk, st, (long)nblk * (st + 4)});
        }
    };
    auto add_geom = [&](const ConvGeom& g, int w_idx, size_t dy_off, size_t in_off, int rows_valid) -> int {
        if (g.smallc()) return UDAPOSE_OK;
        WgParams p;
        double fl = 0.0;
        // byte offsets from the workspace / activation arena / gradient bases in place of pointers (see wgrad_dma_group_kernel)
        const ptrdiff_t drel = sizing ? 0 : (const char*)grads[w_idx] - (const char*)grads[0];
        G.rel.push_back({w_idx, drel});
        CK(conv_wgrad_params(g, (const elem_t*)dy_off, (const elem_t*)in_off, (float*)drel, rows_valid, &p, &fl));
        const int t = wgrad_group_plan(p, beta != 0.f, n.policy.wgrad_stages, n.policy);
        if (t < 0) return UDAPOSE_ERR_UNSUPPORTED;
        G.rel_bytes.push_back((size_t)p.rows_valid * p.wtaps * ((p.flags & WG_FLAG_SWAP) ? p.Co : p.Ci) * sizeof(float));
        if (p.ksplit > 1) {
            const bool swap = (p.flags & WG_FLAG_SWAP) != 0;
            if (det) CK(make_partial(p, (long long)drel, 0, swap ? p.Co : p.Ci));
            else if (beta == 0.f) G.zero.push_back({drel, (size_t)p.rows_valid * p.wtaps * (swap ? p.Co : p.Ci) * sizeof(float)});
        }
        G.rel_cls.push_back(t);
        emit(t, p, fl);
        return UDAPOSE_OK;
    };
    if (upper) {   // head: dy is channel-padded to 64, only the K real rows of dW exist
        ConvGeom hg = n.head.g;
        hg.Co = 64;
        CK(add_geom(hg, n.head.w_idx, n.ws_dyhead, n.head.in_off, n.K));
        G.flops[1] -= 2.0 * n.N * n.Hout * n.Wout * 256.0 * (64 - n.K);   // (count the K real channels only)
    }
    if (lower && n.policy.wgrad_group_stem) {
        // stem (Ci == 8): row-tap form into the padded [Co][KH][8][8] scratch in the workspace (always zeroed, always split:
        // 8192 stages), unpacked into the real [Co][KH][KW][3] gradient after the launch
        WgParams p;
        double fl = 0.0;
        CK(conv_wgrad_params(n.stem.g, (const elem_t*)n.stem.dy_off, (const elem_t*)n.stem.in_off, (float*)n.ws_dwtmp, -2, &p, &fl));
        p.flags |= WG_FLAG_DW_WS;
        const int t = wgrad_group_plan(p, 1, n.policy.wgrad_stages, n.policy);      // (accumulate = 1: atomics into the zeroed scratch)
        if (t != 1) return UDAPOSE_ERR_UNSUPPORTED;
        if (det) CK(make_partial(p, (long long)n.ws_dwtmp, 1, 64));     // ... or partial tiles, summed into the scratch
        emit(t, p, fl);
    }
    CK(for_each_conv_wgrad(n, sel, [&](const ConvL& c) { return add_geom(c.g, c.w_idx, c.dy_off, c.in_off, -1); }));
    if (sizing) { if (need) *need = part_cur; return UDAPOSE_OK; }
    if (part_cur > n.ws_wgpart_bytes) return UDAPOSE_ERR_NOT_PREPARED;      // (the policy's split length changed after the workspace was sized: udapose_net_ws_bytes)
    for (int t = 0; t < WG_CLASSES; ++t) {
        G.d_tab[t].reset();
        G.d_blk[t].reset();
        G.per_xcd[t] = 0;
        if (tab[t].empty()) continue;
        // deal the units' work-groups to the 8 XCDs' lists (wg_deal above)
        std::vector<int> deal[8];
        std::vector<WgUnit> runs;
        wg_deal(units[t], n.policy.wgrad_order, runs, deal);
        std::vector<WgGroupBlk> lst[8];
        for (int x = 0; x < 8; ++x)
            for (int ui : deal[x]) {
                const WgUnit& u = runs[ui];
                for (int l = 0; l < u.nblk; ++l) lst[x].push_back(WgGroupBlk{u.prob, u.base + l});
            }
        size_t per = 0;
        for (int k = 0; k < 8; ++k) per = std::max(per, lst[k].size());
        std::vector<WgGroupBlk> flat(8 * per, WgGroupBlk{-1, 0});
        for (int k = 0; k < 8; ++k) std::copy(lst[k].begin(), lst[k].end(), flat.begin() + k * per);
        CK(G.d_tab[t].upload(tab[t]));
        CK(G.d_blk[t].upload(flat));
        G.per_xcd[t] = (int)per;
    }
    G.d_zero.reset();
    bool granular = !G.zero.empty();
    for (auto& z : G.zero) granular = granular && (z.second % 16 == 0) && ((((size_t)(const char*)grads[0]) + (size_t)z.first) % 16 == 0);
    if (granular) {
        std::vector<ZeroJob> zj;
        for (auto& z : G.zero) zj.push_back(ZeroJob{(long long)z.first, (long long)(z.second / 16)});
        CK(G.d_zero.upload(zj));
    }
    // the split-sum launch's tables: jobs, and one block per UDAPOSE_SPLIT_SUM_CHUNK elements of a job
    G.d_sum.reset();
    G.d_sum_blk.reset();
    G.n_sum_blk = 0; G.n_sum_ws_blk = 0;
    if (!sums.empty()) {
        std::vector<int> blk;
        for (const int ws_jobs : {0, 1})
            for (size_t j = 0; j < sums.size(); ++j) {
                if ((sums[j].dst_ws != 0) != (ws_jobs != 0)) continue;
                for (unsigned c = 0; c < (sums[j].n + UDAPOSE_SPLIT_SUM_CHUNK - 1u) / UDAPOSE_SPLIT_SUM_CHUNK; ++c) {
                    blk.push_back((int)j); blk.push_back((int)c);
                    G.n_sum_ws_blk += ws_jobs;
                }
            }
        CK(G.d_sum.upload(sums));
        CK(G.d_sum_blk.upload(blk));
        G.n_sum_blk = (int)(blk.size() / 2);
    }
    G.h_sum = sums;
    G.k_beta = beta; G.k_stages = n.policy.wgrad_stages; G.k_part = part;
    G.k_det = det; G.k_stem = n.policy.wgrad_group_stem != 0; G.part_bytes = part_cur; G.k_order = n.policy.wgrad_order; G.k_geo_s = n.policy.wgrad_fastgeo_strided;
    return UDAPOSE_OK;
}

// bytes of partial tiles a whole backward pass needs with the plan's current policy (a dry walk of the table builder; part 0 covers parts 1 / 2)
size_t wg_partial_bytes(Net& n) {
    Net::WgGroup G;
    size_t need = 0;
    if (build_wg_group(n, G, nullptr, 0.f, 0, true, &need) != UDAPOSE_OK) return 0;
    return need;
}

// The tables hold OFFSETS (relative to the arenas and to grads[0]), so one pair of tables - overwrite and accumulate mode -
// serves every pass whose gradient tensors keep their relative placement (both per-pass gradient buffers of a step do).
// Only tables built under the plan's current policy qualify (split form, split length, stem), and partial tiles only while the
// workspace size the caller was last given (udapose_net_ws_bytes) holds them.
Net::WgGroup* find_wg_group(Net& n, void* const* grads, float beta, int part) {
    const bool det = n.policy.wgrad_det && n.policy.wgrad_group, stem = n.policy.wgrad_group_stem != 0;
    for (auto& g : n.wg_groups) {
        if (g.k_beta != beta || g.k_stages != n.policy.wgrad_stages || g.k_part != part || g.k_det != det || g.k_stem != stem ||
            g.k_order != n.policy.wgrad_order || g.k_geo_s != n.policy.wgrad_fastgeo_strided) continue;
        if (g.k_det && g.part_bytes > n.ws_wgpart_bytes) continue;
        bool same = true;
        for (auto& r : g.rel)
            if ((const char*)grads[r.first] - (const char*)grads[0] != r.second) { same = false; break; }
        if (same) return &g;
    }
    return nullptr;
}
// net_bind_grads: allocate + upload the grouped weight-gradient tables (both accumulate modes) for this gradient placement.
// Synchronous - never inside a stream capture; net_backward itself never builds them.
int bind_wg_groups(Net& n, void* const* grads) {
    // 3 parts x 2 accumulate modes per gradient placement (a few KB of device tables each).  Tables are never evicted or rebuilt
    // in place: launches captured in a hipGraph hold their device pointers, and a process only ever uses a handful of
    // gradient placements (two per-pass buffers per network).
    for (const int part : {0, 1, 2})
        for (const float beta : {0.f, 1.f}) {
            if (find_wg_group(n, grads, beta, part)) continue;
            n.wg_groups.emplace_back();
            Net::WgGroup* G = &n.wg_groups.back();
            const int rc = build_wg_group(n, *G, grads, beta, part);
            if (rc != UDAPOSE_OK) { n.wg_groups.pop_back(); return rc; }
            G->last_use = ++n.wg_tick;
        }
    return UDAPOSE_OK;
}
// what precedes the grouped launches of one pass (the clears of the atomic form) and what follows them (the split sums, the stem's unpack)
int wg_before(hipStream_t s, Net& n, Net::WgGroup* G, char* ws, void* const* grads, bool with_stem) {
    G->last_use = ++n.wg_tick;
    if (G->d_zero.d) {
        CK(pw_zero_multi(s, G->d_zero.d, (int)G->d_zero.n, grads[0]));
    } else {
        for (auto& z : G->zero)
            if (pw_zero(s, (char*)grads[0] + z.first, z.second) != UDAPOSE_OK) return UDAPOSE_ERR_LAUNCH;
    }
    const ConvGeom& sg = n.stem.g;
    if (with_stem && !G->k_det && pw_zero(s, ws + n.ws_dwtmp, (size_t)sg.Co * sg.KH * 8 * 8 * sizeof(float)) != UDAPOSE_OK) return UDAPOSE_ERR_LAUNCH;
    return UDAPOSE_OK;
}
int wg_after(hipStream_t s, Net& n, Net::WgGroup* G, char* ws, void* const* grads, float beta, bool with_stem, bool sums_done = false) {
    if (G->n_sum_blk && !sums_done) CK(pw_split_sum(s, G->d_sum.d, G->d_sum_blk.d, G->n_sum_blk, ws, (char*)grads[0]));
    const ConvGeom& sg = n.stem.g;
    if (with_stem)
        CK(pw_unpack_strided(s, (const float*)(ws + n.ws_dwtmp), (float*)grads[n.stem.w_idx], sg.Co, sg.KH, sg.KWp(), sg.KW, 8, 3,
                             (long)sg.KH * sg.KW * 3, (long)sg.KW * 3, 3, 1, beta));
    return UDAPOSE_OK;
}
// does any byte the grouped launches of pass A write (the weight gradients of its table, the stem's) belong to a tensor pass B writes?
// (compared as the spans [lowest start, highest end) of each pass's tensors: disjoint buffers never overlap, interleaved ones are
// taken as overlapping - the safe answer)
bool wg_overlap(const Net& n, const Net::WgGroup* GA, void* const* gradsA, const Net::WgGroup* GB, void* const* gradsB, bool with_stem) {
    auto span = [&](const Net::WgGroup* G, void* const* grads, uintptr_t& lo, uintptr_t& hi) {
        lo = UINTPTR_MAX; hi = 0;
        auto add = [&](int idx, size_t bytes) {
            const uintptr_t a = (uintptr_t)grads[idx];
            lo = std::min(lo, a); hi = std::max(hi, a + bytes);
        };
        for (size_t i = 0; i < G->rel.size(); ++i) add(G->rel[i].first, G->rel_bytes[i]);
        if (with_stem) add(n.stem.w_idx, (size_t)n.stem.g.Co * n.stem.g.KH * n.stem.g.KW * 3 * sizeof(float));
    };
    uintptr_t la, ha, lb, hb;
    span(GA, gradsA, la, ha);
    span(GB, gradsB, lb, hb);
    return la < hb && lb < ha;
}
// The grouped launches of one pass (GB == nullptr), or of two passes with equal table shapes as ONE grid per tile class, each inside the
// profiler's bracket.  With policy.timeline every launch stamps behind the last: 8 stamp blocks per list entry and pass.
int launch_wg_classes(hipStream_t s, const Net& n, const Net::WgGroup* GA, const char* actA, char* wsA, void* gA, const Net::WgGroup* GB = nullptr,
                      const char* actB = nullptr, char* wsB = nullptr, void* gB = nullptr) {
    size_t stamped = 0;     // (work-groups of the classes before this one)
    for (int t = 0; t < WG_CLASSES; ++t) {
        if (!GA->per_xcd[t]) continue;
        unsigned long long* stamps = nullptr;
        if (n.policy.timeline) {
            const size_t blocks = (GB ? 16 : 8) * (size_t)GA->per_xcd[t];
            if (stamped + blocks > WG_STAMP_BLOCKS) return UDAPOSE_ERR_ARG;
            stamps = (unsigned long long*)n.policy.timeline + stamped * 8;
            stamped += blocks;
        }
        const int tok = conv_prof_before(s, 2, GB ? GA->flops[t] + GB->flops[t] : GA->flops[t]);
        const int rc = wgrad_group_launch(s, t, GA->d_tab[t].d, GA->d_blk[t].d, GA->per_xcd[t], actA, wsA, gA, GB ? GB->d_tab[t].d : nullptr,
                                          GB ? GB->d_blk[t].d : nullptr, actB, wsB, gB, stamps);
        conv_prof_after(s, tok);
        CK(rc);
    }
    return UDAPOSE_OK;
}
int run_wg_group(hipStream_t s, Net& n, const char* act, char* ws, void* const* grads, float beta, int part) {
    if (n.deferred.G) return UDAPOSE_ERR_NOT_PREPARED;      // (split sums of an earlier pair call are still waiting for their update or flush)
    Net::WgGroup* G = find_wg_group(n, grads, beta, part);
    if (!G) return UDAPOSE_ERR_NOT_PREPARED;
    const bool with_stem = part_sel(n, part).stem && G->k_stem;
    CK(wg_before(s, n, G, ws, grads, with_stem));
    CK(launch_wg_classes(s, n, G, act, ws, grads[0]));
    return wg_after(s, n, G, ws, grads, beta, with_stem);
}
// The grouped weight gradients of TWO passes of this plan (each with its own arenas, gradient tensors and accumulate mode) as ONE
// launch per tile class: the step's two student passes end at about the same time and their weight-gradient launches are fully
// exposed there; one grid of twice the size has half the tail (measured on the launches alone: 2498 us for 64 images against 2 x 1353).
// defer (udapose_net_wgrad_pair_defer): leave the split sums of the gradient tensors to the optimizer sweep of the next udapose_net_fused_update,
// which reads the partial tiles itself - one launch and 2 x (read + write) of the split layers' gradients less on the step's serial tail.  Taken
// only where the sweep can stand in for the sums exactly: one table for both passes, overwriting passes (beta 0: a pass that accumulates needs
// its tensor updated for the NEXT accumulation), whole backward, and an update table bound for these gradient tensors that knows the split jobs.
// *deferred tells the caller whether it was taken.  The stem's sum goes into the workspace and feeds its unpack launch: it still runs here.
int run_wg_pair(hipStream_t s, Net& n, const char* actA, char* wsA, void* const* gradsA, float betaA, const char* actB, char* wsB,
                void* const* gradsB, float betaB, int part, bool defer, int* deferred) {
    if (part < 0 || part > 2 || (n.f32 && !n.strict) || !n.policy.wgrad_group) return UDAPOSE_ERR_ARG;
    DbgSyncScope dbg(n.policy.debug_sync);
    if (deferred) *deferred = 0;
    Net::WgGroup* GA = find_wg_group(n, gradsA, betaA, part);
    Net::WgGroup* GB = find_wg_group(n, gradsB, betaB, part);
    if (!GA || !GB) return UDAPOSE_ERR_NOT_PREPARED;
    if (n.deferred.G) return UDAPOSE_ERR_NOT_PREPARED;
    bool same = true;
    for (int t = 0; t < WG_CLASSES; ++t) same = same && GA->per_xcd[t] == GB->per_xcd[t];
    const bool with_stem = part_sel(n, part).stem && GA->k_stem;
    // One grid runs the two passes' tiles in any order, so their gradient tensors must not share a byte: a pass that accumulates onto
    // the other's result (one buffer, beta 0 then 1) needs the other's stores to have landed - two launches in order.
    if (same && wg_overlap(n, GA, gradsA, GB, gradsB, with_stem)) same = false;
    if (!same) {        // (different table shapes, or overlapping tensors: two launches)
        CK(run_wg_group(s, n, actA, wsA, gradsA, betaA, part));
        return run_wg_group(s, n, actB, wsB, gradsB, betaB, part);
    }
    CK(wg_before(s, n, GA, wsA, gradsA, with_stem));
    CK(wg_before(s, n, GB, wsB, gradsB, with_stem));
    CK(launch_wg_classes(s, n, GA, actA, wsA, gradsA[0], GB, actB, wsB, gradsB[0]));
    // (one table for both passes - equal accumulate modes and the same relative placement of the gradient tensors, so that the jobs'
    // destination offsets hold for both: their split sums share it, one launch over both workspaces)
    const bool pair_sum = GA == GB && GA->n_sum_blk > 0;
    const bool leave = defer && pair_sum && part == 0 && betaA == 0.f && n.upd.jobs.d && n.upd_sum_group == GA && n.upd.k_g == gradsA[0] &&
                       GA->n_sum_blk > GA->n_sum_ws_blk;
    if (leave) {
        const int rest = GA->n_sum_blk - GA->n_sum_ws_blk;
        CK(pw_split_sum(s, GA->d_sum.d, GA->d_sum_blk.d + 2 * rest, GA->n_sum_ws_blk, wsA, (char*)gradsA[0], wsB, (char*)gradsB[0]));
        n.deferred = Net::Deferred{GA, wsA, wsB, (char*)gradsA[0], (char*)gradsB[0]};
        if (deferred) *deferred = 1;
    } else if (pair_sum) {
        CK(pw_split_sum(s, GA->d_sum.d, GA->d_sum_blk.d, GA->n_sum_blk, wsA, (char*)gradsA[0], wsB, (char*)gradsB[0]));
    }
    CK(wg_after(s, n, GA, wsA, gradsA, betaA, with_stem, pair_sum));
    return wg_after(s, n, GB, wsB, gradsB, betaB, with_stem, pair_sum);
}
}  // namespace

int net_wgrad_pair(void* h, hipStream_t s, const void* actA, void* wsA, void* const* gradsA, float betaA, const void* actB, void* wsB,
                   void* const* gradsB, float betaB, int part) {
    return run_wg_pair(s, *(Net*)h, (const char*)actA, (char*)wsA, gradsA, betaA, (const char*)actB, (char*)wsB, gradsB, betaB, part, false, nullptr);
}
int net_wgrad_pair_defer(void* h, hipStream_t s, const void* actA, void* wsA, void* const* gradsA, float betaA, const void* actB, void* wsB,
                         void* const* gradsB, float betaB, int part, int* deferred) {
    return run_wg_pair(s, *(Net*)h, (const char*)actA, (char*)wsA, gradsA, betaA, (const char*)actB, (char*)wsB, gradsB, betaB, part, true, deferred);
}
// the split sums a pair call left to an update that is not going to run: their own launch after all (no mark: nothing to do)
int net_split_sum_flush(void* h, hipStream_t s) {
    Net& n = *(Net*)h;
    const Net::Deferred d = n.deferred;
    if (!d.G) return UDAPOSE_OK;
    n.deferred = Net::Deferred{};
    return pw_split_sum(s, d.G->d_sum.d, d.G->d_sum_blk.d, d.G->n_sum_blk - d.G->n_sum_ws_blk, d.wsA, d.gA, d.wsB, d.gB);
}
// the deal of a grouped launch as a pure host function (tests): units (nblk, stages) -> the runs of every XCD's list in list order, as
// entries (xcd, unit, first work-group of the unit, count), at most `cap` of them; returns the number of entries; modelled finish per XCD
int net_wgrad_deal(const int* nblk, const int* stages, int n_units, int order, int* ent_xcd, int* ent_unit, int* ent_first, int* ent_count, int cap,
                   double* finish_out) {
    if (!nblk || !stages || n_units < 0 || order < 0 || order > 1 || cap < 0) return UDAPOSE_ERR_ARG;
    std::vector<WgUnit> units;
    for (int i = 0; i < n_units; ++i) {
        if (nblk[i] < 1 || stages[i] < 1) return UDAPOSE_ERR_ARG;
        units.push_back(WgUnit{i, 0, nblk[i], stages[i], (long)nblk[i] * (stages[i] + 4)});
    }
    std::vector<WgUnit> runs;
    std::vector<int> lst[8];
    wg_deal(units, order, runs, lst);
    int ne = 0;
    for (int x = 0; x < 8; ++x) {
        for (int ri : lst[x]) {
            if (ne < cap && ent_xcd && ent_unit && ent_first && ent_count) { ent_xcd[ne] = x; ent_unit[ne] = runs[ri].prob; ent_first[ne] = runs[ri].base; ent_count[ne] = runs[ri].nblk; }
            ++ne;
        }
        if (finish_out) finish_out[x] = wg_model_finish(runs, lst[x]);
    }
    return ne;
}

// grads[i] (fp32, same physical layout as params[i]) = beta*grads[i] + d loss / d params[i]; beta in {0,1}
// part 0: the whole backward (one grouped weight-gradient launch per tile class at its end).
// part 1 / part 2: the same backward cut after the first block of layer3 (split_block): part 1 = head, deconvs, layer4, layer3
// and THEIR weight gradients - 94 % of the parameters, a contiguous suffix of the flat gradient buffer, final when part 1 ends;
// part 2 = layer2, layer1, stem and theirs, continuing from the gradient part 1 left in the workspace.  Data parallel:
// the all-reduce of the suffix runs under part 2 (engine.py).  The two parts together enqueue exactly the kernels of part 0
// except that the weight gradients are two grouped launches per tile class instead of one.
// phase 0: the gradient chain, then the grouped weight-gradient launches of this part; 1: the chain only; 2: the grouped launches
// only (every layer owns its dy buffer in the workspace, so a caller may run them on another stream under the chain of part 2).
int net_backward(void* h, hipStream_t s, const float* dout_nchw, const void* const* params, const void* wpack_, void* act_, void* ws_,
                 void* const* grads, float beta, int part, int phase) {
    Net& n = *(Net*)h;
    if (part < 0 || part > 2 || phase < 0 || phase > 2) return UDAPOSE_ERR_ARG;
    if (phase != 0 && !n.policy.wgrad_group) return UDAPOSE_ERR_ARG;
    if (phase == 2) {
        if ((n.f32 && !n.strict) || n.fwd_only) return UDAPOSE_ERR_UNSUPPORTED;
        DbgSyncScope dbg2(n.policy.debug_sync);
        return run_wg_group(s, n, (const char*)act_, (char*)ws_, grads, beta, part);
    }
    DbgSyncScope dbg(n.policy.debug_sync);
    // fp32 / f16x2 modes and forward-only plans keep nothing for a backward; a 'strict' plan's forward left the 16-bit layout's tensors
    if ((n.f32 && !n.strict) || n.fwd_only) return UDAPOSE_ERR_UNSUPPORTED;
    const char* wpack = (const char*)wpack_;
    char* act = (char*)act_;
    char* ws = (char*)ws_;
    Pool pool;
    pool.base = ws;
    for (int i = 0; i < 6; ++i) pool.off[i] = n.ws_gbuf[i];
    const bool grouped = n.policy.wgrad_group != 0;
    if (grouped && (!find_wg_group(n, grads, beta, part))) return UDAPOSE_ERR_NOT_PREPARED;     // (before anything is enqueued)
    const int HWo = n.Hout * n.Wout;
    const int split = split_block(n);
    const bool fused = n.policy.bn_bwd_fused != 0;
    DgradBnStat cur, nxt;
    bool have = false;
    elem_t* dz = nullptr;
    if (part != 2) {
    // head
    elem_t* dyh = (elem_t*)(ws + n.ws_dyhead);
    CK(pw_nchw_f32_to_nhwc_bf16(s, dout_nchw, dyh, n.N, n.K, HWo, 64));
    ConvGeom hg = n.head.g;
    hg.Co = 64;   // dy is channel-padded to 64 (one 64-wide K step)
    float* tmp = (float*)(ws + n.ws_dwtmp);
    if (!grouped) {
        CK(conv_wgrad(s, hg, dyh, (const elem_t*)(act + n.head.in_off), tmp, 0, n.K));
        CK(pw_unpack_strided(s, tmp, (float*)grads[n.head.w_idx], n.K, 1, 1, 1, 256, 256, 256, 0, 0, 1, beta));
    }
    dz = pool.get();
    // Gradients entering the BatchNorm backward of the three deconv layers are kept in fp32: close to the loss the BN
    // projection (g - mean(g) - xhat*mean(g*xhat)) cancels ~90 % of g, so bf16 rounding of g is amplified ~10x in dy
    // (measured against the backward of the bf16-storage emulation: 2.4 % / 8 % / 14 % relative error per layer with
    // bf16 g).  The tensors are small (N*64*64*256 and below).
    //
    // Fused chain (g_bn_bwd_fused): every dgrad launch knows the BatchNorm that consumes its output; its epilogue applies
    // that BN's ReLU mask and reduces sum(g), sum(g*xhat) per m-tile, so a BN backward is ONE launch (column sums of the
    // slab + apply) for the wide layers and finalize + apply for the others.  `cur` describes the pending statistics of dz.
    if (fused) { cur = bn_stat_of(n, n.up[2], n.up_bn[2], params, act, ws, 2); have = true; }
    CK(conv_dgrad(s, hg, dyh, (const elem_t*)(wpack + n.head.wb_off), dz, nullptr, 1, have ? &cur : nullptr));
    // (the head's bias gradient is off the gradient chain: launched behind the first data gradient, not in front of it)
    CK(pw_plane_sum(s, dout_nchw, (float*)grads[n.head.bias_idx], n.N, n.K, HWo, beta));
    // deconv stack
    for (int i = 2; i >= 0; --i) {
        elem_t* dx = nullptr;
        if (fused) {
            if (i > 0) nxt = bn_stat_of(n, n.up[i - 1], n.up_bn[i - 1], params, act, ws, 2);
            else nxt = bn_stat_of(n, n.blocks.back().c3, n.blocks.back().b3, params, act, ws, 1);
        }
        CK(conv_bn_bwd(s, n, n.up[i], n.up_bn[i], params, wpack, act, ws, grads, beta, pool, dz, 1, nullptr, 2, nullptr, &dx, true, i > 0, grouped,
                       have ? &cur : nullptr, fused ? &nxt : nullptr));
        if (fused) cur = nxt;
        pool.put(dz);
        dz = dx;
    }
    } else {
        // part 2 resumes where part 1 stopped: the gradient entering block split-1 sits in the pool buffer part 1 ended on
        // (the buffer sequence is a function of the plan alone), masked for that block's bn3 with its sums in the slab
        if (split < 1 || split >= (int)n.blocks.size() || n.split_dz_idx < 0) return UDAPOSE_ERR_ARG;
        pool.used[n.split_dz_idx] = true;
        dz = (elem_t*)(ws + pool.off[n.split_dz_idx]);
        if (fused) {
            cur = bn_stat_of(n, n.blocks[split - 1].c3, n.blocks[split - 1].b3, params, act, ws, 1);
            cur.rows = conv_dgrad_stat_rows(n.blocks[split].c1.g);
            have = true;
        }
    }
    // bottlenecks, last to first
    const int bi_hi = part == 2 ? split - 1 : (int)n.blocks.size() - 1, bi_lo = part == 1 ? split : 0;
    for (int bi = bi_hi; bi >= bi_lo; --bi) {
        Block& b = n.blocks[bi];
        // bn3 (+ReLU of the block output): g = masked dz feeds the skip branch (written in place unless the producing dgrad
        // already masked it)
        elem_t *dz2 = nullptr, *dz1 = nullptr, *dxd = nullptr, *dxin = nullptr;
        if (fused) nxt = bn_stat_of(n, b.c2, b.b2, params, act, ws, 2);
        CK(conv_bn_bwd(s, n, b.c3, b.b3, params, wpack, act, ws, grads, beta, pool, dz, 0, dz, 1, nullptr, &dz2, true, 0, grouped, have ? &cur : nullptr,
                       fused ? &nxt : nullptr));
        if (fused) { cur = nxt; nxt = bn_stat_of(n, b.c1, b.b1, params, act, ws, 2); }
        CK(conv_bn_bwd(s, n, b.c2, b.b2, params, wpack, act, ws, grads, beta, pool, dz2, 0, nullptr, 2, nullptr, &dz1, true, 0, grouped,
                       have ? &cur : nullptr, fused ? &nxt : nullptr));
        if (fused) cur = nxt;
        pool.put(dz2);
        const elem_t* skip = dz;
        if (b.has_ds) {
            // the downsample BN shares g with bn3 (already masked): its own reduce / apply, no ReLU
            CK(conv_bn_bwd(s, n, b.cd, b.bd, params, wpack, act, ws, grads, beta, pool, dz, 0, nullptr, 0, nullptr, &dxd, true, 0, grouped));
            skip = dxd;
        }
        const bool chain = fused && bi > 0;      // dxin feeds bn3 of the previous block (block 0: the max-pool backward)
        if (chain) nxt = bn_stat_of(n, n.blocks[bi - 1].c3, n.blocks[bi - 1].b3, params, act, ws, 1);
        CK(conv_bn_bwd(s, n, b.c1, b.b1, params, wpack, act, ws, grads, beta, pool, dz1, 0, nullptr, 2, skip, &dxin, true, 0, grouped,
                       have ? &cur : nullptr, chain ? &nxt : nullptr));
        if (chain) cur = nxt;
        pool.put(dz1);
        if (dxd) pool.put(dxd);
        pool.put(dz);
        dz = dxin;
    }
    if (part == 1) {
        for (int i = 0; i < 6; ++i) if ((char*)dz == ws + pool.off[i]) n.split_dz_idx = i;      // (the same value on every pass)
        if (grouped && phase == 0) CK(run_wg_group(s, n, act, ws, grads, beta, 1));
        if (beta == 0.f) {       // backbone.fc lies in part 1's suffix of the gradient buffer (not part of forward: zero)
            if (pw_zero(s, grads[n.fc_w_idx], (size_t)1000 * 2048 * 4) != UDAPOSE_OK) return UDAPOSE_ERR_LAUNCH;
            if (pw_zero(s, grads[n.fc_b_idx], (size_t)1000 * 4) != UDAPOSE_OK) return UDAPOSE_ERR_LAUNCH;
        }
        return UDAPOSE_OK;
    }
    // stem: maxpool -> bn/relu -> conv (its dy stays at ws + stem.dy_off: the weight gradient's operand and net_input_grad's)
    if (n.policy.stem_fused >= 2 && grouped && n.policy.wgrad_group_stem) {
        // the max-pool backward is gathered inside the BN backward's two sweeps: the full-resolution gradient is never stored
        const BnL& sb = n.stem_bn;
        const float* save = (const float*)(act + sb.save_off);
        CK(pw_bn_bwd_pooled(s, dz, (const unsigned char*)(act + n.poolidx_off), n.Hs, n.Ws, (const elem_t*)(act + n.stem.y_off),
                            (elem_t*)(ws + n.stem.dy_off), sb.npix, sb.C, (const float*)params[sb.g_idx], save, save + sb.C, (float*)(ws + n.ws_slab),
                            (float*)(ws + n.ws_coef) + 4096, (float*)grads[sb.g_idx], (float*)grads[sb.b_idx], beta, (const float*)params[sb.b_idx]));
        pool.put(dz);
    } else {
    elem_t* dzs = pool.get();
    CK(pw_maxpool3x3s2_bwd(s, dz, (const unsigned char*)(act + n.poolidx_off), dzs, n.N, n.Hs, n.Ws, 64));
    pool.put(dz);
    elem_t* none = nullptr;
    CK(conv_bn_bwd(s, n, n.stem, n.stem_bn, params, wpack, act, ws, grads, beta, pool, dzs, 0, nullptr, 2, nullptr, &none, false, 0, grouped));
    pool.put(dzs);
    }
    if (grouped && phase == 0) CK(run_wg_group(s, n, act, ws, grads, beta, part));
    // backbone.fc is not part of the forward: zero gradient when overwriting
    if (beta == 0.f && part == 0) {
        if (pw_zero(s, grads[n.fc_w_idx], (size_t)1000 * 2048 * 4) != UDAPOSE_OK) return UDAPOSE_ERR_LAUNCH;
        if (pw_zero(s, grads[n.fc_b_idx], (size_t)1000 * 4) != UDAPOSE_OK) return UDAPOSE_ERR_LAUNCH;
    }
    return UDAPOSE_OK;
}

// d loss / d x (fp32 NCHW) from the stem's dy, which the stem's BatchNorm backward of a pass left at ws + stem.dy_off (both stem paths of
// net_backward; the grouped weight-gradient launch only reads it).  Stateless: the pass is named by its workspace.
int net_input_grad(void* h, hipStream_t s, const void* const* params, void* ws_, float* dx) {
    Net& n = *(Net*)h;
    if ((n.f32 && !n.strict) || n.fwd_only) return UDAPOSE_ERR_UNSUPPORTED;
    DbgSyncScope dbg(n.policy.debug_sync);
    CK(stem_dgrad(s, (const elem_t*)((const char*)ws_ + n.stem.dy_off), (const float*)params[n.stem.w_idx], n.N, n.H, n.W, dx));
    return UDAPOSE_OK;
}

// Apply the running-statistics update (momentum form, counter += 1) of every BN layer from the batch statistics saved in
// `act` by a forward that ran with the update deferred (training | 2): keeps the reference's update ORDER when two
// forwards of one module run concurrently on different streams.
int net_apply_running(void* h, hipStream_t s, const void* act_, void* const* buffers, float momentum) {
    Net& n = *(Net*)h;
    // one launch for all layers through the job table net_bind built for these buffers
    if (!n.d_runjobs.d || n.runjobs_key != buffers[0]) return UDAPOSE_ERR_NOT_PREPARED;
    return pw_bn_running_update_multi(s, n.d_runjobs.d, (int)n.d_runjobs.n, 2048, act_, momentum);
}
int net_bind_grads(void* h, void* const* grads) {
    Net& n = *(Net*)h;
    if (n.f32 && !n.strict) return UDAPOSE_OK;
    if (n.fwd_only) return UDAPOSE_ERR_UNSUPPORTED;
    return bind_wg_groups(n, grads);
}
// index (in .parameters() order) of the first parameter whose gradient is final when net_backward part 1 has run: the first
// parameter of layer3's first block.  Everything from there on (layer3, layer4, fc, upsampling, head) is part 1's.
long long net_grad_split_param(void* h) {
    Net& n = *(Net*)h;
    const int split = split_block(n);
    if (split < 1 || split >= (int)n.blocks.size()) return -1;
    return n.blocks[split].c1.w_idx;
}

// ---- fused optimizer tail: Adam on the student, EMA into the teacher, and the element-type weight packs of BOTH networks'
// plans in one sweep (optim.hip opt_tail_k).  hs / ht: the student's and the teacher's plans (same architecture).
// h_m / h_v: host arrays of the Adam moments per parameter index, NULL entries for parameters without gradient (backbone.fc:
// EMA only).  bind builds the device job table (allocates: outside capture); the update itself only launches.
// kind 1 (SGD with momentum): h_m holds the momentum buffers, h_v is not read.  group_idx (NULL: one group): the parameter group of every
// parameter, at most TAIL_GROUPS of them.
int net_bind_update_groups(void* hs, void* ht, int kind, void* const* params_s, void* const* grads, void* const* h_m, void* const* h_v,
                           void* const* params_t, void* wpack_s_, void* wpack_t_, const int* group_idx) {
    Net& n = *(Net*)hs;
    if (kind != 0 && kind != 1) return UDAPOSE_ERR_ARG;
    if (kind == 0 && !h_v) return UDAPOSE_ERR_ARG;
    int ngroups = 1;
    if (group_idx)
        for (int i = 0; i < n.n_params; ++i) {
            if (group_idx[i] < 0) return UDAPOSE_ERR_ARG;
            if (group_idx[i] >= TAIL_GROUPS) return UDAPOSE_ERR_UNSUPPORTED;
            ngroups = std::max(ngroups, group_idx[i] + 1);
        }
    const Net& nt = *(const Net*)ht;
    // teacher in the f16x2 mode (the reference's precision mix: fp16 student, fp32-grade teacher): its split packs are not written
    // by this sweep (the caller re-packs the teacher's plan with udapose_net_pack_weights after it), the EMA still is
    const bool t_split = nt.f32 == 2;
    // a 'strict' student: the sweep writes its 16-bit data-gradient packs; its split forward packs are refreshed by net_fused_update's pack
    // launch after the sweep (as a split teacher's are by the caller)
    const bool s_split = n.strict != 0;
    if ((n.f32 && !s_split) || nt.f32 == 1 || nt.strict || n.n_params != nt.n_params || (!t_split && (s_split || n.wpack_bytes != nt.wpack_bytes)))
        return UDAPOSE_ERR_UNSUPPORTED;
    char* ws_ = (char*)wpack_s_;
    char* wt_ = (char*)wpack_t_;
    std::vector<TailJob> jobs;
    std::vector<int> bj, bs;
    std::vector<char> covered(n.n_params, 0);
    // the split jobs of these gradient tensors' weight-gradient table (overwriting whole backward, current policy), if it is bound already: a job
    // whose gradient is split carries where the partial tensors lie, so that a sweep can add them itself (udapose_net_wgrad_pair_defer)
    // (the sweep that adds split sums itself has no SGD form: a table bound for SGD never offers it, and udapose_net_wgrad_pair_defer defers nothing)
    const Net::WgGroup* SG = grads[0] && kind == 0 ? find_wg_group(n, grads, 0.f, 0) : nullptr;
    if (SG && (!SG->k_det || SG->n_sum_blk <= SG->n_sum_ws_blk)) SG = nullptr;
    size_t split_found = 0;
    auto push = [&](int idx, void* sd, void* td, void* sx, void* tx, int A, int T, int B) -> int {
        const long long numel = n.param_numel[idx];
        void* const v_idx = kind == 0 ? h_v[idx] : nullptr;
        const int adam = (h_m[idx] && (kind == 1 || v_idx) && grads[idx]) ? 1 : 0;
        if (A) {
            const uintptr_t al = (uintptr_t)params_s[idx] | (uintptr_t)params_t[idx] | (adam ? ((uintptr_t)grads[idx] | (uintptr_t)h_m[idx] | (uintptr_t)v_idx) : 0);
            if ((al & 15) || (A & 63) || (B & 63) || (long long)A * T * B != numel) return UDAPOSE_ERR_UNSUPPORTED;
        }
        jobs.emplace_back();      // (value-initialised: every byte the table upload copies is defined, padding included)
        TailJob& j = jobs.back();
        j.p = (float*)params_s[idx]; j.g = (const float*)grads[idx]; j.m = (float*)h_m[idx]; j.v = (float*)v_idx; j.t = (float*)params_t[idx];
        j.sd = (elem_t*)sd; j.td = (elem_t*)td; j.sx = (elem_t*)sx; j.tx = (elem_t*)tx;
        j.A = A; j.T = T; j.B = B; j.adam = adam; j.n = numel;
        j.group = group_idx ? group_idx[idx] : 0;
        if (SG && adam)
            for (const SumJob& sj : SG->h_sum)
                if (!sj.dst_ws && sj.dst_off == (const char*)grads[idx] - (const char*)grads[0]) {
                    if ((long long)sj.n != numel) return UDAPOSE_ERR_UNSUPPORTED;
                    j.part_off = sj.part_off; j.stride = sj.stride; j.ks = sj.ks;
                    ++split_found;
                }
        const long nb = A ? (long)(A / 64) * (B / 64) * T : (long)((numel + opt_chunk() - 1) / opt_chunk());
        for (long k = 0; k < nb; ++k) { bj.push_back((int)jobs.size() - 1); bs.push_back((int)k); }
        covered[idx] = 1;
        return UDAPOSE_OK;
    };
    auto conv = [&](const ConvL& c) -> int {
        const ConvGeom& g = c.g;
        const int T = g.KH * g.KW;
        if (g.smallc()) return push(c.w_idx, nullptr, nullptr, nullptr, nullptr, 0, 0, 0);     // stem: packed by its own strided launch
        if (!g.transposed)   // master [Co][T][Ci]: fprop pack = cast, dgrad pack = per-tap transpose; the teacher needs the fprop pack
            return push(c.w_idx, s_split ? nullptr : ws_ + c.wf_off, t_split ? nullptr : wt_ + c.wf_off, ws_ + c.wb_off, nullptr, g.Co, T, g.Ci);
        // ConvTranspose2d master [Ci][T][Co]: dgrad pack = cast, fprop pack = per-tap transpose
        return push(c.w_idx, ws_ + c.wb_off, nullptr, s_split ? nullptr : ws_ + c.wf_off, t_split ? nullptr : wt_ + c.wf_off, g.Ci, T, g.Co);
    };
    CK(for_each_conv(n, conv));
    CK(push(n.head.w_idx, s_split ? nullptr : ws_ + n.head.wf_off, t_split ? nullptr : wt_ + n.head.wf_off, nullptr, nullptr, 0, 0, 0));      // [K][256]: the fprop pack is a cast
    for (int i = 0; i < n.n_params; ++i)
        if (!covered[i]) CK(push(i, nullptr, nullptr, nullptr, nullptr, 0, 0, 0));                   // BN vectors, head bias, backbone.fc
    if (SG) {       // (every split job of the table must have found its parameter, or no sweep may stand in for the sums)
        size_t want = 0;
        for (const SumJob& sj : SG->h_sum) want += sj.dst_ws ? 0 : 1;
        if (split_found != want) SG = nullptr;
    }
    n.upd_sum_group = nullptr;
    Net::UpdTab& u = n.upd;
    CK(u.upload(jobs, bj, bs));
    u.k_ps = params_s[0]; u.k_pt = params_t[0]; u.k_g = grads[0]; u.k_m = h_m[0]; u.k_ws = wpack_s_; u.k_wt = wpack_t_;
    u.kind = kind; u.ngroups = ngroups;
    n.upd_sum_group = SG;
    return UDAPOSE_OK;
}
int net_bind_update(void* hs, void* ht, void* const* params_s, void* const* grads, void* const* h_m, void* const* h_v, void* const* params_t,
                    void* wpack_s_, void* wpack_t_) {
    return net_bind_update_groups(hs, ht, 0, params_s, grads, h_m, h_v, params_t, wpack_s_, wpack_t_, nullptr);
}

namespace {
// lr / step / gscale: the host's values, read only where states[0] is NULL (one Adam group without device state)
// ema_dev: NULL, or {alpha, 1 - alpha} in device memory, read by the sweep in place of alpha / oma (the udapose_net_fused_update*_dev forms)
int fused_update(void* hs, void* ht, hipStream_t s, int kind, void* const* params_s, void* const* grads, void* const* h_m, void* const* params_t,
                 void* wpack_s_, void* wpack_t_, float lr, float beta1, float beta2, float eps, int nesterov, int step, float gscale, int ngroups,
                 float* const* states, const float* wds, float alpha, float oma, int do_adam, long long grad2_delta, const float* ema_dev) {
    Net& n = *(Net*)hs;
    const Net& nt = *(const Net*)ht;
    DbgSyncScope dbg(n.policy.debug_sync);
    const Net::UpdTab& u = n.upd;
    if (!u.jobs.d || u.k_ps != params_s[0] || u.k_pt != params_t[0] || u.k_g != grads[0] || u.k_m != h_m[0] || u.k_ws != wpack_s_ || u.k_wt != wpack_t_ ||
        u.kind != kind || u.ngroups != ngroups)
        return UDAPOSE_ERR_NOT_PREPARED;
    // split sums a pair call left to this sweep: it must be the sweep of exactly those two gradient buffers
    const Net::Deferred d = n.deferred;
    if (d.G && (d.G != n.upd_sum_group || d.gA != (char*)grads[0] || grad2_delta != (long long)(d.gB - d.gA))) return UDAPOSE_ERR_NOT_PREPARED;
    n.deferred = Net::Deferred{};
    CK(opt_tail(s, u.jobs.d, u.blk_job.d, u.blk_sub.d, u.nblocks(), kind, lr, beta1, beta2, eps, nesterov, step, gscale, ngroups, states, wds, alpha, oma, do_adam,
                grad2_delta, 1, d.G ? d.wsA : nullptr, d.G ? d.wsB : nullptr, ema_dev));
    // the two packs that are not a cast or a per-tap transpose of a whole tensor: the stem's 3 -> 8 channel gather (both
    // networks) and the head's zero-padded dgrad pack (student)
    if (n.strict)   // 'strict' student: its split forward packs (stem included) from the updated weights, one pack launch (net_bind's table)
        CK(net_pack_weights(hs, s, (const void* const*)params_s, wpack_s_, 0));
    else
        CK(pack_conv(s, n, n.stem, (const void* const*)params_s, (char*)wpack_s_));
    if (nt.f32 != 2) CK(pack_conv(s, nt, nt.stem, (const void* const*)params_t, (char*)wpack_t_));
    CK(pw_pack_strided(s, (const float*)params_s[n.head.w_idx], (elem_t*)((char*)wpack_s_ + n.head.wb_off), 256, 1, 1, 1, 64, n.K, 1, 0, 0, 256));
    return UDAPOSE_OK;
}
}  // namespace

int net_fused_update(void* hs, void* ht, hipStream_t s, void* const* params_s, void* const* grads, void* const* h_m, void* const* params_t,
                     void* wpack_s_, void* wpack_t_, float lr, float beta1, float beta2, float eps, float wd, int step, float gscale,
                     float* dev_state, float alpha, float oma, int do_adam, long long grad2_delta, const float* ema_dev) {
    return fused_update(hs, ht, s, 0, params_s, grads, h_m, params_t, wpack_s_, wpack_t_, lr, beta1, beta2, eps, 0, step, gscale, 1, &dev_state, &wd, alpha,
                        oma, do_adam, grad2_delta, ema_dev);
}
// kind 0: Adam (beta1, beta2, eps); kind 1: SGD (beta1 = momentum, nesterov).  Every group's device state is required: lr, grad_scale, the counter
// and the found-inf mark are read from it.
int net_fused_update_groups(void* hs, void* ht, hipStream_t s, int kind, void* const* params_s, void* const* grads, void* const* h_m,
                            void* const* params_t, void* wpack_s_, void* wpack_t_, float beta1, float beta2, float eps, int nesterov, int ngroups,
                            float* const* states, const float* wds, float alpha, float oma, int do_opt, long long grad2_delta, const float* ema_dev) {
    if (ngroups < 1 || ngroups > TAIL_GROUPS || !states || !wds) return UDAPOSE_ERR_ARG;
    for (int g = 0; g < ngroups; ++g)
        if (!states[g]) return UDAPOSE_ERR_ARG;
    return fused_update(hs, ht, s, kind, params_s, grads, h_m, params_t, wpack_s_, wpack_t_, 0.f, beta1, beta2, eps, nesterov, 0, 1.f, ngroups, states, wds,
                        alpha, oma, do_opt, grad2_delta, ema_dev);
}
