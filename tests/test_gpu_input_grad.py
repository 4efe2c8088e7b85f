"""Input gradients through PoseResNet on the MI355X: the stem's data-gradient kernel (csrc/stem_dgrad.hip, udapose_stem_dgrad) per element
against float64 in both builds, its exact and refused cases, and x.grad of the module (udapose_net_input_grad behind the gradient chain) -
unchanged parameter gradients, frozen parameters, merge_wgrad, the adjoint identity with the stem's weight gradient, the fp64 oracle, a
captured step, and the cases that stay refused."""
import ctypes as C
import math
import warnings

import pytest
import torch

from helpers import fp64_conv as fc
from helpers import stem_dgrad_fp64 as S64

pytestmark = pytest.mark.gpu

ELEM = {"bf16": torch.bfloat16, "fp16": torch.float16}
# (N, H, W): one tile smaller than a work-group's 32x32 pixels; one full tile; several tiles per image and images per launch; ragged tiles in both
# directions (20 x 12 quads); a thin strip with W % 4 != 0 (8-byte stores) and a last tile one quad wide
SHAPES = [(1, 8, 8), (1, 32, 32), (2, 64, 96), (3, 40, 24), (2, 10, 130)]
ERR_ARG = -1


def _operands(N, H, W, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    dy = torch.randn(N, H // 2, W // 2, 64, device="cuda", generator=gen).to(dtype)
    w = S64.round_to(torch.randn(64, 3, 7, 7, device="cuda", generator=gen) * 147 ** -0.5, dtype)
    return dy, w


def _guarded(N, H, W, lead):
    """(whole byte buffer filled with 0xFF, its dx view [N, 3, H, W] that starts `lead` bytes in)."""
    nbytes = N * 3 * H * W * 4
    buf = torch.full((lead + nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + nbytes].view(torch.float32).view(N, 3, H, W)


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_kernel_against_float64_per_element(kind, N, H, W):
    """dy and w pre-rounded to the element type (the reference reads the same operands); fp64_conv's bar for 16-bit data gradients.  Then the
    same launch into guarded buffers at 256-, 8- and 4-byte offsets (16-, 8- and 4-byte stores): the same bits, the guards untouched."""
    from uda_poseestimation_amd import ops
    dtype = ELEM[kind]
    dy, w = _operands(N, H, W, dtype, 1000 * H + W)
    ref, absref = S64.stem_dgrad(dy, w)
    got = ops.stem_dgrad(dy, w)
    torch.cuda.synchronize()
    tau, rho = fc.check(got, ref, absref, torch.float32, *fc.BOUNDS[("16bit", "dgrad")], what=f"stem_dgrad {kind} {(N, H, W)}")
    print(f"stem_dgrad {kind} N={N} {H}x{W}: tau {tau:.3g} rho {rho:.3g} (bars {fc.BOUNDS[('16bit', 'dgrad')]})")
    assert torch.equal(ops.stem_dgrad(dy, w), got), "two calls differ"
    for lead in (256, 8, 4):
        buf, dx = _guarded(N, H, W, lead)
        ops.stem_dgrad(dy, w, dx=dx)
        torch.cuda.synchronize()
        assert torch.equal(dx, got), f"offset {lead}: result differs"
        assert bool((buf[:lead] == 0xFF).all()) and bool((buf[lead + dx.numel() * 4:] == 0xFF).all()), f"offset {lead}: guard bytes written"


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_single_element_footprints_are_exact(kind):
    """One non-zero dy element: dx is that value times the rounded filter, placed at (2*oy + ky - 3, 2*ox + kx - 3) and clipped at the border -
    one exact product per output, so bit equality.  Positions: the four corners, an edge, the interior, and both sides of a tile boundary
    (20 x 36 quads: 2 x 3 tiles).  Zero dy gives zeros over a NaN-filled buffer."""
    from uda_poseestimation_amd import ops
    dtype = ELEM[kind]
    N, H, W = 2, 40, 72
    Ho, Wo = H // 2, W // 2
    _, w = _operands(1, 8, 8, dtype, 7)
    spots = [(0, 0, 0, 0), (0, 0, Wo - 1, 63), (1, Ho - 1, 0, 31), (1, Ho - 1, Wo - 1, 32), (0, 0, 7, 5), (1, 9, 6, 40), (0, 15, 15, 17),
             (0, 16, 16, 8), (1, 15, 32, 63)]
    for i, (n, oy, ox, co) in enumerate(spots):
        v = (-1.5, 2.0, 0.75)[i % 3]
        dy = torch.zeros(N, Ho, Wo, 64, device="cuda", dtype=dtype)
        dy[n, oy, ox, co] = v
        want = torch.zeros(N, 3, H, W, device="cuda")
        for ky in range(7):
            for kx in range(7):
                iy, ix = 2 * oy + ky - 3, 2 * ox + kx - 3
                if 0 <= iy < H and 0 <= ix < W:
                    want[n, :, iy, ix] = v * w[co, :, ky, kx]
        dx = torch.full((N, 3, H, W), float("nan"), device="cuda")
        ops.stem_dgrad(dy, w, dx=dx)
        assert torch.equal(dx, want), f"footprint of dy[{n}, {oy}, {ox}, {co}]: {int((dx != want).sum())} elements differ"
    dx = torch.full((N, 3, H, W), float("nan"), device="cuda")
    ops.stem_dgrad(torch.zeros(N, Ho, Wo, 64, device="cuda", dtype=dtype), w, dx=dx)
    assert bool((dx == 0).all())


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_kernel_refuses_bad_arguments_and_writes_nothing(kind):
    from uda_poseestimation_amd import _hip
    L = _hip.lib(kind)
    dy = torch.ones(1, 8, 8, 64, device="cuda", dtype=ELEM[kind])
    w = torch.ones(64, 7, 7, 3, device="cuda")
    dx = torch.full((1, 3, 16, 16), 7.0, device="cuda")
    s, p = _hip.stream(), _hip.ptr
    cases = {"odd H": (p(dy), p(w), 1, 15, 16, p(dx)), "odd W": (p(dy), p(w), 1, 16, 15, p(dx)), "W = 6": (p(dy), p(w), 1, 16, 6, p(dx)),
             "H = 6": (p(dy), p(w), 1, 6, 16, p(dx)), "N = 0": (p(dy), p(w), 0, 16, 16, p(dx)), "null dy": (None, p(w), 1, 16, 16, p(dx)),
             "null w": (p(dy), None, 1, 16, 16, p(dx)), "null dx": (p(dy), p(w), 1, 16, 16, None),
             "dx inside dy": (p(dy), p(w), 1, 16, 16, dy.data_ptr() + 64)}
    for what, a in cases.items():
        assert L.udapose_stem_dgrad(s, *a) == ERR_ARG, what
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all()) and bool((dy == 1).all())
    assert L.udapose_stem_dgrad(s, p(dy), p(w), 1, 16, 16, p(dx)) == 0


# ---------------------------------------------------------------------------------------------------------------- the module
K, NB, S = 16, 2, 64
SCALE = 1024.0          # loss scale of every module run here (fp16 gradients stay in range; x.grad carries it like every p.grad)


def _tiny(sd=None):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(11)
    m = pr._pose_resnet("t", K, pr.Bottleneck_default, [1, 1, 1, 1], False, False)
    if sd is not None:
        m.load_state_dict(sd)
    return m.cuda().train()


@pytest.fixture(scope="module")
def tiny_setup():
    from uda_poseestimation_amd import synthetic
    sd = {k: v.clone() for k, v in _tiny().cpu().state_dict().items()}
    x, lab, wt = (t.cuda() for t in synthetic.keypoint_batch(NB, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=3))
    return sd, x, lab, wt


def _run(net, x, lab, wt, x_grad, merge=False):
    """One forward + backward: (output, {name: gradient clone}, x.grad or None)."""
    from uda_poseestimation_amd.lib.models.loss import JointsMSELoss
    for p in net.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(x_grad)
    net.merge_wgrad = merge
    y = net(xin)
    (JointsMSELoss()(y, lab, wt) * SCALE).backward()
    if merge:
        net.finish_wgrad()
    net.merge_wgrad = False
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    return y.detach().clone(), grads, (None if xin.grad is None else xin.grad.clone())


@pytest.mark.parametrize("prec", ["bf16", "fp16", "strict"])
def test_module_input_gradient_leaves_everything_else_unchanged(tiny_setup, prec):
    """x.grad exists (fp32, x's shape, finite); the output and every parameter gradient are bit for bit those of a run whose input does not
    require grad; with every parameter frozen x.grad has the same bits and no parameter gets a gradient; the same under merge_wgrad."""
    sd, x, lab, wt = tiny_setup
    net = _tiny(sd)
    net.precision = prec
    y0, g0, xg0 = _run(net, x, lab, wt, False)
    assert xg0 is None and len(g0) >= 60
    y1, g1, xg1 = _run(net, x, lab, wt, True)
    assert xg1 is not None, "x.grad is None"
    assert xg1.dtype == torch.float32 and xg1.shape == x.shape and bool(torch.isfinite(xg1).all()) and float(xg1.abs().max()) > 0
    assert torch.equal(y1, y0) and g1.keys() == g0.keys()
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
    y2, g2, xg2 = _run(net, x, lab, wt, True, merge=True)
    assert torch.equal(y2, y0) and torch.equal(xg2, xg1) and g2.keys() == g0.keys()
    for n in g0:
        assert torch.equal(g2[n], g0[n]), f"merge_wgrad: {n}"
    for p in net.parameters():
        p.requires_grad_(False)
    for merge in (False, True):
        y3, g3, xg3 = _run(net, x, lab, wt, True, merge=merge)
        assert torch.equal(y3, y0) and torch.equal(xg3, xg1) and not g3 and all(p.grad is None for p in net.parameters())


# |sum(x_r * x.grad) - sum(W_r * conv1.weight.grad)| / (sum|x_r * x.grad| + sum|W_r * conv1.weight.grad|), measured on an MI355X (the tiny network above,
# N = 2, 64x64): bf16 7.58e-10, fp16 1.60e-9, strict 4.33e-9.  The bar is 4x the worst (the convention of fp64_conv.BOUNDS).  (Far below the
# 1.2e-6 the fp32-accumulation bounds allow: rounding errors of either sign average out over the 24576 terms; and both sums nearly vanish, a
# training-mode BatchNorm's dy being orthogonal to its input - which is why the gap is normalised by the absolute sums.)
ADJOINT_BAR = 1.8e-8


@pytest.mark.parametrize("prec", ["bf16", "fp16", "strict"])
def test_adjoint_identity_with_the_stem_weight_gradient(tiny_setup, prec):
    """The stem convolution has no bias, so with x_r, W_r the operands rounded to the element type, sum(x_r * x.grad) and
    sum(W_r * conv1.weight.grad) are both sum(dy * conv(x_r, W_r)): the data gradient and the weight gradient of one dy, each accumulated in
    fp32 in its own order.  Compared in float64, normalised by the two absolute sums."""
    sd, x, lab, wt = tiny_setup
    net = _tiny(sd)
    net.precision = prec
    dtype = torch.bfloat16 if prec == "bf16" else torch.float16
    _, g, xg = _run(net, x, lab, wt, True)
    xr, wr = S64.round_to(x, dtype).double(), S64.round_to(net.backbone.conv1.weight.detach(), dtype).double()
    a, b = xr * xg.double(), wr * g["backbone.conv1.weight"].double()
    gap = abs(float(a.sum()) - float(b.sum())) / (float(a.abs().sum()) + float(b.abs().sum()))
    print(f"adjoint identity {prec}: sum(x_r * x.grad) {float(a.sum()):.9e}  sum(W_r * dW) {float(b.sum()):.9e}  normalised gap {gap:.3e}")
    assert gap < ADJOINT_BAR, (prec, gap)


# measured on an MI355X against the float64 oracle (trained PoseResNet-101, N = 2, 128x128, JointsMSE), loss scale divided out:
#   fp16    x.grad cosine 0.987851, relative L2 1.561e-01   (conv1.weight.grad: cosine 0.993957, relative L2 1.100e-01)
#   strict  x.grad cosine 0.999791, relative L2 2.044e-02   (conv1.weight.grad: cosine 0.999903, relative L2 1.393e-02)
#   bf16    x.grad cosine 0.921318, relative L2 3.958e-01   (conv1.weight.grad: cosine 0.946122, relative L2 3.306e-01)
# The bars (cosine above, relative L2 below) are twice the measured distance (tests/test_gpu_grad_schedules.py A3).  Whatever was measured, the
# fp16 backward (fp16, strict) also keeps cosine > 0.95, tests/test_gpu_fp16.py's gradient bar; the bf16 backward keeps the bar this network's
# bf16 parameter gradients have in tests/test_gpu_trained.py, cosine > 0.9 (its stem weight gradient itself is at 0.946 in the same run).
ORACLE_BARS = {"fp16": (1 - 2 * (1 - 0.987851), 2 * 1.561e-01, 0.95), "strict": (1 - 2 * (1 - 0.999791), 2 * 2.044e-02, 0.95),
               "bf16": (1 - 2 * (1 - 0.921318), 2 * 3.958e-01, 0.9)}


def test_input_gradient_against_the_fp64_oracle(trained_r101_k16):
    """x.grad of the session's trained PoseResNet-101 on unseen images against float64 autograd of oracle.pose_resnet_ref with the same weights
    (training-mode BatchNorm, JointsMSE): cosine and relative L2, for the fp16-backward precisions the bars hold for and bf16 beside them.
    conv1.weight.grad's figures are printed for comparison only (a weight gradient averages over far more terms)."""
    import uda_poseestimation_amd.lib.models as models
    from oracle.pose_resnet_ref import pose_resnet101_ref
    from uda_poseestimation_amd import synthetic
    from uda_poseestimation_amd.lib.models.loss import JointsMSELoss
    sd = trained_r101_k16[0]
    x, lab, wt = synthetic.keypoint_batch(NB, num_keypoints=16, image_size=128, heatmap_size=32, seed=7)
    ref = pose_resnet101_ref(16).double().train()
    ref.load_state_dict(sd)
    x64 = x.double().requires_grad_(True)
    y64 = ref(x64)
    ((((y64.reshape(NB, 16, -1) - lab.double().reshape(NB, 16, -1)) ** 2) * 0.5) * wt.double().reshape(NB, 16, 1)).mean().backward()
    rx, rw = x64.grad.flatten(), ref.backbone.conv1.weight.grad.flatten()
    net = models.pose_resnet101(num_keypoints=16, pretrained_backbone=False)
    net.load_state_dict(sd)
    net = net.cuda().train()

    def dist(a, r):
        a = a.detach().cpu().double().flatten() / SCALE
        return float(a @ r) / math.sqrt(float(a @ a) * float(r @ r)), float((a - r).norm() / r.norm())

    rows = {}
    for prec in ("bf16", "fp16", "strict"):
        net.precision = prec
        for p in net.parameters():
            p.grad = None
        xin = x.cuda().requires_grad_(True)
        (JointsMSELoss()(net(xin), lab.cuda(), wt.cuda()) * SCALE).backward()
        torch.cuda.synchronize()
        assert xin.grad is not None and bool(torch.isfinite(xin.grad).all())
        rows[prec] = dist(xin.grad, rx) + dist(net.backbone.conv1.weight.grad, rw)
        print(f"x.grad vs fp64 oracle, {prec}: cosine {rows[prec][0]:.6f} relative L2 {rows[prec][1]:.3e}   "
              f"(conv1.weight.grad: cosine {rows[prec][2]:.6f} relative L2 {rows[prec][3]:.3e})")
    for prec, (cos_bar, rel_bar, cos_floor) in ORACLE_BARS.items():
        cos, rel = rows[prec][:2]
        assert cos > max(cos_bar, cos_floor) and rel < rel_bar, (prec, cos, rel)


def test_captured_step_replays_the_input_gradient(tiny_setup):
    """forward + loss + backward with a static input that requires grad, captured: a replay's x.grad is the eager result bit for bit, and after
    the static input is overwritten the replay follows the new input."""
    from uda_poseestimation_amd import synthetic
    from uda_poseestimation_amd.lib.models.loss import JointsMSELoss
    sd, x, lab, wt = tiny_setup
    x2 = synthetic.keypoint_batch(NB, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=4)[0].cuda()
    net = _tiny(sd)
    net.precision = "bf16"
    crit = JointsMSELoss()
    eager = [_run(net, xe, lab, wt, True)[2] for xe in (x, x2)]       # (also builds the plan and binds its tables: nothing allocates under capture)
    assert not torch.equal(eager[0], eager[1])
    xs = x.clone().requires_grad_(True)
    for p in net.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        (crit(net(xs), lab, wt) * SCALE).backward()
    for want, src in ((eager[0], x), (eager[1], x2), (eager[0], x)):
        with torch.no_grad():
            xs.copy_(src)
            xs.grad.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(xs.grad, want)


def test_net_input_grad_refuses_plans_that_keep_no_backward(tiny_setup):
    """udapose_net_input_grad on a forward-only plan (bf16 and f16x2) returns UDAPOSE_ERR_UNSUPPORTED, on null arguments UDAPOSE_ERR_ARG;
    nothing is written."""
    from uda_poseestimation_amd import _hip
    sd, x, lab, wt = tiny_setup
    net = _tiny(sd)
    dx = torch.full_like(x, 3.0)
    for prec in ("bf16", "f16x2"):
        net.precision = prec
        with torch.no_grad():
            net(x)
        hd = net._last_hd
        assert hd.fwd_only and hd.precision == prec
        pa = net._pointers()[0]
        assert hd.L.udapose_net_input_grad(hd.h, _hip.stream(), pa, _hip.ptr(hd.ws), _hip.ptr(dx)) == -3, prec
        assert hd.L.udapose_net_input_grad(hd.h, _hip.stream(), pa, None, _hip.ptr(dx)) == ERR_ARG
        assert hd.L.udapose_net_input_grad(hd.h, _hip.stream(), pa, _hip.ptr(hd.ws), None) == ERR_ARG
        assert hd.L.udapose_net_input_grad(None, _hip.stream(), pa, _hip.ptr(hd.ws), _hip.ptr(dx)) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((dx == 3.0).all())


def test_cases_that_stay_refused(tiny_setup):
    sd, x, lab, wt = tiny_setup
    net = _tiny(sd)
    net.precision = "bf16"
    xin = x.clone().requires_grad_(True)
    net.split_backward = True
    y = net(xin)
    with pytest.raises(RuntimeError, match="split_backward"):
        y.sum().backward()
    net.split_backward = False
    net._drop_pending_step()
    net.precision = "f16x2"
    with pytest.raises(RuntimeError, match="forward-only"):
        net(xin)
    net.precision = "bf16"
    net.eval()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = net(xin)
    assert y.grad_fn is None and not y.requires_grad
    for p in net.parameters():
        p.requires_grad_(False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = net(xin)
    assert y.grad_fn is None and not y.requires_grad
