"""GramCoralLoss (csrc/coral.hip) on the MI355X against tests/helpers/coral_fp64.py.

The truth is fp64: the reference's D x D expression under torch's autograd (`direct`) where D <= 4096 after down-sampling, the Gram form with
its closed-form gradients (`gram`; equal to `direct` to 1e-12, tests/test_coral_cpu.py) above that.  Error measure: the loss relative to the
truth; a gradient as max|delta| / max|gradient|.  The bar is not a constant: on the same inputs the two restatements are evaluated in torch
fp32 on the CPU (`direct` only where its D x D matrices fit, D <= 4096), the larger of their errors is e32, and the device must be within
4 x e32 - the margin of 4 is for a different summation order."""
import functools

import pytest
import torch

from helpers import coral_fp64 as C64

pytestmark = pytest.mark.gpu

EPS = float(torch.finfo(torch.float32).eps)
SHAPES = [(2, 1, 2, 2, 1), (3, 2, 4, 6, 2), (4, 3, 8, 8, 1), (5, 2, 9, 7, 3), (4, 2, 8, 12, 4), (3, 2, 5, 7, 2), (8, 3, 16, 16, 2),
          (2, 3, 5, 7, 1),          # D = 105: less than one 64-column tile pair, a ragged last tile
          (33, 1, 8, 8, 1),         # 66 rows padded to 96
          (64, 2, 8, 8, 1),         # the row limit: 128 rows
          (4, 16, 64, 64, 4),
          (32, 16, 64, 64, 1)]      # the full 256-work-group grid
DIRECT_MAX_D = 4096


def _crit(d):
    from uda_poseestimation_amd.lib.models.loss import GramCoralLoss
    return GramCoralLoss(d)


def _errs(got, want):
    """(loss relative error, dsrc error, dtgt error) of a (loss, dsrc, dtgt) triple against the truth"""
    l, gs, gt = [x.detach().double().cpu() for x in got]
    wl, ws, wt = want
    return (abs(float(l) - float(wl)) / abs(float(wl)), float((gs - ws).abs().max()) / float(ws.abs().max()),
            float((gt - wt).abs().max()) / float(wt.abs().max()))


def _yardstick(src, tgt, d, want):
    """e32 per quantity: the larger error of the fp32 restatements on these inputs"""
    s32, t32 = src.float(), tgt.float()
    Dd = src.shape[1] * (src.shape[2] // d) * (src.shape[3] // d)
    e = _errs(C64.gram(s32, t32, d), want)
    if Dd <= DIRECT_MAX_D:
        e = tuple(max(a, b) for a, b in zip(e, _errs(C64.direct_with_grads(s32, t32, d), want)))
    return e


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs (fp32-representable, so that the device and the fp64 truth see the same numbers), the truth, e32: computed once per shape"""
    N, K, H, W, d = shape
    src, tgt = [x.float().double() for x in C64.heatmaps(N, K, H, W, seed=1000 + sum(shape))]
    Dd = K * (H // d) * (W // d)
    want = C64.direct_with_grads(src, tgt, d) if Dd <= DIRECT_MAX_D else C64.gram(src, tgt, d)
    return src, tgt, want, _yardstick(src, tgt, d, want)


def _device(src, tgt, d, scale=None):
    s = src.float().cuda().requires_grad_(True)
    t = tgt.float().cuda().requires_grad_(True)
    loss = _crit(d)(s, t)
    gs, gt = torch.autograd.grad(loss if scale is None else loss * scale, (s, t))
    return loss.detach(), gs, gt


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_both_gradients_against_fp64(shape):
    src, tgt, want, e32 = _case(shape)
    got = _device(src, tgt, shape[4])
    torch.cuda.synchronize()
    err = _errs(got, want)
    print(f"coral {shape}: loss {float(got[0]):.9e} (fp64 {float(want[0]):.9e})  device err loss/dsrc/dtgt {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}  "
          f"e32 {e32[0]:.2e} {e32[1]:.2e} {e32[2]:.2e}")
    assert got[0].dtype == torch.float32 and got[1].shape == src.shape and got[2].shape == tgt.shape
    assert all(torch.isfinite(g).all() for g in got)
    for name, e, y in zip(("loss", "dsrc", "dtgt"), err, e32):
        assert e <= 4.0 * y, f"{name}: device error {e:.3e} above 4 x e32 = {4.0 * y:.3e}"


def test_ill_conditioned_pair_is_no_worse_than_fp32_gram_arithmetic():
    """tgt = src + 1e-3 randn: Gss^2 + Gtt^2 - 2 Gst^2 cancels.  Recorded on the CPU at (8,4,16,16): fp32 Gram arithmetic 7.6e-4 relative, the
    D x D form 2e-8.  The device's Gram entries are fp32 sums, its centring and the three-term sum fp64."""
    N, K, H, W = 8, 4, 16, 16
    src, _ = C64.heatmaps(N, K, H, W, seed=77)
    src = src.float().double()
    tgt = (src + 1e-3 * torch.randn(N, K, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(78))).float().double()
    want = C64.direct_with_grads(src, tgt, 1)
    e_gram = _errs(C64.gram(src.float(), tgt.float(), 1), want)
    e_dir = _errs(C64.direct_with_grads(src.float(), tgt.float(), 1), want)
    got = _device(src, tgt, 1)
    torch.cuda.synchronize()
    err = _errs(got, want)
    print(f"ill-conditioned (8,4,16,16): loss {float(got[0]):.9e} (fp64 {float(want[0]):.9e})  device err loss/dsrc/dtgt {err[0]:.2e} {err[1]:.2e} "
          f"{err[2]:.2e}  fp32 gram {e_gram[0]:.2e} {e_gram[1]:.2e} {e_gram[2]:.2e}  fp32 direct {e_dir[0]:.2e} {e_dir[1]:.2e} {e_dir[2]:.2e}")
    for name, e, y in zip(("loss", "dsrc", "dtgt"), err, e_gram):
        assert e <= 4.0 * y, f"{name}: device error {e:.3e} above 4 x the fp32 Gram form's {y:.3e}"


def test_the_same_tensor_twice_gives_exactly_zero_and_zero_gradients():
    """S == 0: the coefficients are zero, so both gradients are (torch's autograd of the reference's expression gives NaN: d sqrt at 0)"""
    for shape in ((4, 3, 8, 8, 1), (5, 2, 9, 7, 3), (33, 1, 8, 8, 1), (8, 3, 16, 16, 2)):
        N, K, H, W, d = shape
        x = C64.heatmaps(N, K, H, W, seed=5)[0].float().cuda().requires_grad_(True)
        loss = _crit(d)(x, x)
        (g,) = torch.autograd.grad(loss, x)           # (the sum of the two inputs' gradients)
        s, t = x.detach().clone().requires_grad_(True), x.detach().clone().requires_grad_(True)
        l2 = _crit(d)(s, t)
        gs, gt = torch.autograd.grad(l2, (s, t))
        torch.cuda.synchronize()
        assert float(loss) == 0.0 and float(l2) == 0.0, shape
        for t_ in (g, gs, gt):
            assert torch.equal(t_, torch.zeros_like(t_)), shape


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_two_calls_on_the_same_inputs_agree_to_the_bit():
    for shape in ((8, 3, 16, 16, 2), (33, 1, 8, 8, 1), (4, 16, 64, 64, 4)):
        src, tgt, _, _ = _case(shape)
        a, b = _device(src, tgt, shape[4]), _device(src, tgt, shape[4])
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(_bits(x), _bits(y)), shape


def test_forward_and_backward_replayed_from_a_graph_equal_eager_to_the_bit():
    N, K, H, W, d = 8, 4, 32, 32, 2
    crit = _crit(d)
    first = [x.float().cuda() for x in C64.heatmaps(N, K, H, W, seed=30)]
    s, t = first[0].clone().requires_grad_(True), first[1].clone().requires_grad_(True)
    scale = torch.tensor(3.0, device="cuda")

    def run(a, b):
        loss = crit(a, b)
        ga, gb = torch.autograd.grad(loss * scale, (a, b))
        return [loss, ga, gb]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(s, t)
        run(s, t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(s, t)
    for i in range(3):
        fresh = [x.float().cuda() for x in C64.heatmaps(N, K, H, W, seed=31 + i)]
        with torch.no_grad():
            s.copy_(fresh[0])
            t.copy_(fresh[1])
        graph.replay()
        eager = run(fresh[0].clone().requires_grad_(True), fresh[1].clone().requires_grad_(True))
        torch.cuda.synchronize()
        for j, (c, e) in enumerate(zip(captured, eager)):
            assert torch.equal(_bits(c), _bits(e)), (i, j)
        assert float(eager[0]) > 0 and float(eager[1].abs().max()) > 0


def test_the_abi_refuses_what_it_cannot_run_and_the_class_raises():
    from uda_poseestimation_amd._hip import lib, ptr, stream
    L = lib()
    N, K, H, W = 2, 1, 4, 4
    src, tgt = [x.float().cuda() for x in C64.heatmaps(N, K, H, W, seed=1)]
    assert L.udapose_coral_ws_bytes(N, K, H, W, 1) > 0
    ws = torch.empty(L.udapose_coral_ws_bytes(N, K, H, W, 1) // 8, dtype=torch.float64, device="cuda")
    coef = torch.zeros(32 * 32, device="cuda")
    loss = torch.zeros((), device="cuda")
    ds, dt = torch.empty_like(src), torch.empty_like(tgt)
    fwd = [ptr(src), ptr(tgt), N, K, H, W, 1, ptr(ws), ptr(coef), ptr(loss)]
    bwd = [ptr(src), ptr(tgt), ptr(coef), None, N, K, H, W, 1, ptr(ds), ptr(dt)]
    assert L.udapose_coral_fwd(stream(), *fwd) == 0 and L.udapose_coral_bwd(stream(), *bwd) == 0
    torch.cuda.synchronize()

    def changed(args, i, v):
        a = list(args)
        a[i] = v
        return a

    for i in (0, 1, 7, 8, 9):           # null src, tgt, ws, coef, loss
        assert L.udapose_coral_fwd(stream(), *changed(fwd, i, None)) == -1, i
    for i in (0, 1, 2, 9, 10):          # null src, tgt, coef, dsrc, dtgt (gscale may be null)
        assert L.udapose_coral_bwd(stream(), *changed(bwd, i, None)) == -1, i
    for i_f, i_b, v in ((2, 4, 1), (2, 4, 65), (2, 4, 0), (6, 8, 0), (6, 8, -2), (6, 8, 5)):     # N = 1, 65, 0; down = 0, -2; down 5 of a 4x4 map
        assert L.udapose_coral_fwd(stream(), *changed(fwd, i_f, v)) == -1, (i_f, v)
        assert L.udapose_coral_bwd(stream(), *changed(bwd, i_b, v)) == -1, (i_b, v)
    for args in ((1, K, H, W, 1), (65, K, H, W, 1), (N, K, H, W, 0), (N, K, H, W, 5), (N, K, 8, 3, 4)):
        assert L.udapose_coral_ws_bytes(*args) == -1, args
    torch.cuda.synchronize()
    crit = _crit(1)
    for n in (1, 65):
        with pytest.raises(ValueError):
            crit(torch.zeros(n, 1, 4, 4, device="cuda"), torch.zeros(n, 1, 4, 4, device="cuda"))
    with pytest.raises(ValueError):
        crit(torch.zeros(4, 1, 4, 4, device="cuda"), torch.zeros(4, 2, 4, 4, device="cuda"))
    with pytest.raises(ValueError):
        crit(torch.zeros(4, 1, 4, 4, device="cuda"), torch.zeros(3, 1, 4, 4, device="cuda"))


@pytest.mark.parametrize("shape", [(3, 2, 5, 7, 2), (4, 2, 8, 12, 2), (5, 2, 9, 7, 3), (4, 2, 8, 12, 4), (3, 2, 9, 10, 4)], ids=lambda s: "x".join(map(str, s)))
def test_the_backward_writes_every_pixel_of_nan_filled_buffers(shape):
    """The gradient buffers are never cleared beforehand: off the down-sampling footprints (and in the remainder rows / columns) the kernel
    writes explicit zeros."""
    from uda_poseestimation_amd._hip import lib, ptr, stream
    L = lib()
    N, K, H, W, d = shape
    s64, t64 = [x.float().double() for x in C64.heatmaps(N, K, H, W, seed=200 + sum(shape))]
    src, tgt = s64.float().cuda(), t64.float().cuda()
    mp = (2 * N + 31) // 32 * 32
    ws = torch.empty(L.udapose_coral_ws_bytes(N, K, H, W, d) // 8, dtype=torch.float64, device="cuda")
    coef = torch.full((mp * mp,), float("nan"), device="cuda")
    loss = torch.full((), float("nan"), device="cuda")
    ds, dt = torch.full_like(src, float("nan")), torch.full_like(tgt, float("nan"))
    assert L.udapose_coral_fwd(stream(), ptr(src), ptr(tgt), N, K, H, W, d, ptr(ws), ptr(coef), ptr(loss)) == 0
    assert L.udapose_coral_bwd(stream(), ptr(src), ptr(tgt), ptr(coef), None, N, K, H, W, d, ptr(ds), ptr(dt)) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(coef).all() and torch.isfinite(ds).all() and torch.isfinite(dt).all()
    off = C64._up(torch.ones(N, K, H // d, W // d, dtype=torch.float64), (N, K, H, W), d) == 0
    assert bool(off.any()) == (d > 2 or H % d != 0 or W % d != 0)        # (d = 2 on even sizes: every pixel is in a footprint)
    for g in (ds.cpu(), dt.cpu()):
        assert torch.equal(g[off], torch.zeros_like(g[off])) and (g[~off] != 0).all()
    want = C64.gram(s64, t64, d)
    err = _errs((loss, ds, dt), want)
    e32 = _yardstick(s64, t64, d, want)
    print(f"coral nan-filled {shape}: device err {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}  e32 {e32[0]:.2e} {e32[1]:.2e} {e32[2]:.2e}")
    assert all(e <= 4.0 * y for e, y in zip(err, e32))


# ---------------------------------------------------------------------------------------------- the step with the criterion
TK_, TN, TS = 4, 2, 64


def _net(sd=None):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(23)
    m = pr._pose_resnet("t", TK_, pr.Bottleneck_default, [1, 1, 1, 1], False, False)
    if sd is not None:
        m.load_state_dict(sd)
    return m.cuda()


@pytest.fixture(scope="module")
def setup():
    from uda_poseestimation_amd import synthetic
    sd = {k: v.clone() for k, v in _net().cpu().state_dict().items()}
    b = synthetic.mean_teacher_batch(TN, num_keypoints=TK_, image_size=TS, heatmap_size=TS // 4, seed=51)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    return sd, (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])


def _trainer(sd, coral):
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    tr = MeanTeacherTrainer(_net(sd), _net(sd), lr=1e-3, image_size=TS, heatmap_size=TS // 4, precision="bf16")
    if coral:
        tr.coral_criterion, tr.lambda_coral = _crit(2), 0.5
    return tr


def _flat_grad(tr, args):
    from uda_poseestimation_amd import warp
    th_s = warp.recon_thetas(args[5], TN, tr.ratio, "cuda")
    th_t = [warp.recon_thetas(args[6], TN, tr.ratio, "cuda")]
    st = tr._forward_part(args[0], args[1], args[2], args[3], [args[4]], th_s, th_t)
    tr._loss_backward_part(st, None)
    tr._sync_grads()
    tr.student.finish_grads()
    torch.cuda.synchronize()
    return tr.student._flat_grad.clone()


def test_eager_step_with_the_criterion(setup):
    sd, args = setup
    tr = _trainer(sd, True)
    out = tr.train_step(*args)
    torch.cuda.synchronize()
    assert set(out) >= {"loss_all", "loss_s", "loss_c", "loss_coral", "y_s", "y_t_stu"}
    ls, lc, lk, la = (float(out[k]) for k in ("loss_s", "loss_c", "loss_coral", "loss_all"))
    # loss_all = (loss_s + 1.0 * loss_c) + 0.5 * loss_coral in fp32: the two products are exact, each of the two sums rounds by at most
    # half an ulp of a partial sum that is no larger than the total (all terms are >= 0): 2 x 2^-24 = 2^-23 of the total, and second order
    want = ls + tr.lambda_c * lc + 0.5 * lk
    print(f"coral step: loss_s {ls:.6e} loss_c {lc:.6e} loss_coral {lk:.6e} loss_all {la:.9e} (sum {want:.9e})")
    assert lk > 0 and abs(la - want) <= 1.001 * EPS * want
    # loss_coral is the criterion's value on the maps the step returned
    y_s, y_t = out["y_s"].float().cpu().double(), out["y_t_stu"].float().cpu().double()
    assert y_s.shape == (TN, TK_, TS // 4, TS // 4) and y_t.shape == y_s.shape
    truth = C64.direct_with_grads(y_s, y_t, 2)
    e32 = _yardstick(y_s, y_t, 2, truth)[0]
    err = abs(lk - float(truth[0])) / float(truth[0])
    print(f"coral step: loss_coral device err {err:.2e}, e32 {e32:.2e}")
    assert err <= 4.0 * e32
    # the criterion reaches the student's gradient
    g1, g0 = _flat_grad(_trainer(sd, True), args), _flat_grad(_trainer(sd, False), args)
    assert torch.isfinite(g1).all() and torch.isfinite(g0).all() and not torch.equal(g1, g0)
    print(f"coral step: max|grad with - grad without| {float((g1 - g0).abs().max()):.3e}, max|grad| {float(g0.abs().max()):.3e}")


def _state(tr):
    out = [p.detach().clone() for p in list(tr.student.parameters()) + list(tr.teacher.parameters())]
    for p in tr.student.parameters():
        st = tr.stu_optimizer.state.get(p)
        if st:
            out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    return out


def test_three_captured_steps_with_the_criterion_equal_three_eager_steps_to_the_bit(setup):
    from uda_poseestimation_amd.engine import GraphedTrainStep
    sd, args = setup
    tr_g, tr_e = _trainer(sd, True), _trainer(sd, True)
    gs = GraphedTrainStep(tr_g, *args, warmup=1)          # (the warm-up step is a real step: the twin takes it eagerly)
    tr_e.train_step(*args)
    for _ in range(3):
        og = gs.step(*args)
        oe = tr_e.train_step(*args)
        torch.cuda.synchronize()
        for k in ("loss_all", "loss_s", "loss_c", "loss_coral"):
            assert torch.equal(_bits(og[k].float().reshape(1)), _bits(oe[k].float().reshape(1))), k
    sg, se = _state(tr_g), _state(tr_e)
    assert len(sg) == len(se)
    for i, (a, b) in enumerate(zip(sg, se)):
        assert torch.equal(a, b), f"tensor {i} differs between the captured and the eager step"
    name0 = next(n for n, _ in tr_g.student.named_parameters())
    assert not torch.equal(sg[0], sd[name0].cuda())
    # the deferred read-back carries the term, after the existing entries
    gs.step_async(*args)
    m = gs.flush_metrics()
    assert m["loss_coral"] == float(gs.out["loss_coral"]) and m["loss_c"] == float(gs.out["loss_c"]) and "loss_ent" not in m
    assert gs._mvec.numel() == 5 + TK_ + 1
    gs.release()


def test_a_trainer_without_the_criterion_returns_the_keys_and_metrics_layout_it_did(setup):
    from uda_poseestimation_amd.engine import GraphedTrainStep
    from uda_poseestimation_amd.lib.models.loss import EntLoss
    sd, args = setup
    out = _trainer(sd, False).train_step(*args)
    assert set(out) == {"loss_all", "loss_s", "loss_c", "y_s", "tea_mask", "y_t_tea_recon", "y_t_stu_recon"}
    tr = _trainer(sd, False)
    gs = GraphedTrainStep(tr, *args, warmup=1)
    gs.step(*args)
    torch.cuda.synchronize()
    assert gs._mvec.numel() == 5 + TK_ and gs._mextra == []
    assert set(gs.out) == {"loss_all", "loss_s", "loss_c", "y_s", "tea_mask", "y_t_tea_recon", "y_t_stu_recon", "acc_s", "acc_avg_cnt"}
    gs.step_async(*args)
    m = gs.flush_metrics()
    assert set(m) == {"loss_all", "loss_s", "loss_c", "acc_s", "cnt_s", "acc_per_keypoint"} and len(m["acc_per_keypoint"]) == TK_
    gs.release()
    # with an entropy criterion and no CORAL criterion: one appended entry, as before
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    tr = MeanTeacherTrainer(_net(sd), _net(sd), lr=1e-3, image_size=TS, heatmap_size=TS // 4, precision="bf16", ent_criterion=EntLoss(), lambda_ent=0.1)
    gs = GraphedTrainStep(tr, *args, warmup=1)
    gs.step_async(*args)
    m = gs.flush_metrics()
    assert gs._mvec.numel() == 5 + TK_ + 1 and gs._mextra == ["loss_ent"] and m["loss_ent"] == float(gs._mvec[5 + TK_])
    gs.release()
