"""Adversarial views on the MI355X (uda_poseestimation_amd/adversarial.py, PoseResNet.input_grad_only, MeanTeacherTrainer.adv_eps): a probe
leaves no trace on the module; the view is the ascent direction of the probe loss, against random directions of the same length; projected
steps stay inside the ball; a trainer step with the switch on is, to the bit, the step without it on the view it made - eager and captured."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

K, NB, S = 16, 2, 64
SCALE = 1024.0          # loss scale of the fp16 probes and steps here (fp16 gradients stay in range)
EPS = 0.05 * math.sqrt(3 * S * S)       # RMS 0.05 per element: large against a 16-bit forward's noise (inputs are ~N(0, 1))
DEFAULT_KEYS = {"loss_all", "loss_s", "loss_c", "y_s", "tea_mask", "y_t_tea_recon", "y_t_stu_recon"}


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


def _probe_loss(lab, wt):
    from uda_poseestimation_amd.lib.models.loss import JointsMSELoss
    crit = JointsMSELoss()
    return lambda y: crit(y, lab, wt)


def _run(net, x, lab, wt, merge):
    """One ordinary forward + backward (gradients cleared first): (output, {name: gradient clone})."""
    for p in net.parameters():
        p.grad = None
    net.merge_wgrad = merge
    y = net(x)
    (_probe_loss(lab, wt)(y) * SCALE).backward()
    if merge:
        net.finish_wgrad()
    net.merge_wgrad = False
    torch.cuda.synchronize()
    return y.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}


def _pending(net):
    """The per-step state a backward leaves on the module, as comparable values."""
    gs = net._grad_state
    return (None if gs is None else list(gs), list(net._pending_wg), list(net._pending_lower), net._split_sum_hd, list(net._deferred_bn))


def _state(net):
    return ({n: b.clone() for n, b in net.named_buffers()}, {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()},
            _pending(net))


def _assert_untouched(net, before, what):
    bufs, grads, pending = before
    torch.cuda.synchronize()
    for n, b in net.named_buffers():
        assert torch.equal(b, bufs[n]), f"{what}: buffer {n} changed"
    for n, p in net.named_parameters():
        if grads[n] is None:
            assert p.grad is None, f"{what}: {n}.grad appeared"
        else:
            assert p.grad is not None and torch.equal(p.grad, grads[n]), f"{what}: {n}.grad changed"
    assert _pending(net) == pending and pending[1:] == ([], [], None, []), f"{what}: pending-step state changed"


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_a_probe_leaves_no_trace(tiny_setup, prec, merge):
    """With p.grad = None and with gradients present, adversarial_view (one and three probes) changes no p.grad, no BatchNorm buffer, no
    num_batches_tracked and no pending-step state; and the ordinary forward + backward that follows gives the output and the 62 gradient
    tensors of a module that never ran a probe."""
    from uda_poseestimation_amd import adversarial
    sd, x, lab, wt = tiny_setup
    fresh, net = _tiny(sd), _tiny(sd)
    fresh.precision = net.precision = prec
    gs = SCALE if prec == "fp16" else None
    y0, g0 = _run(fresh, x, lab, wt, merge)
    assert len(g0) == 62
    assert any("num_batches_tracked" in n for n, _ in net.named_buffers())
    net.merge_wgrad = merge
    before = _state(net)
    assert all(v is None for v in before[1].values())
    for steps in (1, 3):
        x_adv, gn = adversarial.adversarial_view(net, x, _probe_loss(lab, wt), EPS, steps=steps, grad_scale=gs)
        _assert_untouched(net, before, f"{prec} steps {steps}, no gradients")
        assert bool((gn > 0).all()) and not torch.equal(x_adv, x) and not x_adv.requires_grad
    net.merge_wgrad = False
    y1, g1 = _run(net, x, lab, wt, merge)
    assert torch.equal(y1, y0) and g1.keys() == g0.keys()
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
    # gradients present: they keep their bits, and the next accumulate-free run is still the fresh module's
    net.merge_wgrad = merge
    before = _state(net)
    assert sum(v is not None for v in before[1].values()) == 62
    for norm in ("l2", "linf"):
        adversarial.adversarial_view(net, x, _probe_loss(lab, wt), EPS if norm == "l2" else 0.05, norm=norm, steps=2, grad_scale=gs)
        _assert_untouched(net, before, f"{prec} {norm}, gradients present")
    net.merge_wgrad = False
    fresh_bufs = {n: b.clone() for n, b in fresh.named_buffers()}
    y2, g2 = _run(net, x, lab, wt, merge)
    y3, g3 = _run(fresh, x, lab, wt, merge)
    assert torch.equal(y2, y3)
    for n in g3:
        assert torch.equal(g2[n], g3[n]), n
    for (n, a), (_, b) in zip(net.named_buffers(), fresh.named_buffers()):
        assert torch.equal(a, b), n          # (two ordinary forwards each: the same running statistics, the same counters)
    assert any(not torch.equal(b, fresh_bufs[n]) for n, b in fresh.named_buffers())


def _loss_at(net, x, lab, wt):
    """The probe loss of a training-mode forward (batch statistics) at x, no gradient kept."""
    with torch.no_grad():
        return float(_probe_loss(lab, wt)(net(x)))


# The float64 CPU oracle (oracle/pose_resnet_ref.PoseResNetRef on these weights, training-mode BatchNorm, the same loss, seed-3 batch, random
# directions from torch.Generator().manual_seed(100 + i), i < 8, normalised per sample) at eps = 0.05 * sqrt(3 * 64 * 64) = 5.5426:
#   loss at x 2.403251e-02; gain along the gradient direction +9.028e-05; gains along the 8 random directions -1.02e-05 ... +1.97e-05:
#   a margin of 4.58x between the gradient direction's gain and the best random direction's (the condition asks for at least 2x).
#   three projected steps (step 2.5 eps / 3): gain +1.870e-04 (l2); linf at eps 0.05: one step +9.92e-05, three steps +1.617e-04.
# The MI355X reproduces these (bf16: gain +1.141e-04, random -8.23e-06 ... +2.17e-05; fp16: +9.710e-05, -1.02e-05 ... +1.95e-05).
# Forward noise measured on an MI355X, |loss(16-bit forward) - loss(fp32-grade f16x2 forward)| at the one-step and the three-step views:
#   bf16 l2 2.63e-07 / 6.41e-07, bf16 linf 8.57e-07 / 1.16e-06, fp16 l2 7.26e-08 / 5.77e-08, fp16 linf 8.20e-08 / 1.36e-07 - the worst is the
#   allowance below (the three-step views measured +3.3e-05 ... +1.1e-04 ABOVE the one-step views).
LOSS_NOISE = 1.16e-6


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_the_view_is_the_ascent_direction(tiny_setup, prec):
    """The probe loss at x_adv exceeds the loss at x and the loss at x + eps * r / ||r|| for each of 8 seeded random r."""
    from uda_poseestimation_amd import adversarial
    sd, x, lab, wt = tiny_setup
    net = _tiny(sd)
    net.precision = prec
    x_adv, gn = adversarial.adversarial_view(net, x, _probe_loss(lab, wt), EPS, grad_scale=SCALE if prec == "fp16" else None)
    dist = (x_adv - x).double().reshape(NB, -1).norm(dim=1)
    assert float((dist - EPS).abs().max()) < 1e-5 * EPS and bool((gn > 0).all())
    l0, la = _loss_at(net, x, lab, wt), _loss_at(net, x_adv, lab, wt)
    rand = []
    for i in range(8):
        r = torch.randn(x.shape, generator=torch.Generator().manual_seed(100 + i), dtype=torch.float64)
        r = (r / r.reshape(NB, -1).norm(dim=1).reshape(NB, 1, 1, 1) * EPS).float().cuda()
        rand.append(_loss_at(net, x + r, lab, wt))
    print(f"ascent {prec}: loss {l0:.6e} -> {la:.6e} (gain {la - l0:+.3e}); random directions' gains " + " ".join(f"{v - l0:+.2e}" for v in rand))
    assert la > l0 and all(la > v for v in rand), (l0, la, rand)


@pytest.mark.parametrize("norm,eps", [("l2", EPS), ("linf", 0.05)])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_projected_steps_stay_inside_the_ball(tiny_setup, prec, norm, eps):
    """steps = 3: the iterate is inside the ball around x, and its loss is not below the one-step view's minus the forward noise."""
    from uda_poseestimation_amd import adversarial
    sd, x, lab, wt = tiny_setup
    net = _tiny(sd)
    net.precision = prec
    gs = SCALE if prec == "fp16" else None
    x1, _ = adversarial.adversarial_view(net, x, _probe_loss(lab, wt), eps, norm=norm, grad_scale=gs)
    x3, _ = adversarial.adversarial_view(net, x, _probe_loss(lab, wt), eps, norm=norm, steps=3, grad_scale=gs)
    d = (x3 - x).double()
    if norm == "l2":
        assert float(d.reshape(NB, -1).norm(dim=1).max()) <= eps * (1 + 1e-5)
    else:
        assert float(d.abs().max()) <= eps * (1 + 2.0 ** -23) + 2.0 ** -23 * float(x.abs().max())
    l1, l3 = _loss_at(net, x1, lab, wt), _loss_at(net, x3, lab, wt)
    net.precision = "f16x2"
    noise = [abs(_loss_at(net, p, lab, wt) - l) for p, l in ((x1, l1), (x3, l3))]
    print(f"projected steps {prec} {norm}: loss one step {l1:.6e}, three steps {l3:.6e}; |16-bit - f16x2| at the two views {noise[0]:.2e} {noise[1]:.2e}")
    assert l3 >= l1 - LOSS_NOISE, (l1, l3)


# ---------------------------------------------------------------------------------------------------------------- the trainer
def _args(seed=6):
    from uda_poseestimation_amd import synthetic
    b = synthetic.mean_teacher_batch(NB, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=seed)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    return [g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"]]


def _trainer(sd, precision, seed=5, **kw):
    import numpy as np
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    stu, tea = _tiny(sd), _tiny(sd)
    tr = MeanTeacherTrainer(stu, tea, lr=1e-3, image_size=S, heatmap_size=S // 4, precision=precision, loss_scale_init=SCALE,
                            rng=np.random.RandomState(seed), **kw)
    return stu, tea, tr


def _snap(stu, tea, tr):
    out = [p.detach().clone() for p in list(stu.parameters()) + list(tea.parameters())]
    out += [b.clone() for b in list(stu.buffers()) + list(tea.buffers())]
    for p in stu.parameters():
        st = tr.stu_optimizer.state.get(p)
        if st:
            out += [v.clone() for _, v in sorted(st.items()) if torch.is_tensor(v)]
    return out


def _scaler(tr):
    g = tr.stu_optimizer.state_dict()["param_groups"][0]
    return g.get("step"), g.get("loss_scale"), g.get("growth_tracker")


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: tensor {i} differs"


@pytest.mark.parametrize("precision,occlusion,norm,steps", [("bf16", False, "l2", 1), ("fp16", False, "l2", 1), ("bf16", True, "l2", 1),
                                                            ("fp16", False, "linf", 2)])
def test_step_with_the_switch_is_the_step_on_its_view(tiny_setup, precision, occlusion, norm, steps):
    """Twins in one state (same weights, one common warm-up step, equally seeded generators).  A steps with adv_eps set (after the device
    occlusion in one case); B steps with adv_eps = None, occlusion off, on x_t_stu = A's x_t_stu_adv.  Losses, heat-maps, mask, every
    parameter and BatchNorm buffer of student and teacher, the optimizer's moments and the loss-scale state agree to the bit."""
    sd = tiny_setup[0]
    args = _args()
    kw = dict(recover=([-2.5, -2.5, -2.5], [2.5, 2.5, 2.5]))
    (stu_a, tea_a, tr_a), (stu_b, tea_b, tr_b) = _trainer(sd, precision, **kw), _trainer(sd, precision, **kw)
    for tr in (tr_a, tr_b):
        out0 = tr.train_step(*args)
        assert set(out0) == DEFAULT_KEYS                 # the default step hands out today's keys
    _same(_snap(stu_a, tea_a, tr_a), _snap(stu_b, tea_b, tr_b), "twins after the warm-up step")
    tr_a.adv_eps, tr_a.adv_norm, tr_a.adv_steps = (EPS if norm == "l2" else 0.05), norm, steps
    if occlusion:
        tr_a.device_occlusion, tr_a.occlude_rate, tr_a.occlude_thresh = True, 1.0, 0.0
    out_a = tr_a.train_step(*args)
    assert set(out_a) == DEFAULT_KEYS | {"x_t_stu_adv", "adv_gnorm"}
    x_adv = out_a["x_t_stu_adv"]
    assert bool((out_a["adv_gnorm"] > 0).all()) and not torch.equal(x_adv, args[3]) and float(x_adv.abs().max()) <= 2.5
    if occlusion:
        assert bool(tr_a.occluded.any())
    args_b = list(args)
    args_b[3] = x_adv.clone()
    out_b = tr_b.train_step(*args_b)
    assert set(out_b) == DEFAULT_KEYS
    torch.cuda.synchronize()
    for k in ("loss_all", "loss_s", "loss_c", "y_s", "tea_mask", "y_t_tea_recon", "y_t_stu_recon"):
        assert torch.equal(out_a[k], out_b[k]), k
    _same(_snap(stu_a, tea_a, tr_a), _snap(stu_b, tea_b, tr_b), f"{precision}: after the step")
    assert _scaler(tr_a) == _scaler(tr_b) and _scaler(tr_a)[0] >= 1, (_scaler(tr_a), _scaler(tr_b))


def test_captured_step_with_the_switch(tiny_setup):
    """GraphedTrainStep on a trainer with adv_eps set against its eager twin over three replays, adv_eps halved on the host between them: the
    same bits throughout, the view follows the new radius; a change of adv_norm, adv_steps or on / off after capture is refused."""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    sd = tiny_setup[0]
    args = _args()
    (stu_g, tea_g, tr_g), (stu_e, tea_e, tr_e) = _trainer(sd, "bf16"), _trainer(sd, "bf16")
    for tr in (tr_g, tr_e):
        tr.adv_eps, tr.adv_steps = EPS, 2
    gs = GraphedTrainStep(tr_g, *args, warmup=1)
    assert gs.one_graph
    tr_e.train_step(*args)
    for it in range(3):
        if it == 1:
            tr_g.adv_eps = tr_e.adv_eps = EPS / 2
        out_g = gs.step(*args)
        out_e = tr_e.train_step(*args)
        torch.cuda.synchronize()
        _same(_snap(stu_g, tea_g, tr_g), _snap(stu_e, tea_e, tr_e), f"replay {it}")
        for k in ("loss_all", "loss_c", "y_s", "x_t_stu_adv", "adv_gnorm"):
            assert torch.equal(out_g[k], out_e[k]), (it, k)
        dist = (out_g["x_t_stu_adv"] - args[3]).double().reshape(NB, -1).norm(dim=1)
        assert float((dist - tr_g.adv_eps).abs().max()) < 1e-5 * EPS, (it, dist)       # (two steps of 1.25 eps: on the sphere)
    for name, bad, good in (("adv_norm", "linf", "l2"), ("adv_steps", 1, 2), ("adv_eps", None, EPS / 2)):
        setattr(tr_g, name, bad)
        with pytest.raises(RuntimeError, match=name):
            gs.step(*args)
        setattr(tr_g, name, good)
    gs.step(*args)
    gs.release()
    # enabling after capture
    _, _, tr_n = _trainer(sd, "bf16")
    gs_n = GraphedTrainStep(tr_n, *args, warmup=1)
    assert set(gs_n.step(*args)) >= DEFAULT_KEYS and "x_t_stu_adv" not in gs_n.out
    tr_n.adv_eps = EPS
    with pytest.raises(RuntimeError, match="adv_eps"):
        gs_n.step(*args)
    gs_n.release()
