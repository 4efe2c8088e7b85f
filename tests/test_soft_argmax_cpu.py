"""Soft-argmax decode and coordinate losses, the part that needs no GPU: the plain-torch restatement
(tests/helpers/soft_argmax_fp64.py, the oracle of tests/test_gpu_soft_argmax.py) against independent forms - torch.softmax for the
whole map, a brute-force Python loop for the window, the closed-form gradient against autograd - the sub-pixel experiment that motivates
the feature, and the public surface: names, defaults, refusals, the C ABI's declarations, the trainer's unchanged signature."""
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import soft_argmax_fp64 as S64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gaussian_maps(cx, cy, H, W, sigma=2.0, dtype=torch.float64):
    """[B,K,H,W] exp(-((x - cx)^2 + (y - cy)^2) / (2 sigma^2)) for centres [B,K]."""
    y, x = torch.arange(H, dtype=dtype)[:, None], torch.arange(W, dtype=dtype)[None, :]
    return torch.exp(-((x - cx[..., None, None]) ** 2 + (y - cy[..., None, None]) ** 2) / (2 * sigma * sigma))


def peaked_maps(H, W, peaks, seed):
    """One map per (x, y) in `peaks`, [1,len,H,W]: noise in [0, 1) with a bump of height 2 at the peak and a shoulder beside it."""
    g = torch.Generator().manual_seed(seed)
    hm = torch.rand(1, len(peaks), H, W, generator=g, dtype=torch.float64)
    for k, (x, y) in enumerate(peaks):
        hm[0, k, y, x] = 2.0
        hm[0, k, min(y + 1, H - 1), max(x - 1, 0)] += 0.7
    return hm


def border_peaks(H, W):
    return [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2), (W // 2, H // 2), (2, 3)]


def test_whole_map_decode_is_softmax_times_grid():
    g = torch.Generator().manual_seed(1)
    for H, W, beta in ((7, 9, 1.0), (16, 16, 10.0), (12, 5, 3.5)):
        hm = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
        p = torch.softmax(beta * hm.reshape(2, 3, -1), -1).reshape(2, 3, H, W)
        want = torch.stack([(p.sum(2) * torch.arange(W, dtype=torch.float64)).sum(-1), (p.sum(3) * torch.arange(H, dtype=torch.float64)).sum(-1)], -1)
        got, maxv = S64.decode(hm, beta, None)
        assert got.shape == (2, 3, 2) and maxv.shape == (2, 3, 1)
        assert float((got - want).abs().max()) <= 1e-12
        assert torch.equal(maxv.reshape(2, 3), hm.reshape(2, 3, -1).max(-1).values)


@pytest.mark.parametrize("H,W", [(7, 9), (16, 16)])
def test_window_decode_is_the_brute_force_loop(H, W):
    peaks = border_peaks(H, W)
    hm = peaked_maps(H, W, peaks, seed=H)
    for window, beta in ((0, 10.0), (1, 10.0), (3, 30.0), (5, 10.0), (40, 1.0)):
        got, _ = S64.decode(hm, beta, window)
        for k, (px, py) in enumerate(peaks):
            a = hm[0, k].tolist()
            m = max(max(r) for r in a)
            assert a[py][px] == m
            z = sx = sy = 0.0
            for y in range(H):
                for x in range(W):
                    if abs(x - px) <= window and abs(y - py) <= window:
                        e = math.exp(beta * (a[y][x] - m))
                        z, sx, sy = z + e, sx + e * x, sy + e * y
            assert abs(float(got[0, k, 0]) - sx / z) <= 1e-12 and abs(float(got[0, k, 1]) - sy / z) <= 1e-12, (window, k)
        if window == 0:
            assert torch.equal(got[0], torch.tensor(peaks, dtype=torch.float64))


def test_ties_decode_round_the_first_maximum_and_nan_is_the_largest_value():
    hm = torch.zeros(1, 3, 6, 8, dtype=torch.float64)
    hm[0, 0, 1, 2] = hm[0, 0, 4, 6] = 1.0           # two equal maxima: the first in flat order
    hm[0, 1, 5, 7], hm[0, 1, 2, 1], hm[0, 1, 3, 3] = 9.0, float("nan"), float("nan")
    hm[0, 2, 3, 4] = float("inf")
    assert S64.first_argmax(hm).tolist() == [[1 * 8 + 2, 2 * 8 + 1, 3 * 8 + 4]]
    c, m = S64.decode(hm, 10.0, 0)
    assert c[0, 0].tolist() == [2.0, 1.0] and torch.isnan(c[0, 1:]).all() and torch.isnan(m[0, 1]) and torch.isinf(m[0, 2])


def test_autograd_gradient_is_the_closed_form():
    g = torch.Generator().manual_seed(2)
    for H, W, beta, window in ((7, 9, 1.0, None), (16, 16, 10.0, 5), (16, 16, 30.0, 3), (7, 9, 10.0, 0)):
        hm = peaked_maps(H, W, border_peaks(H, W), seed=3).requires_grad_(True)
        up = torch.randn(1, hm.shape[1], 2, generator=g, dtype=torch.float64)
        c, _ = S64.decode(hm, beta, window)
        c.backward(up)
        want = S64.decode_gradient(hm, up, beta, window)
        assert float((hm.grad - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        if window == 0:
            assert not hm.grad.any()


def subpixel_experiment():
    """64x64 Gaussians, sigma = 2, at uniformly random sub-pixel centres at least 8 px from the border; B = 8, K = 16, seed 0."""
    g = torch.Generator().manual_seed(0)
    centres = 8 + (63 - 16) * torch.rand(8, 16, 2, generator=g, dtype=torch.float64)
    return gaussian_maps(centres[..., 0], centres[..., 1], 64, 64), centres


def test_subpixel_experiment_soft_argmax_beats_argmax_by_two_orders():
    hm, centres = subpixel_experiment()
    err = lambda c: float((c - centres).norm(dim=-1).mean())
    soft, hard = err(S64.decode(hm, 10.0, 5)[0]), err(S64.argmax_decode(hm)[0])
    print(f"mean error: soft-argmax(beta=10, window=5) {soft:.4f} px, arg-max {hard:.3f} px")
    assert soft <= 0.01 and hard >= 0.3


def test_losses_are_their_definitions():
    g = torch.Generator().manual_seed(4)
    hm = torch.randn(2, 3, 8, 10, generator=g, dtype=torch.float64)
    xy = torch.rand(2, 3, 2, generator=g, dtype=torch.float64) * 7
    w = torch.tensor([[1.0, 0.0, 0.5], [2.0, 1.0, 0.0]], dtype=torch.float64)
    c, _ = S64.decode(hm, 10.0, 2)
    d = (c - xy) / torch.tensor([10.0, 8.0], dtype=torch.float64)
    assert abs(float(S64.joints_soft_argmax(hm, xy, w[..., None], 10.0, 2, "l1")) - float((d.abs().sum(-1) * w).mean())) <= 1e-15
    assert torch.allclose(S64.joints_soft_argmax(hm, xy, None, 10.0, 2, "l2", "none"), (0.5 * d * d).sum(-1).mean(-1), rtol=1e-14, atol=0)
    # heat-map targets: arg-max coordinates, and a map without a positive maximum counts for nothing
    tgt = torch.rand(2, 3, 8, 10, generator=g, dtype=torch.float64)
    tgt[1, 1] = 0.0
    txy, tmax = S64.argmax_decode(tgt)
    assert txy[1, 1].tolist() == [0.0, 0.0] and float(tmax[1, 1]) == 0.0
    present = (tmax > 0).double().reshape(2, 3)
    assert present.sum() == 5
    assert float(S64.joints_soft_argmax(hm, tgt, w, 10.0, 2)) == float(S64.joints_soft_argmax(hm, txy, w * present, 10.0, 2))
    tm = torch.tensor([[True, False, True], [True, True, False]])
    want = S64.coord_loss(hm, txy, tm.double(), 10.0, 2, "l2")
    assert float(S64.cons_soft_argmax(hm, tgt, tm, 10.0, 2, "l2")) == float(want)
    soft = S64.cons_soft_argmax(hm, tgt, None, 10.0, 2, "l1", "soft")
    assert float(soft) == float(S64.coord_loss(hm, S64.decode(tgt, 10.0, 2)[0], None, 10.0, 2, "l1"))


def test_pck_from_coordinates_is_the_oracles_accuracy():
    from oracle.keypoints_ref import accuracy_ref, get_max_preds_ref
    rng = np.random.RandomState(0)
    out, tgt = rng.rand(5, 4, 12, 12).astype(np.float32), rng.rand(5, 4, 12, 12).astype(np.float32)
    tgt[:, 2] = 0.0
    acc, avg, cnt, pred = accuracy_ref(out, tgt, 2.0)
    acc2, avg2, cnt2, dist = S64.pck(pred, get_max_preds_ref(tgt)[0], 12, 12, 2.0)
    assert np.array_equal(acc, acc2) and avg == avg2 and cnt == cnt2 == 3 and acc[2] == -1 and np.isnan(dist[:, 2]).all()


def test_names_defaults_and_refusals_under_the_drop_in_names(tmp_path):
    code = f'''
import sys
sys.path.insert(0, {os.path.join(ROOT, "uda_poseestimation_amd")!r})
import _dropin; _dropin.install()
from lib.models.loss import JointsSoftArgmaxLoss, ConsSoftArgmaxLoss, JointsMSELoss
from lib.keypoint_detection import soft_argmax, accuracy, accuracy_device, get_max_preds
import uda_poseestimation_amd.lib.models.loss as real
import uda_poseestimation_amd.lib.keypoint_detection as kd
assert JointsSoftArgmaxLoss is real.JointsSoftArgmaxLoss and ConsSoftArgmaxLoss is real.ConsSoftArgmaxLoss and soft_argmax is kd.soft_argmax
import inspect, torch
d = lambda f: {{k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}}
assert d(soft_argmax) == dict(beta=10.0, window=None)
assert d(accuracy) == dict(hm_type="gaussian", thr=0.5, decode="argmax") and d(accuracy_device) == dict(thr=0.5, decode="argmax")
assert d(JointsSoftArgmaxLoss.__init__) == dict(beta=10.0, window=None, norm="l1", reduction="mean")
assert d(ConsSoftArgmaxLoss.__init__) == dict(beta=10.0, window=None, norm="l1", tea_decode="argmax")
assert d(JointsSoftArgmaxLoss.forward) == dict(target_weight=None) and d(ConsSoftArgmaxLoss.forward) == dict(valid_mask=None, tea_mask=None)
j = JointsSoftArgmaxLoss()
assert (j.beta, j.window, j.norm, j.reduction) == (10.0, None, "l1", "mean")
x, y = torch.randn(2, 3, 4, 4, requires_grad=True), torch.rand(2, 3, 4, 4)
calls = [lambda: soft_argmax(x), lambda: soft_argmax(x.detach(), 10.0, 2), lambda: j(x, y, torch.ones(2, 3, 1)), lambda: j(x, torch.zeros(2, 3, 2)),
         lambda: JointsSoftArgmaxLoss(window=1, norm="l2", reduction="none")(x, y), lambda: ConsSoftArgmaxLoss()(x, y),
         lambda: ConsSoftArgmaxLoss(window=1, tea_decode="soft")(x, y, tea_mask=torch.ones(2, 3, dtype=torch.bool)),
         lambda: accuracy(x.detach(), y, decode="soft"), lambda: accuracy_device(x.detach(), y, decode=soft_argmax)]
if not torch.cuda.is_available():
    calls.append(lambda: soft_argmax(x.detach().numpy()))
for i, c in enumerate(calls):
    try:
        c()
    except RuntimeError as e:
        assert "MI355X" in str(e) and "no CPU fallback" in str(e), e
    else:
        raise AssertionError(f"call {{i}}: a CPU tensor was accepted")
try:
    ConsSoftArgmaxLoss()(x, y, valid_mask=torch.ones(2, 4, 4, dtype=torch.bool))
except ValueError as e:
    assert "valid_mask" in str(e)
else:
    raise AssertionError("valid_mask was accepted")
for bad in (lambda: soft_argmax(x, beta=0.0), lambda: soft_argmax(x, beta=-1.0), lambda: soft_argmax(x, beta=float("inf")),
            lambda: soft_argmax(x, beta=float("nan")), lambda: soft_argmax(x, window=-2), lambda: JointsSoftArgmaxLoss(beta=0.0),
            lambda: JointsSoftArgmaxLoss(norm="l3"), lambda: ConsSoftArgmaxLoss(tea_decode="hard")):
    try:
        bad()
    except ValueError:
        pass
    else:
        raise AssertionError("a bad argument was accepted")
assert JointsSoftArgmaxLoss(reduction="sum")(x, y) is None
print("SOFT-ARGMAX-OK")
'''
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SOFT-ARGMAX-OK" in r.stdout, r.stdout + r.stderr


def test_the_source_is_built_and_the_exports_are_documented():
    """(The four exports' prototypes and ctypes rows:
    test_host_cpu.py::test_ctypes_signatures_and_policy_fields_match_the_header.)"""
    assert "softargmax.hip" in open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "Makefile")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`udapose_{n}`" in doc for n in ("soft_argmax_fwd", "soft_argmax_bwd", "coord_loss_fwd", "coord_loss_bwd"))


def test_the_trainer_and_validate_take_the_feature_without_a_new_trainer_parameter():
    from uda_poseestimation_amd.engine import MeanTeacherTrainer, validate
    from uda_poseestimation_amd.lib.models.loss import ConsLoss, ConsSoftArgmaxLoss, JointsMSELoss, JointsSoftArgmaxLoss
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    assert list(inspect.signature(MeanTeacherTrainer.__init__).parameters) == [
        "self", "student", "teacher", "lr", "teacher_alpha", "lambda_c", "mask_ratio", "sigma", "image_size", "heatmap_size", "use_sgd", "style_net",
        "recover", "s2t_freq", "t2s_freq", "s2t_alpha", "t2s_alpha", "rng", "occlude_rate", "occlude_thresh", "occlude_size", "image_px", "precision",
        "loss_scale_init", "loss_scale_interval", "grad_comm", "criterion", "con_criterion", "ent_criterion", "lambda_ent", "params", "warp_mode"]
    ps = inspect.signature(validate).parameters
    assert list(ps) == ["batches", "model", "criterion", "decode"] and ps["decode"].default == "argmax"
    net = lambda: pr._pose_resnet("t", 4, pr.Bottleneck_default, [1, 1, 1, 1], False, False)
    tr = MeanTeacherTrainer(net(), net())
    assert type(tr.criterion) is JointsMSELoss and type(tr.con_criterion) is ConsLoss
    mse, sa, cons = JointsMSELoss(), JointsSoftArgmaxLoss(window=5), ConsSoftArgmaxLoss(window=5)
    crit = lambda y, l, w: mse(y, l, w) + 0.1 * sa(y, l, w)
    tr = MeanTeacherTrainer(net(), net(), criterion=crit, con_criterion=cons)
    assert tr.criterion is crit and tr.con_criterion is cons
    for cls in (JointsSoftArgmaxLoss, ConsSoftArgmaxLoss):
        assert "baked into a captured step" in " ".join(cls.__doc__.split())
