"""Soft-max heat-map losses, the part that needs no GPU: the plain-torch restatement (tests/helpers/softmax_losses_fp64.py, the
oracle of tests/test_gpu_softmax_losses.py) reproduces what the reference's own classes returned (tests/golden/softmax_losses.npz,
made by tests/golden/make_golden_softmax_losses.py), and the public surface exists: the classes under the reference's names,
their refusal of CPU tensors, CoralLoss's refusal, the trainer's keywords."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import softmax_losses_fp64 as R64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_cases(golden_dir):
    """[(prefix, {name: tensor}, {name: recorded result})] of the two map sizes."""
    z = np.load(os.path.join(golden_dir, "softmax_losses.npz"))
    out = []
    for ci in range(len(z["sizes"])):
        pre = f"c{ci}_"
        d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        out.append((pre, d))
    return out


def restated(d, dtype=torch.float64):
    """Every recorded quantity, recomputed by the restatement in `dtype`: {name: tensor}."""
    f = lambda a: torch.from_numpy(d[a]).to(dtype)
    stu, tea, w = f("stu"), f("tea"), f("weight")
    tm, valid = torch.from_numpy(d["tea_mask"]), torch.from_numpy(d["valid"])
    got = {}
    for eps_name, eps, lab in (("eps", 1e-6, "label"), ("eps0", 0.0, "label"), ("eps0pos", 0.0, "label_pos")):
        for red in ("mean", "none"):
            got[f"kl_{eps_name}_{red}_w"] = R64.joints_kl(stu, f(lab), w, red, eps)
            got[f"kl_{eps_name}_{red}"] = R64.joints_kl(stu, f(lab), None, red, eps)
    for red in ("mean", "none"):
        got[f"ent_{red}"] = R64.entropy(stu, -1, red)
        got[f"ent_{red}_some"] = R64.entropy(stu, float(d["thr_some"]), red)
        got[f"ent_{red}_none"] = R64.entropy(stu, float(d["thr_none"]), red)
    for fn, tag in ((R64.cons_softmax, "csm"), (R64.cons_kl, "ckl")):
        got[f"{tag}_plain"] = fn(stu, tea)
        got[f"{tag}_mask"] = fn(stu, tea, tea_mask=tm)
        got[f"{tag}_valid"] = fn(stu, tea, valid_mask=valid)
        got[f"{tag}_both"] = fn(stu, tea, valid_mask=valid, tea_mask=tm)
    return got


def test_golden_inputs_hold_the_cases_the_losses_must_survive(golden_dir):
    for pre, d in golden_cases(golden_dir):
        assert (d["weight"] == 0).any() and (d["weight"] == 1).any()
        assert (d["label"].reshape(15, -1).sum(1) == 0).sum() == 1 and (d["label_pos"].reshape(15, -1).sum(1) > 0).all()
        assert (~d["tea_mask"]).any() and d["tea_mask"].any() and (~d["valid"]).any() and d["valid"].any()
        assert np.abs(d["stu"]).max() > 75 and np.abs(d["tea"]).max() > 75
        # an all-zero label row: finite with epsilon > 0, NaN with epsilon = 0
        assert np.isfinite(d["kl_eps_mean"]) and np.isnan(d["kl_eps0_mean"]) and np.isfinite(d["kl_eps0pos_mean"])
        assert np.isfinite(d["kl_eps_none"]).all() and np.isnan(d["kl_eps0_none"]).sum() == 1
        # the thresholds: one selects some rows, one none (the mean of nothing is NaN)
        assert np.isfinite(d["ent_mean_some"]) and d["ent_mean_some"] < d["ent_mean"] and np.isnan(d["ent_mean_none"])
        assert d["ent_none"].shape == (3,) and d["ent_none_some"].shape == ()
        # logits of magnitude 80 did not overflow anything
        assert all(np.isfinite(d[k]).all() for k in d if k.startswith(("csm_", "ent_mean", "kl_eps_")) and not k.endswith("_none"))
        # what the reference's ConsKLLoss returns when it is actually run: NaN, in every combination
        assert all(np.isnan(d[f"ckl_{n}"]) for n in ("plain", "mask", "valid", "both"))


def test_fp64_restatement_reproduces_every_golden_value_of_the_reference(golden_dir):
    n = 0
    for pre, d in golden_cases(golden_dir):
        got = restated(d)
        for name, v in got.items():
            want = d[name]
            g = v.numpy()
            assert g.shape == want.shape, (pre, name, g.shape, want.shape)
            assert np.array_equal(np.isnan(g), np.isnan(want)), (pre, name, g, want)
            np.testing.assert_allclose(g, want, rtol=1e-6, atol=0, equal_nan=True, err_msg=pre + name)
            n += 1
        assert R64.joints_kl(torch.from_numpy(d["stu"]), torch.from_numpy(d["label"]), None, "sum") is None
    assert n == 2 * 26


def test_log_target_extension_is_the_kl_divergence(golden_dir):
    """ConsKLLoss(log_target=True) has no recorded reference (the reference has no such argument): its restatement is checked against
    torch's own kl_div with log_target=True."""
    for pre, d in golden_cases(golden_dir):
        stu, tea = torch.from_numpy(d["stu"]).double(), torch.from_numpy(d["tea"]).double()
        B, K = stu.shape[:2]
        lp, lt = torch.log_softmax(stu.reshape(B, K, -1), -1), torch.log_softmax(tea.reshape(B, K, -1), -1)
        want = torch.nn.functional.kl_div(lp, lt, reduction="none", log_target=True).mean()
        got = R64.cons_kl(stu, tea, log_target=True)
        assert torch.isfinite(got) and abs(float(got) - float(want)) <= 1e-12 * abs(float(want))


def test_classes_import_under_the_reference_names_and_refuse_cpu_tensors(tmp_path):
    code = f'''
import sys, warnings
sys.path.insert(0, {os.path.join(ROOT, "uda_poseestimation_amd")!r})
import _dropin; _dropin.install()
from lib.models.loss import JointsMSELoss, JointsKLLoss, EntLoss, ConsLoss, ConsSoftmaxLoss, ConsKLLoss, CoralLoss
import uda_poseestimation_amd.lib.models.loss as real
assert JointsKLLoss is real.JointsKLLoss and EntLoss is real.EntLoss and ConsSoftmaxLoss is real.ConsSoftmaxLoss and ConsKLLoss is real.ConsKLLoss
import torch
x, y = torch.randn(2, 3, 4, 4, requires_grad=True), torch.rand(2, 3, 4, 4)
assert JointsKLLoss().reduction == "mean" and JointsKLLoss().epsilon == 0. and JointsKLLoss("none", 1e-6).epsilon == 1e-6
assert EntLoss().reduction == "mean" and ConsKLLoss().log_target is False
calls = [lambda: JointsKLLoss()(x, y, torch.ones(2, 3, 1)), lambda: JointsKLLoss("none", 1e-6)(x, y), lambda: EntLoss()(x),
         lambda: EntLoss("none")(x, 0.5), lambda: ConsSoftmaxLoss()(x, y, tea_mask=torch.ones(2, 3, dtype=torch.bool)),
         lambda: ConsSoftmaxLoss()(x, y, valid_mask=torch.ones(2, 4, 4, dtype=torch.bool)), lambda: ConsKLLoss()(x, y),
         lambda: ConsKLLoss(log_target=True)(x, y)]
for c in calls:
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            c()
    except RuntimeError as e:
        assert "MI355X" in str(e) and "no CPU fallback" in str(e), e
    else:
        raise AssertionError("a CPU tensor was accepted")
assert JointsKLLoss("sum")(x, y) is None and EntLoss("sum")(x) is None
for args in ((1,), (2, None)):
    try:
        CoralLoss(*args)
    except NotImplementedError as e:
        assert "covariance" in str(e)
    else:
        raise AssertionError("CoralLoss was constructed")
print("LOSSES-OK")
'''
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "LOSSES-OK" in r.stdout, r.stdout + r.stderr


def test_trainer_accepts_the_new_criteria_and_keeps_its_defaults():
    import inspect
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    from uda_poseestimation_amd.lib.models.loss import ConsLoss, ConsSoftmaxLoss, EntLoss, JointsKLLoss, JointsMSELoss
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    sig = inspect.signature(MeanTeacherTrainer.__init__).parameters
    assert all(sig[k].default is None for k in ("criterion", "con_criterion", "ent_criterion")) and sig["lambda_ent"].default == 0.0
    net = lambda: pr._pose_resnet("t", 4, pr.Bottleneck_default, [1, 1, 1, 1], False, False)
    tr = MeanTeacherTrainer(net(), net())
    assert type(tr.criterion) is JointsMSELoss and type(tr.con_criterion) is ConsLoss and tr.ent_criterion is None
    kl, cs, en = JointsKLLoss(epsilon=1e-6), ConsSoftmaxLoss(), EntLoss()
    tr = MeanTeacherTrainer(net(), net(), criterion=kl, con_criterion=cs, ent_criterion=en, lambda_ent=0.1)
    assert tr.criterion is kl and tr.con_criterion is cs and tr.ent_criterion is en and tr.lambda_ent == 0.1
