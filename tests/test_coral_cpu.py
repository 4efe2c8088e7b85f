"""CORAL without a GPU: the pixel rule of the down-sampling against F.interpolate, the n x n Gram form and its closed-form gradients against
the reference's D x D expression under fp64 autograd, GramCoralLoss under the reference's module name and its refusal of CPU tensors,
CoralLoss's standing refusal, the trainer's two attributes, the C ABI's declarations."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import coral_fp64 as C64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 1, 2, 2, 1), (3, 2, 4, 6, 2), (4, 3, 8, 8, 1), (5, 2, 9, 7, 3), (4, 2, 8, 12, 4), (3, 2, 5, 7, 2), (8, 3, 16, 16, 2)]


@pytest.mark.parametrize("d", [2, 3, 4])
@pytest.mark.parametrize("hw", [(8, 12), (12, 12), (9, 7), (13, 10), (5, 7), (16, 16)])
def test_down_is_the_bilinear_interpolation_of_the_reference(d, hw):
    H, W = hw
    x = torch.randn(3, 2, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(H * 100 + W * 10 + d))
    want = torch.nn.functional.interpolate(x, scale_factor=1 / d, mode="bilinear")
    got = C64.down(x, d)
    assert got.shape == want.shape == (3, 2, H // d, W // d)
    assert float((got - want).abs().max()) <= 1e-15 * float(x.abs().max())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gram_form_equals_the_reference_expression_and_its_autograd(shape):
    N, K, H, W, d = shape
    src, tgt = C64.heatmaps(N, K, H, W, seed=sum(shape))
    want, ws, wt = C64.direct_with_grads(src, tgt, d)
    got, gs, gt = C64.gram(src, tgt, d)
    assert float(want) > 0
    assert abs(float(got) - float(want)) <= 1e-12 * float(want)
    for g, w in ((gs, ws), (gt, wt)):
        assert g.shape == w.shape and float(w.abs().max()) > 0
        assert float((g - w).abs().max()) <= 1e-12 * float(w.abs().max())


def test_gram_coral_loss_imports_under_the_reference_name_and_refuses_cpu_tensors(tmp_path):
    code = f'''
import sys
sys.path.insert(0, {os.path.join(ROOT, "uda_poseestimation_amd")!r})
import _dropin; _dropin.install()
from lib.models.loss import GramCoralLoss, CoralLoss
import uda_poseestimation_amd.lib.models.loss as real
assert GramCoralLoss is real.GramCoralLoss
import torch
assert GramCoralLoss().coral_downsample == 1 and GramCoralLoss(2).coral_downsample == 2
x, y = torch.randn(4, 3, 8, 8, requires_grad=True), torch.randn(4, 3, 8, 8, requires_grad=True)
try:
    GramCoralLoss(2)(x, y)
except RuntimeError as e:
    assert "MI355X" in str(e) and "no CPU fallback" in str(e), e
else:
    raise AssertionError("a CPU tensor was accepted")
for bad in (0, -1, 1.5):
    try:
        GramCoralLoss(bad)
    except ValueError:
        pass
    else:
        raise AssertionError("coral_downsample %r was accepted" % (bad,))
for args in ((1,), (2, None)):
    try:
        CoralLoss(*args)
    except NotImplementedError as e:
        assert "covariance" in str(e)
    else:
        raise AssertionError("CoralLoss was constructed")
assert "GramCoralLoss" in CoralLoss.__doc__
print("CORAL-OK")
'''
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CORAL-OK" in r.stdout, r.stdout + r.stderr


def test_trainer_carries_a_coral_criterion_with_the_defaults_none_and_zero():
    """The constructor's parameter list is pinned by two earlier tests, so the criterion and its weight are attributes of the trainer."""
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    net = lambda: pr._pose_resnet("t", 4, pr.Bottleneck_default, [1, 1, 1, 1], False, False)
    tr = MeanTeacherTrainer(net(), net())
    assert tr.coral_criterion is None and tr.lambda_coral == 0.0
