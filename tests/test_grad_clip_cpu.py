"""Clipping by global norm without a GPU: the numpy restatement of grad_sumsq_k / grad_clip_k's order (helpers/fp64_gradnorm.emu) meets the
derived bar against the exact reference in the value regimes a - f of helpers/fp64_optim.regime, the coefficient is the host restatement of
the stored norm to the bit, every planted fault fails one of the two in at least one regime, and the new surface (optimizer keywords,
header prototypes, ctypes rows) is what the issue names while the trainer's constructor keeps its parameter list."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from helpers import fp64_gradnorm as gn
from helpers import fp64_optim as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 3, 5, 4095, 4096, 4097, 9001, 515)
ALIGNED = (True,) * 7 + (False,)             # (the last tensor takes the scalar loop, as an unaligned one does)
_CACHE = {}


def _groups(regime, with_g2, two_groups=False):
    """The tensors of SIZES cut from one regime vector (+ a second buffer from the regime's next step), as ref_norm / emu take them."""
    key = (regime, with_g2, two_groups)
    if key not in _CACHE:
        n = sum(SIZES)
        _, g, gs = fo.regime(regime, n, 31)
        g2 = fo.regime(regime, n, 31, step=1)[1] if with_g2 else None
        cut = lambda v: [v[sum(SIZES[:i]):sum(SIZES[:i + 1])].numpy() for i in range(len(SIZES))]
        ts, t2 = cut(g), (cut(g2) if with_g2 else None)
        if two_groups:           # (the second group at four times the first's grad_scale)
            groups = [(ts[:4], t2[:4] if t2 else None, gs), (ts[4:], t2[4:] if t2 else None, gs * 4.0)]
            aligned = [ALIGNED[:4], ALIGNED[4:]]
        else:
            groups, aligned = [(ts, t2, gs)], [ALIGNED]
        _CACHE[key] = (groups, aligned, gn.ref_norm(groups), gn.count(groups))
    return _CACHE[key]


def _max_norms(ref):
    """Half the norm (the clip is active), twice the norm and +inf (it is not)."""
    r = float(ref) if not isinstance(ref, float) else 1.0
    r = r if r > 0 else 1.0
    return (0.5 * r, 2.0 * r, math.inf)


def _passes(regime, with_g2, two_groups, fault=None):
    groups, aligned, ref, n = _groups(regime, with_g2, two_groups)
    for m in _max_norms(ref):
        norm, coef = gn.emu(groups, m, aligned, fault)
        try:
            gn.check_norm(norm, ref, n, f"regime {regime}")
        except AssertionError:
            return False
        if not gn.same_bits(coef, gn.coef_host(norm, m)):
            return False
        if m == math.inf and float(ref) > 0 and float(coef) != 1.0:
            return False
    return True


CASES = [(r, g2, two) for r in fo.REGIMES for g2 in (False, True) for two in (False, True)]


@pytest.mark.parametrize("regime,with_g2,two_groups", CASES)
def test_emulation_meets_the_bar(regime, with_g2, two_groups):
    groups, aligned, ref, n = _groups(regime, with_g2, two_groups)
    assert not isinstance(ref, float), "the regimes hold finite gradients only"
    for m in _max_norms(ref):
        norm, coef = gn.emu(groups, m, aligned)
        meas = gn.check_norm(norm, ref, n, f"regime {regime} g2 {with_g2} groups {1 + two_groups}")
        assert meas <= 20 + n / 2 ** 21, "the derivation's count of double roundings (helpers/fp64_gradnorm) does not hold"
        assert gn.same_bits(coef, gn.coef_host(norm, m))
        if float(ref) > 0:
            assert (float(coef) == 1.0) == (m > float(ref)), (m, float(ref), float(coef))
        if m == math.inf:
            assert float(coef) == 1.0          # measure only: exactly 1.0f


def test_regime_f_does_not_overflow_the_accumulator():
    """Elements that are only just finite in fp32 (+-FLT_MAX, +-3e38 pre-multiplied by 65536): their squares (1e77) are ordinary doubles."""
    groups, aligned, ref, n = _groups("f", False)
    x = np.concatenate(groups[0][0])
    assert (np.abs(x) >= 3e38).sum() >= 20 and np.isfinite(x).all()
    parts = np.concatenate([gn.emu_partials(g) for g in groups[0][0]])
    assert np.isfinite(parts).all() and parts.max() > 1e77
    norm, _ = gn.emu(groups, 1.0, aligned)
    assert math.isfinite(float(norm)) and float(norm) > 1e33           # FLT_MAX / 65536 and up: the unscaled gradient's norm fits fp32
    with np.errstate(all="ignore"):
        assert not np.isfinite(gn.emu(groups, 1.0, aligned, fault="fp32_accumulate")[0])


def test_beyond_fp32_range_is_inf_and_coef_zero():
    g = np.full(8, 3e38, np.float32)
    groups = [([g], None, 1.0)]
    ref = gn.ref_norm(groups)
    norm, coef = gn.emu(groups, 1.0)
    assert float(ref) > gn.FLT_MAX and float(norm) == math.inf and float(coef) == 0.0
    gn.check_norm(norm, ref, 8, "beyond fp32's range")
    # a NaN gradient without a scaler: a NaN coefficient, torch's behaviour with error_if_nonfinite=False
    g[3] = np.nan
    norm, coef = gn.emu([([g], None, 1.0)], 1.0)
    assert math.isnan(float(norm)) and math.isnan(float(coef)) and math.isnan(gn.ref_norm([([g], None, 1.0)]))


@pytest.mark.parametrize("fault", gn.FAULTS)
def test_each_planted_fault_fails_in_some_regime(fault):
    failed = [c for c in CASES if not _passes(*c, fault=fault)]
    assert failed, f"planted fault {fault!r} passes the bar and the coefficient check in every regime"
    if fault in ("tail_skipped", "last_block_dropped", "g2_ignored", "state4_forgotten"):
        assert len(failed) >= 2


def test_surface():
    """Signatures and defaults of the optimizer surface, the header's prototypes and the ctypes rows of the three entry points."""
    from uda_poseestimation_amd import _hip, optim
    for cls in (optim.FusedAdam, optim.FusedSGD):
        ps = inspect.signature(cls.__init__).parameters
        assert list(ps)[-1] == "max_grad_norm" and ps["max_grad_norm"].default is None
        for name in ("grad_norm", "clip_coef", "max_grad_norm", "sync_hyper"):
            assert hasattr(cls, name), name
        assert isinstance(cls.max_grad_norm, property) and cls.max_grad_norm.fset is not None
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "udapose.h")).read(), flags=re.S)
    capi = open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "capi.hip")).read()
    vp, ci, ll = _hip.vp, _hip.ci, _hip.ll
    want = {"udapose_grad_sumsq": (ci, [vp, vp, vp, vp, vp, ci, ll, vp, vp]),
            "udapose_grad_clip": (ci, [vp, vp, vp, vp, ci, vp, vp]),
            "udapose_grad_clip_restore": (ci, [vp, ci, vp, vp])}
    for name, sig in want.items():
        assert _hip._SIGS[name] == sig and name in _hip.EXPORTS
        assert re.search(r"^int " + name + r"\s*\(", hdr, flags=re.M), f"{name} has no prototype in include/udapose.h"
        assert f"int {name}(" in capi
    for macro, val in (("UDAPOSE_CLIP_MAX_NORM", 0), ("UDAPOSE_CLIP_NORM", 1), ("UDAPOSE_CLIP_COEF", 2), ("UDAPOSE_CLIP_SAVED", 4),
                       ("UDAPOSE_CLIP_FLOATS", 12)):
        assert re.search(rf"#define {macro} {val}\b", hdr), macro
    assert (optim.CLIP_MAX_NORM, optim.CLIP_NORM, optim.CLIP_COEF, optim.CLIP_SAVED, optim.CLIP_FLOATS) == (0, 1, 2, 4, 12)
    # the existing check entry point keeps its prototype
    assert _hip._SIGS["udapose_grad_scaler_check2"] == (ci, [vp, vp, vp, vp, vp, ci, vp, ll])


def test_optimizer_attribute_and_state_dict_on_the_host():
    """max_grad_norm: validated, one value in every group and in the defaults, kept by state_dict / load_state_dict; None disables."""
    import torch
    from uda_poseestimation_amd import optim
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    opt = optim.FusedSGD([{"params": [a]}, {"params": [b], "lr": 0.5}], lr=0.1)
    assert opt.max_grad_norm is None and opt.grad_norm() is None and opt.clip_coef() is None
    opt.max_grad_norm = 2
    assert opt.max_grad_norm == 2.0 and [g["max_grad_norm"] for g in opt.param_groups] == [2.0, 2.0] and opt.defaults["max_grad_norm"] == 2.0
    sd = opt.state_dict()
    assert [g["max_grad_norm"] for g in sd["param_groups"]] == [2.0, 2.0]
    fresh = optim.FusedSGD([{"params": [a]}, {"params": [b], "lr": 0.5}], lr=0.1, max_grad_norm=float("inf"))
    assert fresh.max_grad_norm == math.inf
    fresh.load_state_dict(sd)
    assert fresh.max_grad_norm == 2.0
    old = {"state": {}, "param_groups": [{k: v for k, v in g.items() if k != "max_grad_norm"} for g in sd["param_groups"]]}
    fresh.max_grad_norm = 3.0
    fresh.load_state_dict(old)                 # a checkpoint from before the keyword keeps the current setting
    assert fresh.max_grad_norm == 3.0
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            opt.max_grad_norm = bad
    with pytest.raises(ValueError):
        optim.FusedAdam([a], max_grad_norm=-2.0)
    opt.max_grad_norm = None
    assert opt.max_grad_norm is None and opt.grad_norm() is None


def test_trainer_constructor_is_unchanged_and_forwards_the_attribute():
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    assert list(inspect.signature(MeanTeacherTrainer.__init__).parameters) == [
        "self", "student", "teacher", "lr", "teacher_alpha", "lambda_c", "mask_ratio", "sigma", "image_size", "heatmap_size", "use_sgd", "style_net",
        "recover", "s2t_freq", "t2s_freq", "s2t_alpha", "t2s_alpha", "rng", "occlude_rate", "occlude_thresh", "occlude_size", "image_px", "precision",
        "loss_scale_init", "loss_scale_interval", "grad_comm", "criterion", "con_criterion", "ent_criterion", "lambda_ent", "params", "warp_mode"]
    assert isinstance(MeanTeacherTrainer.max_grad_norm, property) and MeanTeacherTrainer.max_grad_norm.fset is not None
    assert "max_grad_norm" in inspect.getsource(GraphedTrainStep._frozen_hyper)
    assert "grad_norm" in inspect.getsource(GraphedTrainStep._capture_metrics)
