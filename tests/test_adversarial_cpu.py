"""Adversarial views, the host side (no GPU): the float64 restatement the GPU tests measure csrc/perturb.hip against
(tests/helpers/perturb_fp64.py) reproduces closed forms in both modes, and the feature is declared, bound, built, documented and switched
off by default on the trainer."""
import math
import os
import re

import pytest
import torch

from helpers import perturb_fp64 as P64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _x(N=2, C=3, HW=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, C, HW, generator=g, dtype=torch.float64)


def test_l2_one_hot_gradient_moves_one_element_by_eps():
    x = _x()
    g = torch.zeros_like(x)
    g[0, 1, 4], g[1, 2, 7] = 3.0, -0.25
    out, gn = P64.perturb(x, g, 0.5, "l2")
    want = x.clone()
    want[0, 1, 4] += 0.5
    want[1, 2, 7] -= 0.5
    assert torch.equal(out, want) and gn.tolist() == [3.0, 0.25]


def test_l2_gradient_parallel_to_the_offset():
    """g = a * (x - x0), a > 0: d = (1 + step / ||x - x0||) (x - x0), scaled back to length eps where longer."""
    x0 = _x(seed=1)
    off = _x(seed=2)
    x = x0 + off
    r = off.reshape(2, -1).norm(dim=1)
    for eps, step, active in ((100.0, 0.5, False), (0.9 * float(r.min()), 0.5, True)):
        out, _ = P64.perturb(x, 7.0 * off, eps, "l2", x0=x0, step=step)
        length = r + step
        assert bool((length > eps).all()) == active
        scale = torch.where(length > eps, torch.full_like(r, eps), length) / r
        want = x0 + off * scale.reshape(2, 1, 1)
        assert float((out - want).abs().max()) < 1e-13
        got_r = (out - x0).reshape(2, -1).norm(dim=1)
        assert float((got_r - torch.minimum(length, torch.full_like(r, eps))).abs().max()) < 1e-12


def test_l2_projection_inactive_and_active_with_a_general_gradient():
    x0, x, g = _x(seed=3), _x(seed=3) + 0.01 * _x(seed=4), _x(seed=5)
    u = g / g.reshape(2, -1).norm(dim=1).reshape(2, 1, 1)
    d = (x - x0) + 0.2 * u
    out, _ = P64.perturb(x, g, 10.0, "l2", x0=x0, step=0.2)          # inside the ball: no projection
    assert float((out - (x0 + d)).abs().max()) < 1e-14
    out, _ = P64.perturb(x, g, 0.1, "l2", x0=x0, step=0.2)           # outside: on the sphere, same direction
    dn = d.reshape(2, -1).norm(dim=1).reshape(2, 1, 1)
    assert bool((dn > 0.1).all())
    assert float((out - (x0 + d * (0.1 / dn))).abs().max()) < 1e-14
    assert float(((out - x0).reshape(2, -1).norm(dim=1) - 0.1).abs().max()) < 1e-14
    # x0 None and step None: the one-step form
    out, _ = P64.perturb(x, g, 0.3, "l2")
    assert float((out - (x + 0.3 * u)).abs().max()) < 1e-14


def test_linf_closed_forms():
    x = _x(seed=6)
    g = _x(seed=7)
    g[0, 0, 0] = 0.0
    out, _ = P64.perturb(x, g, 0.25, "linf")
    assert torch.equal(out, x + 0.25 * torch.sign(g)) and out[0, 0, 0] == x[0, 0, 0]          # sign(0) = 0
    x0 = x - 0.2 * torch.sign(_x(seed=8))                                                 # offsets of +-0.2
    out, _ = P64.perturb(x, g, 0.25, "linf", x0=x0, step=0.1)
    d = out - x0
    assert float(d.abs().max()) <= 0.25 + 1e-15
    same = torch.sign(g) == torch.sign(x - x0)              # moving further out: 0.2 + 0.1 clipped to 0.25; moving back: 0.2 - 0.1
    assert float((d[same].abs() - 0.25).abs().max()) < 1e-15
    back = (torch.sign(g) == -torch.sign(x - x0))
    assert float((d[back].abs() - 0.1).abs().max()) < 1e-15


def test_clamp_is_per_channel_and_last():
    x = _x(seed=9)
    g = _x(seed=10)
    lo, hi = [-0.1, -0.2, -0.3], [0.1, 0.2, 0.3]
    for norm in ("l2", "linf"):
        free, _ = P64.perturb(x, g, 0.5, norm)
        out, _ = P64.perturb(x, g, 0.5, norm, clamp=(lo, hi))
        for c in range(3):
            assert torch.equal(out[:, c], free[:, c].clamp(lo[c], hi[c]))
        assert bool((free.abs() > 0.3).any())


def test_degenerate_samples_are_left_alone():
    x = _x(N=4, seed=11)
    g = _x(N=4, seed=12)
    g[0, 0, 3], g[1, 2, 1], g[2] = float("nan"), float("inf"), 0.0
    for norm in ("l2", "linf"):
        out, gn = P64.perturb(x, g, 0.5, norm)
        assert torch.equal(out[:3], x[:3]) and gn[:3].tolist() == [0.0, 0.0, 0.0]
        alone, gn1 = P64.perturb(x[3:], g[3:], 0.5, norm)
        assert torch.equal(out[3:], alone) and gn[3] == gn1[0] and math.isclose(float(gn[3]), float(g[3].norm()), rel_tol=1e-15)
        out, _ = P64.perturb(x, g, 0.5, norm, clamp=([-0.1] * 3, [0.1] * 3))
        assert torch.equal(out[:3], x[:3].clamp(-0.1, 0.1))
    out, _ = P64.perturb(x, g, 0.5, "linf", per_sample_rule=False)           # the one-launch form: element by element
    assert out[0, 0, 3] == x[0, 0, 3] and out[1, 2, 1] == x[1, 2, 1] + 0.5 and out[0, 0, 4] != x[0, 0, 4]


def test_feature_is_declared_bound_built_and_documented():
    import ctypes as C
    from uda_poseestimation_amd import _hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "udapose.h")).read(), flags=re.S)
    assert re.search(r"^long long udapose_perturb_ws_bytes\(int N, int C, int HW\);", hdr, flags=re.M)
    assert re.search(r"^int udapose_perturb\(void\* stream, const float\* x, const float\* g, const float\* x0, int N, int C, int HW, int mode, "
                     r"const float\* eps_dev,\s+const float\* step_dev, const float\* lo, const float\* hi, void\* ws, float\* out, float\* gnorm\);",
                     hdr, flags=re.M)
    vp, ci = C.c_void_p, C.c_int
    assert _hip._SIGS["udapose_perturb_ws_bytes"] == (C.c_longlong, [ci, ci, ci])
    assert _hip._SIGS["udapose_perturb"] == (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp])
    csrc = os.path.join(ROOT, "uda_poseestimation_amd", "csrc")
    capi = open(os.path.join(csrc, "capi.hip")).read()
    assert "int udapose_perturb(" in capi and "long long udapose_perturb_ws_bytes(" in capi
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "perturb.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.16" in design and "udapose_perturb" in design and "input_grad_only" in design
    assert "adv_eps" in open(os.path.join(ROOT, "README.md")).read()


def test_ws_query_runs_on_the_host():
    from uda_poseestimation_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "uda_poseestimation_amd", "csrc"), "-j8"], check=True)
    L = _hip.lib()
    assert L.udapose_perturb_ws_bytes(32, 3, 256 * 256) == 2 * 32 * 48 * 4          # 48 work-groups of 4096 elements per sample
    assert L.udapose_perturb_ws_bytes(5, 1, 7) == 2 * 5 * 4
    assert L.udapose_perturb_ws_bytes(1, 3, 1 << 22) == 2 * 64 * 4                  # capped at 64 work-groups per sample
    assert L.udapose_perturb_ws_bytes(0, 3, 8) == -1 and L.udapose_perturb_ws_bytes(1, 0, 8) == -1 and L.udapose_perturb_ws_bytes(1, 3, 0) == -1


def test_trainer_switch_defaults_and_view_arguments():
    """The four attributes exist with the stated defaults (the constructor's parameter list is unchanged: pinned elsewhere), and the
    functional forms refuse what they document."""
    import inspect
    from uda_poseestimation_amd import adversarial
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    src = inspect.getsource(MeanTeacherTrainer.__init__)
    assert 'self.adv_eps, self.adv_norm, self.adv_steps, self.adv_step = None, "l2", 1, None' in src
    assert not {"adv_eps", "adv_norm", "adv_steps", "adv_step"} & set(inspect.signature(MeanTeacherTrainer.__init__).parameters)
    assert adversarial.NORMS == {"l2": 0, "linf": 1} and adversarial.MAX_STEPS == 4
    assert adversarial.default_step(0.5, 1) is None and adversarial.default_step(0.5, 4) == 2.5 * 0.5 / 4
    with pytest.raises(ValueError, match="steps"):
        adversarial.adversarial_view(None, torch.zeros(1, 3, 8, 8), None, 0.1, steps=5)
    with pytest.raises(ValueError, match="norm"):
        adversarial.adversarial_view(None, torch.zeros(1, 3, 8, 8), None, 0.1, norm="l1")
    with pytest.raises(RuntimeError, match="MI355X"):
        adversarial.perturb(torch.zeros(1, 3, 8), torch.zeros(1, 3, 8), 0.1)
    sig = inspect.signature(adversarial.perturb)
    assert list(sig.parameters) == ["x", "grad", "eps", "norm", "x0", "step", "clamp", "out", "want_norm"]
    sig = inspect.signature(adversarial.adversarial_view)
    assert list(sig.parameters) == ["model", "x", "loss_fn", "eps", "norm", "steps", "step", "clamp", "grad_scale"]
