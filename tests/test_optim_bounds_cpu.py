"""The optimizer references and their bars (tests/helpers/fp64_optim.py) on the CPU, and the multi-tensor table key.

The references are right: over three steps adam() and sgd(), iterated in float64, equal torch.optim.Adam / torch.optim.SGD run in float64
(rtol 1e-12) for every combination tests/test_gpu_optim_forms.py uses - weight decay, grad_scale, Nesterov, momentum = 0, a restored step
count of 1000; scaler_trajectory() equals torch.amp.GradScaler on the CPU device over that module's flag sequences.

The bars hold and bite: the float32 numpy emulation of each kernel's order of operations passes them in every value regime (a) .. (f) of
the GPU module, and each planted fault fails them in every regime with a non-zero gradient that exercises it:
  eps inside the root, eps divided by the bias correction, bc2 applied to v instead of its root, the bias corrections of step t - 1, beta2
      used for m, weight decay after the moments or decoupled, a skipped element: regimes a, b, c, e, f; grad_scale applied after the
      square: regime f (the scale is 1 elsewhere); Nesterov's gr + mu * b replaced by b, a skipped element: every regime.
  the first SGD step: a zero buffer gives the same number as the gradient (dampening is 0), so the fault planted is "the first step trusts
      the buffer's contents"; the tests pre-fill the buffer, as a skipped fp16 step can leave it.
  EMA with one fused rounding: bit comparison.
What the parameter-only rtol = 2e-6 comparison of tests/test_gpu_hotpath.py accepts and what it does not is measured in
test_what_the_old_parameter_comparison_sees.

The table key: _MultiTensorTable.key_of is pure Python over data_ptr() and numel(), so it runs on CPU tensors."""
import numpy as np
import pytest
import torch

from helpers import fp64_optim as fo

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
N = 4097 + 257

# (weight_decay, grad_scale regime or None, step count restored before the first step, second gradient buffer)
ADAM_COMBOS = [(0.0, False, 0, False), (1e-4, False, 0, False), (0.0, False, 1000, False), (1e-4, True, 1000, False), (1e-4, True, 0, True)]
# (momentum, weight_decay, nesterov, grad_scale)
SGD_COMBOS = [(0.9, 1e-4, True, 1.0), (0.9, 0.0, False, 1.0), (0.0, 0.0, False, 1.0), (0.9, 1e-4, True, 0.5), (0.0, 1e-4, False, 1.0)]


# ---- the references equal torch in float64 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("wd,scaled,t0,two", ADAM_COMBOS)
def test_adam_reference_equals_torch_float64(wd, scaled, t0, two):
    gen = torch.Generator().manual_seed(11)
    gs = 1.0 / 65536 if scaled else 1.0
    p = (torch.randn(N, generator=gen) * 0.05).double()
    m = (torch.randn(N, generator=gen) * 0.01).double() if t0 else torch.zeros(N, dtype=torch.float64)
    v = (torch.rand(N, generator=gen) * 1e-3).double() if t0 else torch.zeros(N, dtype=torch.float64)
    tp = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([tp], lr=fo.f32(LR), betas=(fo.f32(B1), fo.f32(B2)), eps=fo.f32(EPS), weight_decay=fo.f32(wd))
    if t0:
        opt.state[tp] = {"step": torch.tensor(float(t0)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    for step in range(3):
        g = torch.randn(N, generator=gen) * 0.05 / gs
        g2 = torch.randn(N, generator=gen) * 0.05 / gs if two else None
        gsum = g.double() if g2 is None else (g + g2).double()           # (g + g2 in fp32, as axpy leaves it)
        tp.grad = gsum * fo.f32(gs)
        opt.step()
        r = fo.adam(p, g, m, v, LR, B1, B2, EPS, t0 + step + 1, wd, gs, g2, exact_bc=True)
        rr = fo.adam(p, g, m, v, LR, B1, B2, EPS, t0 + step + 1, wd, gs, g2)
        # the fp32-rounded bias corrections of the device state move the step by at most two roundings
        assert bool(((rr["d"][0] - r["d"][0]).abs() <= 2.01 * fo.U * r["d"][0].abs()).all())
        assert torch.equal(rr["m"][0], r["m"][0]) and torch.equal(rr["v"][0], r["v"][0])
        p, m, v = p + r["d"][0], r["m"][0], r["v"][0]
        st = opt.state[tp]
        torch.testing.assert_close(p, tp.detach(), rtol=1e-12, atol=0)
        # (m is a sum that can cancel: 1e-12 of the magnitude of its terms, its absref)
        assert bool(((m - st["exp_avg"]).abs() <= 1e-12 * r["m"][1]).all())
        torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-12, atol=1e-300)
        for name in ("m", "v", "d"):           # (fl(g + g2) may exceed |g| + |g2| by its own rounding)
            assert bool((r[name][1] >= r[name][0].abs() * (1 - 2.0 ** -22)).all()), name
        assert not bool(r["over"].any())


@pytest.mark.parametrize("mu,wd,nesterov,gs", SGD_COMBOS)
def test_sgd_reference_equals_torch_float64(mu, wd, nesterov, gs):
    gen = torch.Generator().manual_seed(12)
    p = (torch.randn(N, generator=gen) * 0.05).double()
    buf = torch.full((N,), 3.0, dtype=torch.float64)          # (the first step must not read it)
    tp = torch.nn.Parameter(p.clone())
    opt = torch.optim.SGD([tp], lr=fo.f32(1e-2), momentum=fo.f32(mu), weight_decay=fo.f32(wd), nesterov=nesterov)
    for step in range(3):
        g = torch.randn(N, generator=gen) * 0.05 / gs
        tp.grad = g.double() * fo.f32(gs)
        opt.step()
        r = fo.sgd(p, g, buf, 1e-2, mu, wd, nesterov, step == 0, gs)
        p, buf = p + r["d"][0], r["b"][0]
        torch.testing.assert_close(p, tp.detach(), rtol=1e-12, atol=0)
        if mu != 0:
            assert bool(((buf - opt.state[tp]["momentum_buffer"]).abs() <= 1e-12 * r["b"][1]).all())
        assert bool((r["d"][1] >= r["d"][0].abs() * (1 - 1e-15)).all()) and bool((r["b"][1] >= r["b"][0].abs() * (1 - 1e-15)).all())


SCALER_FLAGS = ("000000000000", "100100100100", "001000110001", "111111111111")


@pytest.mark.parametrize("flags", SCALER_FLAGS)
def test_scaler_trajectory_equals_torch_gradscaler(flags):
    """torch.amp.GradScaler works on the CPU device in the installed torch (2.10): scale and growth tracker after every update(), the
    optimizer stepping on clean steps only, and the un-scaling factor 1 / scale (seen in how far a gradient of 1 moves the parameter)."""
    sc = torch.amp.GradScaler("cpu", init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.SGD([p], lr=1.0)
    traj = fo.scaler_trajectory(flags, 65536.0, 2.0, 0.5, 3)
    assert len(traj) == 12
    steps, gscale = 0, 1.0 / 65536.0
    for f, (scale, tracker, gs_next, count) in zip(flags, traj):
        sc.scale(torch.zeros(1))
        p.grad = torch.full((3,), float("inf") if f == "1" else 1.0)
        before = float(p.detach()[0])
        sc.step(opt)
        sc.update()
        moved = before - float(p.detach()[0])
        steps += int(moved != 0)
        assert moved == (0.0 if f == "1" else gscale), (flags, moved, gscale)
        assert (sc.get_scale(), sc._get_growth_tracker(), steps) == (scale, tracker, count), (flags, sc.get_scale(), scale)
        assert gs_next == float(np.float32(1.0) / np.float32(scale))
        gscale = gs_next


# ---- the bars hold for a faithful fp32 kernel and bite on a wrong one ------------------------------------------------------------------

def _adam_run(regime, wd, t0, fault, two=False, steps=3, n=N, check=True):
    """Three steps of the fp32 emulation (state carried in fp32, as the device does), each checked against the one-step reference.  Returns
    the worst measured k per output; raises AssertionError where a bar is missed."""
    p, _, gs = fo.regime(regime, n, 5)
    m = np.zeros(n, np.float32)
    v = np.zeros(n, np.float32)
    if t0:
        gen = torch.Generator().manual_seed(3)
        m = (torch.randn(n, generator=gen) * 0.01).numpy() if regime != "d" else m
        v = (torch.rand(n, generator=gen) * 1e-3).numpy() if regime != "d" else v
    p = p.numpy()
    k = fo.K("adam", wd, two)
    worst = {}
    for step in range(steps):
        _, g, _ = fo.regime(regime, n, 5, step)
        g2 = None
        if two:                                            # (a second buffer of half the size; the only-just-finite elements stay in the first)
            g2 = fo.regime(regime, n, 6, step)[1] * 0.5
            g2[g.abs() > 1e38] = 0.0
        pn, mn, vn = fo.emu_adam(p, g, m, v, LR, B1, B2, EPS, t0 + step + 1, wd, gs, g2, fault)
        ref = fo.adam(p, g, m, v, LR, B1, B2, EPS, t0 + step + 1, wd, gs, g2)
        if check:
            out = fo.check_adam(torch.from_numpy(p), torch.from_numpy(pn), torch.from_numpy(mn), torch.from_numpy(vn), ref, k,
                                f"regime {regime} wd {wd} t0 {t0} step {step} fault {fault}")
            for name, (meas, ratio) in out.items():
                worst[name] = max(worst.get(name, 0.0), ratio)
        if regime == "d" and wd == 0 and t0 == 0:          # g = 0 on m = v = 0: the step is exactly 0 (0 / (0 + eps)), never NaN
            assert np.array_equal(pn, p) and not mn.any() and not vn.any()
        p, m, v = pn, mn, vn
    return worst, p


def _sgd_run(regime, mu, wd, nesterov, fault, steps=3, n=N):
    p, _, gs = fo.regime(regime, n, 7)
    p = p.numpy()
    buf = np.full(n, 3.0, np.float32)               # the first step must overwrite it, not read it
    worst = {}
    for step in range(steps):
        _, g, _ = fo.regime(regime, n, 7, step)
        first = step == 0
        pn, bn = fo.emu_sgd(p, g, buf, 1e-2, mu, wd, nesterov, first, gs, None, fault)
        ref = fo.sgd(p, g, buf, 1e-2, mu, wd, nesterov, first, gs)
        out = fo.check_sgd(torch.from_numpy(p), torch.from_numpy(pn), torch.from_numpy(bn), ref, fo.K("sgd", wd, False, nesterov, first),
                           f"regime {regime} mu {mu} wd {wd} nesterov {nesterov} step {step} fault {fault}")
        for name, (meas, ratio) in out.items():
            worst[name] = max(worst.get(name, 0.0), ratio)
        p, buf = pn, bn
    return worst


@pytest.mark.parametrize("regime", fo.REGIMES)
def test_fp32_emulations_pass_the_bars(regime):
    for wd in (0.0, 1e-4):
        for t0 in (0, 1000):
            worst, _ = _adam_run(regime, wd, t0, None, two=(wd != 0 and t0 == 0))
            assert all(r <= 1.0 for r in worst.values()), worst
    for mu, wd, nesterov, _ in SGD_COMBOS:
        worst = _sgd_run(regime, mu, wd, nesterov, None)
        assert all(r <= 1.0 for r in worst.values()), worst


def _caught(run):
    try:
        run()
    except AssertionError:
        return True
    return False


# fault -> the regimes that must catch it (with weight decay 1e-4 where the fault is about weight decay)
NONZERO = ("a", "b", "c", "e", "f")
ADAM_CATCH = {f: NONZERO for f in fo.ADAM_FAULTS}
ADAM_CATCH["gscale_after_square"] = ("f",)                # (grad_scale is 1 elsewhere)


@pytest.mark.parametrize("fault", fo.ADAM_FAULTS)
def test_each_planted_adam_fault_fails_the_bars(fault):
    wd = 1e-4 if fault.startswith("wd_") else 0.0
    t0 = 1 if fault == "bc_of_t_minus_1" else 0                # (at t = 1 the corrections of step 0 are 0: start from the second step)
    for regime in ADAM_CATCH[fault]:
        assert _caught(lambda: _adam_run(regime, wd, t0, fault)), f"{fault} passes the bars in regime {regime}"


@pytest.mark.parametrize("fault", fo.SGD_FAULTS)
def test_each_planted_sgd_fault_fails_the_bars(fault):
    for regime in ("a", "b", "c", "e", "f"):
        assert _caught(lambda: _sgd_run(regime, 0.9, 1e-4, True, fault)), f"{fault} passes the bars in regime {regime}"


def test_what_the_old_parameter_comparison_sees():
    """test_fused_optimizers_match_torch (tests/test_gpu_hotpath.py) restated on the CPU: its shapes, its N(0,1) draws, four default-Adam
    steps, np.allclose(p, p_ref, rtol=2e-6, atol=2e-7) on the parameters only.  Per element that tolerance is 2.2e-6 at |p| = 1 against a
    step of 1e-3: it accepts a step 0.05 % too long in most elements, eps divided by the bias correction in all but a few dozen of 97,000
    and eps inside the root in 19 of 20 (the bias correction 0.03 of the first steps magnifies a misplaced eps; only elements with a small
    |g| show it).  Measured here, and contrary to what one might expect, the comparison as a whole does reject both eps faults at its
    97,000 elements - through those few elements; a tensor of a thousand elements would mostly pass.  What it cannot see at all: the moments
    (never compared), and Adam's weight decay and grad_scale (never run) - every fault in them passes it.  The new bars reject each of
    these faults in every regime that exercises it (the tests above)."""
    gen = torch.Generator().manual_seed(0)
    shapes = [(64, 3, 7, 7), (256,), (128, 64, 3, 3), (5000,), (16, 256, 1, 1)]
    p0 = [torch.randn(s, generator=gen).reshape(-1).numpy() for s in shapes]
    grads = [[torch.randn(s, generator=gen).reshape(-1).numpy() for s in shapes] for _ in range(4)]
    p0, grads = np.concatenate(p0), [np.concatenate(g) for g in grads]
    n = p0.size

    def run(fault, lr=LR, wd=0.0):
        p, m, v = p0, np.zeros(n, np.float32), np.zeros(n, np.float32)
        for step, g in enumerate(grads):
            p, m, v = fo.emu_adam(p, g, m, v, lr, B1, B2, EPS, step + 1, wd, fault=fault)
        return p

    good = run(None)
    rejected = lambda p: int((~np.isclose(p, good, rtol=2e-6, atol=2e-7)).sum())
    r_root, r_bc, r_long = rejected(run("eps_in_sqrt")), rejected(run("eps_over_bc2")), rejected(run(None, LR * 1.0005))
    print(f"old comparison, elements rejected of {n}: eps in the root {r_root}, eps / bc2 {r_bc}, a step 0.05 % too long {r_long}")
    assert 0 < r_bc < n // 1000 and 0 < r_root < n // 10 and r_long < n // 2
    # with the default weight_decay = 0 and grad_scale = 1 the faults in those terms change nothing: the old test cannot see them
    for fault in ("wd_after_moments", "wd_decoupled", "gscale_after_square"):
        assert np.array_equal(run(fault), good), fault


def test_ema_reference_and_the_fused_rounding_fault():
    gen = torch.Generator().manual_seed(2)
    t, s = torch.randn(N, generator=gen), torch.randn(N, generator=gen)
    for alpha in (0.999, 0.9, 0.5, 0.0):
        want = fo.ema(t, s, alpha)
        a, b = torch.tensor(alpha, dtype=torch.float32), torch.tensor(1.0 - alpha, dtype=torch.float32)
        assert fo.bits_differ(want, (t * a) + (s * b)) == 0                 # (torch's CPU fp32 ops round each operation as numpy does)
        # the reference is within 1.5 roundings of float64; with alpha = 0.5 and 0 the products are exact and so is a fused form
        fused = fo.emu_ema(t, s, alpha, "fused")
        if alpha in (0.999, 0.9):
            assert fo.bits_differ(want, fused) > N // 20, alpha
        else:
            assert fo.bits_differ(want, fused) == 0
    # signed zeros, subnormals and the top of the range
    t = torch.tensor([0.0, -0.0, -0.0, 1e-45, -3e-39, 3e38, -3e38, 1e-38], dtype=torch.float32)
    s = torch.tensor([-0.0, -0.0, 0.0, 1e-45, 3e-39, 3e38, -3e38, -1e-38], dtype=torch.float32)
    out = fo.ema(t, s, 0.5)
    assert np.signbit(out[1]) and not np.signbit(out[0]) and not np.signbit(out[2])
    assert np.isfinite(out).all() and out[5] == np.float32(3e38) and out[4] == 0


# ---- the table key -----------------------------------------------------------------------------------------------------------------

def _lists():
    a, b, c = (torch.zeros(n) for n in (5, 7, 3))
    return [a, b, c]


def test_table_key_names_every_tensor_of_every_list():
    from uda_poseestimation_amd.utils import _MultiTensorTable
    key_of = _MultiTensorTable.key_of
    ps, gs = _lists(), _lists()
    base = key_of([ps, gs])
    assert key_of([list(ps), list(gs)]) == base                                    # identical lists
    for which in (0, 1):
        for i in range(3):                                                         # first, middle and last tensor of either list moved
            lists = [list(ps), list(gs)]
            moved = torch.zeros(lists[which][i].numel())
            assert moved.data_ptr() != lists[which][i].data_ptr()
            lists[which][i] = moved
            assert key_of(lists) != base, (which, i)
    # the same length, but one tensor dropped and another added (one parameter lost its gradient while another gained one)
    ps4, gs4 = _lists() + [torch.zeros(4)], _lists() + [torch.zeros(4)]
    k1 = key_of([[ps4[0], ps4[1], ps4[3]], [gs4[0], gs4[1], gs4[3]]])
    k2 = key_of([[ps4[0], ps4[2], ps4[3]], [gs4[0], gs4[2], gs4[3]]])
    assert k1 != k2
    # a tensor of another size at the same address (a view of a larger buffer re-cut)
    big = torch.zeros(16)
    assert key_of([[big[:8]], [big[:8]]]) != key_of([[big[:4]], [big[:4]]])
