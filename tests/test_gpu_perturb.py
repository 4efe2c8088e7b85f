"""csrc/perturb.hip (udapose_perturb) on the MI355X, in both builds of the library: per element against the float64 restatement
(tests/helpers/perturb_fp64.py) at sizes that take the 16-byte and the 4-byte path, one and several work-groups per sample, with guard bytes
around every output and the workspace; the exact linf form, degenerate samples, scale invariance, determinism, capture, bad arguments."""
import math

import pytest
import torch

from helpers import perturb_fp64 as P64

pytestmark = pytest.mark.gpu

KINDS = ["bf16", "fp16"]
# (N, C, HW): one partial work-group; two work-groups per sample (18432 = 4.5 chunks of 4096 -> 5 work-groups of 3688); one work-group,
# HW % 4 == 0; D = 7 and HW = 33: the 4-byte path whatever the alignment
SHAPES = [(1, 3, 64), (2, 3, 64 * 96), (3, 3, 40 * 24), (5, 1, 7), (2, 3, 33)]
U = 2.0 ** -24
ERR_ARG = -1


def _blocks(D):
    """(work-groups per sample, elements per work-group, squares a thread adds): perturb_blocks / perturb_chunk of csrc/perturb.hip."""
    B = min(64, max(1, -(-D // 4096)))
    chunk = (-(-D // B) + 3) // 4 * 4
    return B, chunk, -(-chunk // 256) + 3


def _amp(D):
    """A-priori ceiling on how much the summation scheme can amplify one rounding unit in a sample-wide factor (c = step / ||g||, or
    f = eps / ||d||).  The sum of squares is T sequential fp32 fused adds per thread, 6 butterfly levels, 3 adds over the waves, B - 1 adds
    over the partials, all of non-negative terms: relative error <= (T + 9 + B) u to first order, half of it after the (correctly rounded)
    square root, plus one unit each for the root and the division: delta = ((T + 9 + B) / 2 + 2) u.  The projected form chains three such
    factors (c enters d, d enters ||d||, f scales d) and rounds d and the product once each: A = 3 * delta / u + 4."""
    B, _, T = _blocks(D)
    return 3.0 * ((T + 9 + B) / 2.0 + 2.0) + 4.0


# rho = max over elements of |out - ref| / (u * (A |d_ref| + |x - x0| + |ref|)), d_ref = ref - x0 before the clamp: <= 1 a priori (the last two
# terms are the roundings of x - x0 and of the result).  Measured on an MI355X over every l2 case below (both builds give the same bits):
# worst rho 0.957 per element - the rounding of the result itself, half an ulp, reaches u |ref| wherever |ref| lies just above a power of two and
# the displacement is small, so the per-element measure sits at its ceiling by construction - and 0.110 for | ||out - x0||_2 - eps | under the
# same normalisation with norms in place of elements (0.014 at the largest size: roundings of either sign average out over a norm).
# Each bar is twice the worst measured distance, and never above the a-priori ceiling of 1.
RHO_MEASURED, RHO_NORM_MEASURED = 0.957, 0.110
RHO_BAR, RHO_NORM_BAR = min(2.0 * RHO_MEASURED, 1.0), min(2.0 * RHO_NORM_MEASURED, 1.0)


def _guarded(shape, lead):
    """(byte buffer filled with 0xFF, its fp32 view of `shape` that starts `lead` bytes in)."""
    n = 4 * math.prod(shape)
    buf = torch.full((lead + n + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + n].view(torch.float32).view(shape)


def _intact(buf, lead, view):
    return bool((buf[:lead] == 0xFF).all()) and bool((buf[lead + 4 * view.numel():] == 0xFF).all())


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _operands(N, C, HW, seed, offset=0.0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(N, C, HW, device="cuda", generator=gen)
    g = torch.randn(N, C, HW, device="cuda", generator=gen) * 3.0
    x0 = x - offset * torch.randn(N, C, HW, device="cuda", generator=gen) if offset else None
    return x, g, x0


def _launch(kind, x, g, eps, mode, x0=None, step=None, clamp=None, lead=256, want_norm=True, eps_t=None):
    """udapose_perturb on copies of the operands placed `lead` bytes into guarded buffers; out, gnorm and the workspace are guarded on both
    sides and the guards are checked.  -> (out, gnorm or None)."""
    from uda_poseestimation_amd import _hip
    L = _hip.lib(kind)
    N, C, HW = x.shape
    place = lambda t: None if t is None else _guarded(t.shape, lead)[1].copy_(t)
    xs, gs, zs = place(x), place(g), place(x0)
    obuf, out = _guarded(x.shape, lead)
    nbuf, gn = _guarded((N,), 256)
    wbuf, ws = _guarded((L.udapose_perturb_ws_bytes(N, C, HW) // 4,), 256)
    eps_t = torch.tensor(eps, dtype=torch.float32, device="cuda") if eps_t is None else eps_t
    step_t = None if step is None else torch.tensor(step, dtype=torch.float32, device="cuda")
    lo = hi = None
    if clamp is not None:
        lo, hi = (torch.tensor(v, dtype=torch.float32, device="cuda") for v in clamp)
    p = _hip.ptr
    rc = L.udapose_perturb(_hip.stream(), p(xs), p(gs), p(zs), N, C, HW, {"l2": 0, "linf": 1}[mode], p(eps_t), p(step_t), p(lo), p(hi), p(ws), p(out),
                           p(gn) if want_norm else None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _intact(obuf, lead, out), f"guard bytes around out written (offset {lead})"
    assert _intact(wbuf, 256, ws), "guard bytes around the workspace written"
    if want_norm:
        assert _intact(nbuf, 256, gn), "guard bytes around gnorm written"
    else:
        assert bool((nbuf == 0xFF).all()), "gnorm written though not asked for"
    return out.clone(), (gn.clone() if want_norm else None)


def _rho(out, ref, free, x, x0, eps, clamp, D, on_sphere):
    """(per-element rho, norm rho or None) of an l2 result; see RHO_BAR.  ref: the float64 result, free: the same without the clamp (the
    clamp is 1-Lipschitz: a clamped element errs by no more than its unclamped value does)."""
    x64, z64 = x.double(), (x if x0 is None else x0).double()
    A = _amp(D)
    den = U * (A * (free - z64).abs() + (x64 - z64).abs() + free.abs())
    rho = float(((out.double() - ref).abs() / den).max())
    rho_n = None
    if clamp is None and on_sphere:
        N = x.shape[0]
        r = (out.double() - z64).reshape(N, -1).norm(dim=1)
        den_n = U * (A * eps + (x64 - z64).reshape(N, -1).norm(dim=1) + ref.reshape(N, -1).norm(dim=1))
        rho_n = float(((r - eps).abs() / den_n).max())
    return rho, rho_n


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,C,HW", SHAPES)
def test_l2_per_element_against_float64(kind, N, C, HW):
    """One-step form (x0, step NULL), projection active (step 1.5 eps around an x0 a short way off) and inactive (a large ball), each with and
    without the per-channel clamp, at 256- (16-byte accesses where HW % 4 == 0), 8- and 4-byte pointer offsets: per element under RHO_BAR, and
    where no clamp acts and the result lies on the sphere, | ||out - x0|| - eps | under RHO_NORM_BAR (the same measure over norms).  gnorm against float64."""
    D = C * HW
    eps = _f32(0.05 * math.sqrt(D))
    clamp_v = ([-1.0] * C, [0.5 + 0.25 * c for c in range(C)])
    worst = [0.0, 0.0]
    for form, offset, step, e in (("one-step", 0.0, None, eps), ("projected", 0.01, _f32(1.5 * eps), eps), ("inside", 0.01, _f32(0.5 * eps), _f32(4 * eps))):
        x, g, x0 = _operands(N, C, HW, 1000 * HW + N, offset)
        for clamp in (None, clamp_v):
            ref, gn_ref = P64.perturb(x, g, e, "l2", x0=x0, step=step, clamp=clamp)
            free = P64.perturb(x, g, e, "l2", x0=x0, step=step)[0]
            if form == "projected" and clamp is None:
                assert float(((ref - x0.double()).reshape(N, -1).norm(dim=1) - e).abs().max()) < 1e-12       # (the projection IS active)
            for lead in (256, 8, 4):
                out, gn = _launch(kind, x, g, e, "l2", x0=x0, step=step, clamp=clamp, lead=lead)
                rho, rho_n = _rho(out, ref, free, x, x0, e, clamp, D, form != "inside")
                print(f"perturb l2 {kind} {(N, C, HW)} {form} clamp={clamp is not None} offset {lead}: rho {rho:.3e} norm rho {rho_n}")
                worst = [max(worst[0], rho), max(worst[1], rho_n or 0.0)]
                assert rho <= RHO_BAR, (form, lead, rho)
                assert rho_n is None or rho_n <= RHO_NORM_BAR, (form, lead, rho_n)
                assert float(((gn.double() - gn_ref) / gn_ref).abs().max()) <= 0.5 * (_blocks(D)[2] + 9 + _blocks(D)[0]) * U + U
    print(f"perturb l2 {kind} {(N, C, HW)}: worst rho {worst[0]:.3e}, worst norm rho {worst[1]:.3e} (bars {RHO_BAR:.3e} / {RHO_NORM_BAR:.3e}, ceiling 1)")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,C,HW", SHAPES)
def test_linf_per_element_and_exact_one_step(kind, N, C, HW):
    """linf without projection is x + eps * sign(g) formed in fp32, bit for bit (eps * sign is exact, one rounding in the sum), with and
    without gnorm; around an x0 every element is within the roundings of x - x0, of the step and of the result (no reduction enters)."""
    eps = _f32(0.0625 + 1e-3)
    x, g, x0 = _operands(N, C, HW, 77 * HW + N, 0.05)
    g[0, 0, :3] = 0.0
    want = x + eps * torch.sign(g)
    clamp_v = ([-1.0] * C, [0.5 + 0.25 * c for c in range(C)])
    lo = torch.tensor(clamp_v[0], device="cuda").reshape(1, C, 1)
    hi = torch.tensor(clamp_v[1], device="cuda").reshape(1, C, 1)
    step = _f32(0.4 * eps)
    for lead in (256, 8, 4):
        for want_norm in (False, True):
            out, gn = _launch(kind, x, g, eps, "linf", lead=lead, want_norm=want_norm)
            assert torch.equal(out, want), (lead, want_norm)
            assert bool((out[0, 0, :3] == x[0, 0, :3]).all())          # sign(0) = 0
            out, _ = _launch(kind, x, g, eps, "linf", clamp=clamp_v, lead=lead, want_norm=want_norm)
            assert torch.equal(out, torch.minimum(torch.maximum(want, lo), hi))
        if want_norm:
            assert float(((gn.double() - g.double().reshape(N, -1).norm(dim=1)) / gn.double()).abs().max()) < 64 * U
        for clamp in (None, clamp_v):
            ref, _ = P64.perturb(x, g, eps, "linf", x0=x0, step=step, clamp=clamp)
            if clamp is not None:
                ref_free = P64.perturb(x, g, eps, "linf", x0=x0, step=step)[0]
            else:
                ref_free = ref
            out, _ = _launch(kind, x, g, eps, "linf", x0=x0, step=step, clamp=clamp, lead=lead)
            bound = U * (2 * (x - x0).double().abs() + step + ref_free.abs()) * 1.0001
            assert bool(((out.double() - ref).abs() <= bound).all()), (lead, clamp is not None)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["l2", "linf"])
def test_degenerate_samples_are_left_alone(kind, mode):
    """Five samples: one with a nan, one with an inf, one all zero - those rows come back as x bit for bit (as clamp(x) with a clamp) with
    gnorm 0; the two others are the bits of a run that never saw the bad rows.  Two work-groups per sample."""
    N, C, HW = 5, 3, 1600
    x, g, _ = _operands(N, C, HW, 5)
    g[0, 1, 700], g[2, 2, 1599], g[4] = float("nan"), float("-inf"), 0.0
    eps = 0.5
    for step in (None, 0.75):
        out, gn = _launch(kind, x, g, eps, mode, step=step)
        good, gn_good = _launch(kind, x[[1, 3]].contiguous(), g[[1, 3]].contiguous(), eps, mode, step=step)
        assert torch.equal(out[[0, 2, 4]], x[[0, 2, 4]]) and gn[[0, 2, 4]].tolist() == [0.0, 0.0, 0.0]
        assert torch.equal(out[[1, 3]], good) and torch.equal(gn[[1, 3]], gn_good) and not torch.equal(good, x[[1, 3]])
    out, _ = _launch(kind, x, g, eps, mode, clamp=([-0.3] * 3, [0.2] * 3))
    assert torch.equal(out[[0, 2, 4]], x[[0, 2, 4]].clamp(-0.3, 0.2))
    if mode == "linf":      # the one-launch form (no gnorm, no reduction): element by element, sign(nan) = 0 and sign(-inf) = -1
        out, _ = _launch(kind, x, g, eps, mode, want_norm=False)
        assert torch.equal(out, x + eps * torch.sign(torch.nan_to_num(g, nan=0.0))) and out[0, 1, 700] == x[0, 1, 700] and out[2, 2, 1599] == x[2, 2, 1599] - 0.5


@pytest.mark.parametrize("kind", KINDS)
def test_l2_is_invariant_to_a_power_of_two_scale_and_deterministic(kind):
    """g * 2^k, k in {-10, 10, 16}, gives the bits of g (the squares scale by 2^2k exactly, the root by 2^k, step / norm by 2^-k); gnorm scales
    exactly; two calls give the same bits.  Both paths (16- and 4-byte), one-step and projected."""
    for (N, C, HW), lead in (((2, 3, 64 * 96), 256), ((2, 3, 33), 4)):
        x, g, x0 = _operands(N, C, HW, 9, 0.02)
        eps = _f32(0.05 * math.sqrt(C * HW))
        for z, step in ((None, None), (x0, _f32(1.5 * eps))):
            base, gn = _launch(kind, x, g, eps, "l2", x0=z, step=step, lead=lead)
            again, gn2 = _launch(kind, x, g, eps, "l2", x0=z, step=step, lead=lead)
            assert torch.equal(base, again) and torch.equal(gn, gn2), "two calls differ"
            for k in (-10, 10, 16):
                out, gnk = _launch(kind, x, g * 2.0 ** k, eps, "l2", x0=z, step=step, lead=lead)
                assert torch.equal(out, base), f"k = {k}: {int((out != base).sum())} elements differ"
                assert torch.equal(gnk, gn * 2.0 ** k)


@pytest.mark.parametrize("mode,project", [("l2", False), ("l2", True), ("linf", True)])
def test_captured_launch_replays_and_follows_its_device_operands(mode, project):
    """A captured call replays the eager bits, follows an overwritten g, and follows a changed eps DEVICE scalar."""
    from uda_poseestimation_amd import adversarial
    N, C, HW = 2, 3, 40 * 24
    x, g, x0 = _operands(N, C, HW, 21, 0.02)
    g2 = _operands(N, C, HW, 22)[1]
    eps_t = torch.tensor(0.5, device="cuda")
    step_t = torch.tensor(0.75, device="cuda") if project else None
    z = x0 if project else None
    gs, out = g.clone(), torch.empty_like(x)
    eager = {}
    for name, gg, e in (("g", g, 0.5), ("g2", g2, 0.5), ("eps", g2, 0.125)):
        eager[name] = adversarial.perturb(x, gg, torch.tensor(e, device="cuda"), mode, x0=z, step=step_t, want_norm=True)
    torch.cuda.synchronize()
    assert not torch.equal(eager["g"][0], eager["g2"][0]) and not torch.equal(eager["g2"][0], eager["eps"][0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, gn = adversarial.perturb(x, gs, eps_t, mode, x0=z, step=step_t, out=out, want_norm=True)
    for name, gg, e in (("g", g, 0.5), ("g2", g2, 0.5), ("eps", g2, 0.125), ("g", g, 0.5)):
        gs.copy_(gg)
        eps_t.fill_(e)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[name][0]) and torch.equal(gn, eager[name][1]), name


@pytest.mark.parametrize("kind", KINDS)
def test_bad_arguments_are_refused_and_nothing_is_written(kind):
    from uda_poseestimation_amd import _hip
    L = _hip.lib(kind)
    N, C, HW = 2, 3, 64
    x, g, _ = _operands(N, C, HW, 3)
    x_keep, g_keep = x.clone(), g.clone()
    out = torch.full_like(x, 7.0)
    gn = torch.full((N,), 7.0, device="cuda")
    ws = torch.full((L.udapose_perturb_ws_bytes(N, C, HW) // 4,), 7.0, device="cuda")
    eps = torch.tensor(0.5, device="cuda")
    lo = torch.zeros(C, device="cuda")
    s, p = _hip.stream(), _hip.ptr
    ok = dict(x=p(x), g=p(g), x0=None, N=N, C=C, HW=HW, mode=0, eps=p(eps), step=None, lo=None, hi=None, ws=p(ws), out=p(out), gnorm=p(gn))
    cases = {"null x": dict(x=None), "null g": dict(g=None), "null eps": dict(eps=None), "null out": dict(out=None), "N = 0": dict(N=0),
             "C = 0": dict(C=0), "HW = 0": dict(HW=0), "mode 2": dict(mode=2), "mode -1": dict(mode=-1), "out is g": dict(out=p(g)),
             "out inside g": dict(out=g.data_ptr() + 16), "out ends in g": dict(out=g.data_ptr() - 4 * (N * C * HW - 1)), "lo alone": dict(lo=p(lo)),
             "hi alone": dict(hi=p(lo)), "null ws in l2": dict(ws=None), "null ws in linf with gnorm": dict(ws=None, mode=1)}
    for what, change in cases.items():
        a = dict(ok, **change)
        assert L.udapose_perturb(s, *a.values()) == ERR_ARG, what
    torch.cuda.synchronize()
    for t, what in ((out, "out"), (gn, "gnorm"), (ws, "ws")):
        assert bool((t == 7.0).all()), what
    assert torch.equal(x, x_keep) and torch.equal(g, g_keep)
    assert L.udapose_perturb(s, *dict(ok, ws=None, mode=1, gnorm=None).values()) == 0       # linf without gnorm needs no workspace
    assert L.udapose_perturb(s, *ok.values()) == 0
    assert L.udapose_perturb(s, *dict(ok, out=p(x)).values()) == 0                           # in place
    torch.cuda.synchronize()
    assert torch.equal(out, x) and not torch.equal(x, x_keep)
