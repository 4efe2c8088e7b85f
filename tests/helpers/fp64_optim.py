"""Float64 references of the optimizer kernels of csrc/optim.hip (adam_k, sgd_k and their copies in opt_tail_k's tail1), the exact
references of ema_k and scaler_update_k, float32 emulations of the kernels' order of operations, and the bars the tests hold them to.

References.  adam() and sgd() are float64, computed from the kernel's fp32 inputs of ONE step (parameters, gradients, moments as stored),
with the hyper-parameters as the fp32 values the kernels are passed: f32(lr), f32(beta), f32(eps), f32(weight_decay), f32(grad_scale), and
the device state's f32(1 - beta1^t) and f32(sqrt(1 - beta2^t)), formed in double from the fp32 betas and then rounded, as adam_tick_k does
(bias_corrections(); exact_bc=True leaves them unrounded, which is torch.optim.Adam in float64).  Each output comes with its absref, the
sum of the magnitudes of its terms, in the style of fp64_conv.  A second gradient buffer is added first, g + g2 rounded to fp32 as axpy
would leave it; its absref is |g| + |g2|.

ema() is not float64: the kernel promises the bits of fl(fl(t * a) + fl(s * b)), a = f32(alpha), b = f32(1.0 - alpha) with the difference
formed in double as the host does, so the reference is that expression in numpy float32.  scaler_trajectory() is exact as well.

Bars.  tau = k * 2^-24 against absref, plus half an ulp of the stored fp32 value (check()).  k counts the fp32 roundings on the path from
the inputs to the value, each weighted by how its relative error reaches the output relative to absref.  optim.hip is compiled without
FMA contraction, and HIP's default fp32 division and square root are correctly rounded, so every operation is one rounding of at most
u = 2^-24 relative.  Products never change a relative error's weight and sums of terms of bounded relative error stay bounded by the
largest count relative to the sum of magnitudes, so with A = |g * gs| + |wd * p| the magnitude of the effective gradient gr:

  k_gr  = [g + g2: 1] + [g * gs: 1] + [wd != 0: the product wd * p and the sum, 2]                 (1 .. 4)
  Adam
    m   = fl(fl(m * b1) + fl(fl(1 - b1) * gr)):   k_gr + [1 - b1: 1] + [product: 1] + [sum: 1]                         k_m = k_gr + 3
    v   = fl(fl(v * b2) + fl(fl(fl(1 - b2) * gr) * gr)): gr enters squared (2 k_gr), 1 - b2, two products, the sum     k_v = 2 k_gr + 4
    d   = -fl(fl(lr / bc1) * fl(m / fl(fl(sqrt(v) / bc2) + eps))), the step p_new - p_old.  The stored m carries k_m + 1 (its own final
          rounding); lr / bc1, m / D and the product are 3; in D = sqrt(v) / bc2 + eps the stored v carries (k_v + 1) u of absref_v, which
          the root halves and which weighs r = absref_v / v (1 unless g, g2 and wd * p cancel) - then the root, the division by bc2 and
          the sum are 3 more, all at a weight s = (sqrt(v) / bc2) / D <= 1 that is taken as 1:
                                                                           k_d = (k_m + 1) + 3 + 3 + (k_v + 1) / 2 * r   (14.5 plain, r = 1)
  SGD
    b   = gr on the first step (k_gr), else fl(fl(buf * mu) + gr): the larger term count plus the sum                   k_b = k_gr + 1
    d   = -fl(lr * b): k_b + 1; Nesterov -fl(lr * fl(gr + fl(mu * b))): the product mu * b, the sum, the product        k_d = k_b + 1 | k_b + 3
The step is checked as (p_new - p_old) in float64 against d with half an ulp of p_new granted for the one rounding of the parameter
(check_step()): it is not a tolerance on p.  Second-order terms ((1 + u)^k - 1 - k u < 1e-13) are covered by the half ulp of the stored
value that check() grants on top of a count that already includes the final rounding.  Range: a gradient whose square exceeds FLT_MAX
makes v = +inf in fp32 (so does torch.optim.Adam in fp32); the references return such elements in `over`: there v must be +inf and the
step exactly 0 (m / inf), and they are left out of the tau checks of v and d.

Nothing here is tuned on a device.  tests/test_optim_bounds_cpu.py shows that the emulations (emu_adam, emu_sgd, emu_ema: numpy float32,
operation by operation in the kernels' order) pass these bars in every value regime the GPU test uses and that each planted fault
(the `fault` argument of the emulations) fails them in at least one."""
import math

import numpy as np
import torch

from helpers import fp64_conv as fc

U = 2.0 ** -24
FLT_MAX = 3.4028234663852886e38
F32 = torch.float32


def f32(x):
    """x rounded to fp32, as a Python float (what a kernel receives for a `float` argument)."""
    return float(np.float32(x))


def bias_corrections(beta1, beta2, t, exact=False):
    """(1 - beta1^t, sqrt(1 - beta2^t)) from the fp32 betas in double, rounded to fp32 as adam_tick_k stores them (exact: not rounded)."""
    bc1 = 1.0 - math.pow(f32(beta1), float(t))
    bc2 = math.sqrt(1.0 - math.pow(f32(beta2), float(t)))
    return (bc1, bc2) if exact else (f32(bc1), f32(bc2))


def _d(x):
    return x.detach().double() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=torch.float64)


def _grad(g, g2):
    """(g [+ g2 rounded to fp32], |g| + |g2|) in float64."""
    g = _d(g)
    if g2 is None:
        return g, g.abs()
    g2 = _d(g2)
    return (g + g2).float().double(), g.abs() + g2.abs()


def k_gr(wd=0.0, g2=False):
    return (1 if g2 else 0) + 1 + (2 if wd != 0 else 0)


def K(kind, wd=0.0, g2=False, nesterov=False, first=False):
    """The rounding counts per output (the module docstring derives them).  Adam's 'd' is the part without the v term: check_adam adds
    (k_v + 1) / 2 * absref_v / v per element."""
    kg = k_gr(wd, g2)
    if kind == "adam":
        return {"m": kg + 3, "v": 2 * kg + 4, "d": (kg + 3 + 1) + 3 + 3}
    kb = kg if first else kg + 1
    return {"b": kb, "d": kb + (3 if nesterov else 1)}


def adam(p, g, m, v, lr, beta1, beta2, eps, t, weight_decay=0.0, grad_scale=1.0, g2=None, exact_bc=False):
    """One torch.optim.Adam step (no amsgrad; weight decay added to the gradient) at 1-based step t.  Returns a dict:
    m, v, d = (ref, absref) of the new moments and of the step p_new - p; over = elements whose v exceeds fp32's range."""
    lr, b1, b2, eps, wd, gs = (f32(x) for x in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    bc1, bc2s = bias_corrections(b1, b2, t, exact_bc)
    p, m, v = _d(p), _d(m), _d(v)
    gsum, gabs = _grad(g, g2)
    gr, A = gsum * gs, gabs * abs(gs)
    if wd != 0:
        gr, A = gr + wd * p, A + (wd * p).abs()
    mn, ma = m * b1 + (1 - b1) * gr, (m * b1).abs() + (1 - b1) * A
    vn, va = v * b2 + (1 - b2) * gr * gr, v.abs() * b2 + (1 - b2) * A * A
    over = vn > FLT_MAX
    den = torch.where(over, torch.full_like(vn, math.inf), torch.sqrt(vn)) / bc2s + eps
    step = lr / bc1
    return {"m": (mn, ma), "v": (vn, va), "d": (-step * (mn / den), step * (ma / den)), "over": over}


def sgd(p, g, buf, lr, momentum, weight_decay=0.0, nesterov=False, first=False, grad_scale=1.0, g2=None):
    """One torch.optim.SGD step (dampening 0).  first: the step that initialises the momentum buffer with the gradient.  momentum = 0 keeps
    b = gr (torch keeps no buffer then).  Returns b, d = (ref, absref)."""
    lr, mu, wd, gs = (f32(x) for x in (lr, momentum, weight_decay, grad_scale))
    p, buf = _d(p), _d(buf)
    gsum, gabs = _grad(g, g2)
    gr, A = gsum * gs + wd * p, gabs * abs(gs) + (wd * p).abs()
    b, ba = (gr, A) if first else (buf * mu + gr, (buf * mu).abs() + A)
    s, sa = (gr + mu * b, A + mu * ba) if nesterov else (b, ba)
    return {"b": (b, ba), "d": (-lr * s, lr * sa)}


def ema(t, s, alpha):
    """The bits ema_k promises: fl(fl(t * a) + fl(s * b)) in numpy float32, a = f32(alpha), b = f32(1.0 - alpha).  Returns a numpy array."""
    a, b = np.float32(alpha), np.float32(1.0 - alpha)
    t = np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float32)
    s = np.asarray(s.detach().cpu().numpy() if torch.is_tensor(s) else s, dtype=np.float32)
    with np.errstate(all="ignore"):
        t1 = (t * a).astype(np.float32)
        t2 = (s * b).astype(np.float32)
        return (t1 + t2).astype(np.float32)


def scaler_trajectory(flags, init=65536.0, growth=2.0, backoff=0.5, interval=2000):
    """[(scale, tracker, grad_scale, optimizer step counter)] after every GradScaler.update(), for found-inf flags `flags` (an iterable of
    0 / 1, or a string of '0' / '1').  Exact: fp32 products, 1 / scale rounded to fp32."""
    scale, tr, steps, out = np.float32(init), 0, 0, []
    for f in flags:
        if int(f):
            scale, tr = np.float32(scale * np.float32(backoff)), 0
        else:
            steps, tr = steps + 1, tr + 1
            if tr >= interval:
                scale, tr = np.float32(scale * np.float32(growth)), 0
        out.append((float(scale), tr, float(np.float32(1.0) / scale), steps))
    return out


# ---- checks -----------------------------------------------------------------------------------------------------------------------

def check(got, ref, absref, k, what, keep=None, extra=None):
    """|got - ref| <= k * 2^-24 * absref + half an fp32 ulp of the value (+ `extra`) in every element of `keep` (all when None); k a number
    or a tensor.  Returns the measured k: the largest (|got - ref| - the granted half ulp) / absref in units of 2^-24."""
    g64, r64, a64 = _d(got).reshape(-1), _d(ref).reshape(-1), _d(absref).reshape(-1)
    assert g64.shape == r64.shape == a64.shape, (what, tuple(g64.shape), tuple(r64.shape))
    sel = torch.ones_like(g64, dtype=torch.bool) if keep is None else keep.reshape(-1)
    if not bool(torch.isfinite(g64[sel]).all()):
        bad = int((sel & ~torch.isfinite(g64)).nonzero()[0])
        raise AssertionError(f"{what}: non-finite value {float(g64[bad])} at element {bad} (reference {float(r64[bad]):.6g})")
    hu = torch.maximum(fc.half_ulp(r64, F32), fc.half_ulp(torch.where(torch.isfinite(g64), g64, r64), F32))
    if extra is not None:
        hu = hu + _d(extra).reshape(-1)
    err = torch.where(sel, (g64 - r64).abs(), torch.zeros_like(g64))
    kt = k.reshape(-1).double() if torch.is_tensor(k) else torch.full_like(g64, float(k))
    slack = torch.where(sel, err - (kt * U * a64 + hu), torch.full_like(err, -1.0))
    meas = torch.where(sel, (err - hu).clamp(min=0) / a64.clamp(min=1e-300), torch.zeros_like(err)) / U
    if slack.numel() and float(slack.max()) > 0:
        w = int(slack.argmax())
        raise AssertionError(f"{what}: |got - ref| = {float(err[w]):.4g} > k * 2^-24 * absref + ulp / 2 = {float(kt[w] * U * a64[w] + hu[w]):.4g} at "
                             f"element {w} (got {float(g64[w]):.9g}, ref {float(r64[w]):.9g}, absref {float(a64[w]):.4g}, k {float(kt[w]):.3g}, "
                             f"measured k {float(meas[w]):.3g})")
    ratio = torch.where(sel, meas / kt.clamp(min=1e-300), torch.zeros_like(meas))
    return (float(meas.max()), float(ratio.max())) if meas.numel() else (0.0, 0.0)


def check_adam(p_old, p_new, m_new, v_new, ref, k, what):
    """m, v and the step p_new - p_old of one Adam step against adam()'s result at the counts k = K('adam', ...).  Returns
    {output: (measured k, measured / bar)}."""
    ok = ~ref["over"]
    out = {"m": check(m_new, *ref["m"], k["m"], what + " exp_avg")}
    out["v"] = check(v_new, *ref["v"], k["v"], what + " exp_avg_sq", keep=ok)
    vn, va = ref["v"]
    r = torch.where(vn > 0, va / vn.clamp(min=1e-300), torch.ones_like(vn))
    kd = k["d"] + 0.5 * (k["v"] + 1) * torch.where(ok, r, torch.ones_like(r))
    d = _d(p_new) - _d(p_old)
    out["d"] = check(d, *ref["d"], kd, what + " step", keep=ok, extra=fc.half_ulp(_d(p_new), F32))
    if bool(ref["over"].any()):         # g^2 beyond fp32's range: v = +inf, and the step m / inf is exactly 0
        o = ref["over"].reshape(-1)
        vo, do = _d(v_new).reshape(-1)[o], d.reshape(-1)[o]
        assert bool((vo == math.inf).all()) and bool((do == 0).all()), \
            f"{what}: {int(o.sum())} elements whose v exceeds FLT_MAX: v must be +inf and the step 0, got v {vo[:4].tolist()} step {do[:4].tolist()}"
    return out


def check_sgd(p_old, p_new, b_new, ref, k, what, with_buffer=True):
    out = {}
    if with_buffer:
        out["b"] = check(b_new, *ref["b"], k["b"], what + " momentum_buffer")
    out["d"] = check(_d(p_new) - _d(p_old), *ref["d"], k["d"], what + " step", extra=fc.half_ulp(_d(p_new), F32))
    return out


def bits_differ(a, b):
    """How many elements of two fp32 arrays differ in their bits."""
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32).reshape(-1)
    b = np.ascontiguousarray(b.detach().cpu().numpy() if torch.is_tensor(b) else b, dtype=np.float32).reshape(-1)
    return int((a.view(np.int32) != b.view(np.int32)).sum())


# ---- float32 emulations of the kernels' order of operations (numpy: every operation rounds once, division and root correctly) ------

def _n(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32)


ADAM_FAULTS = ("eps_in_sqrt", "eps_over_bc2", "bc2_on_v", "wd_after_moments", "wd_decoupled", "gscale_after_square", "beta2_for_m", "bc_of_t_minus_1",
               "skip_element")
SGD_FAULTS = ("nesterov_is_b", "first_reads_buffer", "skip_element")


def emu_adam(p, g, m, v, lr, beta1, beta2, eps, t, weight_decay=0.0, grad_scale=1.0, g2=None, fault=None):
    """adam_k (and tail1<KIND_ADAM>) operation by operation in numpy float32.  Returns (p_new, m_new, v_new).  fault: one of ADAM_FAULTS."""
    f = np.float32
    lr, b1, b2, eps, wd, gs = (f(x) for x in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    bc1, bc2s = (f(x) for x in bias_corrections(b1, b2, t - 1 if fault == "bc_of_t_minus_1" else t))
    p, g, m, v = _n(p), _n(g), _n(m), _n(v)
    one = f(1.0)
    with np.errstate(all="ignore"):
        if g2 is not None:
            g = g + _n(g2)
        gr = g * gs
        if wd != 0 and fault not in ("wd_after_moments", "wd_decoupled"):
            gr = gr + wd * p
        mb = b2 if fault == "beta2_for_m" else b1
        mi = m * mb + (one - mb) * gr
        sq = ((one - b2) * g * g) * gs if fault == "gscale_after_square" else (one - b2) * gr * gr
        vi = v * b2 + sq
        step = lr / bc1
        if fault == "eps_in_sqrt":
            den = np.sqrt(vi + eps) / bc2s
        elif fault == "eps_over_bc2":
            den = (np.sqrt(vi) + eps) / bc2s
        elif fault == "bc2_on_v":
            den = np.sqrt(vi / bc2s) + eps
        else:
            den = np.sqrt(vi) / bc2s + eps
        upd = mi / den
        if fault == "wd_after_moments" and wd != 0:
            upd = upd + wd * p
        pn = p - step * upd
        if fault == "wd_decoupled" and wd != 0:
            pn = pn - lr * wd * p
        if fault == "skip_element":
            i = min(pn.size - 1, 4095)
            pn.reshape(-1)[i], mi.reshape(-1)[i], vi.reshape(-1)[i] = p.reshape(-1)[i], m.reshape(-1)[i], v.reshape(-1)[i]
    return pn.astype(f), mi.astype(f), vi.astype(f)


def emu_sgd(p, g, buf, lr, momentum, weight_decay=0.0, nesterov=False, first=False, grad_scale=1.0, g2=None, fault=None):
    """sgd_k (and tail1<KIND_SGD>) in numpy float32.  Returns (p_new, buf_new).  fault: one of SGD_FAULTS."""
    f = np.float32
    lr, mu, wd, gs = (f(x) for x in (lr, momentum, weight_decay, grad_scale))
    p, g, buf = _n(p), _n(g), _n(buf)
    with np.errstate(all="ignore"):
        if g2 is not None:
            g = g + _n(g2)
        gr = g * gs + wd * p
        # (first_reads_buffer: the first step trusts the buffer to hold zeros instead of overwriting it with the gradient - the same number
        # on a fresh buffer, and wrong after a skipped step or on a buffer that was never cleared: the tests pre-fill it)
        b = gr.copy() if first and fault != "first_reads_buffer" else buf * mu + gr
        s = (b if fault == "nesterov_is_b" else gr + mu * b) if nesterov else b
        pn = p - lr * s
        if fault == "skip_element":
            i = min(pn.size - 1, 4095)
            pn.reshape(-1)[i], b.reshape(-1)[i] = p.reshape(-1)[i], buf.reshape(-1)[i]
    return pn.astype(f), b.astype(f)


def emu_ema(t, s, alpha, fault=None):
    """ema_k in numpy float32 (the reference itself); fault 'fused': one rounding, fl(t * a + s * b), as an FMA-contracted build gives."""
    if fault != "fused":
        return ema(t, s, alpha)
    a, b = float(np.float32(alpha)), float(np.float32(1.0 - alpha))
    t64, s64 = _n(t).astype(np.float64), _n(s).astype(np.float64)
    # fl(fma(t, a, fl(s * b))): the product s * b rounded, the other kept exact inside the fused operation
    with np.errstate(all="ignore"):
        return (t64 * a + (s64 * b).astype(np.float32).astype(np.float64)).astype(np.float32)


# ---- the value regimes of tests/test_gpu_optim_forms.py (on the CPU generator: the same numbers in the CPU and the GPU test) -------

REGIMES = ("a", "b", "c", "d", "e", "f")
F_SCALE = 65536.0


def regime(name, n, seed, step=0):
    """(p, g, grad_scale) fp32 CPU tensors of n elements for value regime `name` at step `step` (p is the initial parameter: only step 0's is
    used).  a: p, g ~ 0.05 N(0,1).  b: |g| ~ 1e-8 N(0,1): sqrt(v) comparable with eps.  c: log-uniform |g| in [1e-15, 1e3], random signs, a
    tenth exactly 0.  d: g = 0.  e: p = 0 exactly, g as in a.  f: gradients pre-multiplied by 65536 with grad_scale = 1 / 65536; the elements
    at positions 0 mod 997 carry +-FLT_MAX and +-3e38, scaled values that are only just finite."""
    gen = torch.Generator().manual_seed(seed * 1000 + step * 7 + REGIMES.index(name))
    p = torch.randn(n, generator=gen) * 0.05
    g = torch.randn(n, generator=gen) * 0.05
    gs = 1.0
    if name == "b":
        g = torch.randn(n, generator=gen) * 1e-8
    elif name == "c":
        e = torch.rand(n, generator=gen, dtype=torch.float64) * 18.0 - 15.0
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
        g = (torch.pow(10.0, e)).float() * sign
        g[torch.rand(n, generator=gen) < 0.1] = 0.0
    elif name == "d":
        g = torch.zeros(n)
    elif name == "e":
        p = torch.zeros(n)
    elif name == "f":
        g = g * F_SCALE
        edge = torch.tensor([FLT_MAX, -3e38, 3e38, -FLT_MAX], dtype=torch.float32)
        idx = torch.arange(0, n, 997)
        g[idx] = edge[(idx // 997 + step) % 4]
        gs = 1.0 / F_SCALE
    return p.float(), g.float(), gs
