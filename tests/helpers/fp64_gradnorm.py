"""References, host restatement, order emulation and the bar of gradient clipping by global norm (csrc/optim.hip: grad_sumsq_k,
grad_clip_k; include/udapose.h udapose_grad_sumsq / udapose_grad_clip).

Definition (include/udapose.h).  Per parameter group g with gradient tensors g_i, an optional second buffer g2_i and the fp32 grad_scale gs_g:
  x_i = fl32(g_i + g2_i),  S_g = sum_i x_i^2,  total = sum_g gs_g^2 * S_g,  norm = fl32(sqrt(total)),
  coef = fl32(min(1, f64(max_norm) / (f64(norm) + 1e-6))), formed from the STORED fp32 norm (a NaN stays a NaN).

Reference.  ref_norm() is exact: every x_i is an integer times a power of two, so sum x_i^2 is summed in integers (per exponent, 24-bit halves
in int64, then Python integers), gs_g^2 and the sum over the groups are Fractions, and the square root is an integer square root carried
to 2^-120 relative.  It is returned as a Fraction (or +inf / nan as a float when an x_i is not finite); nothing in it rounds at double
precision, so it needs no allowance of its own.

The bar, derived and not tuned:  |norm - ref| <= half an fp32 ulp of ref + n * 2^-53 * ref,  n = the element count.
The kernels accumulate in double.  x_i^2 is exact in double (24-bit significands), so the only errors are the additions, and every term is
non-negative: an addition's rounding is at most 2^-53 of a partial sum that is itself at most the total, so the relative error of S is at
most 2^-53 times the largest number of additions any one square passes through (no cancellation).  In its block that is at most
4096 / 256 = 16 in the thread's own accumulator and 6 + 3 in the tree; in the finisher at most ceil(nblocks / 256) in a thread and 9 in
the tree: 34 + nblocks / 256 in all, with nblocks <= n / 4096 + the number of tensors.  The product gs^2 * S (exact when gs is a power
of two, as in every regime used here), the sum over the groups and the double square root add at most 3 more, and the root halves all
that came before it: the norm's relative error before its rounding to fp32 is at most (34 + nblocks / 256 + 2) / 2 + 1 = 19 + nblocks /
512 units of 2^-53, below n * 2^-53 for n >= 20.  For n < 20 every block's thread adds at most one square to 0.0 (exact) and the trees add
at most n - 1 non-zero terms to one another, so the total carries at most n - 1 roundings (+ 1 for a second group) and the norm at most
n / 2 + 1 <= n of them for n >= 2; a single element's square and its double root give one rounding.  The final conversion to fp32 is the
half ulp.  bar() evaluates this in exact rational arithmetic.

emu() restates the kernels' order in numpy float64 (thread-strided accumulation in 4096-element blocks, the 16-byte path's quads and
scalar tail, the shuffle tree per wave, the four waves in order; the finisher likewise over the partials); its `fault` argument plants the
faults tests/test_grad_clip_cpu.py shows the bar and the coefficient check to catch.  Nothing here is tuned on a device."""
import math
from fractions import Fraction

import numpy as np
import torch

FLT_MAX = 3.4028234663852886e38
CHUNK, TPB = 4096, 256

FAULTS = ("fp32_accumulate", "square_after_scale_fp32", "g2_ignored", "tail_skipped", "last_block_dropped", "state4_forgotten", "no_clamp",
          "coef_from_unrounded_total")


def _n32(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32).reshape(-1)


def x_of(g, g2=None):
    """fl32(g + g2) as a float32 array: the value the optimizer sweep forms."""
    g = _n32(g)
    if g2 is None:
        return g
    with np.errstate(all="ignore"):
        return (g + _n32(g2)).astype(np.float32)


def _exact_sumsq(x):
    """sum x^2 of a finite float32 array as a Fraction, in integer arithmetic."""
    x = x[x != 0]
    if x.size == 0:
        return Fraction(0)
    m, e = np.frexp(x.astype(np.float64))                  # x = m * 2^e, 0.5 <= |m| < 1
    mi = np.abs(np.round(m * 2.0 ** 24)).astype(np.int64)   # 24-bit integers (exact for fp32 values, denormals included)
    e = e.astype(np.int64) - 24
    sq = mi * mi                                            # < 2^48
    order = np.argsort(e, kind="stable")
    e, sq = e[order], sq[order]
    starts = np.flatnonzero(np.concatenate(([True], e[1:] != e[:-1])))
    hi = np.add.reduceat(sq >> 24, starts)
    lo = np.add.reduceat(sq & 0xFFFFFF, starts)
    total = Fraction(0)
    for ex, h, l in zip(e[starts].tolist(), hi.tolist(), lo.tolist()):
        total += Fraction((h << 24) + l) * Fraction(2) ** (2 * ex)
    return total


def _sqrt_fraction(q, bits=120):
    """sqrt of a non-negative Fraction to 2^-bits relative, as a Fraction."""
    if q == 0:
        return Fraction(0)
    k = bits + max(0, q.denominator.bit_length() - q.numerator.bit_length()) // 2 + 1
    return Fraction(math.isqrt((q.numerator << (2 * k)) // q.denominator), 1 << k)


def ref_norm(groups):
    """The exact norm.  groups: [(tensors, tensors2 or None, grad_scale)], tensors = a list of arrays / tensors.  A Fraction, or float
    +inf / nan when some fl32(g + g2) is not finite (nan wins over inf, as in the sum)."""
    total, bad = Fraction(0), None
    for gs_, g2s, gs in groups:
        x = np.concatenate([x_of(g, None if g2s is None else g2s[i]) for i, g in enumerate(gs_)]) if gs_ else np.zeros(0, np.float32)
        if np.isnan(x).any():
            return math.nan
        if np.isinf(x).any():
            bad = math.inf
            continue
        total += Fraction(float(np.float32(gs))) ** 2 * _exact_sumsq(x)
    return bad if bad is not None else _sqrt_fraction(total)


def count(groups):
    return sum(int(_n32(g).size) for gs_, _, _ in groups for g in gs_)


def half_ulp32(ref):
    """Half an fp32 ulp at `ref` (a non-negative Fraction), as a Fraction."""
    if ref == 0:
        return Fraction(1, 2 ** 150)
    e = ref.numerator.bit_length() - ref.denominator.bit_length()
    if Fraction(2) ** e > ref:
        e -= 1                                              # 2^e <= ref < 2^(e+1)
    return Fraction(2) ** (max(e, -126) - 24)


def bar(ref, n):
    return half_ulp32(ref) + n * Fraction(1, 2 ** 53) * ref


def check_norm(got, ref, n, what):
    """`got` (the stored fp32 norm) against the exact reference at the bar.  Returns (|got - ref| - half ulp) / (2^-53 ref), the measured
    count of double roundings (<= 0: inside the half ulp alone)."""
    got = float(got)
    if isinstance(ref, float):                              # +inf / nan
        assert (math.isnan(got) if math.isnan(ref) else got == ref), f"{what}: norm {got}, reference {ref}"
        return 0.0
    if ref > Fraction(FLT_MAX) + half_ulp32(Fraction(FLT_MAX)):
        assert got == math.inf, f"{what}: the total is beyond fp32's range, norm must be +inf, got {got}"
        return 0.0
    assert math.isfinite(got), f"{what}: norm {got}, reference {float(ref):.9g}"
    err, b = abs(Fraction(got) - ref), bar(ref, n)
    meas = float((err - half_ulp32(ref)) / (Fraction(1, 2 ** 53) * ref)) if ref else 0.0
    assert err <= b, (f"{what}: |norm - ref| = {float(err):.6g} > half an fp32 ulp + n * 2^-53 * ref = {float(b):.6g} (norm {got!r}, ref "
                      f"{float(ref)!r}, n {n}, measured {meas:.3g} double roundings beyond the half ulp)")
    return meas


def coef_host(norm, max_norm):
    """The coefficient's bits from a read-back: fl32(min(1, f64(fl32(max_norm)) / (f64(norm) + 1e-6))), a NaN kept.  numpy float32."""
    with np.errstate(all="ignore"):
        c = np.float64(np.float32(max_norm)) / (np.float64(np.float32(norm)) + np.float64(1e-6))
        return np.float32(np.float64(1.0) if c > 1.0 else c)


def same_bits(a, b):
    return np.float32(a).view(np.int32) == np.float32(b).view(np.int32)


# ---- the kernels' order in numpy ------------------------------------------------------------------------------------------------------

def _tree(acc):
    """block_sum: lane i += lane i + 32, 16, .. 1 inside each wave of 64, then ((w0 + w1) + w2) + w3."""
    a = acc.reshape(TPB // 64, 64).copy()
    off = 32
    while off:
        a[:, :off] = a[:, :off] + a[:, off:2 * off]
        off >>= 1
    return ((a[0, 0] + a[1, 0]) + a[2, 0]) + a[3, 0]


def _strided(acc, vals):
    """thread t adds vals[t], vals[t + 256], ... in order."""
    k = -(-vals.size // TPB)
    pad = np.zeros(k * TPB, vals.dtype)
    pad[:vals.size] = vals
    for row in pad.reshape(k, TPB):
        acc = acc + row                                     # (+ 0.0 is exact for the threads a short row does not reach)
    return acc


def emu_partials(g, g2=None, aligned=True, gs=1.0, fault=None):
    """grad_sumsq_k over one tensor: the per-block partial sums (float64).  aligned: the 16-byte path (quads, then the scalar tail)."""
    x = x_of(g, None if fault == "g2_ignored" else g2)
    acc_t = np.float64
    with np.errstate(all="ignore"):
        if fault == "fp32_accumulate":
            sq, acc_t = (x * x).astype(np.float32), np.float32
        elif fault == "square_after_scale_fp32":
            y = (x * np.float32(gs)).astype(np.float32)
            sq = (y * y).astype(np.float32).astype(np.float64)
        else:
            sq = x.astype(np.float64) ** 2
        out = []
        for off in range(0, x.size, CHUNK):
            c = sq[off:off + CHUNK]
            acc = np.zeros(TPB, acc_t)
            if aligned:
                n4 = c.size // 4
                k = -(-n4 // TPB)
                quads = np.zeros((k * TPB, 4), acc_t)
                quads[:n4] = c[:n4 * 4].reshape(n4, 4)
                for rows in quads.reshape(k, TPB, 4):
                    for e in range(4):
                        acc = acc + rows[:, e]
                if fault != "tail_skipped":
                    acc = _strided(acc, c[n4 * 4:])
            else:
                acc = _strided(acc, c)
            out.append(_tree(acc))
    return np.asarray(out, acc_t)


def emu(groups, max_norm, aligned=None, fault=None):
    """grad_sumsq_k per tensor and grad_clip_k over every group: (norm, coef) as numpy float32.  groups as for ref_norm(); aligned: per
    group a list of flags per tensor (None: all on the 16-byte path)."""
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for gi, (gs_, g2s, gs) in enumerate(groups):
            parts = [emu_partials(g, None if g2s is None else g2s[i], True if aligned is None else aligned[gi][i], gs, fault)
                     for i, g in enumerate(gs_)]
            parts = np.concatenate(parts) if parts else np.zeros(0)
            if fault == "last_block_dropped":
                parts = parts[:-1]
            S = np.float64(_tree(_strided(np.zeros(TPB, parts.dtype), parts)))
            gsd = np.float64(1.0) if fault in ("state4_forgotten", "square_after_scale_fp32") else np.float64(np.float32(gs))
            total = total + gsd * gsd * S
        norm_d = np.sqrt(total)
        norm = np.float32(norm_d)
        if fault == "coef_from_unrounded_total":
            c = np.float64(np.float32(max_norm)) / (norm_d + np.float64(1e-6))
            coef = np.float32(np.float64(1.0) if c > 1.0 else c)
        elif fault == "no_clamp":
            coef = np.float32(np.float64(np.float32(max_norm)) / (np.float64(norm) + np.float64(1e-6)))
        else:
            coef = coef_host(norm, max_norm)
    return norm, coef
