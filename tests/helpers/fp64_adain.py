"""Float64 reference of the library's AdaIN kernel (csrc/adain.hip), its bars, the value regimes its tests use, and a float32 emulation
of the kernel's arithmetic in its summation order.  Tensors are [N, HW, C] (the library's [N, 1, HW, C] with the unit axis dropped), on
any device; the emulation is numpy on the CPU.

Reference, from the stored inputs (after rounding to the storage type; split: the joined value), all float64:
  mean, unbiased variance + eps (eps as the float32 the kernel is handed), std, out = alpha * ((x - mc) / sdc * sds + ms) + (1 - alpha) * x.

Bars.  u = 2^-24.  The kernel sums d = x - k and d^2 about some per-channel number k: per lane a sequential fp32 chain of ceil(HW / 128)
terms, three xor steps in fp32, the rest in fp64: L = ceil(HW / 128) + 3 fp32 additions on the longest path.
  sum d    is off by at most (L + 1) u sum|d|          (L additions, one rounding of x - k)
  sum d^2  is off by at most (L + 2) u sum d^2         (L fused multiply-adds, two roundings of x - k)
  (HW - 1) var = sum d^2 - (sum d)^2 / HW  is then off by at most (L + 2) u S2 + 2 (L + 1) u (sum|d|)^2 / HW <= (3 L + 4) u S2 (Cauchy-
  Schwarz), S2 = sum d^2 = (HW - 1) var + HW (mean - k)^2.
What S2 is depends on k, and the bar must not: it allows any k inside the channel's own range, for which (mean - k)^2 <= max|x - mean|^2:
  |var_got - var| <= T (var + HW / (HW - 1) max|x - mean|^2),  T = 3 (L + 6) u     (= T var (1 + HW / (HW - 1) * (kappa - 1)),
                                                                                    kappa = 1 + max|x - mean|^2 / var the conditioning
                                                                                    of the channel: about 1 + 3.5^2 for Gaussian data,
                                                                                    whatever its mean; about HW with one far outlier)
  |mean_got - mean| <= (L + 6) u * 2 max|x - mean| + half an fp32 ulp        (sum|d| / HW <= mean|x - mean| + |mean - k|)
A two-pass algorithm (k = the mean) and a pivot at any pixel of the channel meet these; sums about zero do not once mean^2 / var
exceeds kappa by the few units that the worst-case count leaves (mean / std = 100: 10^4 against 13).  std is compared through its
square, std_got^2 against var + eps, with 2 u (1 + u) (var + eps) more for the fp32 rounding of std.
  out: the kernel forms x * k0 + k1 in fp32, k0 = alpha * (sds / sdc) + (1 - alpha), k1 = alpha * (ms - mc * (sds / sdc)) (alpha == 0: 1 and -0,
  the content bit for bit): 8 roundings
  of terms whose magnitudes sum to absref = alpha * ((|x| + |mc|) * sds / sdc + |ms|) + (1 - alpha) |x|, plus what the bars of the four
  statistics allow to reach the output, alpha * (|x - mc| r (rho_c + rho_s) + r E_mean_c + E_mean_s) with r = sds / sdc and rho the
  relative bar of a std, plus half an ulp of the stored type."""
import numpy as np
import torch

from helpers import fp64_conv as fc

U32 = 2.0 ** -24
APL = 128                   # pixel lanes of the kernel's work-group
REGIMES = "abcdefghi"       # channel c of a test tensor is in regime REGIMES[c % 9]; h = magnitude 1e-4, i = magnitude 1e3


def lane_chain(HW):
    return -(-HW // APL)


def chain(HW):
    """L: fp32 additions on the longest path of a channel's sum."""
    return lane_chain(HW) + 3


def f32(v):
    return float(np.float32(v))


def make(N, HW, C, seed):
    """fp32 [N, HW, C] on the CPU with the value regimes mixed across the channels (c % 9), so that one launch sees all of them:
    a ReLU-like max(0, N(0.3, 1)); b mean / std = 30; c mean / std = 100; d mean 100, std 0.01; e constant non-zero; f all zero; g = d with
    the first pixel 0; h magnitude 1e-4; i magnitude 1e3."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, HW, C, generator=g)
    x = torch.empty(N, HW, C)
    for c in range(C):
        r, zc = REGIMES[c % 9], z[:, :, c]
        if r == "a":
            v = (zc + 0.3).clamp(min=0.0)
        elif r == "b":
            v = 30.0 + zc
        elif r == "c":
            v = 100.0 + zc
        elif r in "dg":
            v = 100.0 + 0.01 * zc
            if r == "g":
                v[:, 0] = 0.0
        elif r == "e":
            v = torch.full_like(zc, 1.7 + 0.1 * c)
        elif r == "f":
            v = torch.zeros_like(zc)
        elif r == "h":
            v = 1e-4 * (zc + 0.5)
        else:
            v = 1e3 * (zc + 0.5)
        x[:, :, c] = v
    return x


def channels_of(regime, C):
    return [c for c in range(C) if REGIMES[c % 9] == regime]


def split_cpu(v):
    """The f16x2 format of csrc/common.h restated on fp32 values: (h, l) fp16 with h = fp16(c), l = fp16((c - h) * 2048), c = v clamped to
    +-65504 (NaN becomes -65504, as fminf(fmaxf(v, -65504), 65504) leaves it)."""
    v = v.float()
    c = torch.where(torch.isnan(v), torch.full_like(v, -65504.0), v.clamp(-65504.0, 65504.0))
    h = c.half()
    l = ((c - h.float()) * 2048.0).half()
    return h, l


def join_cpu(h, l):
    return h.float() + l.float() * (1.0 / 2048.0)


def split_bytes(v):
    """fp32 [..., C] (C % 8 == 0) -> the split tensor's memory as fp16 [..., C / 8, 2, 8]: every 8 channels are [8 h][8 l]."""
    h, l = split_cpu(v)
    shp = v.shape[:-1] + (v.shape[-1] // 8, 1, 8)
    return torch.cat([h.reshape(shp), l.reshape(shp)], -2)


def stats(x64, eps):
    """{mean, var, maxdev2, vpe (variance + eps), std} per (n, c) of x64 [N, HW, C]."""
    HW = x64.shape[1]
    mean = x64.mean(1)
    dev = x64 - mean[:, None, :]
    var = (dev * dev).sum(1) / (HW - 1)
    vpe = var + f32(eps)
    return {"mean": mean, "var": var, "maxdev2": (dev * dev).amax(1), "vpe": vpe, "std": vpe.sqrt(), "HW": HW}


def stat_bars(st):
    """(E_mean, E_vpe): the absolute bars of the fp32 mean and of std^2 = variance + eps; functions of HW and of the data alone."""
    HW, L = st["HW"], chain(st["HW"])
    e_mean = (L + 6) * U32 * 2.0 * st["maxdev2"].sqrt() + fc.half_ulp(st["mean"], torch.float32)
    e_vpe = 3 * (L + 6) * U32 * (st["var"] + HW / (HW - 1.0) * st["maxdev2"]) + 2 * U32 * (1 + U32) * st["vpe"]
    return e_mean, e_vpe


def kappa(st):
    """The conditioning factor 1 + max|x - mean|^2 / var of every channel (1 where the channel is constant)."""
    return 1.0 + torch.where(st["var"] > 0, st["maxdev2"] / st["var"].clamp(min=1e-300), torch.zeros_like(st["var"]))


def check_stats(got_mean, got_std, st, what):
    """got_* fp32 [N, C] against st under stat_bars(); returns (worst |mean error| / bar, worst |std^2 error| / bar, worst relative error of
    std^2)."""
    e_mean, e_vpe = stat_bars(st)
    gm, gs = got_mean.double(), got_std.double()
    assert bool(torch.isfinite(gm).all()) and bool(torch.isfinite(gs).all()), f"{what}: non-finite statistics"
    rm = (gm - st["mean"]).abs() / e_mean
    dv = (gs * gs - st["vpe"]).abs()
    rv = dv / e_vpe
    i, j = int(rm.argmax()), int(rv.argmax())
    C = gm.shape[-1]
    over = lambda r: "".join(sorted({REGIMES[c % 9] for c in (r > 1).any(0).nonzero().reshape(-1).tolist()}))
    assert float(rm.max()) <= 1, f"{what}: mean of (n, c) = ({i // C}, {i % C}) [regime {REGIMES[i % C % 9]}] off by {float(rm.max()):.3g} bars: got " \
                                 f"{float(gm.reshape(-1)[i]):.9g}, ref {float(st['mean'].reshape(-1)[i]):.9g}; regimes over the bar: {over(rm)}"
    assert float(rv.max()) <= 1, f"{what}: std^2 of (n, c) = ({j // C}, {j % C}) [regime {REGIMES[j % C % 9]}] off by {float(rv.max()):.3g} bars: got " \
                                 f"{float((gs * gs).reshape(-1)[j]):.9g}, ref {float(st['vpe'].reshape(-1)[j]):.9g} (relative error " \
                                 f"{float((dv / st['vpe']).reshape(-1)[j]):.3g}, kappa {float(kappa(st).reshape(-1)[j]):.3g}); regimes over the bar: {over(rv)}"
    return float(rm.max()), float(rv.max()), float((dv / st["vpe"]).max())


def out_ref(x64, sc, ss, alpha):
    """(ref, absref, extra): the output in float64, the magnitudes of the kernel's terms, and what the statistics' bars let through."""
    a = f32(alpha)
    mc, ms = sc["mean"][:, None, :], ss["mean"][:, None, :]
    r = (ss["std"] / sc["std"])[:, None, :]
    ref = a * ((x64 - mc) * r + ms) + (1.0 - a) * x64
    absref = abs(a) * ((x64.abs() + mc.abs()) * r + ms.abs()) + abs(1.0 - a) * x64.abs()
    emc, evc = stat_bars(sc)
    ems, evs = stat_bars(ss)
    rho = lambda ev, st: (ev / (2 * st["vpe"])) * (1 + ev / st["vpe"])
    extra = abs(a) * ((x64 - mc).abs() * r * (rho(evc, sc) + rho(evs, ss))[:, None, :] + r * emc[:, None, :] + ems[:, None, :])
    return ref, absref, extra


TAU_OUT = 8 * U32
MAXVAL = {torch.bfloat16: 3.3e38, torch.float16: 65504.0, torch.float32: 3.4e38, "split": 65504.0}


def check_out(got, ref, absref, extra, dtype, what):
    """|got - ref| <= TAU_OUT * absref + extra + half an ulp of the stored type, and finite wherever the reference (plus its bar) is
    inside the type's range.  Returns (measured tau over absref after the ulp and `extra` are taken off, worst error / bar)."""
    g = got.double()
    bar0 = TAU_OUT * absref + extra
    inside = ref.abs() + bar0 < MAXVAL[dtype]
    bad = inside & ~torch.isfinite(g)
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: non-finite output at {fc.locate(got.shape, i)} where the reference is {float(ref.reshape(-1)[i]):.6g}")
    hu = torch.maximum(fc.half_ulp(ref, dtype), fc.half_ulp(torch.where(inside, g, ref), dtype))
    err = torch.where(inside, (g - ref).abs(), torch.zeros_like(ref))
    ratio = err / (bar0 + hu)
    i = int(ratio.argmax())
    t_meas = float(((err - hu - extra).clamp(min=0) / absref.clamp(min=1e-300)).max())
    if float(ratio.max()) > 1:
        C = got.shape[-1]
        raise AssertionError(f"{what}: |got - ref| = {float(err.reshape(-1)[i]):.4g} > bar {float((bar0 + hu).reshape(-1)[i]):.4g} (got "
                             f"{float(g.reshape(-1)[i]):.8g}, ref {float(ref.reshape(-1)[i]):.8g}, absref {float(absref.reshape(-1)[i]):.4g}, from the "
                             f"statistics {float(extra.reshape(-1)[i]):.4g}) at {fc.locate(got.shape, i)} [regime {REGIMES[i % C % 9]}]")
    return t_meas, float(ratio.max())


# ---- the kernel's arithmetic in fp32 numpy ------------------------------------------------------------------------------------------

def emulate_sums(x, pivot):
    """x fp32 numpy [HW, C] -> (k, s1, s2) float64 [C]: the sums of d = x - k and d^2 in the kernel's order - 128 lanes, each sequential in
    fp32 over pixels lane, lane + 128, ... with a fused multiply-add for the square; three xor steps in fp32 over the 8 lanes of a wave
    that hold one channel; the 16 waves in fp64.  pivot: True = the channel's first pixel (the kernel), False = 0 (the one-pass formula)."""
    HW, C = x.shape
    x = x.astype(np.float32)
    k = x[0].copy() if pivot else np.zeros(C, np.float32)
    n = lane_chain(HW) * APL
    xp = np.zeros((n, C), np.float32)
    xp[:HW] = x
    live = (np.arange(n) < HW).reshape(-1, APL, 1)
    xp = xp.reshape(-1, APL, C)
    s1, s2 = np.zeros((APL, C), np.float32), np.zeros((APL, C), np.float32)
    for j in range(xp.shape[0]):
        d = (xp[j] - k).astype(np.float32)
        n1 = (s1 + d).astype(np.float32)
        n2 = (s2.astype(np.float64) + d.astype(np.float64) * d.astype(np.float64)).astype(np.float32)        # fma: one rounding
        s1, s2 = np.where(live[j], n1, s1), np.where(live[j], n2, s2)
    lane = np.arange(APL)
    for o in (1, 2, 4):                 # thread bits 3..5 = pixel-lane bits 0..2
        s1, s2 = (s1 + s1[lane ^ o]).astype(np.float32), (s2 + s2[lane ^ o]).astype(np.float32)
    a1, a2 = np.zeros(C), np.zeros(C)
    for w in range(APL // 8):
        a1, a2 = a1 + s1[8 * w].astype(np.float64), a2 + s2[8 * w].astype(np.float64)
    return k.astype(np.float64), a1, a2


def emulate_stats(x, eps, pivot):
    """(mean fp32, std fp32, variance + eps before the clamp) of x fp32 numpy [HW, C] as the kernel's first 64 threads form them."""
    HW = x.shape[0]
    k, a1, a2 = emulate_sums(x, pivot)
    d = a1 / HW
    v = (a2 - a1 * d) / (HW - 1) + float(np.float32(eps))
    return (k + d).astype(np.float32), np.sqrt(np.maximum(v, 0.0)).astype(np.float32), v


def emulate_out(x, mc, sdc, ms, sds, alpha):
    """x * k0 + k1 in fp32 (fused) from the fp32 statistics."""
    a = np.float32(alpha)
    if a == 0:          # (the kernel's alpha == 0 form: coefficients 1 and -0)
        return x.astype(np.float32).copy()
    with np.errstate(all="ignore"):
        r = (sds / sdc).astype(np.float32)
        k0 = (a * r).astype(np.float32) + (np.float32(1) - a)
        k1 = (a * (ms - (mc * r).astype(np.float32)).astype(np.float32)).astype(np.float32)
        return (x.astype(np.float64) * k0.astype(np.float64) + k1.astype(np.float64)).astype(np.float32)
