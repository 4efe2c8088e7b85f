"""Float64 references of the library's training-mode BatchNorm and max-pool kernels, on the operands' device, in the library's layout
(activations [..., C] with the channel last; statistics slabs [rows][2][C]).  Every op returns (ref, absref) - the op on the operands and
the sum of the magnitudes of its terms - so that helpers.fp64_conv.check() and half_ulp() serve them unchanged.

The references take what the kernel is handed, not what an ideal layer would see: finalize() sums the slab's own fp32 entries, apply()
uses the device's own fp32 scale and shift, backward() the saved fp32 mean and invstd.  Each kernel is then held to its own rounding.

Bars: tau = (L + 6) * 2^-24 per element (tau_of), L = the longest sequential fp32 accumulation chain of the form (0 where the sums are
fp64), 6 = the handful of fp32 operations around it; rho is the same constant.  Finalize outputs are compared in fp32 ulps (check_ulps).
A sequential fp32 sum of L terms is off by at most L * 2^-24 of the sum of magnitudes, so a correct kernel cannot exceed these."""
import torch

from helpers import fp64_conv as fc

U32 = 2.0 ** -24


def tau_of(L):
    return (L + 6) * U32


def stream_chain(npix, C):
    """L of bn_bwd_reduce_k: ceil(ppb / pstep) additions per thread, then pstep LDS rows added by one thread."""
    pstep = 256 // (C // 8)
    rows = max(1, min(1024, -(-npix // pstep)))
    ppb = -(-npix // rows)
    return -(-ppb // pstep) + pstep


def chunk_P(npix, C, target=1024):
    """Pixels per work-group of the channel-chunked forms (policy value `target` work-groups; 1 = 1024)."""
    S = max(1, min(64, (target if target > 1 else 1024) // (C // 64)))
    return (-(-npix // S) + 31) // 32 * 32


def chunk_chain(npix, C):
    """L of bn_bwd_reduce_chunk_k: P / 32 additions per thread, then 32 LDS rows."""
    return chunk_P(npix, C) // 32 + 32


def ulp32(mag):
    return 2.0 * fc.half_ulp(mag, torch.float32)


def check_ulps(got, ref, mag, n, what):
    """|got - ref| <= n ulps (fp32) of `mag` (the value, or the sum of its terms' magnitudes), per channel; returns the worst, in ulps."""
    g64 = got.double()
    assert bool(torch.isfinite(g64).all()), f"{what}: non-finite"
    u = (g64 - ref).abs() / ulp32(torch.maximum(mag.double().abs(), ref.abs()))
    worst = float(u.max())
    assert worst <= n, f"{what}: {worst:.3g} ulps at channel {int(u.argmax())} (bar {n}): got {float(g64.reshape(-1)[u.argmax()]):.9g}, ref " \
                       f"{float(ref.reshape(-1)[u.argmax()]):.9g}"
    return worst


# ---- forward ---------------------------------------------------------------------------------------------------------------------

def finalize(slab, count, gamma, beta, pre_bias=None, momentum=0.1, eps=1e-5, running_mean=None, running_var=None):
    """slab fp32 [rows][2][C] -> {name: (ref, mag)}: mean, invstd, scale, shift, unbiased variance, running statistics.  var < 0 is
    clamped and count == 1 leaves the variance biased, as the kernel does; momentum and eps are taken as the fp32 values the kernel gets."""
    s = slab.double().sum(0)
    mean = s[0] / count
    var = (s[1] / count - mean * mean).clamp(min=0.0)
    mmag = mean.abs()
    if pre_bias is not None:
        mean = mean + pre_bias.double()
        mmag = mmag + pre_bias.double().abs()
    eps = float(torch.tensor(eps, dtype=torch.float32))
    m = float(torch.tensor(momentum, dtype=torch.float32))
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    unb = var * count / (count - 1.0) if count > 1 else var
    out = {"mean": (mean, mmag), "invstd": (invstd, invstd), "scale": (scale, scale.abs()),
           "shift": (shift, beta.double().abs() + (mean * scale).abs()), "unbiased_var": (unb, unb)}
    if running_mean is not None:
        rm, rv = running_mean.double(), running_var.double()
        out["running_mean"] = ((1 - m) * rm + m * mean, ((1 - m) * rm).abs() + (m * mean).abs())
        out["running_var"] = ((1 - m) * rv + m * unb, ((1 - m) * rv).abs() + (m * unb).abs())
    return out


def apply(y, scale, shift, res=None, relu=False):
    """relu?(y * scale + shift [+ res]) on the given scale / shift; absref = |y * scale| + |shift| + |res|."""
    t = y.double() * scale.double()
    ref, absref = t + shift.double(), t.abs() + shift.double().abs()
    if res is not None:
        ref, absref = ref + res.double(), absref + res.double().abs()
    return (torch.relu(ref) if relu else ref), absref


def mask_bits(mask, C):
    """bit mask [npix * C / 8] bytes (bit e of byte i: channel 8 * (i % (C / 8)) + e) -> bool [npix, C]."""
    b = (mask.reshape(-1, 1).to(torch.int32) >> torch.arange(8, device=mask.device, dtype=torch.int32)) & 1
    return b.reshape(-1, C).bool()


def split_h(z):
    """The h halves of a split tensor [npix, C] (int32 storage: 32 bytes per 8 channels = [8 h][8 l]) as fp16 [npix, C]."""
    npix, C = z.shape
    return z.view(torch.float16).reshape(npix, C // 8, 2, 8)[:, :, 0, :].reshape(npix, C)


# ---- backward --------------------------------------------------------------------------------------------------------------------

def relu_mask_from_y(y, mean, invstd, gamma, beta, gout=None):
    """The relu == 2 mask: y * sc + sh > 0 with sc = gamma * invstd, sh = beta - mean * sc, from the fp32 parameters in fp64.  An element is
    undecided when |pre64| <= 8 * 2^-24 * (|y * sc| + |beta| + |mean * sc|) - an fp32 evaluation may land on either side; there the
    device's own decision is read from gout (dz has no zeros).  Returns (keep, number undecided)."""
    sc = gamma.double() * invstd.double()
    t, ms = y.double() * sc, mean.double() * sc
    pre = t + (beta.double() - ms)
    keep = pre > 0
    und = pre.abs() <= 8 * U32 * (t.abs() + beta.double().abs() + ms.abs())
    und &= pre != 0           # (a planted exact zero - every intermediate exact in fp32 as well - is decided: the test is strictly > 0)
    n = int(und.sum())
    if n and gout is not None:
        keep = torch.where(und, gout.double() != 0, keep)
    return keep, n


def backward(dz, y, mean, invstd, gamma, keep=None):
    """g = dz where keep (all of it when keep is None), S1 = sum g, S2 = sum g * xhat, dy = ca * (g - S1 / M - xhat * S2 / M) with
    xhat = (y - mean) * invstd, ca = gamma * invstd.  Returns {"g": g, "dy": (ref, absref), "dbeta": (S1, A1), "dgamma": (S2, A2)} with
    the absolute sums A1 = sum |g|, A2 = sum |g * xhat|: the error of the sums is relative to these, not to S1, S2, which cancel."""
    y64 = y.double().reshape(-1, y.shape[-1])
    g = dz.double().reshape(y64.shape)
    if keep is not None:
        g = torch.where(keep.reshape(y64.shape), g, torch.zeros_like(g))
    M = y64.shape[0]
    xhat = (y64 - mean.double()) * invstd.double()
    S1, S2, A1, A2 = g.sum(0), (g * xhat).sum(0), g.abs().sum(0), (g * xhat).abs().sum(0)
    ca = gamma.double() * invstd.double()
    dy = ca * (g - S1 / M - xhat * S2 / M)
    absref = ca.abs() * (g.abs() + A1 / M + xhat.abs() * A2 / M)
    return {"g": g, "xhat": xhat, "dy": (dy, absref), "dbeta": (S1, A1), "dgamma": (S2, A2)}


def backward_pre(g, y, mean, invstd, gamma, slab):
    """The pre-reduced form: g already masked, the sums are those of the given fp32 slab [rows][2][C] (fp64 in the kernel: L = 0)."""
    y64 = y.double().reshape(-1, y.shape[-1])
    g64 = g.double().reshape(y64.shape)
    M = y64.shape[0]
    s, a = slab.double().sum(0), slab.double().abs().sum(0)
    xhat = (y64 - mean.double()) * invstd.double()
    ca = gamma.double() * invstd.double()
    dy = ca * (g64 - s[0] / M - xhat * s[1] / M)
    absref = ca.abs() * (g64.abs() + s[0].abs() / M + xhat.abs() * s[1].abs() / M)
    return {"dy": (dy, absref), "dbeta": (s[0], a[0]), "dgamma": (s[1], a[1])}


# ---- max-pool --------------------------------------------------------------------------------------------------------------------

def _pool_fwd(x, K, stride, pad, Ho, Wo):
    """Value and winning tap (kh * K + kw) of every window: the first in-range tap, then `v > best or isnan(v)` in (kh, kw) scan order -
    torch's rule: the first maximum wins, a NaN wins over everything before it and is only displaced by a later NaN."""
    N, H, W, C = x.shape
    x = x.double()
    dev = x.device
    best = torch.full((N, Ho, Wo, C), float("-inf"), dtype=torch.float64, device=dev)
    idx = torch.zeros((N, Ho, Wo, C), dtype=torch.int64, device=dev)
    seen = torch.zeros((1, Ho, Wo, 1), dtype=torch.bool, device=dev)
    for kh in range(K):
        h = torch.arange(Ho, device=dev) * stride - pad + kh
        for kw in range(K):
            w = torch.arange(Wo, device=dev) * stride - pad + kw
            ok = ((h >= 0) & (h < H))[:, None] & ((w >= 0) & (w < W))[None, :]
            v = x[:, h.clamp(0, H - 1)][:, :, w.clamp(0, W - 1)]
            ok4 = ok[None, :, :, None]
            take = ok4 & (~seen | (v > best) | torch.isnan(v))
            best = torch.where(take, v, best)
            idx = torch.where(take, torch.full_like(idx, kh * K + kw), idx)
            seen = seen | ok4
    return best, idx


def maxpool3x3s2(x):
    """3x3 / stride 2 / pad 1 on NHWC: (value, tap 0..8)."""
    H, W = x.shape[1:3]
    return _pool_fwd(x, 3, 2, 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1)


def maxpool2x2_ceil(x):
    """2x2 / stride 2 / ceil mode on NHWC: (value, tap 0..3)."""
    H, W = x.shape[1:3]
    return _pool_fwd(x, 2, 2, 0, (H + 1) // 2, (W + 1) // 2)


def _pool_bwd(dy, idx, K, stride, pad, H, W):
    N, Ho, Wo, C = dy.shape
    d = dy.double()
    dev = d.device
    dx = torch.zeros(2, N, H * W, C, dtype=torch.float64, device=dev)
    for kh in range(K):
        h = torch.arange(Ho, device=dev) * stride - pad + kh
        for kw in range(K):
            w = torch.arange(Wo, device=dev) * stride - pad + kw
            ok = ((h >= 0) & (h < H))[:, None] & ((w >= 0) & (w < W))[None, :]
            pix = (h.clamp(0, H - 1)[:, None] * W + w.clamp(0, W - 1)[None, :]).reshape(-1)
            c = torch.where((idx == kh * K + kw) & ok[None, :, :, None], d, torch.zeros_like(d)).reshape(N, Ho * Wo, C)
            dx[0].index_add_(1, pix, c)
            dx[1].index_add_(1, pix, c.abs())
    return dx[0].reshape(N, H, W, C), dx[1].reshape(N, H, W, C)


def maxpool3x3s2_bwd(dy, idx, H, W):
    """Every output's gradient to its winning tap: the fp64 sum of the <= 4 windows that contain a pixel -> (ref, absref)."""
    return _pool_bwd(dy, idx, 3, 2, 1, H, W)


def maxpool2x2_ceil_bwd(x, dy, relu_mask=False):
    """Gradient of maxpool2x2_ceil at x (winning taps recomputed from x), optionally times the producer's ReLU mask x > 0."""
    H, W = x.shape[1:3]
    _, idx = maxpool2x2_ceil(x)
    ref, absref = _pool_bwd(dy, idx, 2, 2, 0, H, W)
    if relu_mask:
        keep = x.double() > 0
        ref, absref = torch.where(keep, ref, torch.zeros_like(ref)), torch.where(keep, absref, torch.zeros_like(absref))
    return ref, absref


def check_exact(got, ref, what):
    """got == ref element for element, a NaN matching only a NaN (values of a max-pool, winning taps, masks, shadows)."""
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    g, r = got.double(), ref.double()
    bad = ~((g == r) | (torch.isnan(g) & torch.isnan(r)))
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {fc.locate(got.shape, i)}: got "
                             f"{float(g.reshape(-1)[i])!r}, expected {float(r.reshape(-1)[i])!r}")


def check_sums(got, ref, absref, tau, what):
    """Per-channel sums (dbeta, dgamma): |got - ref| <= tau * absref + half an fp32 ulp, absref = the sum of magnitudes.  No whole-vector
    condition relative to ||ref||: the sums cancel, their error does not.  Returns (measured tau, 0)."""
    g, r, a = got.double(), ref.double(), absref.double()
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite"
    hu = torch.maximum(fc.half_ulp(r, torch.float32), fc.half_ulp(g, torch.float32))
    err = (g - r).abs()
    slack = err - (tau * a + hu)
    t_meas = float(((err - hu).clamp(min=0) / a.clamp(min=1e-300)).max())
    c = int(slack.argmax())
    assert float(slack[c]) <= 0, f"{what}: channel {c}: |got - ref| = {float(err[c]):.4g} > tau * sum|.| + ulp/2 = {float((tau * a + hu)[c]):.4g} " \
                                 f"(got {float(g[c]):.8g}, ref {float(r[c]):.8g}, sum|.| {float(a[c]):.4g}; measured tau {t_meas:.3g}, bar {tau:.3g})"
    return t_meas, 0.0
