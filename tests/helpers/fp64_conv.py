"""Float64 reference of the library's convolutions, and the per-element / whole-tensor checker the convolution tests use.

Layouts are the library's: activations NHWC; weights in the "physical" layout [A][taps][B] the weight gradient uses - [Co][taps][Ci]
for a convolution, [Ci][taps][Co] for a transposed one - with taps = KH * KWp (the Ci == 8 stem pads its 7 filter columns to 8, so
its weight gradient has an 8th column tap that is a real correlation, and its forward weight is zero there).  Every op returns
(ref, absref): the op on the operands, and the same op on |operands|, both float64 on the operands' device.

The ops are tap loops: for every filter tap, a gather of input pixels (zero / reflection padding, nearest x2 upsample folded into the
index) and one float64 matmul.  A transposed convolution is the adjoint of the direct convolution from its output back to its input,
so its three faces are the direct ones with the roles of forward and data gradient swapped.

check(): |got - ref| <= tau * absref + ulp_out(|got|, |ref|) / 2 for every element (a local fault: one wrong tile, one border
column), and ||got - ref||_2 <= rho * ||ref||_2 + the expected output-rounding norm (a thin, spread fault: one dropped 64-pixel stage
of a weight-gradient reduction).  A failure names the worst element and the m-tile / n-tile it lies in."""
from dataclasses import dataclass

import torch

MANT = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24, torch.float64: 53}
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126, torch.float64: -1022}
# "split": the f16x2 storage h + l * 2^-11 (two fp16 numbers) read back as fp32: l = fp16((v - h) * 2^11) is off by at most 2^(e - 23) of v = m * 2^e,
# and the fp32 join h + l * 2^-11 rounds once more (2^(e - 24)): within half an ulp of a 22-bit significand; l's subnormal spacing 2^-24 scaled by 2^-11
# gives the floor 2^-36
MANT["split"] = 22
MIN_EXP["split"] = -14


@dataclass(frozen=True)
class Geom:
    N: int
    Hi: int
    Wi: int
    Ci: int
    Co: int
    KH: int
    KW: int
    stride: int = 1
    pad: int = 0
    transposed: bool = False
    reflect: bool = False
    upsample: bool = False

    @property
    def kwp(self):
        return (self.KW + 7) // 8 * 8 if self.Ci == 8 else self.KW

    @property
    def taps(self):
        return self.KH * self.kwp

    @property
    def Ho(self):
        if self.transposed:
            return (self.Hi - 1) * self.stride - 2 * self.pad + self.KH
        return ((self.Hi << int(self.upsample)) + 2 * self.pad - self.KH) // self.stride + 1

    @property
    def Wo(self):
        if self.transposed:
            return (self.Wi - 1) * self.stride - 2 * self.pad + self.KW
        return ((self.Wi << int(self.upsample)) + 2 * self.pad - self.KW) // self.stride + 1

    def direct(self):
        """The direct convolution whose data gradient is this transposed one: from (Ho, Wo, Co) to (Hi, Wi, Ci)."""
        assert self.transposed and not self.reflect and not self.upsample
        return Geom(self.N, self.Ho, self.Wo, self.Co, self.Ci, self.KH, self.KW, self.stride, self.pad)


def geom_of(d):
    """Geom of an ops.conv_desc descriptor."""
    return Geom(d.N, d.Hi, d.Wi, d.Ci, d.Co, d.KH, d.KW, d.stride, d.pad, bool(d.transposed), bool(d.reflect), bool(d.upsample))


def phys_weight(w, g):
    """torch-layout weight ([Co, Ci, KH, KW]; transposed: [Ci, Co, KH, KW]) -> float64 [A][KH * KWp][B] (stem: channels and filter
    columns zero-padded to 8)."""
    w = w.detach().double()
    if g.Ci == 8 and not g.transposed:
        wp = torch.zeros(w.shape[0], 8, g.KH, g.kwp, dtype=torch.float64, device=w.device)
        wp[:, :w.shape[1], :, :g.KW] = w
        w = wp
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], g.taps, w.shape[1]).contiguous()


def _axis_index(n_out, n_in, stride, off, reflect, upsample, device):
    """Input index along one axis for output positions 0..n_out-1 at tap offset `off`, or -1 (zero padding)."""
    i = torch.arange(n_out, device=device) * stride + off
    if reflect:
        L = n_in << int(upsample)
        i = torch.where(i < 0, -i, i)
        i = torch.where(i >= L, 2 * (L - 1) - i, i)
        return i >> int(upsample)
    if upsample:
        L = n_in << 1
        return torch.where((i >= 0) & (i < L), i >> 1, torch.full_like(i, -1))
    return torch.where((i >= 0) & (i < n_in), i, torch.full_like(i, -1))


def _gather_plan(g, device):
    """[(tap, flat input pixel index [Ho*Wo], valid mask)] of a direct convolution."""
    out = []
    for kh in range(g.KH):
        ih = _axis_index(g.Ho, g.Hi, g.stride, kh - g.pad, g.reflect, g.upsample, device)
        for kw in range(g.kwp):
            iw = _axis_index(g.Wo, g.Wi, g.stride, kw - g.pad, g.reflect, g.upsample, device)
            ok = (ih[:, None] >= 0) & (iw[None, :] >= 0)
            idx = (ih.clamp(min=0)[:, None] * g.Wi + iw.clamp(min=0)[None, :]).reshape(-1)
            out.append((kh * g.kwp + kw, idx, ok.reshape(-1)))
    return out


def _fprop_direct(g, x, w):
    N = x.shape[0]
    X = x.double().reshape(N, g.Hi * g.Wi, g.Ci)
    W = w.double()
    y = torch.zeros(N, g.Ho * g.Wo, g.Co, dtype=torch.float64, device=x.device)
    for t, idx, ok in _gather_plan(g, x.device):
        if not bool(ok.any()):
            continue
        xg = X[:, idx] * ok[None, :, None]
        y += xg @ W[:, t, :].T
    return y.reshape(N, g.Ho, g.Wo, g.Co)


def _dgrad_direct(g, dy, w):
    N = dy.shape[0]
    D = dy.double().reshape(N, g.Ho * g.Wo, g.Co)
    W = w.double()
    dx = torch.zeros(N, g.Hi * g.Wi, g.Ci, dtype=torch.float64, device=dy.device)
    for t, idx, ok in _gather_plan(g, dy.device):
        if not bool(ok.any()):
            continue
        dx.index_add_(1, idx[ok], (D[:, ok] @ W[:, t, :]))
    return dx.reshape(N, g.Hi, g.Wi, g.Ci)


def _wgrad_direct(g, dy, x):
    N = x.shape[0]
    X = x.double().reshape(N, g.Hi * g.Wi, g.Ci)
    D = dy.double().reshape(N * g.Ho * g.Wo, g.Co)
    dw = torch.zeros(g.Co, g.taps, g.Ci, dtype=torch.float64, device=x.device)
    for t, idx, ok in _gather_plan(g, x.device):
        if not bool(ok.any()):
            continue
        xg = (X[:, idx] * ok[None, :, None]).reshape(N * g.Ho * g.Wo, g.Ci)
        dw[:, t, :] = D.T @ xg
    return dw


def _fprop(g, x, w):
    return _dgrad_direct(g.direct(), x, w) if g.transposed else _fprop_direct(g, x, w)


def _dgrad(g, dy, w):
    return _fprop_direct(g.direct(), dy, w) if g.transposed else _dgrad_direct(g, dy, w)


def _wgrad(g, dy, x):
    return _wgrad_direct(g.direct(), x, dy) if g.transposed else _wgrad_direct(g, dy, x)


def fprop(g, x, w):
    """y = conv(x, w): x NHWC [N, Hi, Wi, Ci], w physical [A][taps][B] -> (ref, absref) NHWC [N, Ho, Wo, Co]."""
    return _fprop(g, x, w), _fprop(g, x.double().abs(), w.double().abs())


def dgrad(g, dy, w):
    """dx = conv^T(dy, w): dy NHWC [N, Ho, Wo, Co] -> (ref, absref) NHWC [N, Hi, Wi, Ci]."""
    return _dgrad(g, dy, w), _dgrad(g, dy.double().abs(), w.double().abs())


def wgrad(g, dy, x):
    """dW = sum over pixels of dy (x) x: -> (ref, absref) in the physical weight layout ([Co][taps][Ci]; transposed [Ci][taps][Co])."""
    return _wgrad(g, dy, x), _wgrad(g, dy.double().abs(), x.double().abs())


def half_ulp(v, dtype):
    """Half a unit in the last place of |v| (float64) in `dtype`, subnormals included."""
    a = v.double().abs()
    e = torch.frexp(a)[1].to(torch.float64) - 1                 # a = m * 2^e, 1 <= m < 2
    e = torch.where(a > 0, e, torch.full_like(e, MIN_EXP[dtype])).clamp(min=MIN_EXP[dtype])
    return torch.pow(2.0, e - (MANT[dtype] - 1)) * 0.5


def locate(shape, flat, bm=(64, 128), bn=64):
    """Coordinates of flat element `flat` of a tensor of `shape`, and the m-tile / n-tile it lies in (rows m = all leading dimensions
    flattened, as the implicit GEMM numbers output pixels; columns = the last dimension)."""
    coords, r = [], int(flat)
    for s in reversed(shape):
        coords.append(r % s)
        r //= s
    coords = tuple(reversed(coords))
    m, c = int(flat) // shape[-1], coords[-1]
    tiles = ", ".join(f"m-tile {m // b} of {b} rows" for b in bm)
    return f"element {coords} (row m = {m}, column {c}): {tiles}, n-tile {c // bn} of {bn} columns"


def measure(got, ref, absref, out_dtype):
    """(tau_measured, rho_measured): the smallest tau and rho the element and whole-tensor conditions of check() would pass with."""
    got, ref, absref = got.double(), ref.double(), absref.double()
    err = (got - ref).abs()
    hu = torch.maximum(half_ulp(ref, out_dtype), half_ulp(got, out_dtype))
    over = (err - hu).clamp(min=0) / absref.clamp(min=1e-300)
    tau = float(over.max()) if over.numel() else 0.0
    rnorm = float(ref.norm()) or 1e-300
    rho = max(float(err.norm()) - _rounding_norm(hu), 0.0) / rnorm
    return tau, rho


def _rounding_norm(hu):
    # expected L2 norm of round-to-nearest errors (uniform in +-ulp/2: rms = (ulp/2) / sqrt(3)), with a margin that the fluctuation of a
    # sum of many independent squares needs; small tensors get the worst case
    n = hu.numel()
    return float(hu.norm()) * (0.75 if n >= 4096 else 1.0)


def check(got, ref, absref, out_dtype, tau, rho, what="", bm=(64, 128), bn=64):
    """Assert |got - ref| <= tau * absref + ulp_out/2 everywhere and ||got - ref|| <= rho * ||ref|| + the output rounding's norm.
    out_dtype: the type `got` was stored in (bf16 / fp16 outputs carry one rounding of the fp32 accumulator).  Returns the measured
    (tau, rho).  Raises AssertionError naming the worst element and its tiles."""
    assert got.shape == ref.shape == absref.shape, (what, tuple(got.shape), tuple(ref.shape))
    g64, r64, a64 = got.double(), ref.double(), absref.double()
    if not bool(torch.isfinite(g64).all()):
        bad = int((~torch.isfinite(g64)).reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: non-finite output at {locate(got.shape, bad, bm, bn)}")
    err = (g64 - r64).abs()
    hu = torch.maximum(half_ulp(r64, out_dtype), half_ulp(g64, out_dtype))
    slack = err - (tau * a64 + hu)
    worst = int(slack.reshape(-1).argmax())
    t_meas, r_meas = measure(got, ref, absref, out_dtype)
    if float(slack.reshape(-1)[worst]) > 0:
        raise AssertionError(f"{what}: |got - ref| = {float(err.reshape(-1)[worst]):.4g} > tau * absref + ulp/2 = "
                             f"{float((tau * a64 + hu).reshape(-1)[worst]):.4g} (got {float(g64.reshape(-1)[worst]):.6g}, ref "
                             f"{float(r64.reshape(-1)[worst]):.6g}, absref {float(a64.reshape(-1)[worst]):.4g}, tau {tau:g}; measured tau "
                             f"{t_meas:.3g}) at {locate(got.shape, worst, bm, bn)}")
    bar = rho * float(r64.norm()) + _rounding_norm(hu)
    if float(err.norm()) > bar:
        worst = int(err.reshape(-1).argmax())
        raise AssertionError(f"{what}: ||got - ref|| / ||ref|| = {float(err.norm()) / (float(r64.norm()) or 1e-300):.4g} exceeds rho {rho:g} "
                             f"+ the output rounding (measured rho {r_meas:.3g}); largest error {float(err.reshape(-1)[worst]):.4g} at "
                             f"{locate(got.shape, worst, bm, bn)}")
    return t_meas, r_meas


# Bars per operand kind and op: (tau, rho).  "16bit": bf16 / fp16 operands (products exact in fp32) accumulated in fp32; "f32": the exact
# fp32 MFMA path; "split": f16x2 operands (h + l * 2^-11, three fp16 MFMAs per K step).  Each bar is about 4x the worst value measured on an
# MI355X over tests/test_gpu_conv_forms.py (every forced form at small ragged shapes and every benchmarked geometry, both 16-bit builds):
#   16bit fprop tau 1.07e-7 rho 2.56e-7 | 16bit dgrad tau 1.17e-7 rho 1.77e-7 | 16bit wgrad tau 1.57e-7 rho 5.45e-7
#   f32 fprop tau 4.58e-7 rho 1.53e-6   | split fprop tau 2.39e-7 rho 5.28e-7
# (fp32 unit roundoff is 6e-8: the f16x2 forward is fp32-grade - within the exact fp32 path's own bars - as DESIGN.md states.)
BOUNDS = {
    ("16bit", "fprop"): (5e-7, 1e-6),
    ("16bit", "dgrad"): (5e-7, 1e-6),
    ("16bit", "wgrad"): (6e-7, 2e-6),
    ("f32", "fprop"): (2e-6, 6e-6),
    ("split", "fprop"): (1e-6, 2e-6),
}
