"""Fourier Domain Adaptation (Yang & Soatto, CVPR 2020) as a style network without weights (csrc/fda.hip; no counterpart in the reference).

The content image keeps its phase and takes the style image's amplitude on the lowest spatial frequencies, |u|, |v| <= b with
b = floor(min(H, W) * beta).  Only that window changes, so no FFT is taken: (2b+1) x (b+1) direct DFT coefficients per image plane and a
synthesis of the same rank,

    out = content + IDFT2(dF),   dF = alpha * (A_style - A_content) * F_content / |F_content|   on the window, zero elsewhere.

`FDANet` is a drop-in for `Style_net.Net` as the training loop uses it (train_human.py:345-358): `style_net(content, style, alpha, clamp=...)[2]`
is the transferred batch; `MeanTeacherTrainer(style_net=FDANet(...))` and `GraphedTrainStep` take each batch's spectrum once per step and run one
apply launch per direction.  fp32 NCHW in and out, sample i pairs with sample i, no autograd (the loop runs the transfer under no_grad).

With `mean` / `std` the tensors are taken as normalised images (raw - mean_c) / std_c and the transfer is FDA of the RAW images, expressed in
normalised units: normalisation changes only the DC coefficient's sign and amplitude, so only that coefficient is treated differently."""
import math

import torch
import torch.nn as nn

from ... import _hip
from ..._hip import check, lib, ptr

MAX_B = 63          # UDAPOSE_FDA_MAX_B (include/udapose.h)
MAX_DIM = 4096      # UDAPOSE_FDA_MAX_DIM


def window(H, W, beta):
    """b: the half-width of the swapped block of coefficients."""
    return int(math.floor(min(H, W) * beta))


def _image(t, what):
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor, got {type(t).__name__}")
    _hip.require_cuda(t)
    if t.dim() != 4:
        raise ValueError(f"{what} must be NCHW, got {t.dim()} dimensions")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {t.dtype} (16-bit images are out of scope: cast them)")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous NCHW")
    return t


def _check_window(H, W, b):
    if b < 0 or 2 * b + 1 > min(H, W):
        raise ValueError(f"window b = {b} does not fit a {H} x {W} image: 0 <= b and 2 b + 1 <= min(H, W) (the window must not reach the Nyquist row)")
    if b > MAX_B or H > MAX_DIM or W > MAX_DIM:
        raise NotImplementedError(f"window b = {b} on {H} x {W}: the kernels hold b <= {MAX_B} and H, W <= {MAX_DIM}")


def _spec_real(spec, N, C, b, what):
    """[N, C, 2b+1, b+1, 2] fp32 view of a spectrum given as complex64 [N, C, 2b+1, b+1] or as that real tensor."""
    if not torch.is_tensor(spec):
        raise TypeError(f"{what} must be a tensor")
    _hip.require_cuda(spec)
    s = torch.view_as_real(spec) if spec.is_complex() else spec
    if s.dtype != torch.float32 or tuple(s.shape) != (N, C, 2 * b + 1, b + 1, 2) or not s.is_contiguous():
        raise ValueError(f"{what} must be a contiguous complex64 [{N}, {C}, {2 * b + 1}, {b + 1}] spectrum (low_freq_spectrum), got "
                         f"{spec.dtype} {tuple(spec.shape)}")
    return s


def _per_channel(v, C, dev, what):
    if v is None:
        return None
    t = torch.as_tensor(v, dtype=torch.float32).detach().reshape(-1)
    if t.numel() != C:
        raise ValueError(f"{what} must have one value per channel ({C}), got {t.numel()}")
    return t.to(dev).contiguous()


def low_freq_spectrum(x, b, out=None):
    """complex64 [N, C, 2b+1, b+1]: G[u, v] = sum_y sum_x x[y, x] exp(-2 pi i (u y / H + v x / W)) at row u + b (u = -b .. b), column v = 0 .. b."""
    x = _image(x, "x")
    N, C, H, W = x.shape
    b = int(b)
    _check_window(H, W, b)
    if N * C == 0:
        raise ValueError("x has no planes")
    if out is None:
        out = torch.empty(N, C, 2 * b + 1, b + 1, dtype=torch.complex64, device=x.device)
    s = _spec_real(out, N, C, b, "out")
    nbytes = lib().udapose_fda_ws_bytes(N * C, H, W, b)
    if nbytes < 0:
        check(int(nbytes), "fda_ws_bytes")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    check(lib().udapose_fda_spectrum(_hip.stream(), ptr(x), N * C, H, W, b, ptr(ws), ptr(s)), "fda_spectrum")
    return out


def _apply(content, spec_c, spec_s, b, alpha, clamp, mean, std, out):
    content = _image(content, "content")
    N, C, H, W = content.shape
    _check_window(H, W, b)
    sc, ss = _spec_real(spec_c, N, C, b, "spec_content"), _spec_real(spec_s, N, C, b, "spec_style")
    dev = content.device
    alpha_dev, a = None, 1.0
    if torch.is_tensor(alpha):
        if not alpha.is_cuda or alpha.dtype != torch.float32 or alpha.numel() != 1:
            raise ValueError("alpha as a tensor must be one float32 element on the device")
        alpha_dev = alpha
    else:
        a = float(alpha)
        if not 0.0 <= a <= 1.0:
            raise ValueError(f"alpha must be in [0, 1], got {a}")
    lo = hi = None
    if clamp is not None:
        lo, hi = _per_channel(clamp[0], C, dev, "clamp[0]"), _per_channel(clamp[1], C, dev, "clamp[1]")
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    if out is None:
        out = torch.empty_like(content)
    elif (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or out.shape != content.shape or not out.is_contiguous()):
        raise ValueError("out must be a contiguous float32 device tensor of the content's shape")
    check(lib().udapose_fda_apply(_hip.stream(), ptr(content), ptr(sc), ptr(ss), ptr(out), N * C, C, H, W, b, a, ptr(alpha_dev), ptr(lo), ptr(hi),
                                  ptr(mean), ptr(std)), "fda_apply")
    return out


def _pair(content, style):
    content, style = _image(content, "content"), _image(style, "style")
    if content.shape != style.shape:
        raise ValueError(f"content {tuple(content.shape)} and style {tuple(style.shape)} must have the same shape (sample i pairs with sample i)")
    return content, style


def fda_transfer(content, style, beta=0.01, alpha=1.0, clamp=None, mean=None, std=None):
    """FDA of `content` towards `style` (fp32 NCHW on the device, equal shapes) -> fp32 NCHW.  clamp = (lo[C], hi[C]) is applied to the result;
    mean / std [C]: the tensors are normalised images and the transfer is that of the raw ones (module docstring)."""
    return FDANet(beta, mean, std)(content, style, alpha, clamp)[2]


class NormalisedStyleNet(nn.Module):
    """What the style nets without weights share: the optional per-channel mean / std of normalised images, kept as host values and uploaded once
    per device.  No parameters, no buffers."""

    def __init__(self, mean=None, std=None):
        super().__init__()
        if (mean is None) != (std is None):
            raise ValueError("mean and std go together")
        self.mean = None if mean is None else [float(v) for v in torch.as_tensor(mean).reshape(-1).tolist()]
        self.std = None if std is None else [float(v) for v in torch.as_tensor(std).reshape(-1).tolist()]
        if self.std is not None and not all(s > 0 and math.isfinite(s) for s in self.std):
            raise ValueError("std must be positive")
        self._norm = {}             # device -> (mean, std) as device tensors: uploaded once per device, outside any captured step

    def _norm_on(self, C, dev):
        if self.mean is None:
            return None, None
        if len(self.mean) != C or len(self.std) != C:
            raise ValueError(f"mean / std have {len(self.mean)} / {len(self.std)} values for images of {C} channels")
        hit = self._norm.get(dev)
        if hit is None:
            hit = self._norm[dev] = (torch.tensor(self.mean, dtype=torch.float32, device=dev), torch.tensor(self.std, dtype=torch.float32, device=dev))
        return hit


class FDANet(NormalisedStyleNet):
    """`Style_net.Net`'s call form without weights: forward(content, style, alpha, clamp) -> (None, None, g_t).  No parameters, no buffers."""

    def __init__(self, beta=0.01, mean=None, std=None):
        super().__init__(mean, std)
        self.beta = float(beta)

    def window_of(self, img):
        return window(img.shape[-2], img.shape[-1], self.beta)

    def spectrum(self, img, out=None):
        """The window's coefficients of every plane of `img` (complex64 [N, C, 2b+1, b+1]); `out`: write them there."""
        with torch.no_grad():
            img = _image(img, "img")
            return low_freq_spectrum(img, self.window_of(img), out=out)

    def transfer(self, content, spec_content, spec_style, alpha=1.0, clamp=None, out=None):
        """g_t of forward(content, style, alpha, clamp) from the two images' spectrum().  alpha: a float in [0, 1] or a one-element fp32 device
        tensor that is read when the kernel runs (a captured launch then follows the step's draw)."""
        with torch.no_grad():
            content = _image(content, "content")
            mean, std = self._norm_on(content.shape[1], content.device)
            return _apply(content, spec_content, spec_style, self.window_of(content), alpha, clamp, mean, std, out)

    def forward(self, content, style, alpha=1.0, clamp=None):
        content, style = _pair(content, style)
        return None, None, self.transfer(content, self.spectrum(content), self.spectrum(style), alpha, clamp)
