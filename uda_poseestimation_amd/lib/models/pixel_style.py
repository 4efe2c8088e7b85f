"""Histogram matching and colour-statistics transfer as style networks without weights (csrc/pixel_style.hip; no counterpart in the reference).

With FDA (lib/models/fda.py) these are the classical pixel-level domain bridges.  `PixelStyleNet(mode, mean, std)` is a drop-in for `Style_net.Net`
as the training loop uses it: `style_net(content, style, alpha, clamp=...)[2]` is the transferred batch; `MeanTeacherTrainer(style_net=...)` and
`GraphedTrainStep` summarise each batch once per step (`spectrum`) and run one launch per direction (`transfer`).  fp32 NCHW in and out, contiguous,
equal shapes, sample i pairs with sample i, no autograd (the loop runs the transfer under no_grad).

Without `mean` / `std` the tensors are raw images in [0, 1]; with them they are (raw - mean_c) / std_c.

LEVEL of a pixel:  l = (int) min(max(rint((x * std_c + mean_c) * 255), 0), 255), in fp32 (x * std_c + mean_c is one fused multiply-add).  The clamp
comes before the cast: out-of-range, infinite and NaN pixels land on a bound.  For tensors that came from 8-bit images through the normalisation the
level is the original byte; for any other float image it is a QUANTISATION to 256 levels - the transfer then moves a pixel by the shift of its level
and keeps the pixel's distance to that level.

SUMMARY of a batch (`summary`, alias `spectrum`): int32 [N, R], R = C * 256 + (8 if C == 3 else 0); `split_summary` gives the two views:
    [:, c * 256 + k]     the number of pixels of channel c at level k
    [:, 768:774]         (C == 3) three int64, low word first: sum l_0 l_1, sum l_0 l_2, sum l_1 l_2; words 774, 775 are zero
Exact integers, bit-reproducible; every mode needs only this (per-channel sum l and sum l^2 follow from the histogram).

TRANSFER:  out = x + alpha * (T - l) * inv_c,  inv_c = 1 / (255 * std_c), then the optional per-channel clamp.  alpha = 0 returns x to the bit, and the
sub-level residue of x survives.  T, the target level, per mode:
    "hist"      scikit-image's match_histograms per channel, on integer cumulative counts (H * W <= 2^24)
    "meanstd"   the reference's calc_mean_std / adain (lib/models/Style_net.py:4-29) on pixels: per channel mean and unbiased variance in raw units,
                T / 255 = (l / 255 - mu_c) * sqrt(var_s + eps) / sqrt(var_c + eps) + mu_s   (H * W >= 2)
    "cholesky"  C == 3: T / 255 = L_s L_c^-1 (l / 255 - mu_c) + mu_s, L = chol(Sigma + eps I), Sigma the unbiased 3 x 3 covariance in raw units - the
                linear colour transfer that also moves cross-channel correlation   (H * W >= 2)
What is derived per plane or sample (the 256-entry table T - k, two coefficients, the 3 x 4 matrix) is computed in fp64 from the integers and rounded
once to fp32; the per-pixel work is fp32."""
import math

import torch

from ... import _hip
from ..._hip import check, lib, ptr
from .fda import NormalisedStyleNet, _image, _pair, _per_channel

MODES = {"hist": 0, "meanstd": 1, "cholesky": 2}       # UDAPOSE_PIXEL_HIST / _MEANSTD / _CHOLESKY (include/udapose.h)
MAX_HW = 1 << 24                                       # UDAPOSE_PIXEL_MAX_HW
SHARE = 4096                                           # UDAPOSE_PIXEL_SHARE: the pixels of a plane that one work-group covers


def summary_words(C):
    """int32 words of one sample's row of a summary."""
    return C * 256 + (8 if C == 3 else 0)


def split_summary(summary, C):
    """(histograms int32 [N, C, 256], cross sums int64 [N, 3] or None) of a summary: views where possible, no kernel."""
    N = summary.shape[0]
    hist = summary[:, :C * 256].reshape(N, C, 256)
    cross = summary[:, 768:774].contiguous().view(torch.int64) if C == 3 else None
    return hist, cross


def _check_plane(N, C, H, W):
    if N * C == 0 or H * W == 0:
        raise ValueError("the images have no planes or no pixels")
    if H * W > MAX_HW:
        raise NotImplementedError(f"{H} x {W} planes: the kernels count up to H * W = 2^24 pixels per plane")


def _norm_tensors(mean, std, C, dev):
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    return _per_channel(mean, C, dev, "mean"), _per_channel(std, C, dev, "std")


def _summary_of(t, N, C, what):
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor")
    _hip.require_cuda(t)
    if t.dtype != torch.int32 or tuple(t.shape) != (N, summary_words(C)) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous int32 [{N}, {summary_words(C)}] summary (PixelStyleNet.summary), got {t.dtype} {tuple(t.shape)}")
    return t


def _summarize(x, mean, std, out):
    x = _image(x, "x")
    N, C, H, W = x.shape
    _check_plane(N, C, H, W)
    if out is None:
        out = torch.empty(N, summary_words(C), dtype=torch.int32, device=x.device)
    s = _summary_of(out, N, C, "out")
    check(lib().udapose_pixel_summary(_hip.stream(), ptr(x), N, C, H, W, ptr(mean), ptr(std), ptr(s)), "pixel_summary")
    return out


def level_histograms(x, mean=None, std=None):
    """int32 [N, C, 256]: the number of pixels of every plane of `x` (fp32 NCHW on the device) at each level (module docstring)."""
    with torch.no_grad():
        x = _image(x, "x")
        m, s = _norm_tensors(mean, std, x.shape[1], x.device)
        return split_summary(_summarize(x, m, s, None), x.shape[1])[0]


def _apply(content, sum_c, sum_s, mode, eps, alpha, clamp, mean, std, out):
    content = _image(content, "content")
    N, C, H, W = content.shape
    _check_plane(N, C, H, W)
    if mode == "cholesky" and C != 3:
        raise ValueError(f"mode 'cholesky' moves the 3 x 3 colour covariance: images of 3 channels, got {C}")
    if mode != "hist" and H * W < 2:
        raise ValueError(f"mode {mode!r} needs the unbiased variance of a plane: H * W >= 2, got {H} x {W}")
    sc, ss = _summary_of(sum_c, N, C, "sum_content"), _summary_of(sum_s, N, C, "sum_style")
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
    if out is None:
        out = torch.empty_like(content)
    elif (not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or out.shape != content.shape or not out.is_contiguous()):
        raise ValueError("out must be a contiguous float32 device tensor of the content's shape")
    check(lib().udapose_pixel_transfer(_hip.stream(), ptr(content), ptr(sc), ptr(ss), ptr(out), N, C, H, W, MODES[mode], eps, a, ptr(alpha_dev), ptr(lo),
                                       ptr(hi), ptr(mean), ptr(std)), "pixel_transfer")
    return out


def pixel_style_transfer(content, style, mode="hist", alpha=1.0, clamp=None, mean=None, std=None, eps=1e-5):
    """`content` moved towards `style` (fp32 NCHW on the device, equal shapes) -> fp32 NCHW.  mode: "hist", "meanstd" or "cholesky" (module
    docstring); clamp = (lo[C], hi[C]) is applied to the result; mean / std [C]: the tensors are normalised images."""
    return PixelStyleNet(mode, mean, std, eps)(content, style, alpha, clamp)[2]


class PixelStyleNet(NormalisedStyleNet):
    """`Style_net.Net`'s call form without weights: forward(content, style, alpha, clamp) -> (None, None, g_t).  No parameters, no buffers."""

    def __init__(self, mode="hist", mean=None, std=None, eps=1e-5):
        super().__init__(mean, std)
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: one of {tuple(MODES)}")
        self.mode, self.eps = mode, float(eps)
        if not (self.eps > 0 and math.isfinite(self.eps)):
            raise ValueError("eps must be positive")

    def summary(self, img, out=None):
        """The level histograms (and, for 3 channels, cross sums) of every sample of `img`: int32 [N, summary_words(C)]; `out`: write them there."""
        with torch.no_grad():
            img = _image(img, "img")
            mean, std = self._norm_on(img.shape[1], img.device)
            return _summarize(img, mean, std, out)

    spectrum = summary              # the name the trainer's style adapter looks for

    def transfer(self, content, sum_content, sum_style, alpha=1.0, clamp=None, out=None):
        """g_t of forward(content, style, alpha, clamp) from the two images' summary().  alpha: a float in [0, 1] or a one-element fp32 device
        tensor that is read when the kernel runs (a captured launch then follows the step's draw)."""
        with torch.no_grad():
            content = _image(content, "content")
            mean, std = self._norm_on(content.shape[1], content.device)
            return _apply(content, sum_content, sum_style, self.mode, self.eps, alpha, clamp, mean, std, out)

    def forward(self, content, style, alpha=1.0, clamp=None):
        content, style = _pair(content, style)
        return None, None, self.transfer(content, self.summary(content), self.summary(style), alpha, clamp)
