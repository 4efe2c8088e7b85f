"""What every heat-map wrapper of this package does to its operands before a launch, stated once: the fp32 rows of a [B,K,...] batch, the
per-(b,k) factor and mask WITH their size check (the kernels index both by row), the per-pixel `valid_mask` selection, the gradient
scalar, and the one caller of udapose_heatmap_argmax.  lib/models/loss.py, lib/models/Style_net.py, lib/keypoint_detection.py, utils.py
and warp.py import it at module level; it imports none of them.
"""
import collections

import torch

from . import _hip
from ._hip import check, lib, ptr


def f32c(t):
    """`t` detached, fp32 and contiguous (itself where it already is both: no launch)."""
    return t.detach().float().contiguous()


def rows(t):
    """(R, HW) of a [B,K,...] batch: its B*K rows and the elements of one."""
    B, K = t.shape[:2]
    return B * K, t.numel() // (B * K)


def bk_factor(weight, R, what="target_weight"):
    """The per-(b,k) float factor as R contiguous floats (None stays None).  ValueError, before anything is converted, for another size."""
    if weight is None:
        return None
    if weight.numel() != R:
        raise ValueError(f"{what} must have B*K elements")
    return f32c(weight).reshape(-1)


def bk_mask(mask, R, what="tea_mask"):
    """The per-(b,k) mask as R bytes (None stays None): bool storage is read as it is (0 / 1: no conversion launch), anything else is
    `!= 0`.  ValueError, before anything is converted, for another size."""
    if mask is None:
        return None
    if mask.numel() != R:
        raise ValueError(f"{what} must have B*K elements")
    if mask.dtype == torch.bool and mask.is_contiguous():
        return mask.detach().view(torch.uint8).reshape(-1)
    return (mask.detach() != 0).to(torch.uint8).reshape(-1).contiguous()


def valid_selection(valid, like):
    """loss_map[valid_mask].mean() (the reference's loss.py:129-130, 149-150, 170-171): the boolean selection over (b, h, w) of the
    [B,K,H,W] batch `like` as bytes, and how many it selects, counted on the device (a 0-d float tensor: nothing is read back).
    (None, None) without a valid_mask; IndexError, as boolean indexing raises, for a mask of another shape."""
    if valid is None:
        return None, None
    shape = (like.shape[0],) + tuple(like.shape[2:])
    if tuple(valid.shape) != shape:
        raise IndexError(f"valid_mask shape {tuple(valid.shape)} does not index loss_map {shape}")
    v = (valid.detach() != 0).to(torch.uint8).reshape(-1).contiguous()
    cnt = torch.empty((), dtype=torch.float32, device=v.device)
    check(lib().udapose_mask_count(_hip.stream(), ptr(v), v.numel(), ptr(cnt)), "mask_count")
    return v, cnt


def gscale(g):
    """The incoming gradient of a scalar loss as one device float (the backward kernels read it there: no synchronisation)."""
    return g.detach().float().reshape(1).contiguous()


def grad_like_input(ctx, d):
    """The fp32 gradient `d` in the shape and dtype of the input that `ctx.shape` and `ctx.in_dtype` were taken from."""
    return d.reshape(ctx.shape).to(ctx.in_dtype)


_PATCH_CACHE = {}


def _gauss_patch(sigma, device):
    """The (6*sigma+1)^2 un-normalised Gaussian exactly as the reference's utils.py:93-98 builds it (host, once per sigma)."""
    key = (float(sigma), type(sigma) is int, str(device))
    if key not in _PATCH_CACHE:
        tmp_size = 3 * sigma
        if float(tmp_size) != int(tmp_size):
            raise NotImplementedError("rectify on the device needs 3*sigma to be an integer (reference uses sigma=2 or 1.0)")
        size = 2 * tmp_size + 1
        x = torch.arange(0, size, 1).float()
        y = x.unsqueeze(1)
        x0 = y0 = size // 2
        g = torch.exp(- ((x - x0) ** 2 + (y - y0) ** 2) / (2 * sigma ** 2))
        _PATCH_CACHE[key] = (g.contiguous().to(device), int(tmp_size))
    return _PATCH_CACHE[key]


ArgMax = collections.namedtuple("ArgMax", "maxv idx xy rect")


def heatmap_argmax(hm, *, maxv=False, idx=False, xy=False, rectify_sigma=None):
    """udapose_heatmap_argmax - one sweep - on an fp32 contiguous CUDA batch [B,K,H,W], writing the outputs the caller names (the others are
    None in the result):
      maxv [B,K] float32    the maximum of every map (NaN counts as the largest value)
      idx [B,K] int32       its first flat index y * W + x
      xy [B,K,2] float32    (x, y) of that index, (0, 0) where the maximum is <= 0 (get_max_preds' masking)
      rect [B,K,H,W] float32, for rectify_sigma = sigma: the reference's `rectify` - the Gaussian patch of that sigma stamped at xy into a
                            zero map."""
    B, K, H, W = hm.shape

    def new(want, shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=hm.device) if want else None

    patch, rad = (None, 0) if rectify_sigma is None else _gauss_patch(rectify_sigma, hm.device)
    out = ArgMax(new(maxv, (B, K)), new(idx, (B, K), torch.int32), new(xy, (B, K, 2)), new(rectify_sigma is not None, hm.shape))
    check(lib().udapose_heatmap_argmax(_hip.stream(), ptr(hm), B * K, H, W, ptr(out.maxv), ptr(out.idx), ptr(out.xy), ptr(out.rect), ptr(patch), rad),
          "heatmap_argmax")
    return out
