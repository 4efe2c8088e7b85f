"""Plain-torch restatement of the soft-argmax decode (lib.keypoint_detection.soft_argmax) and of the two coordinate losses
(JointsSoftArgmaxLoss, ConsSoftArgmaxLoss of lib/models/loss.py), written from their definitions: the window is a boolean mask round the
first flat arg-max, the losses get their gradients from autograd.  The reference has no soft-argmax, so nothing is taken from it.
It runs in whatever dtype its inputs have: in fp64 it is the oracle of tests/test_gpu_soft_argmax.py, in fp32 it is the "reference
arithmetic" whose own error against fp64 sets the device's bound (tests/test_soft_argmax_cpu.py checks it against independent forms).
"""
import numpy as np
import torch


def first_argmax(hm):
    """[B,K] first flat arg-max of every map, NaN counting as the largest value (numpy's argmax: the first occurrence)."""
    B, K = hm.shape[:2]
    return torch.from_numpy(hm.detach().cpu().numpy().reshape(B, K, -1).argmax(2))


def window_mask(idx, H, W, window):
    """bool [B,K,H*W]: the pixels within `window` (Chebyshev) of the arg-max, the whole map for window None."""
    B, K = idx.shape
    if window is None:
        return torch.ones(B, K, H * W, dtype=torch.bool)
    i = torch.arange(H * W)
    x, y = (i % W)[None, None], (i // W)[None, None]
    xs, ys = (idx % W)[..., None], (idx // W)[..., None]
    return ((x - xs).abs() <= window) & ((y - ys).abs() <= window)


def decode(hm, beta=10.0, window=None):
    """(coords [B,K,2] (x, y) in pixel-index units, maxvals [B,K,1]).  The arg-max (and with it the shift m) is a constant."""
    B, K, H, W = hm.shape
    rows = hm.reshape(B, K, H * W)
    idx = first_argmax(hm).to(rows.device)
    m = rows.detach().gather(2, idx[..., None])
    sel = window_mask(idx.cpu(), H, W, window).to(rows.device)
    e = torch.where(sel, torch.exp(beta * (rows - m)), torch.zeros((), dtype=rows.dtype, device=rows.device))
    p = e / e.sum(-1, keepdim=True)
    i = torch.arange(H * W, device=rows.device)
    x, y = (i % W).to(rows.dtype), (i // W).to(rows.dtype)
    return torch.stack([(p * x).sum(-1), (p * y).sum(-1)], -1), m


def decode_gradient(hm, g, beta=10.0, window=None):
    """The closed form of d <coords, g> / d hm: beta p_i ((x_i - cx) gx + (y_i - cy) gy) inside the window, 0 outside."""
    B, K, H, W = hm.shape
    rows = hm.detach().reshape(B, K, H * W)
    idx = first_argmax(hm)
    sel = window_mask(idx, H, W, window)
    m = rows.gather(2, idx[..., None])
    e = torch.where(sel, torch.exp(beta * (rows - m)), torch.zeros((), dtype=rows.dtype))
    p = e / e.sum(-1, keepdim=True)
    i = torch.arange(H * W)
    x, y = (i % W).to(rows.dtype), (i // W).to(rows.dtype)
    cx, cy = (p * x).sum(-1, keepdim=True), (p * y).sum(-1, keepdim=True)
    return (beta * p * ((x - cx) * g[..., :1] + (y - cy) * g[..., 1:])).reshape(B, K, H, W)


def argmax_decode(hm):
    """get_max_preds: (coords [B,K,2] zeroed where the maximum is <= 0, maxvals [B,K,1]) in hm's dtype."""
    B, K, H, W = hm.shape
    idx = first_argmax(hm).to(hm.device)
    maxv = hm.detach().reshape(B, K, -1).gather(2, idx[..., None])
    xy = torch.stack([idx % W, idx // W], -1).to(hm.dtype)
    return xy * (maxv > 0).to(hm.dtype), maxv


def _l(d, norm):
    return d.abs() if norm == "l1" else 0.5 * d * d


def coord_loss(output, xy, factor=None, beta=10.0, window=None, norm="l1", reduction="mean"):
    """factor[b,k] * (l((cx - tx) / W) + l((cy - ty) / H)); 'mean' over the B*K key points, 'none' the per-sample means [B]."""
    B, K, H, W = output.shape
    c, _ = decode(output, beta, window)
    xy = xy.to(c.dtype).reshape(B, K, 2)
    per = _l((c[..., 0] - xy[..., 0]) / W, norm) + _l((c[..., 1] - xy[..., 1]) / H, norm)
    if factor is not None:
        per = per * factor.to(c.dtype).reshape(B, K)
    if reduction == "mean":
        return per.mean()
    if reduction == "none":
        return per.mean(dim=-1)
    return None


def joints_soft_argmax(output, target, target_weight=None, beta=10.0, window=None, norm="l1", reduction="mean"):
    """target: [B,K,2] coordinates or [B,K,H,W] heat-maps (arg-max decode; a map whose maximum is <= 0 gets factor 0)."""
    B, K = output.shape[:2]
    factor = None if target_weight is None else target_weight.reshape(B, K)
    if target.dim() == 4:
        target, maxv = argmax_decode(target)
        present = (maxv > 0).reshape(B, K).to(output.dtype)
        factor = present if factor is None else factor.to(output.dtype) * present
    return coord_loss(output, target, factor, beta, window, norm, reduction)


def cons_soft_argmax(stu, tea, tea_mask=None, beta=10.0, window=None, norm="l1", tea_decode="argmax"):
    with torch.no_grad():
        xy = argmax_decode(tea)[0] if tea_decode == "argmax" else decode(tea, beta, window)[0]
    factor = None if tea_mask is None else (tea_mask != 0)
    return coord_loss(stu, xy, factor, beta, window, norm, "mean")


def pck(pred, gt, h, w, thr=0.5):
    """oracle.keypoints_ref.accuracy_ref from decoded coordinates [B,K,2]: (acc [K], avg, cnt); also the normalised distances [B,K]
    (NaN where the ground truth does not count) so that a test can see how far each lies from the threshold."""
    pred, gt = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    B, K = pred.shape[:2]
    norm = np.array([h, w], dtype=np.float64) / 10
    acc, dist = np.zeros(K), np.full((B, K), np.nan)
    tot, cnt = 0.0, 0
    for c in range(K):
        hits, n = 0, 0
        for b in range(B):
            if gt[b, c, 0] > 1 and gt[b, c, 1] > 1:
                dist[b, c] = np.linalg.norm(pred[b, c] / norm - gt[b, c] / norm)
                n += 1
                hits += dist[b, c] < thr
        acc[c] = hits / n if n else -1
        if acc[c] >= 0:
            tot += acc[c]
            cnt += 1
    return acc, (tot / cnt if cnt else 0), cnt, dist
