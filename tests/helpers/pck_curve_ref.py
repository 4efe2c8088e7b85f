"""Numpy restatement of the evaluation meter (csrc/pck_curve.hip; the definitions: include/udapose.h), twice.

`state_fp32` / `state_fp32_heatmaps` follow the device's fp32 operation order exactly - every difference, product, sum, quotient and root
is one correctly rounded fp32 operation there (no FMA), which is what numpy does on float32 arrays - and predict the int64 state
[K, T + 3] (hits[0..T-1], count, epe_q, nonfinite) BIT FOR BIT.  `distances_fp64` gives the same quantities in fp64: the exact distances
the derived tolerances of tests/test_gpu_pck_curve.py are measured against.  `argmax_preds` is the reference's get_max_preds
(lib/keypoint_detection.py:9-37; numpy's arg-max takes the first index on ties and a NaN as the maximum, as the device does).
"""
import numpy as np

EPE_SCALE = 65536
EPE_LIMIT = np.float32(2.0 ** 46)


def argmax_preds(hm):
    """[B,K,H,W] -> [B,K,2] float32 (x, y), (0, 0) where the maximum is not > 0."""
    B, K, H, W = hm.shape
    flat = np.asarray(hm, dtype=np.float32).reshape(B, K, -1)
    idx = flat.argmax(2)
    maxv = np.take_along_axis(flat, idx[..., None], 2)[..., 0]
    preds = np.stack([idx % W, idx // W], -1).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return preds * (maxv > 0)[..., None].astype(np.float32)


def _visible(gt, visible, norm):
    with np.errstate(invalid="ignore"):
        vis = (np.asarray(visible) != 0) if visible is not None else (gt[..., 0] > 1) & (gt[..., 1] > 1)
        if norm is not None:
            n = np.asarray(norm)
            vis = vis & (np.isfinite(n) & (n > 0))[:, None]
    return vis


def state_fp32(pred, gt, thr, nh, nw, visible=None, norm=None):
    """pred, gt [B,K,2]; thr [T] ascending; nh, nw the two size terms (H / 10, W / 10) as the C call takes them; visible [B,K] or None (the
    `> 1` rule on gt); norm [B] or None.  Returns the int64 state [K, T + 3] one launch adds."""
    f = np.float32
    pred, gt, thr = np.asarray(pred, dtype=f), np.asarray(gt, dtype=f), np.asarray(thr, dtype=f)
    nh, nw = f(nh), f(nw)
    px, py, tx, ty = pred[..., 0], pred[..., 1], gt[..., 0], gt[..., 1]
    with np.errstate(all="ignore"):
        ex, ey = px - tx, py - ty
        e = np.sqrt(ex * ex + ey * ey)
        if norm is not None:
            d = e / np.asarray(norm, dtype=f)[:, None]
        else:
            dx, dy = px / nh - tx / nh, py / nw - ty / nw
            d = np.sqrt(dx * dx + dy * dy)
        assert e.dtype == f and d.dtype == f
        vis = _visible(gt, visible, norm)
        hit = (d[..., None] < thr) & vis[..., None]                      # [B,K,T]: the T independent compares (NaN hits nothing)
        fin = e < EPE_LIMIT                                              # (false for NaN and inf)
        q = np.where(vis & fin, np.rint(np.where(fin, e, 0).astype(np.float64) * EPE_SCALE), 0).astype(np.int64)
    K, T = pred.shape[1], thr.size
    state = np.zeros((K, T + 3), dtype=np.int64)
    state[:, :T] = hit.sum(0)
    state[:, T] = vis.sum(0)
    state[:, T + 1] = q.sum(0)
    state[:, T + 2] = (vis & ~fin).sum(0)
    return state


def state_fp32_heatmaps(out, target, thr, norm=None):
    """The fused form: both tensors [B,K,H,W] decoded by arg-max, nh = H / 10 and nw = W / 10 rounded to fp32."""
    H, W = out.shape[2:]
    return state_fp32(argmax_preds(out), argmax_preds(target), thr, np.float32(H / 10.0), np.float32(W / 10.0), None, norm)


def distances_fp64(pred, gt, nh, nw, visible=None, norm=None):
    """(d, e, vis) in fp64 from the fp32 inputs: the normalised distance (nh, nw as the device holds them, fp32 values), the end-point
    error in pixels and the visibility [B,K]."""
    pred, gt = np.asarray(pred, dtype=np.float32).astype(np.float64), np.asarray(gt, dtype=np.float32).astype(np.float64)
    nh, nw = float(np.float32(nh)), float(np.float32(nw))
    ex, ey = pred[..., 0] - gt[..., 0], pred[..., 1] - gt[..., 1]
    with np.errstate(all="ignore"):
        e = np.sqrt(ex * ex + ey * ey)
        if norm is not None:
            d = e / np.asarray(norm, dtype=np.float32).astype(np.float64)[:, None]
        else:
            d = np.sqrt((ex / nh) ** 2 + (ey / nw) ** 2)
    return d, e, _visible(gt, visible, norm)


# ------------------------------------------------------------------------------------------------ the golden cases (tests/golden/pck_curve.npz)
GOLDEN_CASES = (("c64x64", (3, 5, 64, 64), 11), ("c48x64", (4, 21, 48, 64), 12), ("c12x20", (2, 16, 12, 20), 13))


def _blob(plane, x, y, peak):
    H, W = plane.shape
    for xx, yy, v in ((x - 1, y, 0.5), (x + 1, y, 0.5), (x, y - 1, 0.5), (x, y + 1, 0.5), (x, y, 1.0)):
        if 0 <= xx < W and 0 <= yy < H:
            plane[yy, xx] = v * peak


def golden_inputs(shape, seed):
    """Seeded (output, target) heat-map pairs [B,K,H,W] float32: sparse maps, one five-pixel blob each, the prediction's at an integer
    offset of up to 6 pixels from the target's.  Joint 0 is invisible in every sample (x <= 1, or a target plane of all -1), joint 1 in
    sample 0 only; joint 2's prediction is a plane of all zeros in sample 0 (decoded (0, 0)); on maps 20 wide joints 3 and 4 sit one and
    two rows off with no column offset, which is d = 0.5 and d = 1.0 exactly (nw = 2): thresholds hit as ties."""
    B, K, H, W = shape
    rs = np.random.RandomState(seed)
    out, tgt = np.zeros(shape, dtype=np.float32), np.zeros(shape, dtype=np.float32)
    for b in range(B):
        for k in range(K):
            tx, ty = int(rs.randint(2, W - 1)), int(rs.randint(2, H - 1))
            dx, dy = int(rs.randint(-6, 7)), int(rs.randint(-6, 7))
            peak = float(rs.uniform(0.3, 1.0))
            if k == 0 and b % 2 == 0:
                tgt[b, k] = -1.0
            elif k == 0:
                tx = b % 2
                _blob(tgt[b, k], tx, ty, 1.0)
            elif k == 1 and b == 0:
                ty = 1
                _blob(tgt[b, k], tx, ty, 1.0)
            else:
                _blob(tgt[b, k], tx, ty, 1.0)
            if W == 20 and k in (3, 4):
                dx, dy = 0, (k - 2) * (1 if ty + 2 < H else -1)
            if k == 2 and b == 0:
                continue
            _blob(out[b, k], min(max(tx + dx, 0), W - 1), min(max(ty + dy, 0), H - 1), peak)
    return out, tgt
