"""Plain-numpy restatement of the two sub-pixel decodes (udapose_refine_decode: the quarter-pixel offset and DARK, the distribution-aware
decode) and of the un-quantised label encoding (udapose_gaussian_labels_subpixel), written from their definitions in include/udapose.h
and DESIGN.md 4.11.  The reference has none of them and OpenCV is not used: the blur is two loops over the taps.
Everything runs in the dtype of the map it is given: in fp64 it is the oracle of tests/test_gpu_dark.py, in fp32 it is the "reference
arithmetic" whose distance to fp64 sets the device's bound (tests/test_dark_cpu.py checks its parts against independent forms).
"""
import numpy as np


def default_sigma(kernel):
    return 0.3 * ((kernel - 1) / 2 - 1) + 0.8


def taps(kernel, sigma=None):
    """fp32 taps t_i = exp(-(i - c)^2 / 2 sigma^2) / sum, computed in double and rounded once; sigma None or <= 0: the default."""
    kernel = int(kernel)
    if kernel < 3 or kernel > 31 or kernel % 2 == 0:
        raise ValueError(f"kernel must be odd and in [3, 31], got {kernel}")
    s = float(sigma) if sigma is not None and sigma > 0 else default_sigma(kernel)
    c = (kernel - 1) // 2
    e = np.exp(-((np.arange(kernel, dtype=np.float64) - c) ** 2) / (2.0 * s * s))
    return (e / e.sum()).astype(np.float32)


def blur(hm, t):
    """Separable blur of [..., H, W] with zero padding of (kernel - 1) / 2 on every side: rows first, then columns, taps added in
    ascending order, in hm's dtype."""
    t = np.asarray(t).astype(hm.dtype)
    k, c = len(t), (len(t) - 1) // 2
    H, W = hm.shape[-2:]
    pad = np.zeros(hm.shape[:-1] + (W + 2 * c,), dtype=hm.dtype)
    pad[..., c:c + W] = hm
    rows = np.zeros_like(hm)
    for j in range(k):
        rows = rows + t[j] * pad[..., j:j + W]
    pad = np.zeros(hm.shape[:-2] + (H + 2 * c, W), dtype=hm.dtype)
    pad[..., c:c + H, :] = rows
    out = np.zeros_like(hm)
    for j in range(k):
        out = out + t[j] * pad[..., j:j + H, :]
    return out


def first_argmax(hm):
    """(flat index [R], maximum [R]) of [R, H, W]: the first flat arg-max, NaN counting as the largest value (numpy's argmax)."""
    rows = hm.reshape(hm.shape[0], -1)
    idx = rows.argmax(1)
    return idx, rows[np.arange(len(idx)), idx]


def derivatives(g, x, y):
    """(dx, dy, dxx, dyy, dxy) of the map g [H, W] at the pixel (x, y) by central differences."""
    dt = g.dtype.type
    dx = dt(0.5) * (g[y, x + 1] - g[y, x - 1])
    dy = dt(0.5) * (g[y + 1, x] - g[y - 1, x])
    dxx = dt(0.25) * (g[y, x + 2] - dt(2) * g[y, x] + g[y, x - 2])
    dyy = dt(0.25) * (g[y + 2, x] - dt(2) * g[y, x] + g[y - 2, x])
    dxy = dt(0.25) * (g[y + 1, x + 1] - g[y - 1, x + 1] - g[y + 1, x - 1] + g[y - 1, x - 1])
    return dx, dy, dxx, dyy, dxy


def taylor_step(dx, dy, dxx, dyy, dxy):
    """-Hess^-1 (dx, dy) in closed form, or None where a guard forbids it: det == 0, or an offset that is not finite."""
    with np.errstate(all="ignore"):
        det = dxx * dyy - dxy * dxy
        if det == 0:
            return None
        ox, oy = -(dyy * dx - dxy * dy) / det, -(dxx * dy - dxy * dx) / det
    if not (np.isfinite(ox) and np.isfinite(oy)):
        return None
    return ox, oy


def dark_decode(hm, kernel=11, sigma=None):
    """[B,K,H,W] -> (coords [B,K,2] (x, y), maxvals [B,K,1], flat_idx [B,K]) in hm's dtype (flat_idx int64)."""
    B, K, H, W = hm.shape
    maps = hm.reshape(B * K, H, W)
    idx, m = first_argmax(maps)
    coords = np.zeros((B * K, 2), dtype=hm.dtype)
    t = taps(kernel, sigma)
    dt = hm.dtype.type
    for r in range(B * K):
        if not m[r] > 0:
            continue
        x, y = int(idx[r] % W), int(idx[r] // W)
        coords[r] = (x, y)
        if not (1 < x < W - 2 and 1 < y < H - 2):
            continue
        with np.errstate(all="ignore"):
            g = blur(maps[r], t)
            gmax = g.reshape(-1)[g.reshape(-1).argmax()]
            if not gmax > 0:
                continue
            g = np.log(np.maximum(g * (m[r] / gmax), dt(1e-10)))
        step = taylor_step(*derivatives(g, x, y))
        if step is not None:
            coords[r] = (dt(x) + step[0], dt(y) + step[1])
    return coords.reshape(B, K, 2), m.reshape(B, K, 1), idx.reshape(B, K)


def quarter_decode(hm):
    """[B,K,H,W] -> (coords, maxvals, flat_idx): the arg-max moved a quarter pixel towards the higher neighbour."""
    B, K, H, W = hm.shape
    maps = hm.reshape(B * K, H, W)
    idx, m = first_argmax(maps)
    coords = np.zeros((B * K, 2), dtype=hm.dtype)
    dt = hm.dtype.type
    for r in range(B * K):
        if not m[r] > 0:
            continue
        x, y = int(idx[r] % W), int(idx[r] // W)
        coords[r] = (x, y)
        if 1 < x < W - 1 and 1 < y < H - 1:
            with np.errstate(all="ignore"):
                d = np.array([maps[r, y, x + 1] - maps[r, y, x - 1], maps[r, y + 1, x] - maps[r, y - 1, x]])
            coords[r] += dt(0.25) * np.nan_to_num(np.sign(d), nan=0.0).astype(hm.dtype)
    return coords.reshape(B, K, 2), m.reshape(B, K, 1), idx.reshape(B, K)


def argmax_decode(hm):
    """get_max_preds: coordinates zeroed where the maximum is <= 0."""
    B, K, H, W = hm.shape
    idx, m = first_argmax(hm.reshape(B * K, H, W))
    xy = np.stack([idx % W, idx // W], -1).astype(hm.dtype) * (m > 0)[:, None]
    return xy.reshape(B, K, 2), m.reshape(B, K, 1), idx.reshape(B, K)


def labels(kp, vis, Hh, Wh, stride_x, stride_y, sigma, rad, subpixel=True, dtype=np.float64):
    """kp [R,2] (x, y) in image pixels, vis [R] -> (target [R,Hh,Wh] in `dtype`, weight [R] fp32).  Centre c = int(kp / stride + 0.5)
    (truncation) and weight = vis, 0 where c is outside the map; the Gaussian sits on kp / stride (subpixel) or on c, inside the
    (2 rad + 1)^2 window round c, where weight > 0.5."""
    kp = np.asarray(kp, dtype=np.float64)
    R = kp.shape[0]
    target, weight = np.zeros((R, Hh, Wh), dtype=dtype), np.asarray(vis, dtype=np.float32).copy()
    ys, xs = np.arange(Hh)[:, None], np.arange(Wh)[None, :]
    for r in range(R):
        ux, uy = kp[r, 0] / stride_x, kp[r, 1] / stride_y
        cx, cy = int(ux + 0.5), int(uy + 0.5)
        if cx >= Wh or cy >= Hh or cx < 0 or cy < 0:
            weight[r] = 0
        if not weight[r] > 0.5:
            continue
        mx, my = (ux, uy) if subpixel else (cx, cy)
        v = np.exp(-((xs - mx) ** 2 + (ys - my) ** 2) / (2.0 * sigma * sigma))
        win = (np.abs(xs - cx) <= rad) & (np.abs(ys - cy) <= rad)
        target[r] = np.where(win, v, 0.0).astype(dtype)
    return target, weight
