"""CORAL (the reference's CoralLoss, lib/models/loss.py:176-208) restated twice, in whatever dtype the inputs have (the tests use fp64 as the
truth and fp32 as the yardstick of what single precision can give):
  direct(src, tgt, d)  the reference's own D x D expression, differentiable by torch's autograd
  gram(src, tgt, d)    the n x n Gram form with its closed-form gradients (what csrc/coral.hip evaluates)
  down(x, d)           the pixel rule that F.interpolate(x, scale_factor=1/d, mode='bilinear') amounts to
and the seeded generator of heat-map-like inputs.  CPU only; nothing here touches the package."""
import torch


def down(x, d):
    """floor(H/d) x floor(W/d) maps: even d - the mean of the central 2x2 pixels of every d x d block (rows and columns d/2-1, d/2); odd d - the
    centre pixel."""
    if d == 1:
        return x
    H, W = x.shape[-2:]
    Ho, Wo = H // d, W // d
    b = x[..., :Ho * d, :Wo * d].reshape(*x.shape[:-2], Ho, d, Wo, d)
    if d % 2:
        return b[..., :, d // 2, :, d // 2]
    lo, hi = d // 2 - 1, d // 2
    return 0.25 * (b[..., :, lo, :, lo] + b[..., :, lo, :, hi] + b[..., :, hi, :, lo] + b[..., :, hi, :, hi])


def direct(src, tgt, d=1):
    """loss.py:183-208 with the .cuda() calls dropped and `down` for the interpolation."""
    src, tgt = down(src, d), down(tgt, d)
    n, c, h, w = tgt.shape
    xs, xt = src.reshape(n, -1), tgt.reshape(n, -1)
    one = torch.ones((1, n), dtype=xs.dtype)
    ms, mt = one @ xs, one @ xt
    cs = (xs.T @ xs - (ms.T @ ms) / n) / (n - 1)
    ct = (xt.T @ xt - (mt.T @ mt) / n) / (n - 1)
    return (cs - ct).pow(2).sum().sqrt() / (4 * (c * h * w) ** 2)


def direct_with_grads(src, tgt, d=1):
    s, t = src.clone().requires_grad_(True), tgt.clone().requires_grad_(True)
    loss = direct(s, t, d)
    gs, gt = torch.autograd.grad(loss, (s, t))
    return loss.detach(), gs, gt


def _up(g, shape, d):
    """the adjoint of `down`: 0.25 of an element's gradient to each of its four pixels (even d), all of it to the centre pixel (odd d)."""
    if d == 1:
        return g
    H, W = shape[-2:]
    Ho, Wo = H // d, W // d
    out = torch.zeros(shape, dtype=g.dtype)
    v = out[..., :Ho * d, :Wo * d].reshape(*shape[:-2], Ho, d, Wo, d)       # (a view: the slice keeps out's strides)
    if d % 2:
        v[..., :, d // 2, :, d // 2] = g
    else:
        for a in (d // 2 - 1, d // 2):
            for b in (d // 2 - 1, d // 2):
                v[..., :, a, :, b] = 0.25 * g
    return out


def gram(src, tgt, d=1):
    """(loss, dsrc, dtgt):  Gab = Hc (Xa Xb^T) Hc,  S = sum(Gss^2 + Gtt^2 - 2 Gst^2) / (n-1)^2,  loss = sqrt(S) / (4 D^2),
    d loss / d Xs = k (Gss Xs - Gst Xt),  d loss / d Xt = k (Gtt Xt - Gst^T Xs),  k = 1 / (2 D^2 sqrt(S) (n-1)^2)."""
    xs4, xt4 = down(src, d), down(tgt, d)
    n = xs4.shape[0]
    xs, xt = xs4.reshape(n, -1), xt4.reshape(n, -1)
    D = xs.shape[1]
    hc = torch.eye(n, dtype=xs.dtype) - torch.ones((n, n), dtype=xs.dtype) / n
    gss, gst, gtt = hc @ (xs @ xs.T) @ hc, hc @ (xs @ xt.T) @ hc, hc @ (xt @ xt.T) @ hc
    S = ((gss ** 2).sum() - 2 * (gst ** 2).sum() + (gtt ** 2).sum()) / (n - 1) ** 2
    S = S.clamp(min=0)
    loss = S.sqrt() / (4 * D ** 2)
    k = 1.0 / (2 * D ** 2 * S.sqrt() * (n - 1) ** 2) if float(S) > 0 else 0.0
    ds = k * (gss @ xs - gst @ xt)
    dt = k * (gtt @ xt - gst.T @ xs)
    return loss, _up(ds.reshape(xs4.shape), src.shape, d), _up(dt.reshape(xt4.shape), tgt.shape, d)


def heatmaps(N, K, H, W, seed, sigma=2.0, noise=0.02):
    """(src, tgt) fp64, drawn independently: one Gaussian bump at a random pixel per map plus `noise` * randn."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1), torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    out = []
    for _ in range(2):
        cy = torch.randint(0, H, (N, K, 1, 1), generator=g).double()
        cx = torch.randint(0, W, (N, K, 1, 1), generator=g).double()
        bump = torch.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / (2 * sigma ** 2))
        out.append(bump + noise * torch.randn(N, K, H, W, generator=g, dtype=torch.float64))
    return out[0], out[1]
