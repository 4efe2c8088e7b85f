"""The skeleton prior (the reference's generate_prior_map, utils.py:111-145) restated in whatever dtype is asked for (the tests use fp64 as the
truth and fp32 on the CPU as the yardstick of what single precision gives), the pairwise joint-distance statistics in numpy fp64, and the seeded
generator of inputs that tests/golden/make_golden_prior_map.py and the tests share.  CPU only; nothing here touches the package.

  decode(preds)                       get_max_preds_torch: (x, y) of the first flat arg-max, zeroed where the maximum is <= 0; the maxima
  weights(std, gamma, epsilon, v3)    the [K,K] table: soft-max over i of -std / gamma with the diagonal at epsilon, or 1 / (1 + std)
  prior_map(mean, std, preds, ...)    out[b,j] = sum_i f[i,j] exp(-(d_i - mean[i,j])^2 / (2 sigma^2)),  f = w  or  conf_i w[i,j] (v3)
  pair_stats(coords, visible)         count, mean, population std and mean of d^2 per pair over the samples where both joints are visible
"""
import numpy as np
import torch

EPSILON = -10e10        # the reference's default


def decode(preds):
    B, K, H, W = preds.shape
    flat = preds.reshape(B, K, -1)
    idx = flat.argmax(-1)
    conf = flat.amax(-1)
    pos = (conf > 0).to(preds.dtype)
    coords = torch.stack([(idx % W).to(preds.dtype) * pos, torch.div(idx, W, rounding_mode="floor").to(preds.dtype) * pos], -1)
    return coords, conf


def weights(std, gamma=2, epsilon=EPSILON, v3=False):
    if v3:
        return 1 / (1 + std)
    t = -std / gamma
    t = t.clone()
    t.fill_diagonal_(epsilon)
    return torch.softmax(t, dim=0)


def prior_map(mean, std, preds, gamma=2, sigma=2, epsilon=EPSILON, v3=False, coords=None, conf=None, dtype=torch.float64):
    """coords / conf: a decode to use instead of this module's own (the NaN cases feed the device's)."""
    preds = preds.to(dtype)
    mean, std = mean.to(dtype), std.to(dtype)
    B, K, H, W = preds.shape
    if coords is None:
        coords, conf = decode(preds)
    coords, conf = coords.to(dtype), conf.to(dtype)
    f = weights(std, gamma, epsilon, v3)
    xx = torch.arange(W, dtype=dtype).view(1, 1, W)
    yy = torch.arange(H, dtype=dtype).view(1, H, 1)
    out = torch.zeros(B, K, H, W, dtype=dtype)
    for i in range(K):
        d = torch.sqrt((xx - coords[:, i, 0].view(B, 1, 1)) ** 2 + (yy - coords[:, i, 1].view(B, 1, 1)) ** 2)         # [B,H,W]
        t = torch.exp(-((d.unsqueeze(1) - mean[i].view(1, K, 1, 1)) ** 2) / (2 * sigma ** 2))                        # [B,K,H,W]
        fi = f[i].view(1, K, 1, 1)
        if v3:
            fi = fi * conf[:, i].view(B, 1, 1, 1)
        out += fi * t
    return out


def rel_err(got, truth):
    """max|got - truth| / max|truth|, in fp64."""
    got, truth = got.double(), truth.double()
    return float((got - truth).abs().max()) / float(truth.abs().max())


def pair_stats(coords, visible):
    """coords [M,K,2] (fp32 values), visible [M,K] -> fp64 [K,K] arrays: count, mean, population std, mean of d^2.  A pair never seen:
    mean 0, std inf."""
    c = np.asarray(coords, dtype=np.float64)
    v = np.asarray(visible) != 0
    diff = c[:, :, None, :] - c[:, None, :, :]
    d2 = (diff ** 2).sum(-1)
    both = (v[:, :, None] & v[:, None, :]).astype(np.float64)
    n = both.sum(0)
    safe = np.maximum(n, 1.0)
    mu = (np.sqrt(d2) * both).sum(0) / safe
    m2 = (d2 * both).sum(0) / safe
    sd = np.sqrt(np.maximum(m2 - mu ** 2, 0.0))
    return n, np.where(n > 0, mu, 0.0), np.where(n > 0, sd, np.inf), m2


def case_inputs(shape, seed, inf_std=False, negative_row=False):
    """Seeded (preds, mean, std) as fp32 numpy arrays.  preds: noise on a 1/256 grid in [0, 1) with one peak of 2 per plane (no two equal maxima);
    mean: the distances of K random points of the map, stretched by up to 20 %; std in [0.3, 4).  inf_std: a third of the off-diagonal std entries
    are +inf (pairs never seen; mean 0 there); negative_row: plane [0, K-1] is all negative with a single largest pixel."""
    B, K, H, W = shape
    rs = np.random.RandomState(seed)
    preds = (np.floor(rs.rand(B, K, H, W) * 256) / 256).astype(np.float32)
    peak = rs.randint(0, H * W, size=(B, K))
    for b in range(B):
        for k in range(K):
            preds[b, k].reshape(-1)[peak[b, k]] = 2.0
    pts = rs.uniform(0, 1, size=(K, 2)) * np.array([W, H])
    mean = (np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1)) * rs.uniform(0.8, 1.2, size=(K, K))).astype(np.float32)
    std = rs.uniform(0.3, 4.0, size=(K, K)).astype(np.float32)
    if inf_std:
        never = (rs.rand(K, K) < 1 / 3) & ~np.eye(K, dtype=bool)
        std[never], mean[never] = np.inf, 0.0
    if negative_row:
        row = -(1 + np.floor(rs.rand(H * W) * 255)) / 256 - 1 / 256
        row[rs.randint(0, H * W)] = -1 / 512
        preds[0, K - 1] = row.reshape(H, W).astype(np.float32)
    return preds, mean, std


# what the golden file holds: (name, shape, seed, gamma, sigma, inf_std, negative_row); every case is recorded in both modes
GOLDEN_SHAPES = ((1, 1, 1, 1), (2, 3, 5, 7), (1, 21, 17, 17), (3, 18, 16, 16), (2, 16, 24, 32))
SETTINGS = ((2, 2), (0.75, 1.25))          # (gamma, sigma): the reference's defaults and one other


def seed_of(shape):
    return 700 + sum(s * (i + 1) for i, s in enumerate(shape))


def golden_cases():
    cases = [("x".join(map(str, s)), s, seed_of(s), 2, 2, False, False) for s in GOLDEN_SHAPES]
    cases.append(("2x3x5x7_g0.75_s1.25", (2, 3, 5, 7), seed_of((2, 3, 5, 7)), 0.75, 1.25, False, False))
    cases.append(("3x18x16x16_g0.75_s1.25", (3, 18, 16, 16), seed_of((3, 18, 16, 16)), 0.75, 1.25, False, False))
    cases.append(("2x5x7x4_infstd", (2, 5, 7, 4), 811, 2, 2, True, False))
    cases.append(("2x3x5x7_negrow", (2, 3, 5, 7), 812, 2, 2, False, True))
    return cases
