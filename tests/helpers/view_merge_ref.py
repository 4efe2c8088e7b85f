"""numpy restatement of the merge of k teacher views by agreement (udapose_view_merge; definitions in include/udapose.h and DESIGN.md 4.17),
written from the definitions: integers for everything discrete, fp32 in the definition's operation order for `mean`, fp64 for `energy`.

views: a sequence of k arrays [..., H, W] float32 of one shape (the leading dimensions are flattened to R planes and restored).
"""
import collections
import math

import numpy as np

Merged = collections.namedtuple("Merged", "mean peaks maxvals inliers n_inliers spread2 agree energy energy_abs")


def plane_decision(planes, radius, min_views):
    """One (sample, joint) plane of k views [k, H, W] -> (peaks [k][2] (x, y), maxvals [k], inlier bit mask, n_inliers, spread2, agree)."""
    k, H, W = planes.shape
    peaks, maxvals, valid = [], [], []
    for v in range(k):
        idx = int(np.argmax(planes[v]))                  # the first flat index of the maximum, row-major
        peaks.append((idx % W, idx // W))
        maxvals.append(planes[v].reshape(-1)[idx])
        valid.append(bool(maxvals[-1] > 0))
    d2 = [[(peaks[a][0] - peaks[b][0]) ** 2 + (peaks[a][1] - peaks[b][1]) ** 2 for b in range(k)] for a in range(k)]
    vs = [v for v in range(k) if valid[v]]
    spread2 = max([d2[a][b] for a in vs for b in vs], default=0)
    mask = 0
    if vs:
        sums = [sum(d2[a][b] for b in vs) for a in vs]
        medoid = vs[sums.index(min(sums))]               # (index of the FIRST minimum: the lowest view on a tie)
        with np.errstate(over="ignore", invalid="ignore"):
            r = np.float32(radius)
            r2 = np.float32(r * r)                       # the product in fp32
            for v in vs:
                if np.float32(d2[v][medoid]) <= r2:
                    mask |= 1 << v
    n = bin(mask).count("1")
    return peaks, maxvals, mask, n, spread2, 1.0 if n >= min_views else 0.0


def _mean32(planes, members):
    """((v_a + v_b) + ...) / (float)len over `members` in view order, every operation rounded to fp32."""
    acc = planes[members[0]].astype(np.float32)
    for v in members[1:]:
        acc = (acc + planes[v]).astype(np.float32)
    return (acc / np.float32(len(members))).astype(np.float32)


def merge(views, radius=2.0, mode="mean", min_views=None, want_energy=False):
    assert mode in ("mean", "trimmed")
    vs = np.stack([np.asarray(v, dtype=np.float32) for v in views])          # [k, ..., H, W]
    k, lead, (H, W) = vs.shape[0], vs.shape[1:-2], vs.shape[-2:]
    min_views = k if min_views is None else int(min_views)
    assert 1 <= k <= 8 and 1 <= min_views <= k
    x = vs.reshape(k, -1, H, W)
    R = x.shape[1]
    mean = np.empty((R, H, W), np.float32)
    peaks = np.zeros((k, R, 2), np.int32)
    maxvals = np.zeros((k, R), np.float32)
    inliers, n_inliers, spread2 = np.zeros(R, np.int32), np.zeros(R, np.int32), np.zeros(R, np.int32)
    agree = np.zeros(R, np.float32)
    for r in range(R):
        p, m, mask, n, s2, ag = plane_decision(x[:, r], radius, min_views)
        peaks[:, r], maxvals[:, r] = np.asarray(p, np.int32), np.asarray(m, np.float32)
        inliers[r], n_inliers[r], spread2[r], agree[r] = mask, n, s2, ag
        members = [v for v in range(k) if (mask >> v) & 1] if (mode == "trimmed" and n > 0) else list(range(k))
        mean[r] = _mean32(x[:, r], members)
    energy = energy_abs = None
    if want_energy:
        x64 = x.astype(np.float64)
        m64 = x64.sum(0) / k
        energy = (((x64 - m64) ** 2).sum(0) / k).mean((-2, -1)).reshape(lead)
        energy_abs = (((np.abs(x64) + np.abs(m64)) ** 2).sum(0) / k).mean((-2, -1)).reshape(lead)      # what the rounding bound scales with
    return Merged(mean.reshape(lead + (H, W)), peaks.reshape((k,) + lead + (2,)), maxvals.reshape((k,) + lead), inliers.reshape(lead),
                  n_inliers.reshape(lead), spread2.reshape(lead), agree.reshape(lead), energy, energy_abs)


def energy_bound(k, H, W, energy_abs):
    """|energy_fp32 - energy_fp64| <= (4k + 8 + ceil(log2(H*W))) * 2^-23 * E_abs: a derived rounding bound (k roundings in m, which enter
    every difference twice; the difference, the square, the k-term sum and the division; a pairwise sum over H*W pixels; the final cast)."""
    return (4 * k + 8 + math.ceil(math.log2(H * W))) * 2.0 ** -23 * energy_abs


# ---------------------------------------------------------------------------------------------- constructed planes
CONSTRUCTED = ("outlier", "first_index_tie", "medoid_tie", "on_radius", "invalid_view", "none_valid")
CONSTRUCTED_RADIUS = 2.0           # the radius the constructed planes are written for ("on_radius": a peak exactly 2 pixels from the medoid)


def _peaked(H, W, x, y, height=1.0, floor=0.0):
    p = np.full((H, W), floor, np.float32)
    p[y % H, x % W] = height
    return p


def constructed_plane(name, k, H, W):
    """k views [k, H, W] of one plane.  Positions are taken modulo the plane, so that every case exists at every size (on a plane too small
    for it a case degenerates, and the restatement says what is expected there)."""
    if name == "outlier":              # every view at (2, 3) but the last, which sits far away
        return np.stack([_peaked(H, W, 2, 3, 1.0 + 0.125 * v) for v in range(k - 1)] + [_peaked(H, W, W - 1, H - 1, 0.75)])
    if name == "first_index_tie":      # two equal maxima in view 0: the first flat index (the upper row) is the peak
        views = [_peaked(H, W, 3, 2, 0.5) for _ in range(k)]
        views[0][(H - 1) % H, 1 % W] = 0.5
        views[0][2 % H, 3 % W] = 0.5
        views[0][1 % H, 4 % W] = 0.5   # flat index (1, 4) < (2, 3) < (H - 1, 1) wherever the plane holds them apart
        return np.stack(views)
    if name == "medoid_tie":           # peaks (0,0), (2,0), (1,3), (1,3)...: views 0 and 1 tie on the sum of squared distances with k = 3
        pos = [(0, 0), (2, 0)] + [(1, 3)] * max(k - 2, 0)
        return np.stack([_peaked(H, W, *pos[v], 1.0) for v in range(k)])
    if name == "on_radius":            # view 1 exactly CONSTRUCTED_RADIUS from the others: d2 == r * r is inside
        return np.stack([_peaked(H, W, 4 if v == 1 else 2, 1, 1.0) for v in range(k)])
    if name == "invalid_view":         # view 0 is non-positive everywhere (its maximum is 0): not valid
        return np.stack([_peaked(H, W, 1, 1, 0.0, floor=-1.0)] + [_peaked(H, W, 3, 3, 1.0) for _ in range(k - 1)])
    if name == "none_valid":
        return np.stack([_peaked(H, W, v, 0, -0.25 if v % 2 else 0.0, floor=-1.0) for v in range(k)])
    raise KeyError(name)
