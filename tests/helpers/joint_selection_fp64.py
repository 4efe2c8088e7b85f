"""Plain-torch restatements of the joint-selection kernels (csrc/select.hip; definitions in include/udapose.h), written from the
definitions and evaluated in whatever dtype their inputs have - float64 in the tests.

Rows:       joints:  rows[n,k] = 0.5 * w[n,k] * mean_hw((p - g)^2)          cons:  rows[n,k] = m[n,k] * mean_hw((s - t)^2)
Selection:  per sample, joint j is BETTER than joint i when rows[j] > rows[i] (largest; < otherwise) or the two are equal and j < i;
            rank(i) = number of candidates better than i; selected = rank < topk.  A zero-factor row (w == 0 / m == 0) is no candidate
            when largest is False and is never selected in either direction.
Loss:       sample[n] = sum of the selected rows / topk (the divisor stays topk), loss = mean_n sample[n].
Thresholds: thr[j] = the k-th smallest (1-indexed) of pool[:, j]; NaN the largest (torch.kthvalue's order).
"""
import torch


def rows_joints(pred, gt, weight=None):
    N, K = pred.shape[:2]
    r = 0.5 * ((pred - gt) ** 2).reshape(N, K, -1).mean(-1)
    return r if weight is None else r * weight.reshape(N, K).to(r.dtype)


def rows_cons(stu, tea, tea_mask=None):
    N, K = stu.shape[:2]
    r = ((stu - tea) ** 2).reshape(N, K, -1).mean(-1)
    return r if tea_mask is None else r * (tea_mask.reshape(N, K) != 0).to(r.dtype)


def ranks(rows, candidate, largest=True):
    """rank[n,i] = the number of candidates j of sample n that are better than i (the definition above, counted pair by pair)."""
    v = rows.detach()
    vi, vj = v[:, :, None], v[:, None, :]
    K = v.shape[1]
    idx = torch.arange(K)
    first = idx[None, None, :] < idx[None, :, None]            # j < i
    better = (vj > vi) if largest else (vj < vi)
    better = better | ((vj == vi) & first)
    return (better & candidate[:, None, :]).sum(-1)


def select(rows, zero_factor, topk, largest=True):
    """(selection bool [N,K], candidate bool [N,K]) of rows [N,K]; zero_factor bool [N,K] or None."""
    zero = torch.zeros_like(rows, dtype=torch.bool) if zero_factor is None else zero_factor.bool()
    cand = torch.ones_like(zero) if largest else ~zero
    return cand & ~zero & (ranks(rows, cand, largest) < topk), cand


def topk_loss(rows, zero_factor, topk, largest=True):
    """(mean, sample [N], selection): differentiable through the rows, the selection held fixed."""
    sel, _ = select(rows, zero_factor, topk, largest)
    sample = torch.zeros(rows.shape[0], dtype=rows.dtype)
    for k in range(rows.shape[1]):                              # in joint order
        sample = sample + torch.where(sel[:, k], rows[:, k], torch.zeros_like(rows[:, k]))
    sample = sample / topk
    return sample.sum() / rows.shape[0], sample, sel


def joints_ohkm(pred, gt, weight, topk):
    N, K = pred.shape[:2]
    zero = None if weight is None else weight.reshape(N, K) == 0
    return topk_loss(rows_joints(pred, gt, weight), zero, topk, True)


def cons_topk(stu, tea, tea_mask, topk, largest=True):
    N, K = stu.shape[:2]
    zero = None if tea_mask is None else tea_mask.reshape(N, K) == 0
    return topk_loss(rows_cons(stu, tea, tea_mask), zero, topk, largest)


def boundary_gap(rows, zero_factor, topk, largest=True):
    """The smallest relative distance, over ALL samples, between the two rows on either side of the selection boundary - the candidates
    of rank topk - 1 and topk - where both exist and are not both zero (two zero rows tie by index, which is exact in any precision).
    inf when no sample has such a pair."""
    zero = torch.zeros_like(rows, dtype=torch.bool) if zero_factor is None else zero_factor.bool()
    cand = torch.ones_like(zero) if largest else ~zero
    rk = ranks(rows, cand, largest)
    gap = float("inf")
    for n in range(rows.shape[0]):
        inside = rows[n][cand[n] & (rk[n] == topk - 1)]
        outside = rows[n][cand[n] & (rk[n] == topk)]
        if inside.numel() == 0 or outside.numel() == 0:
            continue
        a, b = float(inside[0]), float(outside[0])
        if a == 0.0 and b == 0.0:
            continue
        gap = min(gap, abs(a - b) / max(abs(a), abs(b)))
    return gap


def joint_thresholds(pool, k):
    """thr[j] = k-th smallest of pool[:, j] by an explicit sort of every column (torch.sort puts NaN last, the largest)."""
    return torch.stack([torch.sort(pool[:, j]).values[k - 1] for j in range(pool.shape[1])])


def joint_mask(pool, k, act_local, tea_mask=None):
    thr = joint_thresholds(pool, k)
    a = act_local if tea_mask is None else tea_mask.to(act_local.dtype) * act_local
    return a > thr[None, :], thr
