"""Plain-torch restatement of the soft-max heat-map losses (JointsKLLoss, EntLoss, ConsSoftmaxLoss, ConsKLLoss of
lib/models/loss.py), written from their formulas.  It runs in whatever dtype its inputs have: in fp64 it is the oracle of the
device tests (tests/test_softmax_losses_cpu.py pins it to the reference's recorded results first), in fp32 it is the
"reference arithmetic" whose own error against fp64 sets the device's bound.
"""
import math

import torch


def _rows(x):
    B, K = x.shape[:2]
    return x.reshape(B, K, -1)


def joints_kl(output, target, target_weight=None, reduction="mean", epsilon=0.0):
    B, K = output.shape[:2]
    lp = torch.log_softmax(_rows(output), dim=-1)
    q = _rows(target) + epsilon
    q = q / q.sum(dim=-1, keepdim=True)
    loss = (torch.xlogy(q, q) - q * lp).sum(dim=-1)
    if target_weight is not None:
        loss = loss * target_weight.reshape(B, K)
    if reduction == "mean":
        return loss.mean()
    if reduction == "none":
        return loss.mean(dim=-1)
    return None


def entropy(x, threshold=-1, reduction="mean"):
    rows = _rows(x)
    lp = torch.log_softmax(rows, dim=-1)
    ent = -(lp.exp() * lp).sum(dim=-1) / math.log(rows.shape[-1])
    if threshold > 0:
        ent = ent[ent < threshold]
    if reduction == "mean":
        return ent.mean()
    if reduction == "none":
        return ent.mean(dim=-1)
    return None


def _reduce_map(per_elem, shape, valid_mask, tea_mask):
    """[B,K,HW] per-element losses -> mask by (b,k), mean over K, optional (b,h,w) selection, mean."""
    m = per_elem.reshape(shape)
    if tea_mask is not None:
        m = m * (tea_mask != 0).to(m.dtype)[:, :, None, None]
    m = m.mean(dim=1)
    if valid_mask is not None:
        m = m[valid_mask != 0]
    return m.mean()


def cons_softmax(stu, tea, valid_mask=None, tea_mask=None):
    p, pt = torch.softmax(_rows(stu), dim=-1), torch.softmax(_rows(tea), dim=-1)
    d = p - pt
    if tea_mask is not None:
        d = d * (tea_mask != 0).to(d.dtype)[:, :, None]
    return _reduce_map(d * d, stu.shape, valid_mask, None)


def cons_kl(stu, tea, valid_mask=None, tea_mask=None, log_target=False):
    """log_target=False is the reference as written: the teacher's LOG-probabilities t go where KLDivLoss expects probabilities,
    xlogy(t, t) - t * log p with t < 0: NaN wherever the teacher's probability is not exactly 1.  log_target=True is the KL
    divergence pt * (log pt - log p)."""
    lp, lt = torch.log_softmax(_rows(stu), dim=-1), torch.log_softmax(_rows(tea), dim=-1)
    e = lt.exp() * (lt - lp) if log_target else torch.xlogy(lt, lt) - lt * lp
    return _reduce_map(e, stu.shape, valid_mask, tea_mask)
