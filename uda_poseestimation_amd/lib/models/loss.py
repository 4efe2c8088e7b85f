"""Heat-map losses (API mirror of the reference's lib/models/loss.py) on MI355X kernels.

JointsMSELoss and ConsLoss are what the training scripts instantiate (train_human.py:133-134).  JointsKLLoss, EntLoss,
ConsSoftmaxLoss and ConsKLLoss (loss.py:52-173) are the soft-max family a user swaps in (csrc/softmax_loss.hip: a row
soft-max over the H*W pixels of every (b,k) heat-map fused with the loss, its reduction and its backward).  CoralLoss is
defined and refuses construction: see its docstring; GramCoralLoss is the same loss through n x n Gram matrices (csrc/coral.hip).
JointsSoftArgmaxLoss and ConsSoftArgmaxLoss have no counterpart in the reference:
they are losses on the soft-argmax COORDINATES of the student's heat-maps (csrc/softargmax.hip), a gradient on where the peak is.
JointsOHKMMSELoss and ConsTopKLoss train only the `topk` joints of every sample that an order statistic over the rows of JointsMSELoss /
ConsLoss selects (csrc/select.hip: hard key-point mining, small-loss selection).
Each forward is one sweep over the operands (per-(b,k) row partial + a tiny row reduction), each backward one sweep.
"""
import warnings

import torch
import torch.nn as nn

from ... import _hip
from ... import heatmap_args as ha
from ..._hip import check, lib, ptr
from ..keypoint_detection import _decode, _soft_args, soft_argmax


def _reduce_mean(reduction):
    """True for 'mean', False for 'none'.  Any other string: None, and the module's forward returns None - as the reference silently does
    (loss.py:46-49, 92-95)."""
    return True if reduction == 'mean' else False if reduction == 'none' else None


def _mean_only(ctx):
    if not ctx.reduce_mean:
        raise NotImplementedError("backward of reduction='none' is not on the hot path")


def _joints_mse_fwd(o, t, w, want_mean=True):
    """udapose_joints_mse_fwd on fp32 contiguous operands: (rows [R], their mean or None)."""
    R, HW = ha.rows(o)
    rows = torch.empty(R, dtype=torch.float32, device=o.device)
    mean = torch.empty((), dtype=torch.float32, device=o.device) if want_mean else None
    check(lib().udapose_joints_mse_fwd(_hip.stream(), ptr(o), ptr(t), ptr(w), R, HW, ptr(rows), ptr(mean)), "joints_mse_fwd")
    return rows, mean


def _cons_fwd(s, t, m=None, want_mean=True):
    """udapose_cons_loss_fwd on fp32 contiguous operands: (rows [R], their mean or None).  (Style_net's nn.MSELoss is this without a mask.)"""
    R, HW = ha.rows(s)
    rows = torch.empty(R, dtype=torch.float32, device=s.device)
    mean = torch.empty((), dtype=torch.float32, device=s.device) if want_mean else None
    check(lib().udapose_cons_loss_fwd(_hip.stream(), ptr(s), ptr(t), ptr(m), R, HW, ptr(rows), ptr(mean)), "cons_loss_fwd")
    return rows, mean


class _JointsMSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target, weight, reduce_mean):
        _hip.require_cuda(output, target, weight)
        w = ha.bk_factor(weight, ha.rows(output)[0])
        o, t = ha.f32c(output), ha.f32c(target)
        rows, mean = _joints_mse_fwd(o, t, w)
        ctx.save_for_backward(o, t, w)
        ctx.reduce_mean, ctx.shape, ctx.in_dtype = reduce_mean, output.shape, output.dtype
        return mean if reduce_mean else rows.reshape(output.shape[0], output.shape[1])

    @staticmethod
    def backward(ctx, g):
        o, t, w = ctx.saved_tensors
        _mean_only(ctx)
        R, HW = ha.rows(o)
        d = torch.empty_like(o)
        check(lib().udapose_joints_mse_bwd(_hip.stream(), ptr(o), ptr(t), ptr(w), ptr(ha.gscale(g)), R, HW, ptr(d)), "joints_mse_bwd")
        return ha.grad_like_input(ctx, d), None, None, None


class JointsMSELoss(nn.Module):
    """0.5 * (pred - gt)^2 * target_weight[b,k], mean over everything ('mean') or per-(b,k) means ('none')."""

    def __init__(self, reduction='mean'):
        super(JointsMSELoss, self).__init__()
        self.reduction = reduction

    def forward(self, output, target, target_weight=None):
        mean = _reduce_mean(self.reduction)
        return None if mean is None else _JointsMSEFn.apply(output, target, target_weight, mean)


class _ConsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stu, tea, mask, valid):
        _hip.require_cuda(stu, tea, mask, valid)
        R, HW = ha.rows(stu)
        m = ha.bk_mask(mask, R)
        s, t = ha.f32c(stu), ha.f32c(tea)
        v, cnt = ha.valid_selection(valid, stu)
        if v is None:
            mean = _cons_fwd(s, t, m)[1]
        else:
            rows = torch.empty(R, dtype=torch.float32, device=s.device)
            mean = torch.empty((), dtype=torch.float32, device=s.device)
            check(lib().udapose_cons_loss_valid_fwd(_hip.stream(), ptr(s), ptr(t), ptr(m), ptr(v), ptr(cnt), R, stu.shape[1], HW, ptr(rows),
                                                    ptr(mean)), "cons_loss_valid_fwd")
        ctx.save_for_backward(s, t, m, v, cnt)
        ctx.shape, ctx.in_dtype = stu.shape, stu.dtype
        return mean

    @staticmethod
    def backward(ctx, g):
        s, t, m, v, cnt = ctx.saved_tensors
        R, HW = ha.rows(s)
        d = torch.empty_like(s)
        gs = ha.gscale(g)
        if v is not None:
            check(lib().udapose_cons_loss_valid_bwd(_hip.stream(), ptr(s), ptr(t), ptr(m), ptr(v), ptr(cnt), ptr(gs), R, ctx.shape[1], HW, ptr(d)),
                  "cons_loss_valid_bwd")
        else:
            check(lib().udapose_cons_loss_bwd(_hip.stream(), ptr(s), ptr(t), ptr(m), ptr(gs), R, HW, ptr(d)), "cons_loss_bwd")
        return ha.grad_like_input(ctx, d), None, None, None


class ConsLoss(nn.Module):
    """mean over (b,h,w) of mean_c (mask[b,c] * (stu - tea))^2  ==  sum(mask*(stu-tea)^2) / (B*C*H*W); with `valid_mask`
    (bool [B,H,W]) the mean runs over the selected positions only (loss.py:129-130)."""

    def __init__(self):
        super(ConsLoss, self).__init__()

    def forward(self, stu_out, tea_out, valid_mask=None, tea_mask=None):
        return _ConsFn.apply(stu_out, tea_out, tea_mask, valid_mask)


# ---------------------------------------------------------------------------------------------- top-k joint mining
TOPK_MAX_KEYPOINTS = 64     # udapose_topk_select: a wave holds a sample, a lane a joint


def _topk_args(x, topk):
    """(N, K, topk) of a [N,K,...] heat-map batch, or ValueError - before any launch."""
    if x.dim() < 3:
        raise ValueError(f"top-k joint mining needs [N, K, ...] heat-maps, got {tuple(x.shape)}")
    N, K = x.shape[:2]
    if int(topk) != topk or topk < 1:
        raise ValueError(f"topk must be an integer >= 1, got {topk!r}")
    if K > TOPK_MAX_KEYPOINTS:
        raise ValueError(f"top-k joint mining serves K <= {TOPK_MAX_KEYPOINTS} key points, got {K}")
    if topk > K:
        raise ValueError(f"topk = {topk} exceeds the {K} key points of the heat-maps")
    if N < 1 or x.numel() == 0:
        raise ValueError(f"top-k joint mining: empty heat-maps {tuple(x.shape)}")
    return N, K, int(topk)


class _TopKSqdiffFn(torch.autograd.Function):
    """The rows of _JointsMSEFn (cons == False: factor = weight) or _ConsFn (cons == True: factor = mask), then udapose_topk_select over
    them; backward is the squared-difference sweep with the selection as its mask."""

    @staticmethod
    def forward(ctx, a, b, factor, topk, largest, cons, reduce_mean, owner):
        N, K, topk = _topk_args(a, topk)
        _hip.require_cuda(a, b, factor)
        R = N * K
        w = None if cons else ha.bk_factor(factor, R)
        m = ha.bk_mask(factor, R) if cons else None
        x, y = ha.f32c(a), ha.f32c(b)
        rows = (_cons_fwd(x, y, m, want_mean=False) if cons else _joints_mse_fwd(x, y, w, want_mean=False))[0]
        sel = torch.empty(R, dtype=torch.uint8, device=x.device)
        sample = torch.empty(N, dtype=torch.float32, device=x.device)
        mean = torch.empty((), dtype=torch.float32, device=x.device) if reduce_mean else None
        check(lib().udapose_topk_select(_hip.stream(), ptr(rows), ptr(w), ptr(m), N, K, topk, int(bool(largest)), ptr(sel), ptr(sample), ptr(mean)),
              "topk_select")
        if owner is not None:
            owner.last_selection = sel.view(torch.bool).reshape(N, K)       # (the kernel writes 0 / 1: a bool view, not a conversion launch)
        ctx.save_for_backward(x, y, w, sel)
        ctx.cons, ctx.topk, ctx.reduce_mean, ctx.shape, ctx.in_dtype = cons, topk, reduce_mean, a.shape, a.dtype
        return mean if reduce_mean else sample

    @staticmethod
    def backward(ctx, g):
        x, y, w, sel = ctx.saved_tensors
        _mean_only(ctx)
        N, K = ctx.shape[:2]
        d = torch.empty_like(x)
        check(lib().udapose_topk_sqdiff_bwd(_hip.stream(), ptr(x), ptr(y), ptr(w), ptr(sel), ptr(ha.gscale(g)), N, K, ha.rows(x)[1], ctx.topk,
                                            0 if ctx.cons else 1, ptr(d)), "topk_sqdiff_bwd")
        return ha.grad_like_input(ctx, d), None, None, None, None, None, None, None


class JointsOHKMMSELoss(nn.Module):
    """Online hard key-point mining over JointsMSELoss's rows (the OHKM loss of the Simple-Baseline code this PoseResNet comes from):
    mean_n( (1/topk) * sum_{k in top-k of n} 0.5 * w[n,k] * mean_hw((p - g)^2) ), the `topk` joints of every sample with the LARGEST row.
    The rows are exactly JointsMSELoss(reduction='none')'s, so target_weight enters ONCE, as everywhere in this package; the MSRA code
    multiplies prediction and target by it before squaring, i.e. squares it - identical for the 0 / 1 weights the data pipeline emits.
    Ties go to the lower joint index.  A joint of weight 0 keeps its place in the order (its row is 0) and is never selected, so fewer
    than topk joints may train; the divisor stays topk.  reduction='none' returns the per-sample values [N] (forward only).
    `last_selection`: the selection of the last forward, a detached bool [N,K] device tensor (for logging; no synchronisation).
    topk is read at every call and is baked into a captured step's launches: build a new capture to change it."""

    def __init__(self, topk=8, reduction='mean'):
        super(JointsOHKMMSELoss, self).__init__()
        if int(topk) != topk or topk < 1:
            raise ValueError(f"topk must be an integer >= 1, got {topk!r}")
        self.topk, self.reduction = int(topk), reduction
        self.last_selection = None

    def forward(self, output, target, target_weight=None):
        mean = _reduce_mean(self.reduction)
        return None if mean is None else _TopKSqdiffFn.apply(output, target, target_weight, self.topk, True, False, mean, self)


class ConsTopKLoss(nn.Module):
    """The same selection over ConsLoss's rows m[n,k] * mean_hw((stu - tea)^2): mean_n( (1/topk) * sum over the selected joints ).
    largest=True trains the `topk` joints of a sample where student and teacher disagree MOST; largest=False the `topk` where they disagree
    LEAST among the joints tea_mask admits (small-loss selection for noisy pseudo-labels).  A joint the mask rejects is never selected;
    fewer than topk joints may train and the divisor stays topk.  Ties go to the lower joint index.  The selection is per (sample, joint):
    a per-pixel `valid_mask` is refused.  `last_selection` as in JointsOHKMMSELoss; topk and largest are baked into a captured step."""

    def __init__(self, topk=8, largest=True):
        super(ConsTopKLoss, self).__init__()
        if int(topk) != topk or topk < 1:
            raise ValueError(f"topk must be an integer >= 1, got {topk!r}")
        self.topk, self.largest = int(topk), bool(largest)
        self.last_selection = None

    def forward(self, stu_out, tea_out, valid_mask=None, tea_mask=None):
        if valid_mask is not None:
            raise NotImplementedError("ConsTopKLoss selects (sample, joint) rows: a per-pixel valid_mask is not implemented (use tea_mask)")
        return _TopKSqdiffFn.apply(stu_out, tea_out, tea_mask, self.topk, self.largest, True, True, self)


# ---------------------------------------------------------------------------------------------- the soft-max family
class _JointsKLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target, weight, reduce_mean, eps):
        _hip.require_cuda(output, target, weight)
        R, HW = ha.rows(output)
        B, K = output.shape[:2]
        w = ha.bk_factor(weight, R)
        o, t = ha.f32c(output), ha.f32c(target)
        rows = torch.empty(R, dtype=torch.float32, device=o.device)
        stats = torch.empty(5 * R, dtype=torch.float32, device=o.device)
        out = torch.empty(() if reduce_mean else (B,), dtype=torch.float32, device=o.device)
        check(lib().udapose_joints_kl_fwd(_hip.stream(), ptr(o), ptr(t), ptr(w), eps, R, R if reduce_mean else K, HW, ptr(rows), ptr(stats),
                                          ptr(out)), "joints_kl_fwd")
        ctx.save_for_backward(o, t, w, stats)
        ctx.reduce_mean, ctx.eps, ctx.shape, ctx.in_dtype = reduce_mean, eps, output.shape, output.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        o, t, w, stats = ctx.saved_tensors
        _mean_only(ctx)
        R, HW = ha.rows(o)
        d = torch.empty_like(o)
        check(lib().udapose_joints_kl_bwd(_hip.stream(), ptr(o), ptr(t), ptr(w), ctx.eps, ptr(stats), ptr(ha.gscale(g)), R, HW, ptr(d)),
              "joints_kl_bwd")
        return ha.grad_like_input(ctx, d), None, None, None, None


class JointsKLLoss(nn.Module):
    """KL(q || softmax(pred)) per (b,k) heat-map, q = (gt + epsilon) / sum(gt + epsilon), times target_weight[b,k] (RegDA's supervised
    loss, loss.py:52-95): the mean over the B*K maps ('mean') or the reference's `loss.mean(dim=-1)`, shape [B] ('none')."""

    def __init__(self, reduction='mean', epsilon=0.):
        super(JointsKLLoss, self).__init__()
        self.reduction = reduction
        self.epsilon = epsilon

    def forward(self, output, target, target_weight=None):
        mean = _reduce_mean(self.reduction)
        return None if mean is None else _JointsKLFn.apply(output, target, target_weight, mean, float(self.epsilon))


class _EntFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, threshold, reduce_mean):
        _hip.require_cuda(x)
        R, HW = ha.rows(x)
        B, K = x.shape[:2]
        s = ha.f32c(x)
        thr = float(threshold) if threshold > 0 else 0.0
        scalar = reduce_mean or thr > 0        # (a threshold makes the selection 1-D: its mean(dim=-1) is a scalar too, loss.py:111-117)
        rows = torch.empty(R, dtype=torch.float32, device=s.device)
        stats = torch.empty(4 * R, dtype=torch.float32, device=s.device)
        out = torch.empty(() if scalar else (B,), dtype=torch.float32, device=s.device)
        cnt = torch.empty((), dtype=torch.float32, device=s.device)
        check(lib().udapose_entropy_loss_fwd(_hip.stream(), ptr(s), R, R if scalar else K, HW, thr, ptr(rows), ptr(stats), ptr(out), ptr(cnt)),
              "entropy_loss_fwd")
        ctx.save_for_backward(s, rows, stats, cnt)
        ctx.thr, ctx.scalar, ctx.shape, ctx.in_dtype = thr, scalar, x.shape, x.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        s, rows, stats, cnt = ctx.saved_tensors
        if not ctx.scalar:
            raise NotImplementedError("backward of reduction='none' is not on the hot path")
        R, HW = ha.rows(s)
        d = torch.empty_like(s)
        check(lib().udapose_entropy_loss_bwd(_hip.stream(), ptr(s), ptr(rows), ptr(stats), ptr(cnt), ptr(ha.gscale(g)), ctx.thr, R, HW, ptr(d)),
              "entropy_loss_bwd")
        return ha.grad_like_input(ctx, d), None, None


class EntLoss(nn.Module):
    """Entropy of softmax(x) over the pixels of every (b,k) map, divided by log(H*W) (loss.py:97-117).  threshold > 0 keeps the maps
    whose entropy is below it (counted on the device; none kept: NaN, as the mean of an empty tensor)."""

    def __init__(self, reduction='mean'):
        super(EntLoss, self).__init__()
        self.reduction = reduction

    def forward(self, x, threshold=-1):
        mean = _reduce_mean(self.reduction)
        return None if mean is None else _EntFn.apply(x, threshold, mean)


class _ConsProbFn(torch.autograd.Function):
    """mode 0: ConsSoftmaxLoss; 1: ConsKLLoss(log_target=True); 2: ConsKLLoss as the reference evaluates it."""

    @staticmethod
    def forward(ctx, stu, tea, mask, valid, mode):
        _hip.require_cuda(stu, tea, mask, valid)
        R, HW = ha.rows(stu)
        K = stu.shape[1]
        m = ha.bk_mask(mask, R)
        s, t = ha.f32c(stu), ha.f32c(tea)
        v, cnt = ha.valid_selection(valid, stu)
        rows = torch.empty(R, dtype=torch.float32, device=s.device)
        stats = torch.empty(7 * R, dtype=torch.float32, device=s.device)
        out = torch.empty((), dtype=torch.float32, device=s.device)
        if mode == 0:
            check(lib().udapose_cons_softmax_fwd(_hip.stream(), ptr(s), ptr(t), ptr(m), ptr(v), ptr(cnt), R, K, HW, ptr(rows), ptr(stats),
                                                 ptr(out)), "cons_softmax_fwd")
        else:
            check(lib().udapose_cons_kl_fwd(_hip.stream(), ptr(s), ptr(t), ptr(m), ptr(v), ptr(cnt), int(mode == 1), R, K, HW, ptr(rows),
                                            ptr(stats), ptr(out)), "cons_kl_fwd")
        ctx.save_for_backward(s, t, m, v, cnt, stats)
        ctx.mode, ctx.shape, ctx.in_dtype = mode, stu.shape, stu.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        s, t, m, v, cnt, stats = ctx.saved_tensors
        R, HW = ha.rows(s)
        K = ctx.shape[1]
        d = torch.empty_like(s)
        gs = ha.gscale(g)
        if ctx.mode == 0:
            check(lib().udapose_cons_softmax_bwd(_hip.stream(), ptr(s), ptr(t), ptr(m), ptr(v), ptr(cnt), ptr(stats), ptr(gs), R, K, HW, ptr(d)),
                  "cons_softmax_bwd")
        else:
            check(lib().udapose_cons_kl_bwd(_hip.stream(), ptr(s), ptr(t), ptr(m), ptr(v), ptr(cnt), int(ctx.mode == 1), ptr(stats), ptr(gs), R, K,
                                            HW, ptr(d)), "cons_kl_bwd")
        return ha.grad_like_input(ctx, d), None, None, None, None


class ConsSoftmaxLoss(nn.Module):
    """ConsLoss on probabilities: both heat-maps go through a soft-max over their pixels first (loss.py:134-152)."""

    def __init__(self):
        super(ConsSoftmaxLoss, self).__init__()

    def forward(self, stu_out, tea_out, valid_mask=None, tea_mask=None):
        return _ConsProbFn.apply(stu_out, tea_out, tea_mask, valid_mask, 0)


class ConsKLLoss(nn.Module):
    """The reference's ConsKLLoss (loss.py:154-173) hands nn.KLDivLoss (log_target=False) the teacher's LOG-probabilities as its target:
    it evaluates xlogy(t, t) - t * log p with t = log pt < 0, and the logarithm of a negative number is NaN.  Run on the CPU, the
    reference returns NaN for every input of more than one pixel (tests/golden/softmax_losses.npz records it).  ConsKLLoss() reproduces
    that arithmetic literally, as this package does with the reference's other quirks, and warns once.
    ConsKLLoss(log_target=True) is an EXTENSION (the reference's constructor takes no argument): the divergence the code evidently
    intends, mean over (b,h,w) of mean_k tea_mask[b,k] * pt * (log pt - log p), with the same valid_mask selection."""
    _warned = False

    def __init__(self, log_target=False):
        super(ConsKLLoss, self).__init__()
        self.log_target = bool(log_target)

    def forward(self, stu_out, tea_out, valid_mask=None, tea_mask=None):
        if not self.log_target and not ConsKLLoss._warned:
            ConsKLLoss._warned = True
            warnings.warn("ConsKLLoss() mirrors the reference, whose KLDivLoss takes the teacher's log-probabilities as probabilities: the loss "
                          "is NaN for every heat-map of more than one pixel.  ConsKLLoss(log_target=True) computes the KL divergence.",
                          RuntimeWarning, stacklevel=2)
        return _ConsProbFn.apply(stu_out, tea_out, tea_mask, valid_mask, 1 if self.log_target else 2)


# ---------------------------------------------------------------------------------------------- coordinate losses (soft-argmax)
_NORMS = {"l1": 0, "l2": 1}


class _CoordLossFn(torch.autograd.Function):
    """f_r * (l((cx - tx) / W) + l((cy - ty) / H)) per (b,k) row, (cx, cy) the soft-argmax of the row; f_r = weight[r] * (mask[r] != 0)."""

    @staticmethod
    def forward(ctx, output, coords, weight, mask, reduce_mean, beta, window, norm):
        _hip.require_cuda(output, coords, weight, mask)
        B, K, H, W = output.shape
        R = B * K
        if coords.numel() != 2 * R:
            raise ValueError("target coordinates must be [B,K,2]")
        w = ha.bk_factor(weight, R)
        m = ha.bk_mask(mask, R, "the (b,k) mask")
        o, t = ha.f32c(output), ha.f32c(coords)
        rows = torch.empty(R, dtype=torch.float32, device=o.device)
        idx = torch.empty(R, dtype=torch.int32, device=o.device)
        stats = torch.empty(4 * R, dtype=torch.float32, device=o.device)
        out = torch.empty(() if reduce_mean else (B,), dtype=torch.float32, device=o.device)
        check(lib().udapose_coord_loss_fwd(_hip.stream(), ptr(o), ptr(t), ptr(w), ptr(m), R, R if reduce_mean else K, H, W, beta, window, norm,
                                           ptr(rows), ptr(idx), ptr(stats), ptr(out)), "coord_loss_fwd")
        ctx.save_for_backward(o, t, w, m, idx, stats)
        ctx.reduce_mean, ctx.shape, ctx.in_dtype = reduce_mean, output.shape, output.dtype
        ctx.beta, ctx.window, ctx.norm = beta, window, norm
        return out

    @staticmethod
    def backward(ctx, g):
        o, t, w, m, idx, stats = ctx.saved_tensors
        _mean_only(ctx)
        B, K, H, W = ctx.shape
        d = torch.empty_like(o)
        check(lib().udapose_coord_loss_bwd(_hip.stream(), ptr(o), ptr(t), ptr(w), ptr(m), ptr(idx), ptr(stats), ptr(ha.gscale(g)), B * K, H, W,
                                           ctx.beta, ctx.window, ctx.norm, ptr(d)), "coord_loss_bwd")
        return ha.grad_like_input(ctx, d), None, None, None, None, None, None, None


def _coord_args(beta, window, norm):
    if norm not in _NORMS:
        raise ValueError(f"norm must be 'l1' or 'l2', got {norm!r}")
    return _soft_args(beta, window) + (_NORMS[norm],)


def _argmax_decode(hm):
    """(coords [B,K,2], maxvals [B,K,1]) of get_max_preds, on fp32 rows and without a graph."""
    _hip.require_cuda(hm)
    with torch.no_grad():
        return _decode(ha.f32c(hm))


class JointsSoftArgmaxLoss(nn.Module):
    """Supervised loss on the soft-argmax coordinates of `output` (lib.keypoint_detection.soft_argmax(output, beta, window)):
    target_weight[b,k] * (l((cx - tx) / W) + l((cy - ty) / H)) per key point, l = |d| (norm='l1') or 0.5 d^2 ('l2'); the mean over the
    B*K key points ('mean') or per-sample means, shape [B] ('none', forward only), the conventions of JointsMSELoss.
    `target` is [B,K,2] (x, y) in heat-map pixels, or [B,K,H,W] heat-maps: those are decoded by the arg-max kernel, and a key point
    whose target maximum is <= 0 gets factor 0 (it carries no position).  MSE-trained maps need a window (beta=10, window=5).
    beta, window and norm are read at every call and are baked into a captured step's launches: build a new capture to change them."""

    def __init__(self, beta=10.0, window=None, norm="l1", reduction='mean'):
        super(JointsSoftArgmaxLoss, self).__init__()
        _coord_args(beta, window, norm)
        self.beta, self.window, self.norm, self.reduction = beta, window, norm, reduction

    def forward(self, output, target, target_weight=None):
        mean = _reduce_mean(self.reduction)
        if mean is None:
            return None
        beta, window, norm = _coord_args(self.beta, self.window, self.norm)
        present = None
        if target.dim() == 4:
            target, maxv = _argmax_decode(target)
            present = maxv > 0
        return _CoordLossFn.apply(output, target, target_weight, present, mean, beta, window, norm)


class ConsSoftArgmaxLoss(nn.Module):
    """Consistency on coordinates: the student's soft-argmax coordinates against the teacher's decoded ones (never a gradient into the
    teacher), tea_mask[b,k] * (l((cx - tx) / W) + l((cy - ty) / H)), mean over all B*K key points as in ConsLoss.  tea_decode='argmax'
    takes get_max_preds's coordinates of `tea_out` ((0, 0) where its maximum is <= 0), 'soft' the soft-argmax with this loss's beta and
    window.  A pixel selection has no meaning for a coordinate: a `valid_mask` is refused.
    beta, window, norm and tea_decode are baked into a captured step's launches: build a new capture to change them."""

    def __init__(self, beta=10.0, window=None, norm="l1", tea_decode="argmax"):
        super(ConsSoftArgmaxLoss, self).__init__()
        _coord_args(beta, window, norm)
        if tea_decode not in ("argmax", "soft"):
            raise ValueError(f"tea_decode must be 'argmax' or 'soft', got {tea_decode!r}")
        self.beta, self.window, self.norm, self.tea_decode = beta, window, norm, tea_decode

    def forward(self, stu_out, tea_out, valid_mask=None, tea_mask=None):
        if valid_mask is not None:
            raise ValueError("ConsSoftArgmaxLoss compares coordinates: a per-pixel valid_mask selects nothing there (use tea_mask)")
        beta, window, norm = _coord_args(self.beta, self.window, self.norm)
        if self.tea_decode == "argmax":
            tea_xy, _ = _argmax_decode(tea_out)
        else:
            with torch.no_grad():
                tea_xy, _ = soft_argmax(tea_out.detach(), beta, None if window < 0 else window)
        return _CoordLossFn.apply(stu_out, tea_xy, None, tea_mask, True, beta, window, norm)


class CoralLoss(nn.Module):
    """Not available.  The reference's CoralLoss (loss.py:176-208) forms the covariance of the flattened heat-maps, a
    (K*H*W) x (K*H*W) matrix - 65 536 squared, 17 GB in fp32, at K = 16 and 64x64 maps: a dense GEMM workload unrelated to the row
    kernels of this module, and no script of the reference reaches it.  There is no eager fallback, so the constructor refuses.
    The loss itself (without `prior`, a D x D matrix that cannot exist here) is GramCoralLoss below: the same value and gradients
    through n x n Gram matrices."""

    def __init__(self, coral_downsample, prior=None):
        super(CoralLoss, self).__init__()
        raise NotImplementedError("CoralLoss is not implemented on the device: it needs the (K*H*W) x (K*H*W) covariance of the flattened "
                                  "heat-maps (17 GB in fp32 at K = 16, 64x64), a dense GEMM workload that no training script reaches; "
                                  "this package has no eager fallback")


class _GramCoralFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, tgt, down):
        _hip.require_cuda(src, tgt)
        if src.dim() != 4 or tuple(src.shape) != tuple(tgt.shape):
            raise ValueError(f"GramCoralLoss needs two [N,K,H,W] heat-map batches of one shape, got {tuple(src.shape)} and {tuple(tgt.shape)}")
        N, K, H, W = src.shape
        if N < 2 or N > 64:
            raise ValueError(f"GramCoralLoss: the batch size must be 2 ... 64 (a covariance needs two samples; the kernels hold 2N <= 128 rows), got {N}")
        if H // down < 1 or W // down < 1:
            raise ValueError(f"GramCoralLoss: coral_downsample {down} leaves no pixel of a {H}x{W} map")
        s, t = ha.f32c(src), ha.f32c(tgt)
        mp = (2 * N + 31) // 32 * 32
        ws = torch.empty(int(lib().udapose_coral_ws_bytes(N, K, H, W, down)) // 8, dtype=torch.float64, device=s.device)
        coef = torch.empty(mp * mp, dtype=torch.float32, device=s.device)
        out = torch.empty((), dtype=torch.float32, device=s.device)
        check(lib().udapose_coral_fwd(_hip.stream(), ptr(s), ptr(t), N, K, H, W, down, ptr(ws), ptr(coef), ptr(out)), "coral_fwd")
        ctx.save_for_backward(s, t, coef)
        ctx.down, ctx.shape, ctx.dtypes = down, src.shape, (src.dtype, tgt.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        s, t, coef = ctx.saved_tensors
        N, K, H, W = ctx.shape
        ds, dt = torch.empty_like(s), torch.empty_like(t)
        gs = ha.gscale(g)
        check(lib().udapose_coral_bwd(_hip.stream(), ptr(s), ptr(t), ptr(coef), ptr(gs), N, K, H, W, ctx.down, ptr(ds), ptr(dt)), "coral_bwd")
        return ds.to(ctx.dtypes[0]), dt.to(ctx.dtypes[1]), None


class GramCoralLoss(nn.Module):
    """The reference's CoralLoss (loss.py:176-208, without `prior`), called as it is: loss = crit(src_out, tgt_out) on two [N,K,H,W] batches,
    || Cs - Ct ||_F / (4 D^2) with Cs, Ct the D x D covariances over the batch of the flattened (down-sampled) maps, D = K*H'*W'.
    Those matrices are never formed: with Xc the batch-centred N x D data and Gab = Xa_c Xb_c^T (N x N),
    ||Cs - Ct||_F^2 = sum(Gss^2 + Gtt^2 - 2 Gst^2) / (N-1)^2, and the gradients are k (Gss Xs - Gst Xt) and k (Gtt Xt - Gst^T Xs): one
    streaming pass over the 2N x D data forward (exact-fp32 MFMA, finished in fp64), one backward; gradients flow to BOTH inputs.
    coral_downsample = d > 1 is F.interpolate(scale_factor=1/d, mode='bilinear') folded into the loads: the mean of the central 2x2
    pixels of every d x d block (even d), the centre pixel (odd d), floor(H/d) x floor(W/d) of them.
    N must be 2 ... 64.  Where the two covariances are equal (S == 0: e.g. crit(x, x)) the loss is 0 and the gradients are ZERO; torch's
    autograd of the reference's expression gives NaN there (the derivative of sqrt at 0).  Covariances are per rank under data parallel."""

    def __init__(self, coral_downsample=1):
        super(GramCoralLoss, self).__init__()
        if int(coral_downsample) != coral_downsample or coral_downsample < 1:
            raise ValueError(f"coral_downsample must be an integer >= 1, got {coral_downsample!r}")
        self.coral_downsample = int(coral_downsample)

    def forward(self, src_out, tgt_out):
        return _GramCoralFn.apply(src_out, tgt_out, self.coral_downsample)
