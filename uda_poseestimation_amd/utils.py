"""Mean-teacher helpers (API mirror of the reference's utils.py:9-109) on MI355X kernels."""
if not __package__:
    # `from utils import *` with this package's directory on sys.path (train_human.py:29): bind the name `utils` to
    # uda_poseestimation_amd.utils (import returns that module; this top-level copy is discarded)
    import _dropin
    _dropin.alias(["utils"])
    __package__ = "uda_poseestimation_amd"
import ctypes as C

import numpy as np
import torch

from . import _hip
from . import heatmap_args as ha
from ._hip import check, lib, ptr


class _MultiTensorTable:
    """Device tables (addresses, sizes, block -> (tensor, offset)) for the multi-tensor sweeps."""

    def __init__(self, tensor_lists):
        dev = tensor_lists[0][0].device
        chunk = lib().udapose_multi_chunk()
        sizes = [t.numel() for t in tensor_lists[0]]
        blk_t, blk_o = [], []
        for i, n in enumerate(sizes):
            for off in range(0, n, chunk):
                blk_t.append(i)
                blk_o.append(off)
        self.key = self.key_of(tensor_lists)
        self.ptrs = [torch.tensor([t.data_ptr() for t in lst], dtype=torch.int64, device=dev) for lst in tensor_lists]
        self.sizes = torch.tensor(sizes, dtype=torch.int64, device=dev)
        self.blk_t = torch.tensor(blk_t, dtype=torch.int32, device=dev)
        self.blk_o = torch.tensor(blk_o, dtype=torch.int64, device=dev)
        self.nblocks = len(blk_t)

    @staticmethod
    def key_of(tensor_lists):
        """What a table was built from: the address of EVERY tensor of every list, and the sizes.  (The first and last address of a list
        do not identify it: a middle gradient reallocated after zero_grad(set_to_none=True), or one parameter losing its gradient while
        another gains one, leaves both in place - and the sweep would go on reading the old addresses.)"""
        ptr_of, numel = torch.Tensor.data_ptr, torch.Tensor.numel
        return tuple(tuple(map(ptr_of, lst)) for lst in tensor_lists) + (tuple(map(numel, tensor_lists[0])),)


class OldWeightEMA(object):
    """Exponential moving average of the student's PARAMETERS into the teacher (utils.py:9-25), one fused sweep."""

    def __init__(self, target_net, source_net, alpha=0.999):
        self.target_params = list(target_net.parameters())
        self.source_params = list(source_net.parameters())
        self.alpha = alpha
        # None, or a 2-element fp32 DEVICE tensor holding ema_pair(alpha): the sweeps then read the pair from it (udapose_ema_multi_dev, the
        # _dev forms of the fused tail), so that a captured launch follows a ramped alpha.  Whoever sets it keeps it current
        # (MeanTeacherTrainer.sync_schedule with "teacher_alpha" in trainer.scheduled).
        self.alpha_dev = None
        self._table = None
        for p, src_p in zip(self.target_params, self.source_params):
            p.data[:] = src_p.data[:]
        _bump_versions(self.target_params)       # (`.data` writes are invisible to the version counters the pack cache reads)

    def step(self):
        tp = [p.data for p in self.target_params]
        sp = [p.data for p in self.source_params]
        for a, b in zip(tp, sp):
            _hip.require_cuda(a, b)
            if a.dtype != torch.float32 or b.dtype != torch.float32 or a.stride() != b.stride() or a.numel() != b.numel():
                raise RuntimeError("OldWeightEMA needs fp32 teacher/student parameters of identical layout")
        key = _MultiTensorTable.key_of([tp, sp])
        if self._table is None or self._table.key != key:
            self._table = _MultiTensorTable([tp, sp])
        t = self._table
        if self.alpha_dev is not None:
            check(lib().udapose_ema_multi_dev(_hip.stream(), ptr(t.ptrs[0]), ptr(t.ptrs[1]), ptr(t.sizes), ptr(t.blk_t), ptr(t.blk_o), t.nblocks,
                                              ptr(self.alpha_dev)), "ema_multi_dev")
        else:
            alpha, one_minus_alpha = ema_pair(self.alpha)
            check(lib().udapose_ema_multi(_hip.stream(), ptr(t.ptrs[0]), ptr(t.ptrs[1]), ptr(t.sizes), ptr(t.blk_t), ptr(t.blk_o), t.nblocks,
                                          alpha, one_minus_alpha), "ema_multi")
        _bump_versions(self.target_params)


def ema_pair(alpha):
    """(alpha, 1 - alpha) as OldWeightEMA.step hands them to its kernel: the subtraction in Python double (utils.py:22), each value then
    rounded to fp32 by the call (by-value) or by the upload (device form) - the same two fp32 numbers either way."""
    return float(alpha), float(1.0 - alpha)


# ---------------------------------------------------------------------- ramps (the names of utils.py:28-52), host scalars
# Every value is formed by the same double-precision operations in the same order as the reference's, so the results are its bits
# (tests/golden/ramps.npz); the clipping, the curve and the conversion to a Python float are stated once each.
def _clipped(x, upper):
    """x held inside [0, upper], as a numpy double."""
    return np.clip(x, 0.0, upper)


def _falling_logistic(z):
    """1 / (1 + e^z): from 1 (z -> -inf) down to 0."""
    return float(1.0 / (1.0 + np.exp(z)))


def sigmoid_rampup(current, rampup_length):
    """exp(-5 (1 - t / L)^2) with t = current clipped to [0, L]: the rise of Laine & Aila (arXiv:1610.02242) from exp(-5) to 1; L == 0: 1."""
    if rampup_length == 0:
        return 1.0
    remaining = 1.0 - _clipped(current, rampup_length) / rampup_length      # the share of the ramp still ahead, 1 -> 0
    return float(np.exp((-5.0 * remaining) * remaining))


def cosine_rampdown(current, rampdown_length):
    """(cos(pi t / L) + 1) / 2 with t = current clipped to [0, L]: the half cosine of SGDR (arXiv:1608.03983), 1 down to 0.  L == 0 is NaN,
    the reference's 0 / 0."""
    angle = (np.pi * _clipped(current, rampdown_length)) / rampdown_length   # 0 -> pi
    return float(0.5 * (np.cos(angle) + 1.0))


def rev_sigmoid(progress):
    """1 / (1 + exp(10 p - 5)), p = progress clipped to [0, 1]: the logistic curve falling from ~0.993 to ~0.007."""
    return _falling_logistic(10.0 * _clipped(progress, 1.0) - 5.0)


def sigmoid(progress):
    """1 / (1 + exp(5 - 10 p)), p = progress clipped to [0, 1]: the logistic curve rising from ~0.007 to ~0.993 (rev_sigmoid mirrored)."""
    return _falling_logistic(5.0 - 10.0 * _clipped(progress, 1.0))


def ema_alpha_warmup(step, alpha):
    """min(1 - 1 / (step + 1), alpha): the EMA rate of the original mean teacher, which follows the student closely for the first steps
    (0 at step 0: the teacher is the student) and settles at alpha."""
    return min(1.0 - 1.0 / (step + 1), alpha)


def _bump_versions(params):
    """The kernels wrote through raw pointers: bump torch's version counters so that autograd and the executor's
    weight-pack cache (PoseResNet._run_forward) see that the data changed."""
    params = list(params)
    setter = getattr(torch._C._autograd, "_unsafe_set_version_counter", None)
    if setter is not None:
        setter(params, [p._version + 1 for p in params])
    else:   # older torch: a zero-size in-place op through a version-sharing alias
        for p in params:
            p.detach()[:0].zero_()


def get_max_preds_torch_raw(batch_heatmaps):
    """(x = idx % W, y = idx // W) [B,K,2] and the maxima [B,K,1] WITHOUT the max>0 masking: what the occlusion code
    computes inline with amax / view().argmax(-1) (train_human.py:378-381)."""
    _hip.require_cuda(batch_heatmaps)
    r = ha.heatmap_argmax(ha.f32c(batch_heatmaps), maxv=True, idx=True)
    idx, W = r.idx.long(), batch_heatmaps.shape[3]
    return torch.stack([idx % W, idx // W], -1), r.maxv.unsqueeze(-1)


def get_max_preds_torch(batch_heatmaps):
    """utils.py:54-75: (preds [B,K,2] float (x,y) zeroed where max<=0, maxvals [B,K,1])."""
    _hip.require_cuda(batch_heatmaps)
    r = ha.heatmap_argmax(ha.f32c(batch_heatmaps), maxv=True, xy=True)
    return r.xy, r.maxv.unsqueeze(-1).to(batch_heatmaps.dtype)


def rectify(hm, sigma):  # b, c, h, w -> b, c, h, w
    """utils.py:77-109 as ONE kernel: arg-max per (b,c) then the Gaussian patch stamped into a zero map (clipped)."""
    _hip.require_cuda(hm)
    return ha.heatmap_argmax(ha.f32c(hm), rectify_sigma=sigma).rect.to(hm.dtype)


def heatmap_activations(recon):
    """activates = amax over (h,w) per (b,k)  (train_human.py:427), one sweep."""
    _hip.require_cuda(recon)
    return ha.heatmap_argmax(ha.f32c(recon), maxv=True).maxv


def activations_and_rectify(recon, sigma):
    """heatmap_activations(recon) and rectify(recon, sigma) from ONE sweep (the arg-max of a (b,k) plane gives both; the mean-teacher step
    needs both from the teacher's re-warped heat-maps, train_human.py:427 and :431).  Returns (activates [B,K], rectified [B,K,H,W])."""
    _hip.require_cuda(recon)
    r = ha.heatmap_argmax(ha.f32c(recon), maxv=True, rectify_sigma=sigma)
    return r.maxv, r.rect.to(recon.dtype)


MASK_MODES = ("global", "per_joint", "threshold")


def mask_kth_index(mask_ratio, n_pool, mode="global"):
    """The k of confidence_mask: int(mask_ratio * n_pool), 1-indexed into the ascending order of the pool (n_pool: every pooled value in
    "global" mode, the pooled samples in "per_joint" mode); outside 1 ... n_pool: ValueError."""
    k = int(mask_ratio * n_pool)
    if k < 1 or k > n_pool:
        raise ValueError(f"confidence_mask(mode={mode!r}): k = int(mask_ratio * n_pool) = int({mask_ratio} * {n_pool}) = {k} is outside "
                         f"1 ... {n_pool}")
    return k


def confidence_mask(recon, mask_ratio, tea_mask=None, gathered_activates=None, activates=None, *, mode="global", threshold=None):
    """train_human.py:427-430 without the host round trip: activates = amax_{hw}(recon); thr = k-th smallest with
    k = int(mask_ratio * numel); mask = (tea_mask * activates) > thr.  `gathered_activates` (all ranks' activates,
    flattened) makes thr the GLOBAL-batch statistic under data parallelism.  Returns (mask bool [B,K], activates [B,K], thr).
    mode="global" is that, the reference's single batch-wide threshold.  mode="per_joint": one threshold per joint (class-balanced
    self-training) - thr[j] = the k-th smallest of joint j's confidences over the pool's samples (all ranks' with `gathered_activates`),
    k = int(mask_ratio * n_pool) >= 1, thr returned as [K].  mode="threshold": mask = (tea_mask * activates) > threshold, a float or a
    0-d device tensor (read on the device: no synchronisation, and a captured launch follows its value); mask_ratio is ignored.
    mask_ratio may also be a one-element int32 DEVICE tensor ("global" / "per_joint"): it then holds k itself,
    k = mask_kth_index(ratio, n_pool, mode), and the launch reads it from device memory (udapose_kth_mask_dev /
    udapose_joint_kth_mask_dev), so that a captured launch follows a ramped ratio."""
    k_dev = None
    if torch.is_tensor(mask_ratio):
        k_dev = mask_ratio
    if mode not in MASK_MODES:
        raise ValueError(f"confidence_mask: mode {mode!r}: one of {MASK_MODES}")
    if mode == "threshold" and threshold is None:
        raise ValueError("confidence_mask: mode='threshold' needs threshold= (a float or a 0-d device tensor)")
    if k_dev is not None and (k_dev.dtype != torch.int32 or k_dev.numel() != 1):
        raise ValueError("confidence_mask: a tensor mask_ratio must be a one-element int32 device tensor that holds k")
    if mode != "global":
        return _confidence_mask_select(recon, mask_ratio, tea_mask, gathered_activates, activates, mode, threshold, k_dev)
    act = heatmap_activations(recon) if activates is None else activates
    B, K = act.shape
    pool = act.reshape(-1) if gathered_activates is None else gathered_activates.detach().float().reshape(-1).contiguous()
    mask = torch.empty(B, K, dtype=torch.uint8, device=act.device)
    thr = torch.empty((), dtype=torch.float32, device=act.device)
    tm = None if tea_mask is None else tea_mask.detach().float().contiguous()
    if k_dev is not None:
        _hip.require_cuda(k_dev)
        check(lib().udapose_kth_mask_dev(_hip.stream(), ptr(pool), ptr(tm), pool.numel(), ptr(k_dev), ptr(thr), ptr(mask), ptr(act), B * K),
              "kth_mask_dev")
        return mask.view(torch.bool), act, thr
    k = int(mask_ratio * pool.numel())
    check(lib().udapose_kth_mask(_hip.stream(), ptr(pool), ptr(tm), pool.numel(), k, ptr(thr), ptr(mask), ptr(act), B * K), "kth_mask")
    return mask.view(torch.bool), act, thr        # (the kernel writes 0 / 1: a bool view, not a conversion launch)


def _confidence_mask_select(recon, mask_ratio, tea_mask, gathered_activates, activates, mode, threshold, k_dev=None):
    """The per-joint and fixed-threshold forms of confidence_mask (csrc/select.hip): one launch behind the arg-max sweep."""
    B, K = (activates if activates is not None else recon).shape[:2]
    if mode == "per_joint":
        if gathered_activates is not None and gathered_activates.numel() % K:
            raise ValueError(f"confidence_mask: gathered_activates has {gathered_activates.numel()} elements, no multiple of K = {K}")
        n_pool = B if gathered_activates is None else gathered_activates.numel() // K
        k = mask_kth_index(mask_ratio, n_pool, mode) if k_dev is None else 0
    elif torch.is_tensor(threshold) and threshold.numel() != 1:
        raise ValueError(f"confidence_mask: threshold must be a float or a 0-d tensor, got shape {tuple(threshold.shape)}")
    _hip.require_cuda(recon, tea_mask, gathered_activates, activates, threshold if torch.is_tensor(threshold) else None, k_dev)
    act = heatmap_activations(recon) if activates is None else activates.detach().float().contiguous()
    mask = torch.empty(B, K, dtype=torch.uint8, device=act.device)
    tm = None if tea_mask is None else tea_mask.detach().float().contiguous()
    if mode == "per_joint":
        pool = act if gathered_activates is None else gathered_activates.detach().float().reshape(-1).contiguous()
        thr = torch.empty(K, dtype=torch.float32, device=act.device)
        if k_dev is not None:
            check(lib().udapose_joint_kth_mask_dev(_hip.stream(), ptr(pool), n_pool, K, ptr(k_dev), ptr(tm), ptr(act), B, ptr(thr), ptr(mask)),
                  "joint_kth_mask_dev")
        else:
            check(lib().udapose_joint_kth_mask(_hip.stream(), ptr(pool), n_pool, K, k, ptr(tm), ptr(act), B, ptr(thr), ptr(mask)), "joint_kth_mask")
    else:
        if torch.is_tensor(threshold):
            thr = threshold.detach().reshape(())
            if thr.dtype != torch.float32:
                thr = thr.float()
        else:
            thr = torch.full((), float(threshold), dtype=torch.float32, device=act.device)
        check(lib().udapose_thr_mask(_hip.stream(), ptr(act), ptr(tm), B * K, ptr(thr), ptr(mask)), "thr_mask")
    return mask.view(torch.bool), act, thr


PRIOR_MAX_KEYPOINTS = 64
_PRIOR_CACHE = {}       # (tables' storage and version, gamma, epsilon, v3, device) -> (the caller's tensors, mean and weight table on the device)


def _prior_tables(prior, K, gamma, epsilon, v3, device):
    """fp32 device copies of prior['mean'] and of the [K,K] weight table udapose_prior_weights makes of prior['std'].  Cached on what they were
    made from, so a second call uploads and launches nothing (a captured step must find its tables here: call once before capturing)."""
    mean, std = prior["mean"], prior["std"]
    for name, t in (("mean", mean), ("std", std)):
        if not torch.is_tensor(t) or tuple(t.shape) != (K, K):
            raise ValueError(f"generate_prior_map: prior[{name!r}] must be a [{K}, {K}] tensor for {K} heat-map channels, got "
                             f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    key = (mean.data_ptr(), mean._version, str(mean.device), std.data_ptr(), std._version, str(std.device), float(gamma), float(epsilon), bool(v3),
           str(device))
    hit = _PRIOR_CACHE.get(key)
    if hit is None:
        mean_d = mean.detach().to(device=device, dtype=torch.float32).contiguous()
        std_d = std.detach().to(device=device, dtype=torch.float32).contiguous()
        w = torch.empty(K, K, dtype=torch.float32, device=device)
        check(lib().udapose_prior_weights(_hip.stream(), ptr(std_d), K, float(gamma), float(epsilon), int(bool(v3)), ptr(w)), "prior_weights")
        while len(_PRIOR_CACHE) >= 16:
            _PRIOR_CACHE.pop(next(iter(_PRIOR_CACHE)))
        # (the caller's tensors are held too: while the entry lives their addresses cannot be handed to other tables)
        hit = _PRIOR_CACHE[key] = (mean, std, mean_d, w)
    return hit[2], hit[3]


def generate_prior_map(prior, preds, gamma=2, sigma=2, epsilon=-10e10, v3=False, *, multiply=False):
    """utils.py:111-145 as ONE kernel behind the arg-max decode.  prior: {'mean': [K,K], 'std': [K,K]} (CPU or device); preds [B,K,H,W] heat-maps
    (fp32 / fp16 / bf16 on the device).  Joint i, decoded as get_max_preds_torch does, casts a ring of radius mean[i,j] and width sigma for joint j;
    the rings are ensembled with soft-max(-std / gamma) weights over i (diagonal excluded), or with v3=True with conf_i / (1 + std[i,j]).
    multiply=True returns preds.float() * map - what the reference's comment says the map is for - from the same launch.
    Computed in fp32, returned in preds' dtype, without autograd."""
    _hip.require_cuda(preds)
    if preds.dim() != 4:
        raise ValueError(f"generate_prior_map: preds must be [B, K, H, W], got {tuple(preds.shape)}")
    B, K, H, W = preds.shape
    if K > PRIOR_MAX_KEYPOINTS:
        raise ValueError(f"generate_prior_map: {K} key-points (the kernel stages two K x K tables in LDS: K <= {PRIOR_MAX_KEYPOINTS})")
    if B < 1 or K < 1 or H < 1 or W < 1:
        raise ValueError(f"generate_prior_map: empty preds {tuple(preds.shape)}")
    if not (float(sigma) > 0 and np.isfinite(float(sigma))):
        raise ValueError(f"generate_prior_map: sigma must be finite and > 0, got {sigma}")
    if not v3 and not (np.isfinite(float(gamma)) and float(gamma) != 0):
        raise ValueError(f"generate_prior_map: gamma must be finite and non-zero, got {gamma}")
    mean_d, w = _prior_tables(prior, K, gamma, epsilon, v3, preds.device)
    hm = ha.f32c(preds)
    peak = ha.heatmap_argmax(hm, maxv=True, xy=True)
    out = torch.empty_like(hm)
    check(lib().udapose_prior_map(_hip.stream(), ptr(peak.xy), ptr(peak.maxv), ptr(mean_d), ptr(w), ptr(hm) if multiply else None, B, K, H, W, float(sigma),
                                  int(bool(v3)), ptr(out)), "prior_map")
    return out.to(preds.dtype)


class SkeletonPrior(object):
    """Builds the `prior` of generate_prior_map - which the reference takes as given and no script of it computes - from source labels: mean and
    population standard deviation of the distance between every pair of joints, over the samples where both are visible, in heat-map pixels.
    Sums are kept in fp64 on the device (count, sum d, sum d^2 per pair); nothing is read back until the caller asks for a value.
    A pair never seen together gets mean 0 and std +inf, which weighs 0 in both modes of generate_prior_map."""

    def __init__(self, num_keypoints, device="cuda"):
        self.num_keypoints = int(num_keypoints)
        if not 1 <= self.num_keypoints <= PRIOR_MAX_KEYPOINTS:
            raise ValueError(f"SkeletonPrior: num_keypoints must be in [1, {PRIOR_MAX_KEYPOINTS}], got {num_keypoints}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            _hip.require_cuda(torch.empty(0))
        self._acc = None        # fp64 [3][K][K], allocated by the first update

    def update_coords(self, coords, visible):
        """coords [M,K,2] (x, y), visible [M,K] (non-zero = visible)."""
        _hip.require_cuda(coords, visible)
        K = self.num_keypoints
        if coords.dim() != 3 or tuple(coords.shape[1:]) != (K, 2) or tuple(visible.shape) != (coords.shape[0], K):
            raise ValueError(f"SkeletonPrior: coords [M, {K}, 2] and visible [M, {K}] expected, got {tuple(coords.shape)} and {tuple(visible.shape)}")
        M = coords.shape[0]
        if M == 0:
            return self
        c = coords.detach().float().contiguous()
        v = visible.detach().ne(0).to(torch.uint8).contiguous()
        if self._acc is None:
            self._acc = torch.zeros(3, K, K, dtype=torch.float64, device=c.device)
        check(lib().udapose_pair_dist_accumulate(_hip.stream(), ptr(c), ptr(v), M, K, ptr(self._acc)), "pair_dist_accumulate")
        return self

    def update(self, label_s, weight_s=None):
        """label_s [N,K,H,W] heat-map labels, weight_s [N,K] or [N,K,1] (the loaders' target_weight): a joint is visible where its weight is > 0
        and its label's maximum is > 0; its position is the label's arg-max (get_max_preds_torch)."""
        _hip.require_cuda(label_s, weight_s)
        coords, maxv = get_max_preds_torch(label_s)
        visible = maxv.float().reshape(maxv.shape[0], maxv.shape[1]) > 0
        if weight_s is not None:
            visible = visible & (weight_s.detach().reshape(visible.shape) > 0)
        return self.update_coords(coords, visible)

    @property
    def count(self):
        """[K,K] int64 device tensor: how many samples every pair was seen in."""
        K = self.num_keypoints
        if self._acc is None:
            return torch.zeros(K, K, dtype=torch.int64, device=self.device)
        return self._acc[0].to(torch.int64)

    def finalize(self):
        """{'mean', 'std'}: fp32 [K,K] device tensors (new ones on every call) that generate_prior_map accepts."""
        K = self.num_keypoints
        if self._acc is None:
            self._acc = torch.zeros(3, K, K, dtype=torch.float64, device=self.device)
        mean = torch.empty(K, K, dtype=torch.float32, device=self._acc.device)
        std = torch.empty_like(mean)
        check(lib().udapose_pair_dist_finish(_hip.stream(), ptr(self._acc), K, ptr(mean), ptr(std)), "pair_dist_finish")
        return {"mean": mean, "std": std}


def split_saturations(reset=True):
    """How many f16x2 ('fp32-grade' mode) stores since the last reset hit a value outside fp16's range (|v| > 65504 saturates; NaN) - the
    teacher / validate() / style-network forwards of the reference's precision mix.  Sums both library builds; synchronises the device."""
    import ctypes as C
    from . import _hip
    total = 0
    for kind in ("bf16", "fp16"):
        if kind in _hip._libs or kind == "bf16":
            c = C.c_ulonglong(0)
            check(_hip.lib(kind).udapose_split_saturations(int(bool(reset)), C.byref(c)), "split_saturations")
            total += int(c.value)
    return total
