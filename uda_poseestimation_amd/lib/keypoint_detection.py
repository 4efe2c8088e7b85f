"""Arg-max decode and PCK (API mirror of the reference's lib/keypoint_detection.py:9-94) on MI355X kernels, and the soft-argmax
decode the reference lacks (`soft_argmax`, csrc/softargmax.hip: sub-pixel coordinates, differentiable), the two published sub-pixel
decodes (`quarter_decode`, `dark_decode`, csrc/refine.hip: one launch, not differentiable), and the flip test's heat-map side
(`flip_perm`, `flip_back`, `flip_merge`, csrc/flip.hip: flip back, swap left / right joints, average, decode - one launch), and the
evaluation report of a whole set (`PCKMeter`, `PCK_THRESHOLDS`, `JOINT_GROUPS`, `group_accuracy`, csrc/pck_curve.hip: a PCK curve, its
AUC, the end-point error and the reference's joint groups from integer counts kept on the device)), and the geometry of top-down inference
(`boxes_from_keypoints`, `boxes_from_center_scale`, `to_crop_coords`, `to_image_coords`, csrc/box_crop.hip: the reference's boxes and
get_transform, and the way back from heat-map pixels to image pixels on the device), and the instance layer behind `engine.predict`
(`rescore`, `oks_matrix`, `oks_nms`, `OKS_SIGMAS`, csrc/pose_nms.hip: Simple Baselines' pose rescoring and greedy NMS under object-key-point
similarity, on the device).

The reference takes numpy arrays (it is called on `.cpu().numpy()` copies, train_human.py:289,443).  The same calls work
here; torch CUDA tensors are accepted as well and avoid the 2 x 8.4 MB device->host copy per iteration: decode and PCK
run on the device and only K+2 floats and the [B,K,2] coordinates come back.
"""
import numpy as np
import torch

from .. import _hip
from .. import heatmap_args as ha
from .._hip import check, lib, ptr


def _is_numpy(a, what='batch_heatmaps should be numpy.ndarray or a 4-d tensor'):
    """True for a numpy array, False for a tensor; anything else is refused."""
    if not isinstance(a, np.ndarray) and not torch.is_tensor(a):
        raise AssertionError(what)
    return isinstance(a, np.ndarray)


def _like_input(src, t, in_dtype=False):
    """numpy in -> numpy out, tensor in -> tensor out: the device result `t` as the caller of `src` gets it - a numpy array for a numpy
    `src` (in src's dtype with in_dtype=True: heat-maps and maxvals; coordinates stay float32), `t` itself for a tensor."""
    if not isinstance(src, np.ndarray):
        return t
    a = t.cpu().numpy()
    return a.astype(src.dtype, copy=False) if in_dtype else a


def _need_gpu():
    raise RuntimeError("uda_poseestimation_amd.lib.keypoint_detection needs the MI355X (no CPU fallback)")


def _to_device_f32(a):
    """A numpy array (copied to the current CUDA device) or a CUDA tensor as a detached contiguous fp32 tensor; a CPU tensor is refused."""
    if isinstance(a, np.ndarray):
        if not torch.cuda.is_available():
            _need_gpu()
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    _hip.require_cuda(a)
    return ha.f32c(a)


def _workspace(nbytes, device):      # 8-byte aligned device memory for a launcher
    return torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=device)


def _dev_f32(a):
    if isinstance(a, np.ndarray):
        assert a.ndim == 4, 'batch_images should be 4-ndim'
    else:
        assert torch.is_tensor(a) and a.dim() == 4, 'batch_heatmaps should be numpy.ndarray or a 4-d tensor'
    return _to_device_f32(a)


def _decode(hm):
    """The arg-max decode of an fp32 contiguous CUDA batch: (preds [B,K,2], (0, 0) where the maximum is <= 0; maxvals [B,K,1])."""
    r = ha.heatmap_argmax(hm, maxv=True, xy=True)
    return r.xy, r.maxv.unsqueeze(-1)


def get_max_preds(batch_heatmaps):
    """[B,K,H,W] -> (preds [B,K,2] float32 (x,y), maxvals [B,K,1]); numpy in -> numpy out, tensor in -> tensor out."""
    _is_numpy(batch_heatmaps, 'batch_heatmaps should be numpy.ndarray')
    preds, maxv = _decode(_dev_f32(batch_heatmaps))
    return _like_input(batch_heatmaps, preds), _like_input(batch_heatmaps, maxv, True)


class _SoftArgmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hm, beta, window):
        B, K, H, W = hm.shape
        h = ha.f32c(hm)
        coords = torch.empty(B, K, 2, dtype=torch.float32, device=h.device)
        maxv = torch.empty(B, K, 1, dtype=torch.float32, device=h.device)
        idx = torch.empty(B * K, dtype=torch.int32, device=h.device)
        stats = torch.empty(4 * B * K, dtype=torch.float32, device=h.device)
        check(lib().udapose_soft_argmax_fwd(_hip.stream(), ptr(h), B * K, H, W, beta, window, ptr(coords), ptr(maxv), ptr(idx), ptr(stats)),
              "soft_argmax_fwd")
        ctx.save_for_backward(h, idx, stats)
        ctx.beta, ctx.window, ctx.shape, ctx.in_dtype = beta, window, hm.shape, hm.dtype
        ctx.mark_non_differentiable(maxv)
        return coords, maxv

    @staticmethod
    def backward(ctx, g, _gmax):
        h, idx, stats = ctx.saved_tensors
        B, K, H, W = ctx.shape
        d = torch.empty_like(h)
        gc = ha.f32c(g)
        check(lib().udapose_soft_argmax_bwd(_hip.stream(), ptr(h), ptr(gc), ptr(idx), ptr(stats), B * K, H, W, ctx.beta, ctx.window, ptr(d)),
              "soft_argmax_bwd")
        return ha.grad_like_input(ctx, d), None, None


def _soft_args(beta, window):
    """(beta, window) as the kernels take them: beta finite and > 0, window None (the whole map) -> -1."""
    beta = float(beta)
    if not (beta > 0.0 and beta < float("inf")):
        raise ValueError(f"soft-argmax needs a finite beta > 0, got {beta}")
    if window is None:
        return beta, -1
    if int(window) != window or window < 0:
        raise ValueError(f"window must be None (the whole map) or an integer >= 0, got {window!r}")
    return beta, int(window)


def soft_argmax(batch_heatmaps, beta=10.0, window=None):
    """[B,K,H,W] -> (coords [B,K,2] float32 (x,y) in pixel-index units, maxvals [B,K,1]); numpy in -> numpy out, tensor in -> tensor out.
    coords = sum p_i (x_i, y_i) with p = softmax(beta * h) over the pixels within `window` (Chebyshev distance) of the first arg-max,
    the whole map for window=None.  MSE-trained maps have a flat background of thousands of pixels: decode them with a window
    (beta=10, window=5 is what accuracy(decode="soft") uses).  Differentiable for a tensor that requires grad (the arg-max that places
    the window is a constant; the gradient comes back in the input's dtype).  Coordinates are NOT zeroed where maxvals <= 0."""
    is_np = _is_numpy(batch_heatmaps)
    beta, window = _soft_args(beta, window)
    if is_np:
        coords, maxv = _SoftArgmaxFn.apply(_dev_f32(batch_heatmaps), beta, window)
        return _like_input(batch_heatmaps, coords), _like_input(batch_heatmaps, maxv, True)
    assert batch_heatmaps.dim() == 4, 'batch_heatmaps should be numpy.ndarray or a 4-d tensor'
    _hip.require_cuda(batch_heatmaps)
    return _SoftArgmaxFn.apply(batch_heatmaps, beta, window)      # (the tensor itself: the gradient flows to it)


DARK_MAX_PIXELS = 19200      # UDAPOSE_REFINE_MAX_PIXELS (include/udapose.h): the map and its row-blurred copy share one CU's LDS


def _refine(hm, mode, kernel=0, sigma=0.0):
    """udapose_refine_decode on an fp32 contiguous CUDA batch [B,K,H,W]: (coords [B,K,2], maxvals [B,K,1])."""
    B, K, H, W = hm.shape
    coords = torch.empty(B, K, 2, dtype=torch.float32, device=hm.device)
    maxv = torch.empty(B, K, 1, dtype=torch.float32, device=hm.device)
    check(lib().udapose_refine_decode(_hip.stream(), ptr(hm), B * K, H, W, mode, kernel, sigma, ptr(coords), ptr(maxv), None), "refine_decode")
    return coords, maxv


def _dark_args(kernel, sigma, H, W):
    """(kernel, sigma) as the kernel takes them, refused here - before any launch - where it would refuse them."""
    if int(kernel) != kernel or kernel < 3 or kernel > 31 or kernel % 2 == 0:
        raise ValueError(f"DARK needs an odd blur kernel in [3, 31], got {kernel!r}")
    sigma = 0.0 if sigma is None else float(sigma)
    if not sigma < float("inf"):
        raise ValueError(f"DARK needs a finite sigma (None or <= 0: 0.3 * ((kernel - 1) / 2 - 1) + 0.8), got {sigma}")
    if H * W > DARK_MAX_PIXELS:
        raise ValueError(f"DARK decodes maps of up to {DARK_MAX_PIXELS} pixels (the map is blurred in LDS), got {H} x {W}")
    return int(kernel), sigma


def _refine_public(batch_heatmaps, mode, kernel=0, sigma=None):
    """numpy in -> numpy out, tensor in -> tensor out; the arguments are checked before anything is copied or launched."""
    _is_numpy(batch_heatmaps)
    assert batch_heatmaps.ndim == 4, 'batch_heatmaps should be numpy.ndarray or a 4-d tensor'
    kernel, sigma = _dark_args(kernel, sigma, *batch_heatmaps.shape[2:]) if mode == 1 else (0, 0.0)
    coords, maxv = _refine(_dev_f32(batch_heatmaps), mode, kernel, sigma)
    return _like_input(batch_heatmaps, coords), _like_input(batch_heatmaps, maxv, True)


def quarter_decode(batch_heatmaps):
    """[B,K,H,W] -> (coords [B,K,2] float32 (x,y), maxvals [B,K,1]); numpy in -> numpy out, tensor in -> tensor out.  The arg-max of
    get_max_preds moved a quarter pixel towards the higher neighbour in x and in y (the decode of Simple Baselines), where the arg-max has
    both neighbours well inside the map (1 < x < W-1, 1 < y < H-1); equal neighbours move nothing.  (0, 0) where maxvals <= 0, as
    get_max_preds gives.  Not differentiable: the result is detached."""
    return _refine_public(batch_heatmaps, 0)


def dark_decode(batch_heatmaps, kernel=11, sigma=None):
    """[B,K,H,W] -> (coords [B,K,2] float32 (x,y), maxvals [B,K,1]); numpy in -> numpy out, tensor in -> tensor out.  DARK, the
    distribution-aware decode: the map is blurred with a `kernel` x `kernel` Gaussian (odd, 3..31; sigma None: OpenCV's
    0.3 * ((kernel - 1) / 2 - 1) + 0.8, 2.0 at 11), rescaled to its old maximum, and the arg-max of the ORIGINAL map moves by one Newton
    step on the blurred map's logarithm (1 < x < W-2, 1 < y < H-2; left alone where the blurred maximum is <= 0, the Hessian is singular
    or the step is not finite).  With labels drawn at the un-rounded position (TargetViewPipeline(subpixel_labels=True)) it recovers the
    position to < 0.01 px.  One launch, the blurred map never leaves the CU: maps of up to DARK_MAX_PIXELS pixels (ValueError beyond, and
    for a bad kernel, before any launch).  (0, 0) where maxvals <= 0.  Not differentiable: the result is detached."""
    return _refine_public(batch_heatmaps, 1, kernel, sigma)


def _dev_f32c(a, like):
    """What a decode callable returned (tensor or numpy) as an fp32 tensor on `like`'s device."""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return a.detach().to(device=like.device, dtype=torch.float32)


def _decode_pred_max(o, decode):
    """The prediction's coordinates and maxima under `decode`: "argmax", "soft" (soft_argmax(beta=10, window=5)), "quarter" (quarter_decode),
    "dark" (dark_decode(kernel=11)) or a callable hm -> (coords, maxvals).  The soft decodes get the reference's `maxval > 0` zeroing, so
    every decode agrees on which joints are absent ("quarter" and "dark" zero them in their own launch).  -> (coords [B,K,2], maxvals [B,K])"""
    B, K = o.shape[:2]
    if decode == "argmax":
        coords, maxv = _decode(o)
        return coords, maxv.reshape(B, K)
    if decode == "quarter":
        coords, maxv = _refine(o, 0)
        return coords, maxv.reshape(B, K)
    if decode == "dark":
        coords, maxv = _refine(o, 1, *_dark_args(11, None, *o.shape[2:]))
        return coords, maxv.reshape(B, K)
    if decode == "soft":
        coords, maxv = _SoftArgmaxFn.apply(o, 10.0, 5)
    elif callable(decode):
        coords, maxv = decode(o)
        coords, maxv = _dev_f32c(coords, o), _dev_f32c(maxv, o)
    else:
        raise ValueError(f"decode must be 'argmax', 'soft', 'quarter', 'dark' or a callable, got {decode!r}")
    maxv = maxv.detach().reshape(B, K)
    return (coords.detach().reshape(B, K, 2) * (maxv.unsqueeze(-1) > 0).to(torch.float32)).contiguous(), maxv


def _decode_pred(o, decode):
    """`_decode_pred_max`'s coordinates."""
    return _decode_pred_max(o, decode)[0]


def accuracy_device(output, target, thr=0.5, decode="argmax"):
    """`accuracy` without the read-back: (acc [K] float32 with -1 for key points absent from the batch, [avg_acc, cnt],
    pred [B,K,2]) as CUDA tensors on the current stream - no host synchronisation (validate() accumulates them on the
    device and reads the set's averages back once).  decode: how the PREDICTION is decoded (see `accuracy`)."""
    o, t = _dev_f32(output), _dev_f32(target)
    B, K, H, W = o.shape
    pred = _decode_pred(o, decode)
    gt, _ = _decode(t)
    acc = torch.empty(K, dtype=torch.float32, device=o.device)
    avg_cnt = torch.empty(2, dtype=torch.float32, device=o.device)
    check(lib().udapose_pck(_hip.stream(), ptr(pred), ptr(gt), B, K, H / 10.0, W / 10.0, float(thr), ptr(acc), ptr(avg_cnt)), "pck")
    return acc, avg_cnt, pred


def accuracy(output, target, hm_type='gaussian', thr=0.5, decode="argmax"):
    """PCK@(thr/10 of the heat-map size) from GT heat-maps; returns (acc[K], avg_acc, cnt, pred[B,K,2]) like the reference.
    decode: "argmax" (the reference's decode), "soft" (soft_argmax(beta=10, window=5): sub-pixel predictions), "quarter"
    (quarter_decode: Simple Baselines' quarter-pixel offset), "dark" (dark_decode(kernel=11): the distribution-aware decode) or a
    callable hm -> (coords, maxvals).  Only the prediction is decoded that way - the target heat-maps keep the arg-max - and the
    sub-pixel coordinates are zeroed where maxvals <= 0, as the arg-max's are."""
    if hm_type != 'gaussian':
        raise NotImplementedError("only hm_type='gaussian' is used by the reference scripts")
    acc, avg_cnt, pred = accuracy_device(output, target, thr, decode)
    ac = avg_cnt.cpu()
    acc_np = acc.cpu().numpy().astype(np.float64)
    return acc_np, float(ac[0]), int(ac[1]), _like_input(output, pred)


# ---------------------------------------------------------------------------------------------------------------- flip test
# Left / right partner joints per key-point layout (lib/datasets/util.py:186-224 `shufflelr_ori`; the left / right groups of
# lib/datasets/keypoint_dataset.py:93-97,170-177,214-217).  A mirrored hand has no partner joints.
FLIP_PAIRS = {
    "body16": ((0, 5), (1, 4), (2, 3), (10, 15), (11, 14), (12, 13)),
    "animal18": ((0, 1), (3, 4), (5, 6), (8, 9), (10, 11), (12, 13), (14, 15), (16, 17)),
    "animal14": ((0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (12, 13)),
    "hand21": (),
}
_PERM_CACHE = {}      # (permutation, device) -> its device copy: a loop uploads a table once


def flip_perm(flip_pairs, num_keypoints):
    """The channel permutation of a horizontal flip as a CPU int32 tensor [K]: perm[i] = j and perm[j] = i for every pair (i, j), perm[k] = k
    for unpaired joints.  flip_pairs: a sequence of pairs or a key of FLIP_PAIRS.  ValueError for an index outside [0, K), a joint in two
    pairs or a pair (i, i)."""
    if isinstance(flip_pairs, str):
        if flip_pairs not in FLIP_PAIRS:
            raise ValueError(f"unknown flip-pair table {flip_pairs!r}: one of {sorted(FLIP_PAIRS)} or a sequence of pairs")
        flip_pairs = FLIP_PAIRS[flip_pairs]
    K = int(num_keypoints)
    perm = list(range(K))
    for pair in flip_pairs:
        i, j = (int(v) for v in pair)
        if not (0 <= i < K and 0 <= j < K):
            raise ValueError(f"flip pair ({i}, {j}) is out of range for {K} key points")
        if i == j:
            raise ValueError(f"flip pair ({i}, {j}) pairs a joint with itself")
        if perm[i] != i or perm[j] != j:
            raise ValueError(f"flip pair ({i}, {j}): a joint is in two pairs")
        perm[i], perm[j] = j, i
    return torch.tensor(perm, dtype=torch.int32)


def _perm_device(flip_pairs, num_keypoints, device):
    perm = flip_perm(flip_pairs, num_keypoints)
    key = (tuple(perm.tolist()), device)
    d = _PERM_CACHE.get(key)
    if d is None:
        d = _PERM_CACHE[key] = perm.to(device)
    return d


def _flip_merge(a, f, perm, shift, decode, out=None):
    """udapose_flip_merge on fp32 contiguous CUDA heat-maps: a None -> flip back only.  Returns (out, preds, maxvals); the last two None
    without decode.  out: where to write (may be `a`), a new tensor by default."""
    B, K, H, W = f.shape
    if out is None:
        out = torch.empty_like(f)
    preds = maxv = None
    if decode:
        preds = torch.empty(B, K, 2, dtype=torch.float32, device=f.device)
        maxv = torch.empty(B, K, 1, dtype=torch.float32, device=f.device)
    check(lib().udapose_flip_merge(_hip.stream(), ptr(a), ptr(f), ptr(perm), B, K, H, W, int(bool(shift)), int(a is not None), ptr(out),
                                   ptr(maxv), None, ptr(preds)), "flip_merge")
    return out, preds, maxv


def flip_back(output_flipped, flip_pairs, shift=False):
    """The network's heat-maps [B,K,H,W] of a mirrored batch, flipped back: columns reversed and left / right channels swapped
    (`flip_pairs`: a sequence of pairs or a key of FLIP_PAIRS); shift=True moves the result one pixel to the right (column 0 is kept), as
    Simple Baselines does before averaging.  numpy in -> numpy out, tensor in -> tensor out."""
    f = _dev_f32(output_flipped)
    out, _, _ = _flip_merge(None, f, _perm_device(flip_pairs, f.shape[1], f.device), shift, False)
    return _like_input(output_flipped, out, True)


def flip_merge(output, output_flipped, flip_pairs, shift=False, decode=False):
    """The flip test's average: (output + flip_back(output_flipped, flip_pairs, shift)) * 0.5 as [B,K,H,W] fp32.  decode=True returns
    (merged, preds [B,K,2], maxvals [B,K,1]) with the arg-max decode of `merged` (what get_max_preds gives for it) out of the same
    launch.  numpy in -> numpy out, tensor in -> tensor out."""
    a, f = _dev_f32(output), _dev_f32(output_flipped)
    if a.shape != f.shape:
        raise ValueError(f"output {tuple(a.shape)} and output_flipped {tuple(f.shape)} differ in shape")
    out, preds, maxv = _flip_merge(a, f, _perm_device(flip_pairs, f.shape[1], f.device), shift, decode)
    out = _like_input(output, out, True)
    return (out, _like_input(output, preds), _like_input(output, maxv, True)) if decode else out


# ---------------------------------------------------------------------------------------------------------------- evaluation report
# The default PCK curve, in the unit of `accuracy`'s thr (tenths of the heat-map size): 0.5 is the reference's PCK@0.05.
PCK_THRESHOLDS = tuple(0.05 * j for j in range(1, 21))
PCK_MAX_THRESHOLDS = 64      # UDAPOSE_PCK_MAX_THRESHOLDS (include/udapose.h)
PCK_EPE_SCALE = 65536        # UDAPOSE_PCK_EPE_SCALE: epe_q counts 2^-16 px
# The joint groups the reference's tables are printed from, per key-point layout, in the reference's order of names (the `keypoints_group`
# dicts of lib/datasets/keypoint_dataset.py:107-116,145-151,190-199,228-234 over the class attributes :85-92,126-130,161-168,208-212).
JOINT_GROUPS = {
    "body16": {"head": (9,), "shoulder": (12, 13), "elbow": (11, 14), "wrist": (10, 15), "hip": (2, 3), "knee": (1, 4), "ankle": (0, 5),
               "all": (12, 13, 11, 14, 10, 15, 2, 3, 1, 4, 0, 5)},
    "hand21": {"MCP": (1, 5, 9, 13, 17), "PIP": (2, 6, 10, 14, 18), "DIP": (3, 7, 11, 15, 19), "fingertip": (4, 8, 12, 16, 20),
               "all": tuple(range(21))},
    "animal18": {"eye": (0, 1), "chin": (2,), "hoof": (3, 4, 5, 6), "hip": (7,), "knee": (8, 9, 10, 11), "shoulder": (12, 13),
                 "elbow": (14, 15, 16, 17), "all": tuple(range(18))},
    "animal14": {"eye": (0, 1), "hoof": (2, 3, 4, 5), "knee": (6, 7, 8, 9), "elbow": (10, 11, 12, 13), "all": tuple(range(14))},
}


def _joint_groups(groups):
    """A key of JOINT_GROUPS or a mapping name -> joint indices, as {name: tuple of ints}.  ValueError for an unknown key or an empty group."""
    if isinstance(groups, str):
        if groups not in JOINT_GROUPS:
            raise ValueError(f"unknown joint-group table {groups!r}: one of {sorted(JOINT_GROUPS)} or a mapping name -> joint indices")
        return JOINT_GROUPS[groups]
    out = {name: tuple(int(i) for i in idx) for name, idx in dict(groups).items()}
    for name, idx in out.items():
        if not idx:
            raise ValueError(f"joint group {name!r} is empty")
    return out


def group_accuracy(acc, groups):
    """The reference's KeypointDataset.group_accuracy (lib/datasets/keypoint_dataset.py:64-77): for every group the plain mean of the
    listed joints' values, {name: sum(acc[i] for i in joints) / len(joints)}.  groups: a key of JOINT_GROUPS or a mapping."""
    return {name: sum(acc[i] for i in idx) / len(idx) for name, idx in _joint_groups(groups).items()}


def _ascending_f32(thresholds, what, check_range):
    """Numbers as a float32 array that ascends strictly AS fp32 (the device's type) and passes the caller's check_range(t32), or ValueError."""
    try:
        t64 = np.asarray([float(t) for t in thresholds], dtype=np.float64)
    except TypeError:
        raise ValueError(f"thresholds must be a sequence of numbers, got {thresholds!r}") from None
    with np.errstate(over="ignore"):
        t32 = t64.astype(np.float32)
    check_range(t32)
    if not (t32[1:] > t32[:-1]).all():
        raise ValueError(f"{what} must be strictly ascending as fp32, got {list(thresholds)!r}")
    return t32


def _check_thresholds(thresholds):
    """A float32 array [T]: 1 .. PCK_MAX_THRESHOLDS of them, finite, > 0, strictly ascending (the device finds the first hit by bisection)."""
    def check_range(t32):
        if not 1 <= t32.size <= PCK_MAX_THRESHOLDS:
            raise ValueError(f"a PCK curve takes 1 to {PCK_MAX_THRESHOLDS} thresholds, got {t32.size}")
        if not (np.isfinite(t32).all() and (t32 > 0).all()):
            raise ValueError(f"thresholds must be finite and > 0 as fp32, got {list(thresholds)!r}")
    return _ascending_f32(thresholds, "thresholds", check_range)


class _LazyDeviceState:
    """A meter's tensors on the device, `_st`: None until the subclass's _make(device) returns them, when the meter is built (given a
    device, or with a GPU present) or on the first use that brings a CUDA tensor; refused without either."""
    _st = None

    def _init_device(self, device):
        if device is not None or torch.cuda.is_available():
            self._on_device(torch.device("cuda" if device is None else device))

    def _on_device(self, like=None):      # like: a device, or a tensor that lives on one, to make the state on
        if self._st is None:
            device = getattr(like, "device", like)
            if device is None or device.type != "cuda":
                _need_gpu()
            self._st = self._make(device)
        return self._st


def _nan_div(a, b):
    """a / b in fp64, NaN where b == 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.divide(a, b, out=np.full(np.broadcast(a, b).shape, np.nan), where=b != 0)


def _trapezoid(y, x):
    """The trapezoid area under y (last axis) over x, divided by x's range."""
    return ((y[..., 1:] + y[..., :-1]) * 0.5 * np.diff(x)).sum(-1) / (x[-1] - x[0])


class PCKMeter(_LazyDeviceState):
    """The evaluation report of a whole set, accumulated on the device (csrc/pck_curve.hip): per joint the hits at every threshold of a PCK
    curve, the visible count and the end-point error, kept as int64 counts (`state()`: [K, T + 3], columns hits[0..T-1], count, epe_q,
    nonfinite - include/udapose.h).  An update only adds integers, so the state after a set is the same bits whatever the batch size, and
    nothing is read back before `compute()`.

    thresholds: in the unit of `accuracy`'s thr, 1 to 64 of them, finite, > 0, strictly ascending as fp32 (ValueError otherwise); they are
    uploaded once.  The state and the thresholds live on `device` (default: the current CUDA device; without a GPU the meter can be made
    and refuses every update)."""

    def __init__(self, num_keypoints, thresholds=PCK_THRESHOLDS, device=None):
        self.num_keypoints = int(num_keypoints)
        if not 1 <= self.num_keypoints <= 256:
            raise ValueError(f"PCKMeter takes 1 to 256 key points (UDAPOSE_PCK_MAX_KEYPOINTS), got {num_keypoints}")
        self._thr32 = _check_thresholds(thresholds)
        self.thresholds = tuple(float(t) for t in thresholds)
        self._thr = None
        self._init_device(device)

    def _make(self, device):
        self._thr = torch.from_numpy(self._thr32).to(device)
        return torch.zeros(self.num_keypoints, len(self._thr32) + 3, dtype=torch.int64, device=device)

    def reset(self):
        """Zero the state (in place: a captured update keeps adding to the same memory)."""
        self._on_device().zero_()

    def state(self):
        """The raw int64 state [K, T + 3] on the device (the meter's own tensor, not a copy)."""
        return self._on_device()

    def merge(self, other_state):
        """Add another meter's state (a PCKMeter or its int64 `state()` tensor, from any device): ranks or shards of one set."""
        s = self._on_device()
        o = other_state.state() if isinstance(other_state, PCKMeter) else other_state
        if not torch.is_tensor(o) or o.dtype != torch.int64 or o.shape != s.shape:
            raise ValueError(f"merge() takes an int64 state of shape {tuple(s.shape)}")
        s += o.to(s.device)

    def _coords(self, pred, gt, visible, norm, nh, nw):
        """udapose_pck_accumulate on fp32 contiguous CUDA coordinates [B,K,2]."""
        B, K = pred.shape[:2]
        check(lib().udapose_pck_accumulate(_hip.stream(), ptr(pred), ptr(gt), ptr(visible), ptr(norm), B, K, nh, nw, ptr(self._thr),
                                           len(self._thr32), ptr(self._st)), "pck_accumulate")

    def update(self, output, target=None, *, decode="argmax", target_coords=None, visible=None, norm=None):
        """Add a batch.  output: the network's heat-maps [B,K,H,W]; exactly one of target (heat-maps [B,K,H,W], scored against their
        arg-max with the reference's `> 1` visibility rule) and target_coords ([B,K,2], (x, y) in heat-map pixels; visible [B,K], where
        given, says which count - otherwise the same `> 1` rule applies to the coordinates).  decode: as in `accuracy`.  norm [B]: a
        per-sample length in heat-map pixels (head size, box diagonal) to divide the pixel distance by instead of the heat-map size; a
        sample whose length is not finite and > 0 drops out.  "argmax" against heat-map targets is ONE launch that reduces both tensors
        (udapose_pck_accumulate_heatmaps); everything else decodes first and takes udapose_pck_accumulate.  Returns the prediction
        [B,K,2] on the device; nothing is read back.  CPU tensors are refused, shape mismatches raise ValueError, before any launch."""
        if (target is None) == (target_coords is None):
            raise ValueError("update() takes exactly one of target (heat-maps) and target_coords ([B,K,2])")
        if visible is not None and target_coords is None:
            raise ValueError("visible goes with target_coords (heat-map targets carry their own visibility)")
        given = [a for a in (output, target, target_coords, visible, norm) if a is not None]
        if not all(torch.is_tensor(a) for a in given):
            raise ValueError("update() takes torch tensors")
        _hip.require_cuda(*given)
        if output.dim() != 4 or output.shape[1] != self.num_keypoints or output.shape[0] < 1:
            raise ValueError(f"output must be heat-maps [B,{self.num_keypoints},H,W], got {tuple(output.shape)}")
        B, K, H, W = output.shape
        if target is not None and target.shape != output.shape:
            raise ValueError(f"output {tuple(output.shape)} and target {tuple(target.shape)} differ in shape")
        if target_coords is not None and tuple(target_coords.shape) != (B, K, 2):
            raise ValueError(f"target_coords must be [{B},{K},2], got {tuple(target_coords.shape)}")
        if visible is not None and tuple(visible.shape) != (B, K):
            raise ValueError(f"visible must be [{B},{K}], got {tuple(visible.shape)}")
        if norm is not None and tuple(norm.shape) != (B,):
            raise ValueError(f"norm must be [{B}], got {tuple(norm.shape)}")
        self._on_device(output)
        if any(a.device != self._st.device for a in given):
            raise ValueError(f"the meter's state lives on {self._st.device}: every tensor of an update must")
        o = output.detach().float().contiguous()
        if norm is not None:
            norm = norm.detach().float().contiguous()
        if target is not None and isinstance(decode, str) and decode == "argmax":
            pred = torch.empty(B, K, 2, dtype=torch.float32, device=o.device)
            t = target.detach().float().contiguous()
            check(lib().udapose_pck_accumulate_heatmaps(_hip.stream(), ptr(o), ptr(t), ptr(norm), B, K, H, W, ptr(self._thr),
                                                        len(self._thr32), ptr(self._st), ptr(pred)), "pck_accumulate_heatmaps")
            return pred
        pred = _decode_pred(o, decode)
        if target is not None:
            gt = _decode(target.detach().float().contiguous())[0]
        else:
            gt = target_coords.detach().float().contiguous()
            if visible is not None:
                visible = (visible if visible.dtype in (torch.uint8, torch.bool) else visible != 0).contiguous().view(torch.uint8)
        self._coords(pred, gt, visible, norm, H / 10.0, W / 10.0)
        return pred

    def compute(self, groups=None, pixel_scale=1.0):
        """The one read-back: `report()` of the state."""
        return PCKMeter.report(self._on_device().cpu(), self.thresholds, groups, pixel_scale)

    @staticmethod
    def report(state, thresholds, groups=None, pixel_scale=1.0):
        """The report of a CPU int64 state [K, T + 3], in fp64 on the host (pure: no device, no side effect).  Arrays are numpy float64.
          thresholds     as given
          count [K]      visible (sample, joint) pairs (int64); nonfinite [K]: those whose error was not finite (int64)
          pck [K][T]     hits / count, NaN where count == 0
          pck_mean [T]   the mean over the joints with count > 0 (the reference's avg_acc: 0 where no joint was seen)
          pck_micro [T]  total hits / total count (NaN without a visible pair)
          auc            the trapezoid area under pck_mean over [thr[0], thr[-1]] divided by that range; None for T == 1
          auc_per_joint [K]   the same under pck[k] (NaN where count == 0); None for T == 1
          epe [K]        epe_q / 65536 / (count - nonfinite) * pixel_scale: the mean end-point error in heat-map pixels times pixel_scale
                         (NaN without a finite pair); epe_mean: the mean of epe over the joints that have one (NaN without any)
          groups         given `groups` (a key of JOINT_GROUPS or a mapping): per group {"pck" [T], "auc", "epe"}, each the plain mean
                         over the group's joints as group_accuracy takes it (a joint without a value makes its groups' NaN)"""
        thr = np.asarray([float(t) for t in thresholds], dtype=np.float64)
        T = thr.size
        s = state.numpy() if torch.is_tensor(state) else np.asarray(state)
        if s.dtype != np.int64 or s.ndim != 2 or s.shape[1] != T + 3:
            raise ValueError(f"report() takes an int64 state [K, {T + 3}] for {T} thresholds, got {s.dtype} {s.shape}")
        hits, count, q, nonfinite = s[:, :T], s[:, T], s[:, T + 1], s[:, T + 2]
        seen = count > 0
        pck = _nan_div(hits, count[:, None])
        pck_mean = pck[seen].mean(0) if seen.any() else np.zeros(T)
        epe = _nan_div(q / float(PCK_EPE_SCALE), count - nonfinite) * float(pixel_scale)
        rep = {"thresholds": tuple(float(t) for t in thresholds), "count": count.copy(), "nonfinite": nonfinite.copy(), "pck": pck,
               "pck_mean": pck_mean, "pck_micro": _nan_div(hits.sum(0), count.sum()),
               "auc": float(_trapezoid(pck_mean, thr)) if T > 1 else None, "auc_per_joint": _trapezoid(pck, thr) if T > 1 else None,
               "epe": epe, "epe_mean": float(epe[~np.isnan(epe)].mean()) if (~np.isnan(epe)).any() else float("nan")}
        if groups is not None:
            rep["groups"] = {}
            for name, idx in _joint_groups(groups).items():
                if min(idx) < 0 or max(idx) >= s.shape[0]:
                    raise ValueError(f"joint group {name!r} {idx} is out of range for {s.shape[0]} key points")
                ix = list(idx)
                rep["groups"][name] = {"pck": pck[ix].sum(0) / len(ix), "auc": float(rep["auc_per_joint"][ix].sum() / len(ix)) if T > 1 else None,
                                       "epe": float(epe[ix].sum() / len(ix))}
        return rep


# ---------------------------------------------------------------------------------------------------------------- top-down inference: boxes
# A box is (cx, cy, bw, bh, rot_deg) in pixels of its frame, where pixel i covers [i, i + 1); its crop of Ho x Wo pixels is what
# data_gpu.box_crop / udapose_box_crop samples.  Conventions, the reference's own: a heat-map index i stands for input
# coordinate i * stride (generate_target, lib/datasets/util.py:39); crop and resize move key points by (kp - left) * S / w
# (lib/transforms/keypoint_detection.py:47-64); rot has the sign of get_transform's (lib/datasets/util.py:289-316).
def _hw(size):
    """An int S or (H, W) as (H, W) ints >= 1."""
    h, w = (size, size) if isinstance(size, (int, np.integer)) else size
    if int(h) != h or int(w) != w or h < 1 or w < 1:
        raise ValueError(f"a size is a positive int or (height, width), got {size!r}")
    return int(h), int(w)


def check_boxes(boxes):
    """Host boxes as a float64 array [M,5], checked as the device checks them: ValueError naming the first row that has a non-finite
    field or a side that is not positive (as fp32, the device's type)."""
    b = np.asarray(boxes, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != 5 or b.shape[0] < 1:
        raise ValueError(f"boxes must be [M,5] = (cx, cy, bw, bh, rot_deg) with M >= 1, got shape {b.shape}")
    with np.errstate(over="ignore"):
        b32 = b.astype(np.float32)
    for m in range(b.shape[0]):
        if not np.isfinite(b32[m]).all():
            raise ValueError(f"box {m} has a non-finite field: {b[m].tolist()}")
        if not (b32[m, 2] > 0 and b32[m, 3] > 0):
            raise ValueError(f"box {m} has a side that is not positive: bw = {b[m, 2]}, bh = {b[m, 3]}")
    return b


def box_rotation(rot_deg):
    """(cos, sin) of an array of angles in degrees, float64; exact for multiples of 90, as the device takes them from a table."""
    rot = np.asarray(rot_deg, dtype=np.float64)
    c, s = np.cos(np.deg2rad(rot)), np.sin(np.deg2rad(rot))
    r = np.mod(rot, 360.0)
    for deg, (ce, se) in ((0.0, (1.0, 0.0)), (90.0, (0.0, 1.0)), (180.0, (-1.0, 0.0)), (270.0, (0.0, -1.0))):
        c, s = np.where(r == deg, ce, c), np.where(r == deg, se, s)
    return c, s


def to_crop_coords(kp_img, boxes, size):
    """Key points [M,K,2] (x, y) in pixels of the frame -> in pixels of box m's crop of `size` = S or (Ho, Wo), on the host in float64:
    R(rot)^T (kp - (cx, cy)) / (sx, sy) + (Wo / 2, Ho / 2) with sx = bw / Wo, sy = bh / Ho.  For a square box bw = bh = 200 s this is
    the reference's get_transform(c, s, res, rot) @ [x, y, 1] (without transform()'s -1, +1 and int()); for an upright box it is crop +
    resize's (kp - left) * S / w.  Divide by the stride for heat-map pixels."""
    Ho, Wo = _hw(size)
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 5)
    kp = np.asarray(kp_img, dtype=np.float64)
    if kp.ndim != 3 or kp.shape[2] != 2 or kp.shape[0] != b.shape[0]:
        raise ValueError(f"key points must be [M,K,2] for {b.shape[0]} boxes, got {kp.shape}")
    c, s = (a[:, None] for a in box_rotation(b[:, 4]))
    dx, dy = kp[..., 0] - b[:, None, 0], kp[..., 1] - b[:, None, 1]
    x = (c * dx + s * dy) / (b[:, None, 2] / Wo) + Wo / 2
    y = (-s * dx + c * dy) / (b[:, None, 3] / Ho) + Ho / 2
    return np.stack([x, y], axis=-1)


def _coords_to_image(coords, boxes, Ho, Wo, stride_x, stride_y):
    """udapose_coords_to_image on fp32 contiguous CUDA tensors: coords [M,K,2], boxes [M,5] -> [M,K,2]."""
    M, K = coords.shape[:2]
    out = torch.empty(M, K, 2, dtype=torch.float32, device=coords.device)
    check(lib().udapose_coords_to_image(_hip.stream(), ptr(coords), ptr(boxes), M, K, float(stride_x), float(stride_y), Ho, Wo, ptr(out)),
          "coords_to_image")
    return out


def to_image_coords(coords, boxes, input_size, heatmap_size):
    """The way back, on the device (udapose_coords_to_image): coords [M,K,2] (x, y) in heat-map pixels of the crops (what the decodes
    return) -> pixels of the frames, (cx, cy) + R(rot) (((x, y) * stride - (Wo / 2, Ho / 2)) * (sx, sy)), stride = input_size /
    heatmap_size per axis.  The inverse of `to_crop_coords(.) / stride`.  coords and boxes: CUDA tensors or numpy arrays (numpy coords in ->
    numpy out); host boxes are checked (`check_boxes`), a device tensor is not."""
    Ho, Wo = _hw(input_size)
    Hh, Wh = _hw(heatmap_size)
    if not isinstance(coords, np.ndarray) and not torch.is_tensor(coords):
        raise ValueError("coords must be a numpy array or a tensor [M,K,2]")
    if coords.ndim != 3 or coords.shape[2] != 2 or coords.shape[0] < 1 or coords.shape[1] < 1:
        raise ValueError(f"coords must be [M,K,2], got {tuple(coords.shape)}")
    if not torch.is_tensor(boxes):
        hb = check_boxes(boxes)
    if tuple(boxes.shape if torch.is_tensor(boxes) else hb.shape) != (coords.shape[0], 5):
        raise ValueError(f"boxes must be [{coords.shape[0]},5], got {tuple(boxes.shape if torch.is_tensor(boxes) else hb.shape)}")
    c = _to_device_f32(coords)
    bd = _to_device_f32(boxes) if torch.is_tensor(boxes) else torch.from_numpy(hb.astype(np.float32)).to(c.device)
    return _like_input(coords, _coords_to_image(c, bd, Ho, Wo, Wo / Wh, Ho / Hh))


def boxes_from_center_scale(c, s, rot=0):
    """The animal sets' (centre, scale, rotation) crop as boxes [M,5] float64: centre c [M,2] (or [2]), side 200 * s (get_transform's
    `h = 200 * scale`, lib/datasets/util.py:294), rot in degrees with the reference's sign."""
    c = np.asarray(c, dtype=np.float64).reshape(-1, 2)
    s = np.broadcast_to(np.asarray(s, dtype=np.float64).reshape(-1), (c.shape[0],))
    rot = np.broadcast_to(np.asarray(rot, dtype=np.float64).reshape(-1), (c.shape[0],))
    return np.stack([c[:, 0], c[:, 1], 200.0 * s, 200.0 * s, rot], axis=1)


def boxes_from_keypoints(kp, visible, image_size, style="human"):
    """Boxes [M,5] float64 (rot 0) round key points [M,K,2] as the reference's datasets make them.  image_size = (height, width) of the
    frame; visible [M,K] (non-zero = use the joint) or None.
      "human"   get_bounding_box + scale_box(.., 1.5), pad=False (lib/datasets/util.py:87-123, human36m_mt.py:210-213): the square of
                side min(round(1.5 max(w, h)), min(width, height)) moved inside the frame; its pixels left .. right are [left, right + 1)
                here, so cx = left + side / 2.  visible None: every joint counts, as in the reference.
      "animal"  the +-15 px clip and s = max(w, h) / 200 * 1.25 (real_animal_all_mt.py:219-230): extremes of the joints with a
                coordinate > 0 (visible None; the reference's own test, per axis), widened by 15 px and clipped to the frame; centre their
                midpoint, side 1.25 max(w, h) - such boxes leave the frame routinely.
    ValueError for a sample without a joint to use."""
    kp = np.asarray(kp, dtype=np.float64)
    if kp.ndim == 2:
        kp = kp[None]
    if kp.ndim != 3 or kp.shape[2] < 2:
        raise ValueError(f"key points must be [M,K,2], got {kp.shape}")
    height, width = _hw(image_size)
    M = kp.shape[0]
    vis = None if visible is None else np.asarray(visible).reshape(M, -1) != 0
    if style not in ("human", "animal"):
        raise ValueError(f"style must be 'human' or 'animal', got {style!r}")
    out = np.zeros((M, 5), np.float64)
    for m in range(M):
        if style == "human":
            use = np.ones(kp.shape[1], bool) if vis is None else vis[m]
            xs, ys = kp[m, use, 0], kp[m, use, 1]
        else:
            xs = kp[m, kp[m, :, 0] > 0, 0] if vis is None else kp[m, vis[m], 0]
            ys = kp[m, kp[m, :, 1] > 0, 1] if vis is None else kp[m, vis[m], 1]
        if xs.size == 0 or ys.size == 0:
            raise ValueError(f"sample {m} has no joint to build a box from")
        if style == "human":
            left, upper, right, lower = float(xs.min()), float(ys.min()), float(xs.max()), float(ys.max())
            center_x, center_y = (left + right) / 2, (upper + lower) / 2
            side = min(round(1.5 * max(right - left, lower - upper)), min(width, height))
            left, upper = round(center_x - side / 2), round(center_y - side / 2)
            left = min(max(left, 0), width - side)          # (pad=False: moved inside the frame, left edge first as the reference tests it)
            upper = min(max(upper, 0), height - side)
            out[m] = (left + side / 2.0, upper + side / 2.0, side, side, 0.0)
        else:
            y_min, y_max = max(float(ys.min()) - 15, 0.0), min(float(ys.max()) + 15, float(height))
            x_min, x_max = max(float(xs.min()) - 15, 0.0), min(float(xs.max()) + 15, float(width))
            side = 200.0 * (max(x_max - x_min, y_max - y_min) / 200.0 * 1.25)
            out[m] = ((x_min + x_max) / 2.0, (y_min + y_max) / 2.0, side, side, 0.0)
    return out


# ---------------------------------------------------------------------------------------------------------------- top-down inference: instances
# One pose per box -> distinct, scored poses (csrc/pose_nms.hip): Simple Baselines' rescoring and greedy NMS under
# object-key-point similarity.  The reference has neither.  Everything stays on the device: shapes are [M], nothing is compacted.
NMS_MAX_POSES = 4096          # UDAPOSE_NMS_MAX_POSES (include/udapose.h): 64 mask words, one per lane of the walking wave
NMS_MAX_KEYPOINTS = 64        # UDAPOSE_NMS_MAX_KEYPOINTS
# COCO's per-joint constants (cocoapi, PythonAPI/pycocotools/cocoeval.py, `kpt_oks_sigmas`), in COCO's joint order
OKS_SIGMAS = {"coco17": (.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089)}
OKS_UNIFORM_SIGMA = 0.0669    # the mean of COCO's seventeen (1.138 / 17), for skeletons without a published table
_SIGMA_CACHE = {}             # (table, device) -> its device copy
_NMS_THR = {}                 # (name, device) -> [device scalar, the host value it holds]


def oks_sigmas(K):
    """The table for a skeleton of K joints: COCO's for K = 17, else K times OKS_UNIFORM_SIGMA."""
    if int(K) != K or not 1 <= K <= NMS_MAX_KEYPOINTS:
        raise ValueError(f"K must be in [1, {NMS_MAX_KEYPOINTS}], got {K!r}")
    return OKS_SIGMAS["coco17"] if K == 17 else (OKS_UNIFORM_SIGMA,) * int(K)


def _device_key(device):
    """torch.device(device) with the index spelled out ("cuda" and "cuda:0" name one device: one cache slot)."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _sigmas_device(sigmas, K, device):
    """sigmas: None (oks_sigmas(K)), a key of OKS_SIGMAS, K positive numbers, or a CUDA tensor [K] (taken as it is) -> fp32 [K] on the device."""
    if torch.is_tensor(sigmas):
        _hip.require_cuda(sigmas)
        if tuple(sigmas.shape) != (K,):
            raise ValueError(f"sigmas must be [{K}], got {tuple(sigmas.shape)}")
        return ha.f32c(sigmas)
    if sigmas is None:
        sigmas = oks_sigmas(K)
    elif isinstance(sigmas, str):
        if sigmas not in OKS_SIGMAS:
            raise ValueError(f"sigmas {sigmas!r}: the tables are {tuple(OKS_SIGMAS)}")
        sigmas = OKS_SIGMAS[sigmas]
    table = tuple(float(v) for v in sigmas)
    if len(table) != K or not all(np.isfinite(v) and v > 0 for v in table):
        raise ValueError(f"sigmas must be {K} positive numbers, got {table}")
    key = (table, _device_key(device))
    if key not in _SIGMA_CACHE:
        _SIGMA_CACHE[key] = torch.tensor(table, dtype=torch.float32, device=key[1])
    return _SIGMA_CACHE[key]


def nms_threshold(name, value, device):
    """The device scalar that holds threshold `name` ("oks_thr" or "vis_thr") on `device`, uploaded when the host value changed (a
    stream-ordered 4-byte copy, the pattern of MeanTeacherTrainer.sync_view_radius); never inside a capture, whose launches read the scalar.
    There is one scalar per name and device: a captured rescore / oks_nms / predict(nms=) follows a later `nms_threshold(name, new, device)`,
    and follows as well any later eager call that gives another value.  A CUDA tensor of one element is taken as it is (a scalar of the
    caller's own, which nothing here writes).  The first call for a device creates the scalar (an upload): make it, or one eager call
    of the function to capture, ahead of the capture."""
    if name not in ("oks_thr", "vis_thr"):
        raise ValueError(f"the thresholds are 'oks_thr' and 'vis_thr', got {name!r}")
    if torch.is_tensor(value):
        _hip.require_cuda(value)
        if value.numel() != 1 or value.dtype != torch.float32:
            raise ValueError(f"{name} as a tensor must be one fp32 element, got {value.dtype} {tuple(value.shape)}")
        return value
    v = float(value)
    if not np.isfinite(v):
        raise ValueError(f"{name} must be finite, got {value!r}")
    key = (name, _device_key(device))
    slot = _NMS_THR.get(key)
    if slot is None:
        _NMS_THR[key] = slot = [torch.tensor(v, dtype=torch.float32, device=key[1]), v]
    elif v != slot[1] and not torch.cuda.is_current_stream_capturing():
        slot[0].copy_(torch.tensor(v, dtype=torch.float32), non_blocking=True)
        slot[1] = v
    return slot[0]


def _pose_tensor(t, shape, what, dtype=torch.float32):
    """A CUDA tensor of `shape` (None entries are free) as contiguous `dtype` (itself where it already is: a capture follows it)."""
    if not torch.is_tensor(t):
        raise ValueError(f"{what} must be a CUDA tensor, got {type(t).__name__}")
    _hip.require_cuda(t)
    if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError(f"{what} must be {list(shape)}, got {tuple(t.shape)}")
    return t.detach().to(dtype).contiguous()


def _check_mk(M, K):
    if not 1 <= M <= NMS_MAX_POSES:
        raise ValueError(f"1 to {NMS_MAX_POSES} poses a call, got {M}")
    if not 1 <= K <= NMS_MAX_KEYPOINTS:
        raise ValueError(f"1 to {NMS_MAX_KEYPOINTS} key points, got {K}")


def rescore(confidence, box_scores=None, vis_thr=0.2):
    """Simple Baselines' pose score on the device (udapose_pose_rescore): confidence [M,K] CUDA -> score [M] fp32 = the mean of the
    confidences above vis_thr (added in ascending k; 0 when there is none) times box_scores[m] (None: 1)."""
    c = _pose_tensor(confidence, (None, None), "confidence")
    M, K = c.shape
    _check_mk(M, K)
    dev = c.device
    bs = None if box_scores is None else _pose_tensor(box_scores, (M,), "box_scores")
    kp = torch.zeros(M, K, 2, dtype=torch.float32, device=dev)
    boxes = torch.ones(M, 5, dtype=torch.float32, device=dev)
    score, area = torch.empty(M, dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.float32, device=dev)
    order, refused = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.uint8, device=dev)
    check(lib().udapose_pose_rescore(_hip.stream(), ptr(kp), ptr(c), ptr(boxes), None, ptr(bs), ptr(nms_threshold("vis_thr", vis_thr, dev)), M, K,
                                     ptr(score), ptr(order), ptr(area), ptr(refused)), "pose_rescore")
    return score


def oks_matrix(kp_a, area_a, kp_b=None, area_b=None, visible_b=None, sigmas=None):
    """Object-key-point similarity on the device (udapose_oks_matrix), fp32.  kp_a [Ma,K,2] (x, y), area_a [Ma]; sigmas as oks_nms takes them.
    Self form (kp_b None): [Ma,Ma], oks(i, j) = mean_k exp(-d2_k / (2 sigma_k)^2 / ((area_i + area_j) / 2 + eps) / 2), bit-symmetric.
    Rectangular form, predictions against labelled poses kp_b [Mb,K,2], area_b [Mb], visible_b [Mb,K] (None: every joint): [Ma,Mb] with
    COCO's convention - the label's area, the mean over the label's visible joints, 0 for a label without one."""
    a = _pose_tensor(kp_a, (None, None, 2), "kp_a")
    Ma, K = a.shape[:2]
    _check_mk(Ma, K)
    dev = a.device
    sg = _sigmas_device(sigmas, K, dev)
    if kp_b is None:
        if area_b is not None or visible_b is not None:
            raise ValueError("area_b and visible_b belong to the rectangular form: give kp_b")
        ar = _pose_tensor(area_a, (Ma,), "area_a")
        out = torch.empty(Ma, Ma, dtype=torch.float32, device=dev)
        check(lib().udapose_oks_matrix(_hip.stream(), ptr(a), ptr(ar), Ma, None, None, None, Ma, K, ptr(sg), None, None, None, ptr(out), None),
              "oks_matrix")
        return out
    b = _pose_tensor(kp_b, (None, K, 2), "kp_b")
    Mb = b.shape[0]
    _check_mk(Mb, K)
    if area_b is None:
        raise ValueError("the rectangular form needs area_b, the labelled poses' areas")
    arb = _pose_tensor(area_b, (Mb,), "area_b")
    vis = None if visible_b is None else _pose_tensor(visible_b, (Mb, K), "visible_b")
    out = torch.empty(Ma, Mb, dtype=torch.float32, device=dev)
    check(lib().udapose_oks_matrix(_hip.stream(), ptr(a), None, Ma, ptr(b), ptr(arb), ptr(vis), Mb, K, ptr(sg), None, None, None, ptr(out), None),
          "oks_matrix")
    return out


def oks_nms(keypoints, confidence, boxes, frame_idx=None, status=None, box_scores=None, sigmas=None, oks_thr=0.9, vis_thr=0.2,
            want_matrix=False):
    """Rescoring and greedy OKS-NMS on the device (udapose_pose_nms: three launches, nothing read back, capturable).  CUDA tensors:
    keypoints [M,K,2] (x, y) in frame pixels, confidence [M,K], boxes [M,5] (area = bw * bh) - engine.predict's outputs and boxes;
    frame_idx [M] integers (None: all poses on one frame), status [M] uint8 (non-zero: refused; None: none), box_scores [M] (None: 1).
    sigmas: None (COCO's table for K = 17, else uniform OKS_UNIFORM_SIGMA), a key of OKS_SIGMAS, K numbers or a CUDA tensor [K].
    oks_thr, vis_thr: floats, kept in the device scalars of `nms_threshold` (or one-element CUDA tensors of the caller's).
    A pose is refused when its status is non-zero, a coordinate, its area or its score is not finite, or its area is <= 0: it is never
    kept and removes nothing.  The walk: descending score, equal scores by ascending index; a pose not yet removed is kept and removes
    every later pose of its own frame with oks > oks_thr.
    Returns {"score" [M] fp32, "order" [M] int32 (refused poses last), "keep" [M] uint8, "n_keep" [1] int32, "suppressed_by" [M] int32 (the
    kept pose that removed m; -1 for kept and refused poses), "oks" [M,M] fp32 with want_matrix}."""
    kp = _pose_tensor(keypoints, (None, None, 2), "keypoints")
    M, K = kp.shape[:2]
    _check_mk(M, K)
    dev = kp.device
    conf = _pose_tensor(confidence, (M, K), "confidence")
    bx = _pose_tensor(boxes, (M, 5), "boxes")
    fi = None if frame_idx is None else _pose_tensor(frame_idx, (M,), "frame_idx", torch.int32)
    st = None if status is None else _pose_tensor(status, (M,), "status", torch.uint8)
    bs = None if box_scores is None else _pose_tensor(box_scores, (M,), "box_scores")
    sg = _sigmas_device(sigmas, K, dev)
    othr, vthr = nms_threshold("oks_thr", oks_thr, dev), nms_threshold("vis_thr", vis_thr, dev)
    ws = _workspace(lib().udapose_pose_nms_ws_bytes(M), dev)
    out = {"score": torch.empty(M, dtype=torch.float32, device=dev), "order": torch.empty(M, dtype=torch.int32, device=dev),
           "keep": torch.empty(M, dtype=torch.uint8, device=dev), "n_keep": torch.empty(1, dtype=torch.int32, device=dev),
           "suppressed_by": torch.empty(M, dtype=torch.int32, device=dev)}
    if want_matrix:
        out["oks"] = torch.empty(M, M, dtype=torch.float32, device=dev)
    check(lib().udapose_pose_nms(_hip.stream(), ptr(kp), ptr(conf), ptr(bx), ptr(fi), ptr(st), ptr(bs), ptr(sg), ptr(vthr), ptr(othr), M, K,
                                 ptr(ws), ptr(out["score"]), ptr(out["order"]), ptr(out["keep"]), ptr(out["n_keep"]), ptr(out["suppressed_by"]),
                                 ptr(out.get("oks"))), "pose_nms")
    return out


# ---------------------------------------------------------------------------------------------------------------- key-point AP under OKS
# COCO-style evaluation of predict(nms=True)'s poses against labelled ones (csrc/pose_ap.hip): cocoapi's evaluateImg +
# accumulate for key points, on the device.  The defaults are cocoapi's Params for iouType = 'keypoints'.
AP_OKS_THRESHOLDS = tuple(np.linspace(.5, .95, 10))
AP_AREA_RANGES = {"all": (0, 1e10), "medium": (32 ** 2, 96 ** 2), "large": (96 ** 2, 1e10)}
AP_RECALL_POINTS = tuple(np.linspace(.0, 1.00, int(np.round(1.00 / .01)) + 1))
AP_MAX_COMBOS = 64             # UDAPOSE_AP_MAX_COMBOS (include/udapose.h): thresholds x ranges, one per lane of the matching wave
AP_MAX_DETS = 64               # UDAPOSE_AP_MAX_DETS
AP_MAX_RECALL_POINTS = 128     # UDAPOSE_AP_MAX_RECALL_POINTS
AP_MAX_CAPACITY = 1 << 18      # UDAPOSE_AP_MAX_CAPACITY
AP_MAX_FRAMES = 4096           # UDAPOSE_AP_MAX_FRAMES
AP_COUNTS = ("records", "dropped", "refused", "cut", "overflow_frames", "bad_labels")      # counters[0 .. UDAPOSE_AP_COUNTERS)


def _check_ap_thresholds(thresholds):
    """T OKS thresholds as the kernel takes them, a float32 array: each in (0, 1), strictly ascending AS fp32.  ValueError otherwise."""
    def check_range(t32):
        if t32.size < 1 or not (np.isfinite(t32).all() and (t32 > 0).all() and (t32 < 1).all()):
            raise ValueError(f"OKS thresholds must be in (0, 1) as fp32, at least one of them, got {list(thresholds)!r}")
    return _ascending_f32(thresholds, "OKS thresholds", check_range)


class APMeter(_LazyDeviceState):
    """Key-point AP under OKS over a whole set, COCO-style, kept on the device (csrc/pose_ap.hip).  An update matches the
    detections of its frames to the labelled poses (cocoapi's evaluateImg: per frame the `max_dets` best detections, greedily, at every
    threshold and in every area range) and appends one record per detection - its score and a matched / ignored bit per (range, threshold),
    bit a * T + t - to record arrays on the device; `compute()` sorts the records, forms the precision / recall tables (cocoapi's
    accumulate, fp64) and reads them back once.  Nothing else is read back, so an update can be captured, and a replay appends again.

    sigmas: as oks_nms takes them.  thresholds: T values in (0, 1), strictly ascending as fp32.  area_ranges: A named (lo, hi) pairs of
    label areas, the first one the range the headline numbers are taken from; T * A <= 64.  max_dets: 1 .. 64.  recall_points: at most 128,
    uploaded as the fp64 numbers given.  capacity: the records kept, at most 2^18; later ones are dropped and counted.
    Deviations from cocoapi: a label without a visible joint is ignored in every range and matches nothing (cocoapi falls back to a
    box distance); a frame with more than 64 labels is left out whole and counted in `overflow_frames`; no crowd regions."""

    def __init__(self, num_keypoints, sigmas=None, thresholds=AP_OKS_THRESHOLDS, area_ranges=None, max_dets=20, recall_points=AP_RECALL_POINTS,
                 capacity=65536, device=None):
        self.num_keypoints = int(num_keypoints)
        if not 1 <= self.num_keypoints <= NMS_MAX_KEYPOINTS:
            raise ValueError(f"APMeter takes 1 to {NMS_MAX_KEYPOINTS} key points (UDAPOSE_NMS_MAX_KEYPOINTS), got {num_keypoints}")
        self._thr32 = _check_ap_thresholds(thresholds)
        self.thresholds = tuple(float(t) for t in thresholds)
        ranges = dict(AP_AREA_RANGES if area_ranges is None else area_ranges)
        self.area_ranges = {str(n): (float(lo), float(hi)) for n, (lo, hi) in ranges.items()}
        if not self.area_ranges or any(np.isnan(v) for r in self.area_ranges.values() for v in r):
            raise ValueError(f"area_ranges must be named (lo, hi) pairs, at least one, got {area_ranges!r}")
        T, A = len(self._thr32), len(self.area_ranges)
        if T * A > AP_MAX_COMBOS:
            raise ValueError(f"thresholds x area ranges must be at most {AP_MAX_COMBOS} (UDAPOSE_AP_MAX_COMBOS), got {T} x {A} = {T * A}")
        self.max_dets = int(max_dets)
        if not 1 <= self.max_dets <= AP_MAX_DETS or self.max_dets != max_dets:
            raise ValueError(f"max_dets must be an integer in [1, {AP_MAX_DETS}], got {max_dets!r}")
        self._rp64 = np.asarray([float(r) for r in recall_points], dtype=np.float64)
        if not 1 <= self._rp64.size <= AP_MAX_RECALL_POINTS or np.isnan(self._rp64).any():
            raise ValueError(f"1 to {AP_MAX_RECALL_POINTS} recall points, got {self._rp64.size}")
        self.recall_points = tuple(float(r) for r in self._rp64)
        self.capacity = int(capacity)
        if not 1 <= self.capacity <= AP_MAX_CAPACITY or self.capacity != capacity:
            raise ValueError(f"capacity must be an integer in [1, {AP_MAX_CAPACITY}], got {capacity!r}")
        self._sigmas_arg = sigmas
        if sigmas is not None and not torch.is_tensor(sigmas) and not isinstance(sigmas, str):
            table = tuple(float(v) for v in sigmas)
            if len(table) != self.num_keypoints or not all(np.isfinite(v) and v > 0 for v in table):
                raise ValueError(f"sigmas must be {self.num_keypoints} positive numbers, got {table}")
        self._init_device(device)

    def _make(self, device):
        T, A, R, cap = len(self._thr32), len(self.area_ranges), self._rp64.size, self.capacity
        ranges = np.asarray(list(self.area_ranges.values()), dtype=np.float64).astype(np.float32)
        # (the record arrays have one more slot than capacity: merge() sends what does not fit there)
        return {"thr": torch.from_numpy(self._thr32).to(device), "ranges": torch.from_numpy(ranges).to(device),
                "rp": torch.from_numpy(self._rp64).to(device), "sigmas": _sigmas_device(self._sigmas_arg, self.num_keypoints, device),
                "score": torch.zeros(cap + 1, dtype=torch.float32, device=device),
                "matched": torch.zeros(cap + 1, dtype=torch.int64, device=device),
                "ignored": torch.zeros(cap + 1, dtype=torch.int64, device=device),
                "counters": torch.zeros(len(AP_COUNTS) + A, dtype=torch.int64, device=device)}

    def reset(self):
        """Zero the counters (in place: a captured update keeps appending to the same memory); the records behind the count mean nothing."""
        self._on_device()["counters"].zero_()

    def state(self):
        """The raw state on the device, the meter's own tensors: {"score" fp32, "matched", "ignored" int64 words (bit a * T + t), each
        [capacity + 1] with the first counters[0] entries in use; "counters" int64 [6 + A]: AP_COUNTS, then npig per range}."""
        st = self._on_device()
        return {k: st[k] for k in ("score", "matched", "ignored", "counters")}

    def update(self, keypoints, score, frame_idx, gt_keypoints, gt_visible, gt_area, gt_frame, *, num_frames, area=None, valid=None,
               gt_ignore=None):
        """Match one update's detections (keypoints [M,K,2] in frame pixels, score [M], frame_idx [M] integers; valid [M], non-zero = takes
        part, None: all; area [M], None: the key points' extent (max x - min x) * (max y - min y)) to its labelled poses (gt_keypoints
        [G,K,2], gt_visible [G,K], > 0 counts, gt_area [G], gt_frame [G]; gt_ignore [G], non-zero = ignored, None: none) on frames
        [0, num_frames), and append the records.  1 <= M, G, num_frames <= 4096.  CUDA tensors only; shape errors raise ValueError before
        any launch; nothing is read back."""
        kp = _pose_tensor(keypoints, (None, self.num_keypoints, 2), "keypoints")
        M, K = kp.shape[:2]
        _check_mk(M, K)
        sc = _pose_tensor(score, (M,), "score")
        fi = _pose_tensor(frame_idx, (M,), "frame_idx", torch.int32)
        va = None if valid is None else _pose_tensor(valid != 0 if torch.is_tensor(valid) else valid, (M,), "valid", torch.uint8)
        ar = None if area is None else _pose_tensor(area, (M,), "area")
        gk = _pose_tensor(gt_keypoints, (None, K, 2), "gt_keypoints")
        G = gk.shape[0]
        if not 1 <= G <= NMS_MAX_POSES:
            raise ValueError(f"1 to {NMS_MAX_POSES} labelled poses a call, got {G}")
        gv = _pose_tensor(gt_visible, (G, K), "gt_visible")
        ga = _pose_tensor(gt_area, (G,), "gt_area")
        gf = _pose_tensor(gt_frame, (G,), "gt_frame", torch.int32)
        gi = None if gt_ignore is None else _pose_tensor(gt_ignore != 0 if torch.is_tensor(gt_ignore) else gt_ignore, (G,), "gt_ignore", torch.uint8)
        F = int(num_frames)
        if not 1 <= F <= AP_MAX_FRAMES or F != num_frames:
            raise ValueError(f"num_frames must be an integer in [1, {AP_MAX_FRAMES}], got {num_frames!r}")
        st = self._on_device(kp)
        dev = st["counters"].device
        if any(t is not None and t.device != dev for t in (kp, sc, fi, va, ar, gk, gv, ga, gf, gi)):
            raise ValueError(f"the meter's state lives on {dev}: every tensor of an update must")
        ws = _workspace(lib().udapose_ap_match_ws_bytes(M, G, F), dev)      # (a capture keeps its own)
        check(lib().udapose_ap_match(_hip.stream(), ptr(kp), ptr(sc), ptr(fi), ptr(va), ptr(ar), M, ptr(gk), ptr(gv), ptr(ga), ptr(gf), ptr(gi), G, K,
                                     F, ptr(st["sigmas"]), ptr(st["thr"]), len(self._thr32), ptr(st["ranges"]), len(self.area_ranges),
                                     self.max_dets, ptr(ws), ptr(st["score"]), ptr(st["matched"]), ptr(st["ignored"]), self.capacity,
                                     ptr(st["counters"])), "ap_match")

    def update_predict(self, result, frame_idx, gt_keypoints, gt_visible, gt_area, gt_frame, *, num_frames, gt_ignore=None):
        """update() on engine.predict(nms=True)'s dict: its key points, its rescored "score", valid = keep & (status == 0), the area from the
        key points."""
        missing = [k for k in ("keypoints", "score", "keep", "status") if k not in result]
        if missing:
            raise ValueError(f"update_predict() takes predict(nms=True)'s dict: {missing} are missing")
        valid = (result["keep"] != 0) & (result["status"] == 0)
        self.update(result["keypoints"], result["score"], frame_idx, gt_keypoints, gt_visible, gt_area, gt_frame, num_frames=num_frames,
                    valid=valid, gt_ignore=gt_ignore)

    def merge(self, other):
        """Append another meter's records (same tables and capacity rules; any device) after this one's, and add its counts: ranks or
        shards of one set.  Reads the other's record count - the one read-back outside compute()."""
        if not isinstance(other, APMeter):
            raise ValueError("merge() takes an APMeter")
        if (other._thr32.tolist(), other.area_ranges, other.max_dets, other.num_keypoints) != \
                (self._thr32.tolist(), self.area_ranges, self.max_dets, self.num_keypoints):
            raise ValueError("merge() takes a meter with the same thresholds, area ranges, max_dets and key points")
        st, ot = self._on_device(), other._on_device()
        dev = st["counters"].device
        oc = ot["counters"].to(dev)
        n = int(ot["counters"][0])
        c = st["counters"]
        if n:
            at = torch.clamp(torch.arange(n, device=dev) + c[0], max=self.capacity)      # (what does not fit lands in the spare slot)
            for k in ("score", "matched", "ignored"):
                st[k].index_copy_(0, at, ot[k][:n].to(dev))
        total = c[0] + oc[0]
        stored = torch.clamp(total, max=self.capacity)
        c[1:] += oc[1:]
        c[1] += total - stored
        c[0] = stored

    def compute(self):
        """The curve launches (udapose_ap_curve), the one read-back, then `report()`.  Warns when records were dropped or frames left out."""
        st = self._on_device()
        dev = st["counters"].device
        T, A, R = len(self._thr32), len(self.area_ranges), self._rp64.size
        ws = _workspace(lib().udapose_ap_curve_ws_bytes(self.capacity, T, A), dev)
        precision = torch.empty(T, R, A, dtype=torch.float64, device=dev)
        recall = torch.empty(T, A, dtype=torch.float64, device=dev)
        scores = torch.empty(T, R, A, dtype=torch.float32, device=dev)
        check(lib().udapose_ap_curve(_hip.stream(), ptr(st["score"]), ptr(st["matched"]), ptr(st["ignored"]), self.capacity, ptr(st["counters"]), T,
                                     A, ptr(st["rp"]), R, ptr(ws), ptr(precision), ptr(scores), ptr(recall)), "ap_curve")
        parts = [precision.reshape(-1).view(torch.uint8), recall.reshape(-1).view(torch.uint8), st["counters"].view(torch.uint8),
                 scores.reshape(-1).view(torch.uint8)]
        host = torch.cat(parts).cpu().numpy()
        cut = np.cumsum([p.numel() for p in parts])
        p = host[:cut[0]].view(np.float64).reshape(T, R, A)
        r = host[cut[0]:cut[1]].view(np.float64).reshape(T, A)
        cnt = host[cut[1]:cut[2]].view(np.int64)
        s = host[cut[2]:].view(np.float32).reshape(T, R, A)
        rep = APMeter.report(p, r, s, cnt[len(AP_COUNTS):], cnt[:len(AP_COUNTS)], thresholds=self.thresholds, area_ranges=tuple(self.area_ranges))
        if rep["counts"]["dropped"] or rep["counts"]["overflow_frames"]:
            import warnings
            warnings.warn(f"APMeter: {rep['counts']['dropped']} records beyond capacity {self.capacity} were dropped and "
                          f"{rep['counts']['overflow_frames']} frames with more than 64 labels were left out: the numbers are not the whole set's")
        return rep

    @staticmethod
    def report(precision, recall, scores, npig, counts, thresholds=AP_OKS_THRESHOLDS, area_ranges=tuple(AP_AREA_RANGES)):
        """The report of the tables, in fp64 on the host (pure: no device, no side effect), cocoapi's summarize for key points:
          AP            the mean of precision[:, :, first range] over the entries > -1, -1 without one; AR the same over recall
          AP50, AP75    the same at the threshold nearest .5 / .75 (absent when no threshold is within 1e-6 of it); AR50, AR75
          AP_<range>, AR_<range>   for every range; APM / APL (ARM / ARL) alias the ranges named "medium" / "large"
          precision [T,R,A], recall [T,A], scores [T,R,A]; npig [A] int64; counts {records, dropped, refused, cut, overflow_frames,
          bad_labels}; thresholds, area_ranges as given"""
        thr = np.asarray([float(t) for t in thresholds], dtype=np.float64)
        names = tuple(area_ranges)
        p, r, s = np.asarray(precision, dtype=np.float64), np.asarray(recall, dtype=np.float64), np.asarray(scores)
        T, A = thr.size, len(names)
        if p.ndim != 3 or p.shape[0] != T or p.shape[2] != A or r.shape != (T, A) or s.shape != p.shape:
            raise ValueError(f"report() takes precision / scores [{T},R,{A}] and recall [{T},{A}], got {p.shape}, {s.shape}, {r.shape}")
        cnt = np.asarray(counts, dtype=np.int64).reshape(-1)
        if cnt.size != len(AP_COUNTS) or np.asarray(npig).size != A:
            raise ValueError(f"report() takes {len(AP_COUNTS)} counts and npig [{A}]")

        def mean(x):
            x = x[x > -1]
            return float(x.mean()) if x.size else -1.0

        rep = {"AP": mean(p[:, :, 0]), "AR": mean(r[:, 0])}
        for tag, want in (("50", .5), ("75", .75)):
            t = int(np.abs(thr - want).argmin())
            if abs(thr[t] - want) < 1e-6:
                rep["AP" + tag], rep["AR" + tag] = mean(p[t, :, 0]), mean(r[t, 0:1])
        for a, name in enumerate(names):
            rep["AP_" + name], rep["AR_" + name] = mean(p[:, :, a]), mean(r[:, a])
        for short, name in (("M", "medium"), ("L", "large")):
            if name in names:
                rep["AP" + short], rep["AR" + short] = rep["AP_" + name], rep["AR_" + name]
        rep.update({"precision": p, "recall": r, "scores": s, "npig": np.asarray(npig, dtype=np.int64).copy(),
                    "counts": {n: int(v) for n, v in zip(AP_COUNTS, cnt)}, "thresholds": tuple(float(t) for t in thresholds),
                    "area_ranges": names})
        return rep
