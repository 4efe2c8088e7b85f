"""Arg-max decode and PCK (API mirror of the reference's lib/keypoint_detection.py:9-94) on MI355X kernels, and the soft-argmax
decode the reference lacks (`soft_argmax`, csrc/softargmax.hip: sub-pixel coordinates, differentiable), the two published sub-pixel
decodes (`quarter_decode`, `dark_decode`, csrc/refine.hip: one launch, not differentiable), and the flip test's heat-map side
(`flip_perm`, `flip_back`, `flip_merge`, csrc/flip.hip: flip back, swap left / right joints, average, decode - one launch).

The reference takes numpy arrays (it is called on `.cpu().numpy()` copies, train_human.py:289,443).  The same calls work
here; torch CUDA tensors are accepted as well and avoid the 2 x 8.4 MB device->host copy per iteration: decode and PCK
run on the device and only K+2 floats and the [B,K,2] coordinates come back.
"""
import numpy as np
import torch

from .. import _hip
from .._hip import check, lib, ptr


def _dev_f32(a):
    if isinstance(a, np.ndarray):
        assert a.ndim == 4, 'batch_images should be 4-ndim'
        if not torch.cuda.is_available():
            raise RuntimeError("uda_poseestimation_amd.lib.keypoint_detection needs the MI355X (no CPU fallback)")
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    assert torch.is_tensor(a) and a.dim() == 4, 'batch_heatmaps should be numpy.ndarray or a 4-d tensor'
    _hip.require_cuda(a)
    return a.detach().float().contiguous()


def _decode(hm):
    B, K, H, W = hm.shape
    preds = torch.empty(B, K, 2, dtype=torch.float32, device=hm.device)
    maxv = torch.empty(B, K, 1, dtype=torch.float32, device=hm.device)
    check(lib().udapose_heatmap_argmax(_hip.stream(), ptr(hm), B * K, H, W, ptr(maxv), None, ptr(preds), None, None, 0), "heatmap_argmax")
    return preds, maxv


def get_max_preds(batch_heatmaps):
    """[B,K,H,W] -> (preds [B,K,2] float32 (x,y), maxvals [B,K,1]); numpy in -> numpy out, tensor in -> tensor out."""
    is_np = isinstance(batch_heatmaps, np.ndarray)
    if not is_np and not torch.is_tensor(batch_heatmaps):
        raise AssertionError('batch_heatmaps should be numpy.ndarray')
    preds, maxv = _decode(_dev_f32(batch_heatmaps))
    if is_np:
        return preds.cpu().numpy(), maxv.cpu().numpy().astype(batch_heatmaps.dtype, copy=False)
    return preds, maxv


class _SoftArgmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hm, beta, window):
        B, K, H, W = hm.shape
        h = hm.detach().float().contiguous()
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
        gc = g.detach().float().contiguous()
        check(lib().udapose_soft_argmax_bwd(_hip.stream(), ptr(h), ptr(gc), ptr(idx), ptr(stats), B * K, H, W, ctx.beta, ctx.window, ptr(d)),
              "soft_argmax_bwd")
        return d.reshape(ctx.shape).to(ctx.in_dtype), None, None


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
    is_np = isinstance(batch_heatmaps, np.ndarray)
    if not is_np and not torch.is_tensor(batch_heatmaps):
        raise AssertionError('batch_heatmaps should be numpy.ndarray or a 4-d tensor')
    beta, window = _soft_args(beta, window)
    if is_np:
        coords, maxv = _SoftArgmaxFn.apply(_dev_f32(batch_heatmaps), beta, window)
        return coords.cpu().numpy(), maxv.cpu().numpy().astype(batch_heatmaps.dtype, copy=False)
    assert batch_heatmaps.dim() == 4, 'batch_heatmaps should be numpy.ndarray or a 4-d tensor'
    _hip.require_cuda(batch_heatmaps)
    return _SoftArgmaxFn.apply(batch_heatmaps, beta, window)


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
    is_np = isinstance(batch_heatmaps, np.ndarray)
    if not is_np and not torch.is_tensor(batch_heatmaps):
        raise AssertionError('batch_heatmaps should be numpy.ndarray or a 4-d tensor')
    assert batch_heatmaps.ndim == 4, 'batch_heatmaps should be numpy.ndarray or a 4-d tensor'
    kernel, sigma = _dark_args(kernel, sigma, *batch_heatmaps.shape[2:]) if mode == 1 else (0, 0.0)
    coords, maxv = _refine(_dev_f32(batch_heatmaps), mode, kernel, sigma)
    if is_np:
        return coords.cpu().numpy(), maxv.cpu().numpy().astype(batch_heatmaps.dtype, copy=False)
    return coords, maxv


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


def _decode_pred(o, decode):
    """The prediction's coordinates under `decode`: "argmax", "soft" (soft_argmax(beta=10, window=5)), "quarter" (quarter_decode), "dark"
    (dark_decode(kernel=11)) or a callable hm -> (coords, maxvals).  The soft decodes get the reference's `maxval > 0` zeroing, so every
    decode agrees on which joints are absent ("quarter" and "dark" zero them in their own launch)."""
    if decode == "argmax":
        return _decode(o)[0]
    if decode == "quarter":
        return _refine(o, 0)[0]
    if decode == "dark":
        return _refine(o, 1, *_dark_args(11, None, *o.shape[2:]))[0]
    if decode == "soft":
        coords, maxv = _SoftArgmaxFn.apply(o, 10.0, 5)
    elif callable(decode):
        coords, maxv = decode(o)
        coords, maxv = _dev_f32c(coords, o), _dev_f32c(maxv, o)
    else:
        raise ValueError(f"decode must be 'argmax', 'soft', 'quarter', 'dark' or a callable, got {decode!r}")
    B, K = o.shape[:2]
    return (coords.detach().reshape(B, K, 2) * (maxv.detach().reshape(B, K, 1) > 0).to(torch.float32)).contiguous()


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
    is_np = isinstance(output, np.ndarray)
    acc, avg_cnt, pred = accuracy_device(output, target, thr, decode)
    ac = avg_cnt.cpu()
    acc_np = acc.cpu().numpy().astype(np.float64)
    return acc_np, float(ac[0]), int(ac[1]), (pred.cpu().numpy() if is_np else pred)


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
    is_np = isinstance(output_flipped, np.ndarray)
    f = _dev_f32(output_flipped)
    out, _, _ = _flip_merge(None, f, _perm_device(flip_pairs, f.shape[1], f.device), shift, False)
    return out.cpu().numpy().astype(output_flipped.dtype, copy=False) if is_np else out


def flip_merge(output, output_flipped, flip_pairs, shift=False, decode=False):
    """The flip test's average: (output + flip_back(output_flipped, flip_pairs, shift)) * 0.5 as [B,K,H,W] fp32.  decode=True returns
    (merged, preds [B,K,2], maxvals [B,K,1]) with the arg-max decode of `merged` (what get_max_preds gives for it) out of the same
    launch.  numpy in -> numpy out, tensor in -> tensor out."""
    is_np = isinstance(output, np.ndarray)
    a, f = _dev_f32(output), _dev_f32(output_flipped)
    if a.shape != f.shape:
        raise ValueError(f"output {tuple(a.shape)} and output_flipped {tuple(f.shape)} differ in shape")
    out, preds, maxv = _flip_merge(a, f, _perm_device(flip_pairs, f.shape[1], f.device), shift, decode)
    if is_np:
        out = out.cpu().numpy().astype(output.dtype, copy=False)
        return (out, preds.cpu().numpy(), maxv.cpu().numpy().astype(output.dtype, copy=False)) if decode else out
    return (out, preds, maxv) if decode else out

