"""Batched heat-map / image re-warp on the device.

Stands in for the per-sample `tF.affine` triplets of the training loop (train_human.py:361-372, 385-391, 412, 418-423):
translate by (tx/ratio, ty/ratio); rotate by `angle` and scale; shear by (sx, sy) - three sequential resamplings in ONE launch
(results identical to the sequential form).  mode "nearest" (the default, the reference's) evaluates the chain as index maps;
mode "bilinear" (`InterpolationMode.BILINEAR` per stage: four taps, zero padding, every stage clipped on its own) runs the stages
ping-pong in LDS, and its backward is the exact transpose as a gather - no float atomics, bit-reproducible.  The inverse
affine matrices are built on the host in double precision exactly like torchvision's `_get_inverse_affine_matrix`
(torchvision itself is not a dependency); parameters arrive as the collated `aug_param` structure of
lib/transforms/keypoint_detection.py:139: [angle[N], [tx[N], ty[N]], [sx[N], sy[N]], scale[N]].
"""
import collections
import math

import torch

from . import _hip
from . import heatmap_args as ha
from ._hip import check, lib, ptr


def inverse_affine_matrix(angle, translate, scale, shear):
    """torchvision.transforms.functional._get_inverse_affine_matrix with center=(0,0) (tensor inputs)."""
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d / scale, -b / scale, 0.0, -c / scale, a / scale, 0.0]
    m[2] += m[0] * (-tx) + m[1] * (-ty)
    m[5] += m[3] * (-tx) + m[4] * (-ty)
    return m


def _as_list(v, n):
    if torch.is_tensor(v):
        return [float(x) for x in v.tolist()]
    if isinstance(v, (list, tuple)):
        return [float(x) for x in v]
    return [float(v)] * n


def _inv_mats(angle, tx, ty, scale, sx, sy):
    """Vectorised (float64) inverse_affine_matrix for arrays of parameters -> [n, 6]."""
    import numpy as np
    rot, sx, sy = np.radians(angle), np.radians(sx), np.radians(sy)
    a = np.cos(rot - sy) / np.cos(sy)
    b = -np.cos(rot - sy) * np.tan(sx) / np.cos(sy) - np.sin(rot)
    c = np.sin(rot - sy) / np.cos(sy)
    d = -np.sin(rot - sy) * np.tan(sx) / np.cos(sy) + np.cos(rot)
    m0, m1, m3, m4 = d / scale, -b / scale, -c / scale, a / scale
    m2 = m0 * (-tx) + m1 * (-ty)
    m5 = m3 * (-tx) + m4 * (-ty)
    return np.stack([m0, m1, m2, m3, m4, m5], -1)


def pack_aug_param(aug_param, n, out=None):
    """The collated aug_param structure -> one [N,6] float64 host tensor (angle, tx, ty, shear_x, shear_y, scale): what
    udapose_recon_thetas reads.  `out`: a (pinned) host tensor to fill instead of a new one."""
    import numpy as np
    angle, (tx, ty), (sx, sy), scale = aug_param[:4]
    cols = [np.asarray(_as_list(v, n), np.float64) for v in (angle, tx, ty, sx, sy, scale)]
    t = out if out is not None else torch.empty(n, 6, dtype=torch.float64)
    t.numpy()[...] = np.stack(cols, 1)
    return t


def thetas_from_packed(params_dev, ratio, want_fwd=True, want_back=False, fwd=None, back=None):
    """Device-side matrices (udapose_recon_thetas) from a packed [N,6] float64 DEVICE tensor: (theta_fwd [N,3,6] | None,
    theta_back [N,1,6] | None); `fwd` / `back` name existing output tensors (a captured step writes its static ones)."""
    _hip.require_cuda(params_dev)
    assert params_dev.dtype == torch.float64 and params_dev.is_contiguous() and params_dev.shape[1] == 6
    n = params_dev.shape[0]
    if want_fwd and fwd is None:
        fwd = torch.empty(n, 3, 6, dtype=torch.float32, device=params_dev.device)
    if want_back and back is None:
        back = torch.empty(n, 1, 6, dtype=torch.float32, device=params_dev.device)
    check(lib().udapose_recon_thetas(_hip.stream(), ptr(params_dev), n, float(ratio), ptr(fwd) if want_fwd else None,
                                     ptr(back) if want_back else None), "recon_thetas")
    return (fwd if want_fwd else None), (back if want_back else None)


def recon_thetas(aug_param, n, ratio=1.0, device=None):
    """[N,3,6] fp32 matrices of the loop's translate -> rotate+scale -> shear chain for a collated aug_param.  With a CUDA
    `device` the matrices are computed there (double precision, udapose_recon_thetas); without, on the host."""
    import numpy as np
    if device is not None and torch.device(device).type == "cuda":
        return thetas_from_packed(pack_aug_param(aug_param, n).to(device), ratio)[0]
    angle, (tx, ty), (sx, sy), scale = aug_param[:4]
    angle, tx, ty, sx, sy, scale = (np.asarray(_as_list(v, n), np.float64) for v in (angle, tx, ty, sx, sy, scale))
    z, o = np.zeros(n), np.ones(n)
    th = np.stack([_inv_mats(z, tx / ratio, ty / ratio, o, z, z), _inv_mats(angle, z, z, scale, z, z), _inv_mats(z, z, z, o, sx, sy)], 1)
    t = torch.from_numpy(th.astype(np.float32))
    return t.to(device) if device is not None else t


def single_thetas(angle, translate, scale, shear, n, device=None):
    """[N,1,6]: one warp per sample (the occlusion path's warp-back, train_human.py:412)."""
    angle, scale = _as_list(angle, n), _as_list(scale, n)
    tx, ty = _as_list(translate[0], n), _as_list(translate[1], n)
    sx, sy = _as_list(shear[0], n), _as_list(shear[1], n)
    th = torch.empty(n, 1, 6, dtype=torch.float32)
    for i in range(n):
        th[i, 0] = torch.tensor(inverse_affine_matrix(angle[i], [tx[i], ty[i]], scale[i], [sx[i], sy[i]]))
    return th.to(device) if device is not None else th


MODES = ("nearest", "bilinear")
BILINEAR_LDS_BYTES = 150 * 1024         # two fp32 planes must fit (csrc/affine.hip); larger planes run stage by stage from global memory


def interpolation_mode(interpolation):
    """torchvision's `interpolation` argument -> "nearest" | "bilinear": None, 0, "nearest" or an enum whose .value is "nearest";
    2, "bilinear" or an enum whose .value is "bilinear" (InterpolationMode, or PIL's integer codes).  Anything else is refused."""
    v = getattr(interpolation, "value", interpolation)
    if v is None or (isinstance(v, str) and v == "nearest") or (isinstance(v, int) and not isinstance(v, bool) and v == 0):
        return "nearest"
    if (isinstance(v, str) and v == "bilinear") or (isinstance(v, int) and not isinstance(v, bool) and v == 2):
        return "bilinear"
    raise NotImplementedError(f"interpolation {interpolation!r}: only nearest (torchvision's default, the one the reference uses) and "
                              "bilinear have device kernels")


def bilinear_fits_lds(H, W):
    """Whether a bilinear chain over H x W planes takes the one-launch LDS form (which allocates nothing: capturable)."""
    return 2 * int(H) * int(W) * 4 <= BILINEAR_LDS_BYTES


def _chain_call(mode, H, W):
    if mode == "nearest":
        return lib().udapose_affine_nearest
    if mode != "bilinear":
        raise ValueError(f"warp mode {mode!r}: one of {MODES}")
    if not bilinear_fits_lds(H, W) and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"bilinear re-warp of {H}x{W} planes inside a stream capture: two planes exceed the {BILINEAR_LDS_BYTES // 1024} KB "
                           "LDS budget, and the stage-by-stage form allocates scratch memory - run it outside the capture")
    return lib().udapose_affine_bilinear


MIRROR_OUT, MIRROR_IN = 1, 2            # UDAPOSE_MIRROR_OUT / UDAPOSE_MIRROR_IN: the two bits of a sample's `mirror` byte


def _mirror_call(mode):
    return lib().udapose_affine_nearest_mirror if mode == "nearest" else lib().udapose_affine_bilinear_mirror


def _launch(mode, src, dst, th, mirror, perm, backward):
    """The chain's launch, plain (mirror None: exactly the call of the un-mirrored package) or mirrored."""
    N, C, H, W = src.shape
    name = f"affine_{mode}" + ("_bwd" if backward else "")
    if mirror is None:
        check(_chain_call(mode, H, W)(_hip.stream(), ptr(src), ptr(dst), ptr(th), N, C, H, W, th.shape[1], backward), name)
    else:
        check(_mirror_call(mode)(_hip.stream(), ptr(src), ptr(dst), ptr(th), N, C, H, W, th.shape[1], backward, ptr(mirror), ptr(perm)),
              name + "_mirror")


class _WarpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, theta, mode, mirror=None, perm=None):
        _hip.require_cuda(x, theta)
        xin = x.detach().float().contiguous()
        N, C, H, W = xin.shape
        th = theta.detach().float().contiguous()
        assert th.shape[0] == N and th.shape[2] == 6
        out = torch.empty_like(xin)
        _launch(mode, xin, out, th, mirror, perm, 0)
        ctx.save_for_backward(th)
        ctx.mirror, ctx.perm = mirror, perm          # (not differentiable, never written by the package: kept as they are)
        ctx.in_dtype = x.dtype
        ctx.mode = mode
        return out.to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        (th,) = ctx.saved_tensors
        gin = g.detach().float().contiguous()
        dx = torch.empty_like(gin)
        _launch(ctx.mode, gin, dx, th, ctx.mirror, ctx.perm, 1)
        return dx.to(ctx.in_dtype), None, None, None, None


def mirror_perm(flip_pairs, num_channels, device):
    """The joint permutation of a flip as a [C] int32 tensor on `device` (uploaded once per table and device): flip_pairs = a sequence of
    pairs or a key of lib.keypoint_detection.FLIP_PAIRS; () - "hand21" - is the identity."""
    from .lib import keypoint_detection as kd
    perm = kd._perm_device(flip_pairs, num_channels, torch.device(device))
    perm._udapose_involution = int(num_channels)          # (flip_perm builds an involution: _check_mirror need not read it back)
    return perm


def _check_mirror(x, mode, mirror, perm):
    """Everything a mirrored launch relies on, before the launch: ValueError / NotImplementedError."""
    N, C, H, W = x.shape
    if not (torch.is_tensor(mirror) and mirror.is_cuda and mirror.dtype == torch.uint8 and tuple(mirror.shape) == (N,) and mirror.is_contiguous()):
        raise ValueError(f"warp_chain: mirror must be a contiguous uint8 CUDA tensor of shape [{N}] (bit 0 MIRROR_OUT, bit 1 MIRROR_IN)")
    if perm is not None:
        if not (torch.is_tensor(perm) and perm.is_cuda and perm.dtype == torch.int32 and perm.dim() == 1 and perm.is_contiguous()):
            raise ValueError("warp_chain: perm must be a contiguous int32 CUDA tensor [C]")
        if perm.shape[0] != C:
            raise ValueError(f"warp_chain: perm has {perm.shape[0]} entries for {C} channels")
        if getattr(perm, "_udapose_involution", None) != C:
            # read back once per tensor (mirror_perm's tables are cached, so a loop pays this once); a tensor first met inside a stream
            # capture cannot be read: check it before capturing
            if torch.cuda.is_current_stream_capturing():
                raise ValueError("warp_chain: perm has not been checked yet and cannot be read inside a stream capture")
            p = perm.cpu()
            idx = torch.arange(C, dtype=torch.int32)
            if bool(((p < 0) | (p >= C)).any()) or not torch.equal(p[p.long()], idx):
                raise ValueError(f"warp_chain: perm {p.tolist()} is not an involution of 0..{C - 1} (a flip swaps joints in pairs)")
            perm._udapose_involution = C
    if mode == "bilinear" and not bilinear_fits_lds(H, W):
        raise NotImplementedError(f"mirrored bilinear re-warp of {H}x{W} planes: two planes exceed the {BILINEAR_LDS_BYTES // 1024} KB LDS budget "
                                  "and the stage-by-stage form has no mirrored counterpart")


def warp_chain(x, theta, mode="nearest", mirror=None, perm=None):
    """x [N,C,H,W]; theta [N,S,6] inverse affine matrices applied in order 0..S-1 (zero fill); differentiable.  mode: "nearest" or
    "bilinear" (the backward of either is deterministic).
    mirror: None (the plain launch), or a [N] uint8 CUDA tensor of two bits per sample: MIRROR_OUT reverses the columns of
    the chain's output, MIRROR_IN those of its input; perm: None or the [C] int32 device tensor of the flip's joint permutation (an
    involution, `mirror_perm`), applied to the samples with exactly one bit set: out[n, c] comes from x[n, perm[c]].  Forward and backward
    give the bits of the composition of torch.flip(., [-1]), index_select by perm and the plain call."""
    if mode not in MODES:
        raise ValueError(f"warp mode {mode!r}: one of {MODES}")
    if mirror is None:
        if perm is not None:
            raise ValueError("warp_chain: perm without mirror")
        return _WarpFn.apply(x, theta, mode)
    _hip.require_cuda(x, theta)
    _check_mirror(x, mode, mirror, perm)
    return _WarpFn.apply(x, theta, mode, mirror, perm)


def aug_mirror(aug_param, n):
    """The flip flags of a collated aug_param as a uint8 [N] host tensor: None for the reference's 4 entries; the optional 5th entry is
    flip[N] with values 0 or 1 (data_gpu.ViewConfig(flip=)).  ValueError for anything else."""
    if not isinstance(aug_param, (list, tuple)) or len(aug_param) not in (4, 5):
        raise ValueError(f"aug_param: expected (angle, (tx, ty), (shear_x, shear_y), scale[, flip]), got {type(aug_param).__name__} of "
                         f"{len(aug_param) if hasattr(aug_param, '__len__') else '?'} entries")
    if len(aug_param) == 4:
        return None
    f = aug_param[4]
    f = f.detach().cpu() if torch.is_tensor(f) else torch.as_tensor(f)
    if f.dim() != 1 or f.shape[0] != n:
        raise ValueError(f"aug_param: flip has shape {tuple(f.shape)} for a batch of {n}")
    if f.dtype == torch.bool:
        f = f.to(torch.uint8)
    if not bool(((f == 0) | (f == 1)).all()):
        raise ValueError(f"aug_param: flip flags must be 0 or 1, got {f.tolist()}")
    return f.to(torch.uint8).contiguous()


def mean_views(views):
    """Mean of k re-warped teacher heat-map tensors (train_human.py:361-372, `--k` > 1: `torch.mean(recons, dim=0)`): one launch, the k
    values added in view order in fp32 and divided by k."""
    import ctypes as C
    if len(views) == 1:
        return views[0]
    if len(views) > 8:
        raise NotImplementedError("at most 8 teacher views per step (the reference's --k defaults to 1)")
    vs = [v.detach().float().contiguous() for v in views]
    _hip.require_cuda(*vs)
    out = torch.empty_like(vs[0])
    arr = (C.c_void_p * len(vs))(*[v.data_ptr() for v in vs])
    check(lib().udapose_mean_views(_hip.stream(), arr, len(vs), ptr(out), out.numel()), "mean_views")
    return out


MERGE_MODES = {"mean": 0, "trimmed": 1}          # UDAPOSE_MERGE_MEAN / UDAPOSE_MERGE_TRIMMED
MergedViews = collections.namedtuple("MergedViews", "mean peaks maxvals inliers n_inliers spread2 agree energy")


def merge_views(views, radius=2.0, mode="mean", min_views=None, want_energy=False):
    """The k re-warped teacher heat-map tensors [B,K,H,W] merged BY AGREEMENT (udapose_view_merge), one launch in place of
    mean_views.  Per (sample, joint): every view's peak (first flat arg-max, the order of get_max_preds_torch_raw) and maximum; a view is
    valid where its maximum is > 0; the medoid is the valid view with the smallest sum of squared peak distances to the other valid views
    (lowest view on a tie); the inliers are the valid views within `radius` heat-map pixels of the medoid ((float)d2 <= radius * radius).
    mode "mean": the plain mean, the bits of mean_views; "trimmed": the mean of the inliers only, in view order (the plain mean where there
    is none).  agree = 1.0 where at least `min_views` (1..k, default k: every view) are inliers, else 0.0 - the per-joint gate that
    utils.confidence_mask takes as tea_mask=.  `radius`: a float, or a 0-d fp32 device tensor that is read on the device (no
    synchronisation; a captured launch follows its value).  want_energy: also the mean over pixels of the k views' variance.
    -> MergedViews(mean [B,K,H,W], peaks [k,B,K,2] int32 (x, y), maxvals [k,B,K], inliers [B,K] int32 (bit v = view v), n_inliers [B,K]
    int32, spread2 [B,K] int32 (largest squared distance between valid peaks), agree [B,K] fp32, energy [B,K] fp32 | None)."""
    import ctypes as C
    k = len(views)
    if k < 1:
        raise ValueError("merge_views: no views")
    if k > 8:
        raise NotImplementedError("at most 8 teacher views per step (the reference's --k defaults to 1)")
    if mode not in MERGE_MODES:
        raise ValueError(f"merge_views: mode {mode!r}: one of {tuple(MERGE_MODES)}")
    min_views = k if min_views is None else int(min_views)
    if not 1 <= min_views <= k:
        raise ValueError(f"merge_views: min_views = {min_views} is outside 1 ... {k} (the number of views)")
    _hip.require_cuda(*views, radius if torch.is_tensor(radius) else None)
    vs = [v.detach().float().contiguous() for v in views]
    if vs[0].dim() != 4 or any(v.shape != vs[0].shape for v in vs):
        raise ValueError(f"merge_views: the views must share one [B,K,H,W] shape, got {[tuple(v.shape) for v in vs]}")
    B, K, H, W = vs[0].shape
    dev = vs[0].device
    if torch.is_tensor(radius):
        if radius.numel() != 1:
            raise ValueError(f"merge_views: radius must be a float or a 0-d tensor, got shape {tuple(radius.shape)}")
        rad = radius.detach().reshape(())
        if rad.dtype != torch.float32:
            rad = rad.float()
    else:
        rad = torch.full((), float(radius), dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    out = MergedViews(torch.empty_like(vs[0]), torch.empty(k, B, K, 2, **i32), torch.empty(k, B, K, dtype=torch.float32, device=dev),
                      torch.empty(B, K, **i32), torch.empty(B, K, **i32), torch.empty(B, K, **i32),
                      torch.empty(B, K, dtype=torch.float32, device=dev), torch.empty(B, K, dtype=torch.float32, device=dev) if want_energy else None)
    arr = (C.c_void_p * k)(*[v.data_ptr() for v in vs])
    check(lib().udapose_view_merge(_hip.stream(), arr, k, B * K, H, W, MERGE_MODES[mode], ptr(rad), min_views, *[ptr(t) for t in out]), "view_merge")
    return out


def affine(img, angle, translate, scale, shear, interpolation=None, fill=None):
    """`torchvision.transforms.functional.affine` for CUDA tensors as the reference's loop calls it (train_human.py:366-368,
    388-390, 412, 421-423): img [C,H,W] or [N,C,H,W], nearest (the default) or bilinear interpolation (`interpolation_mode` lists the
    accepted spellings; bicubic is refused), zero fill, centre of rotation = image centre;
    differentiable (the student's heat-maps are warped under autograd, :421-423).  One launch of the batched kernel with a
    single stage; the loop's three-call chains can use `warp_chain` / `recon_heatmaps` instead (one launch for the batch)."""
    mode = interpolation_mode(interpolation)
    if fill not in (None, 0, 0.0):
        raise NotImplementedError("only zero fill")
    if not isinstance(shear, (list, tuple)):
        shear = [float(shear), 0.0]
    squeeze = img.dim() == 3
    x = img.unsqueeze(0) if squeeze else img
    m = inverse_affine_matrix(float(angle), [float(translate[0]), float(translate[1])], float(scale), [float(shear[0]), float(shear[1])])
    theta = torch.tensor(m, dtype=torch.float32).reshape(1, 1, 6).expand(x.shape[0], 1, 6).contiguous().to(x.device, non_blocking=True)
    out = warp_chain(x, theta, mode)
    return out.squeeze(0) if squeeze else out


def recon_heatmaps(y, aug_param, ratio, mode="nearest", flip_pairs=None):
    """The loop's heat-map re-warp (train_human.py:361-372 / 418-423) for the whole batch.  aug_param may carry the flip flags of mirrored
    views as a 5th entry (`aug_mirror`): a flagged sample is un-mirrored after the chain, its left / right channels swapped by flip_pairs
    (a sequence of pairs or a key of lib.keypoint_detection.FLIP_PAIRS; () is a valid table) - required then, ValueError before any launch."""
    n = y.shape[0]
    flags = aug_mirror(aug_param, n)
    if flags is None or not bool(flags.any()):
        return warp_chain(y, recon_thetas(aug_param, n, ratio, y.device), mode)
    if flip_pairs is None:
        raise ValueError("recon_heatmaps: the batch has mirrored samples: pass flip_pairs (a sequence of left / right joint pairs, possibly "
                         "empty, or a key of FLIP_PAIRS)")
    perm = mirror_perm(flip_pairs, y.shape[1], y.device)
    return warp_chain(y, recon_thetas(aug_param, n, ratio, y.device), mode, flags.to(y.device), perm)


def _mirror_in(mirror):
    """Flip flags (the MIRROR_OUT byte of the warp to the base frame) -> the MIRROR_IN byte of the warp back to the view."""
    return None if mirror is None else mirror * MIRROR_IN


def occlude_keypoints(x_t_stu, y_t_tea_recon, aug_param_stu, ratio, image_size, occlude_rate, occlude_thresh, occlude_size, rng, mirror=None):
    """Adaptive key-point occlusion of the student's target images (train_human.py:374-412), batched on the device.

    Host side (exactly the reference's draws, in its order, from `rng` = np.random): per sample with at least one confidence
    >= thresh: rand() <= rate ?, choice(candidates), randint (rows), randint (cols).  The confidences / arg-max positions
    come back to the host once (the reference moves them with .cpu() as well).  Device side: the selected images are
    re-warped to the canonical frame (three nearest warps, with the reference's translate/ratio quirk), a random patch
    of the same image is pasted over the chosen key-point, and one inverse warp takes them back.
    Naming follows the reference's index math, not its variable names: `left/right` slice ROWS, `upper/bottom` slice COLUMNS.
    mirror: None, or the [N] uint8 CUDA flip flags of the student's view: a flagged image is un-mirrored after the warp to the canonical
    frame (MIRROR_OUT) and mirrored again ahead of the warp back (MIRROR_IN); images have no joint permutation.
    """
    import numpy as np
    from . import utils as U
    B, K, h, w = y_t_tea_recon.shape
    preds, conf = U.get_max_preds_torch_raw(y_t_tea_recon)          # un-masked positions, like view().argmax(-1)
    conf_np = conf.reshape(B, K).cpu().numpy()
    pos_np = preds.cpu().numpy().astype(np.int64)                   # [B,K,2] = (x, y)
    table = conf_np >= occlude_thresh
    angle, (tx, ty), (sx, sy), scale = aug_param_stu[:4]
    a_, tx_, ty_, sx_, sy_, sc_ = (_as_list(v, B) for v in (angle, tx, ty, sx, sy, scale))
    sel, boxes = [], []
    for b in range(B):
        if table[b].sum() > 0 and rng.rand() <= occlude_rate:
            cand = np.arange(0, K)[table[b]]
            c = rng.choice(cand)
            position = (pos_np[b, c] * ratio).astype(int)
            left, right = max(position[1] - occlude_size, 0), min(position[1] + occlude_size, image_size)
            upper, bottom = max(position[0] - occlude_size, 0), min(position[0] + occlude_size, image_size)
            left_src = rng.randint(image_size - (right - left) + 1)
            upper_src = rng.randint(image_size - (bottom - upper) + 1)
            sel.append(b)
            boxes.append([left, right, upper, bottom, left_src, upper_src])
    if not sel:
        return x_t_stu, sel
    dev = x_t_stu.device
    idx = torch.tensor(sel, device=dev)
    sub = [[v[i] for i in sel] for v in (a_, tx_, ty_, sx_, sy_, sc_)]
    n = len(sel)
    fwd = recon_thetas([sub[0], [sub[1], sub[2]], [sub[3], sub[4]], sub[5]], n, ratio, dev)
    back = single_thetas([-v for v in sub[0]], ([-v / ratio for v in sub[1]], [-v / ratio for v in sub[2]]), [1.0 / v for v in sub[5]],
                         ([-v for v in sub[3]], [-v for v in sub[4]]), n, dev)
    msel = None if mirror is None else mirror.index_select(0, idx).contiguous()
    temp = warp_chain(x_t_stu.index_select(0, idx).float().contiguous(), fwd, mirror=msel).contiguous()
    bx = torch.tensor(boxes, dtype=torch.int32, device=dev)
    maxel = int(max((b[1] - b[0]) * (b[3] - b[2]) for b in boxes)) * temp.shape[1]
    check(lib().udapose_patch_paste(_hip.stream(), ptr(temp), ptr(bx), n, temp.shape[1], temp.shape[2], temp.shape[3], maxel), "patch_paste")
    out = x_t_stu.clone()
    out.index_copy_(0, idx, warp_chain(temp, back, mirror=_mirror_in(msel)).to(x_t_stu.dtype))
    return out, sel


def occlusion_back_thetas(aug_param_stu, n, ratio, device=None):
    """[N,1,6]: the warp back of the occlusion path (train_human.py:412): -angle, (-tx/ratio, -ty/ratio), 1/scale, (-shear)."""
    if device is not None and torch.device(device).type == "cuda":
        return thetas_from_packed(pack_aug_param(aug_param_stu, n).to(device), ratio, want_fwd=False, want_back=True)[1]
    angle, (tx, ty), (sx, sy), scale = aug_param_stu[:4]
    a_, tx_, ty_, sx_, sy_, sc_ = (_as_list(v, n) for v in (angle, tx, ty, sx, sy, scale))
    return single_thetas([-v for v in a_], ([-v / ratio for v in tx_], [-v / ratio for v in ty_]), [1.0 / v for v in sc_],
                         ([-v for v in sx_], [-v for v in sy_]), n, device)


def occlude_keypoints_device(x_t_stu, y_t_tea_recon, theta_fwd, theta_back, u, ratio, image_size, occlude_rate, occlude_thresh, occlude_size,
                             mirror=None):
    """The same occlusion with its DECISIONS taken on the device (udapose_occlusion_pick): no read-back, fixed shapes - the step
    stays capturable.  theta_fwd = recon_thetas(aug_param_stu), theta_back = occlusion_back_thetas(aug_param_stu), u = [N,4]
    uniform [0,1) draws (rate test, key-point choice, patch row / column origin).  Every image goes through the warps; only the
    selected samples keep the result (the others are returned bit-identical).  mirror: as for occlude_keypoints.
    Returns (images, apply [N] uint8)."""
    _hip.require_cuda(x_t_stu, y_t_tea_recon, theta_fwd, theta_back, u)
    B, K, h, w = y_t_tea_recon.shape
    hm = ha.f32c(y_t_tea_recon)
    peak = ha.heatmap_argmax(hm, maxv=True, idx=True)
    boxes = torch.empty(B, 6, dtype=torch.int32, device=hm.device)
    apply = torch.empty(B, dtype=torch.uint8, device=hm.device)
    uu = u.detach().float().contiguous()
    assert tuple(uu.shape) == (B, 4)
    check(lib().udapose_occlusion_pick(_hip.stream(), ptr(peak.maxv), ptr(peak.idx), ptr(uu), B, K, w, float(ratio), int(image_size), float(occlude_rate),
                                       float(occlude_thresh), int(occlude_size), ptr(boxes), ptr(apply)), "occlusion_pick")
    x = x_t_stu.detach().float().contiguous()
    temp = warp_chain(x, theta_fwd, mirror=mirror).contiguous()
    C_ = temp.shape[1]
    check(lib().udapose_patch_paste(_hip.stream(), ptr(temp), ptr(boxes), B, C_, temp.shape[2], temp.shape[3], 4 * occlude_size * occlude_size * C_),
          "patch_paste")
    back = warp_chain(temp, theta_back, mirror=_mirror_in(mirror)).contiguous()
    out = torch.empty_like(x)
    check(lib().udapose_select_rows(_hip.stream(), ptr(out), ptr(back), ptr(x), ptr(apply), B, x[0].numel()), "select_rows")
    return out.to(x_t_stu.dtype), apply
