"""GPU data pipeline of the mean-teacher target views.

The reference feeds its loop from DataLoader workers (`--workers 1` by default, train_human.py:591) that run, per sample and
per view, PIL / torchvision transforms on the host (train_human.py:63-78, lib/datasets/human36m_mt.py:76-161):

    base crop (RandomResizedCrop = F.crop + PIL bilinear F.resize)            -> image [H,W,3] uint8, keypoint2d [K,2]
    student view:  RandomAffineRotation -> ColorJitter -> GaussianBlur(high=0) -> ToTensor -> Normalize, generate_target
    teacher views: the same with the teacher's ranges, k times

At ~1900 img/s that loader cannot keep up.  Here everything after the image decode runs on the device for the whole batch:
the base crop + resize (round 3: PIL's two-pass 8-bit resampler), the affine warp, the colour jitter, the tensor conversion and normalisation, and the Gaussian label maps are HIP kernels
(csrc/augment.hip) that reproduce PIL's integer arithmetic bit for bit; the random parameters (a few floats per sample) and
the key-point algebra (K x 2 per sample) are drawn / computed on the host exactly as lib/transforms/keypoint_detection.py
does, including the `aug_param` tuple that the loop consumes (inverse augmentation, :139).  The result has the collated
8-tuple layout of Appendix D / `default_collate`, ready for MeanTeacherTrainer.train_step or GraphedTrainStep.prefetch.

GaussianBlur (`--blur_stu / --blur_tea`, radius U(0, high) per sample; 0 by default = a copy) is PIL's three-pass box blur in
8.24 fixed point, reproduced bit for bit on the device (udapose_aug_gaussian_blur_u8).

The strong student view of weak-teacher / strong-student consistency training (FixMatch / RandAugment; the reference's student view stops at
ColorJitter + blur): `ViewConfig(strong_ops=k, strong_magnitude=m)` appends k ops drawn from STRONG_OPS - the three ImageEnhance steps above,
ImageOps.autocontrast / equalize / posterize / solarize and ImageEnhance.Sharpness, byte for byte PIL's results (csrc/strong_aug.hip) -
between the colour jitter and the blur, and `ViewConfig(erase=p)` the reference's RandomErasing (lib/transforms/__init__.py:134-179) on the
normalised tensor.  Both are off by default: nothing more is drawn or launched then.

Mirrored views: `ViewConfig(flip=p)` mirrors a sample's base crop with probability p ahead of the view's affine warp - the
view is A(M(base)) - with the key points following the reference's `hflip` (lib/transforms/keypoint_detection.py:108-116, x -> W - 1 - x)
and re-indexed by the left / right joint pairs; the flags travel as a 5th entry of the view's `aug_param`, which the re-warps undo
(warp.recon_heatmaps, the trainers).  Off by default: no draw, no launch, the reference's 4-entry aug_param.

Box crops: `box_crop` cuts boxes (cx, cy, bw, bh, rot_deg) that may leave the frame, be turned or non-square out of uint8
frames and resizes them in one launch (csrc/box_crop.hip) - the device counterpart of the datasets' crop + Resize and crop_ori, the image
side of `engine.predict`; `TargetViewPipeline.box_crop` hands such crops to `view()`.
"""
import math
import random

import numpy as np
import torch

from . import _hip
from ._hip import check, lib, ptr

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# op codes of the strong view, one per image and step: 0 none; 1 brightness, 2 contrast, 3 colour (udapose_aug_color_op's codes);
# 4 autocontrast, 5 equalize, 6 posterize, 7 solarize (udapose_aug_point_op); 8 sharpness (udapose_aug_sharpness_u8)
STRONG_OPS = (0, 1, 2, 3, 4, 5, 6, 7, 8)
STRONG_BINS = 31          # RandAugment's magnitude scale: integers 0 .. 30
# ImageOps.autocontrast's `scale = 255.0 / (hi - lo)` for hi - lo = 1 .. 255, divided by Python as PIL divides it: the device looks it up
AUTOCONTRAST_SCALES = tuple(255.0 / d for d in range(1, 256))


def inverse_affine_matrix_pil(center, angle, translate, scale, shear):
    """torchvision `_get_inverse_affine_matrix` as `F.affine` calls it for a PIL image: centre = (w/2, h/2), angle / shear in
    degrees, translation in pixels -> the 6 coefficients handed to Image.transform(AFFINE)."""
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d / scale, -b / scale, 0.0, -c / scale, a / scale, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def pil_fixed_coefficients(m):
    """PIL's 16.16 fixed-point form of an affine matrix (libImaging affine_fixed): FIX(v) = floor(v * 65536 + 0.5), with the
    half-pixel offset of the first sample folded into the two constants."""
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def pil_box_blur_params(radius, passes=3):
    """PIL's ImageFilter.GaussianBlur(radius) -> (r, ww, fw) of its box-blur passes (libImaging BoxBlur.c `_gaussian_blur_radius`
    and `ImagingLineBoxBlur*`, float32 / uint32 arithmetic as in the C source); radius 0 -> None (PIL returns a copy)."""
    if radius == 0:
        return None
    f = np.float32
    sigma2 = f(f(radius) * f(radius) / f(passes))
    L = f(np.sqrt(12.0 * float(sigma2) + 1.0))
    l = f(np.floor((float(L) - 1.0) / 2.0))
    a = f(f(f(2) * l + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * sigma2)))
    a = f(a / f(f(6) * f(sigma2 - f(f(l + f(1)) * f(l + f(1))))))
    fr = f(l + a)
    r = int(fr)
    ww = int(f(f(1 << 24) / f(fr * f(2) + f(1))))
    fw = ((1 << 24) - (r * 2 + 1) * ww) // 2
    return r, ww & 0xFFFFFFFF, fw & 0xFFFFFFFF


def pil_resample_coeffs(in_size, out_size):
    """PIL's BILINEAR resampling coefficients for one axis of Image.resize (libImaging Resample.c `precompute_coeffs` +
    `normalize_coeffs_8bpc`; box = the whole input): -> (bounds [out,2] int32 = (first source index, tap count), coef [out,ksize] int32
    with 22 fractional bits, ksize).  Python floats are C doubles, the statements follow the C source one by one."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale                   # bilinear_filter.support = 1.0
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k, ww = [], 0.0
        for x in range(xmax):
            t = (x + xmin - center + 0.5) * ss
            if t < 0.0:
                t = -t
            w = 1.0 - t if t < 1.0 else 0.0
            k.append(w)
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
            v = k[x] * (1 << 22)
            coef[xx, x] = int(-0.5 + v) if k[x] < 0 else int(0.5 + v)
        bounds[xx] = (xmin, xmax)
    return bounds, coef, ksize


def draw_resized_crop(rng, width, height, scale=(0.6, 1.3)):
    """RandomResizedCrop.get_params (lib/transforms/keypoint_detection.py:478-505): up to ten draws of a square crop of U(scale) x the
    image area (aspect ratio 1), then its corner; the whole image if none fits.  Same draws in the same order from `rng` (the reference
    uses the global `random` module).  -> (top, left, h, w)"""
    area = height * width
    for _ in range(10):
        target_area = rng.uniform(*scale) * area
        w = int(round(math.sqrt(target_area * 1)))
        h = int(round(math.sqrt(target_area / 1)))
        if 0 < w <= width and 0 < h <= height:
            i = rng.randint(0, height - h)
            j = rng.randint(0, width - w)
            return i, j, h, w
    return 0, 0, height, width


def transform_keypoints(kp, angle, shear_x, shear_y, trans_x, trans_y, scale, width, height):
    """The key-point side of `affine` (lib/transforms/keypoint_detection.py:141-165): rotate / shear / scale about the image
    centre, then translate."""
    ang, sx, sy = np.deg2rad(angle), np.deg2rad(shear_x), np.deg2rad(shear_y)
    a = np.cos(ang - sy) / np.cos(sy)
    b = (-np.cos(ang - sy) * np.tan(sx) / np.cos(sy) - np.sin(ang))
    c = np.sin(ang - sy) / np.cos(sy)
    d = (-np.sin(ang - sy) * np.tan(sx) / np.cos(sy) + np.cos(ang))
    rot = np.array([[scale * a, scale * b], [scale * c, scale * d]])
    kp = np.copy(kp).astype(np.float64)
    kp[:, 0] -= width / 2
    kp[:, 1] -= height / 2
    kp = np.matmul(rot, kp.T).T
    kp[:, 0] += width / 2 + trans_x
    kp[:, 1] += height / 2 + trans_y
    return kp


def mirror_keypoints(keypoints, visible, width, flip_pairs):
    """The key-point side of a horizontal flip for ONE sample: keypoints [K,2+] -> x becomes width - 1 - x (the reference's `hflip`), then rows
    are re-indexed by the flip permutation (lib.keypoint_detection.flip_perm, an involution), so that row j holds the joint that looks like
    j in the mirrored picture; visible [K,...] (or None) is re-indexed the same way.  -> (key points, visible), copies."""
    from .lib import keypoint_detection as kd
    kp = np.array(keypoints, dtype=np.float64, copy=True)
    perm = kd.flip_perm(flip_pairs, kp.shape[0]).numpy()
    kp[:, 0] = (width - 1) - kp[:, 0]
    vis = None if visible is None else np.array(visible, copy=True)[perm]
    return kp[perm], vis


def strong_op_arrays(ops, params, N):
    """The host side of `TargetViewPipeline.strong_`: per-sample op / parameter lists, checked, -> four [L][N] arrays, one row per list
    position: the codes, the codes as udapose_aug_color_op reads them (everything but 1..3 is "none" there), the float parameters (factors
    of 1 / 2 / 3 / 8) and the integer ones (posterize's bits, solarize's cut = ceil(threshold) clipped to [0, 256]: for an integer i,
    PIL's `i < threshold` is `i < ceil(threshold)`).  ValueError: list lengths that do not match N or each other, a code outside
    STRONG_OPS, bits outside 1..8, a factor or threshold that is not finite."""
    if len(ops) != N or len(params) != N:
        raise ValueError(f"strong_: {len(ops)} op lists and {len(params)} parameter lists for a batch of {N}")
    L = len(ops[0]) if N else 0
    color = np.zeros((L, N), np.int32)
    code = np.zeros((L, N), np.int32)
    fpar = np.zeros((L, N), np.float32)
    ipar = np.zeros((L, N), np.int32)
    for n in range(N):
        if len(ops[n]) != L or len(params[n]) != L:
            raise ValueError(f"strong_: sample {n} has {len(ops[n])} ops and {len(params[n])} parameters, sample 0 has {L} ops")
        for j, (o, p) in enumerate(zip(ops[n], params[n])):
            if o not in STRONG_OPS:
                raise ValueError(f"strong_: op code {o!r} is not one of {STRONG_OPS}")
            code[j, n] = o
            if o in (1, 2, 3, 8):
                if not math.isfinite(p):
                    raise ValueError(f"strong_: factor {p!r} of op {o} is not finite")
                fpar[j, n] = p
                if o != 8:
                    color[j, n] = o
            elif o == 6:
                if not (math.isfinite(p) and p == int(p) and 1 <= p <= 8):
                    raise ValueError(f"strong_: posterize keeps 1..8 bits, got {p!r}")
                ipar[j, n] = int(p)
            elif o == 7:
                if not math.isfinite(p):
                    raise ValueError(f"strong_: solarize threshold {p!r} is not finite")
                ipar[j, n] = min(256, max(0, math.ceil(p)))
    return code, color, fpar, ipar


_NORM_CACHE = {}      # (device, mean, std) -> their fp32 device copies: a loop (and a captured launch) uploads them once


def _norm_consts(device, mean, std):
    """mean / std of a normalisation as fp32 [3] tensors on `device`: device tensors pass through, tuples are uploaded once."""
    if torch.is_tensor(mean) and torch.is_tensor(std):
        return mean.to(device=device, dtype=torch.float32).contiguous(), std.to(device=device, dtype=torch.float32).contiguous()
    key = (device, tuple(float(v) for v in mean), tuple(float(v) for v in std))
    c = _NORM_CACHE.get(key)
    if c is None:
        if len(key[1]) != 3 or len(key[2]) != 3:
            raise ValueError("mean and std have one value per channel")
        c = _NORM_CACHE[key] = (torch.tensor(key[1], dtype=torch.float32, device=device), torch.tensor(key[2], dtype=torch.float32, device=device))
    return c


def box_inputs(frames_u8, boxes, frame_idx):
    """The arguments of a box crop, checked, as device tensors: (boxes [M,5] fp32, frame_idx [M] int32, host_checked).  Host boxes (numpy,
    list) go through lib.keypoint_detection.check_boxes - a bad box raises ValueError naming its row, before any launch - and a host
    frame_idx is checked against the frame count; CUDA tensors are taken as they are (the launch reports them in `status`).  frame_idx
    None: box m crops frame m (M == F)."""
    from .lib import keypoint_detection as kd
    _hip.require_cuda(frames_u8)
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.dtype != torch.uint8 or not frames_u8.is_contiguous():
        raise ValueError(f"frames must be a contiguous uint8 tensor [F,Hs,Ws,3], got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    F, dev = frames_u8.shape[0], frames_u8.device
    host = not torch.is_tensor(boxes)
    if host:
        bd = torch.from_numpy(kd.check_boxes(boxes).astype(np.float32)).to(dev, non_blocking=True)
    else:
        _hip.require_cuda(boxes)
        if boxes.dim() != 2 or boxes.shape[1] != 5 or boxes.shape[0] < 1 or boxes.device != dev:
            raise ValueError(f"boxes must be [M,5] on {dev}, got {tuple(boxes.shape)} on {boxes.device}")
        bd = boxes.detach().to(torch.float32).contiguous()
    M = bd.shape[0]
    if frame_idx is None:
        if M != F:
            raise ValueError(f"{M} boxes for {F} frames: give frame_idx [M]")
        fd = torch.arange(M, dtype=torch.int32, device=dev)
    elif torch.is_tensor(frame_idx) and frame_idx.is_cuda:
        if tuple(frame_idx.shape) != (M,) or frame_idx.device != dev or frame_idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"frame_idx must be an integer tensor [{M}] on {dev}")
        fd = frame_idx.to(torch.int32).contiguous()
    else:
        fi = np.asarray(frame_idx)
        if fi.shape != (M,) or not np.issubdtype(fi.dtype, np.integer):
            raise ValueError(f"frame_idx must be {M} integers, got {fi.dtype} {fi.shape}")
        bad = np.nonzero((fi < 0) | (fi >= F))[0]
        if bad.size:
            raise ValueError(f"box {int(bad[0])} names frame {int(fi[bad[0]])} of {F}")
        fd = torch.from_numpy(fi.astype(np.int32)).to(dev, non_blocking=True)
    return bd, fd, host


def box_crop_launch(frames_u8, boxes_d, fidx_d, Ho, Wo, mean_d, std_d, mirror, want_f32, want_u8):
    """udapose_box_crop on checked device arguments -> (out_f32 or None, out_u8 or None, status [M] uint8)."""
    F, Hs, Ws, _ = frames_u8.shape
    M, dev = boxes_d.shape[0], frames_u8.device
    n = 2 * M if mirror else M
    of = torch.empty(n, 3, Ho, Wo, dtype=torch.float32, device=dev) if want_f32 else None
    ou = torch.empty(n, Ho, Wo, 3, dtype=torch.uint8, device=dev) if want_u8 else None
    status = torch.empty(M, dtype=torch.uint8, device=dev)
    check(lib().udapose_box_crop(_hip.stream(), ptr(frames_u8), F, Hs, Ws, ptr(fidx_d), ptr(boxes_d), M, Ho, Wo, ptr(mean_d), ptr(std_d),
                                 int(bool(mirror)), ptr(of), ptr(ou), ptr(status)), "box_crop")
    return of, ou, status


def box_crop(frames_u8, boxes, size, frame_idx=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, mirror=False, out="f32"):
    """Top-down inference's image side (udapose_box_crop, one launch): boxes [M,5] = (cx, cy, bw, bh, rot_deg) in pixels of
    frames_u8 [F,Hs,Ws,3] uint8 CUDA (pixel i covers [i, i + 1)), each resized to `size` = S or (Ho, Wo).  The padded / rotated /
    non-square counterpart of the reference's crop + Resize and crop_ori: a box may leave the frame (zero padding in pixel values, ahead
    of the normalisation), be turned by rot degrees (get_transform's sign) and have bw != bh.  Every output pixel is the mean of
    tx * ty bilinear samples, tx = clamp(ceil(bw / Wo), 1, 8) - an area filter up to 8x reduction; beyond 8x the box is under-sampled (the
    tap cap).  This is NOT PIL's resampling filter: `TargetViewPipeline.resized_crop` keeps PIL's bits for square boxes inside the frame.
    frame_idx [M]: the frame of every box (several boxes may name one frame); None: box m crops frame m.
    out="f32": [M,3,Ho,Wo] fp32, (value / 255 - mean) / std as `to_tensor`; out="u8": [M,Ho,Wo,3] uint8, min(255, floor(value + 0.5)).
    mirror=True: 2M images, the crops followed by their column-reversed copies (ops.hflip_batch(keep_original=True)'s layout) out of the
    same launch.  boxes as a numpy array or a list are checked on the host (ValueError naming the row; frame_idx likewise) and the crops
    are returned; boxes as a CUDA tensor are not read here: (crops, status [M] uint8) comes back, status 1 = refused (a non-finite field,
    bw or bh <= 0, a frame index outside the frames), its crop all zero pixel values."""
    Ho, Wo = _crop_size(size)
    if out not in ("f32", "u8"):
        raise ValueError(f"out must be 'f32' or 'u8', got {out!r}")
    bd, fd, host = box_inputs(frames_u8, boxes, frame_idx)
    _check_frame_size(frames_u8)
    md, sd = _norm_consts(frames_u8.device, mean, std)
    of, ou, status = box_crop_launch(frames_u8, bd, fd, Ho, Wo, md, sd, mirror, out == "f32", out == "u8")
    crops = of if out == "f32" else ou
    return crops if host else (crops, status)


def _crop_size(size):
    from .lib import keypoint_detection as kd
    Ho, Wo = kd._hw(size)
    if Ho > 1024 or Wo > 1024:
        raise ValueError(f"a box crop is at most 1024 x 1024, got {Ho} x {Wo}")
    return Ho, Wo


def _check_frame_size(frames_u8):
    if frames_u8.shape[0] < 1 or not (1 <= frames_u8.shape[1] <= 8192 and 1 <= frames_u8.shape[2] <= 8192):
        raise ValueError(f"frames of 1 .. 8192 pixels a side, at least one, got {tuple(frames_u8.shape)}")


class ViewConfig:
    """Ranges of one view's augmentation = the reference's `--rotation_* --shear_* --translate_* --scale_* --color_*` flags
    (train_human.py:535-557)."""

    def __init__(self, rotation=180, shear=(-30, 30), translate=(0.05, 0.05), scale=(0.6, 1.3), color=0.25, blur=0.0, flip=0.0, strong_ops=0,
                 strong_magnitude=9, erase=0.0, erase_value=(0.4914, 0.4822, 0.4465)):
        self.degrees = (-rotation, rotation) if isinstance(rotation, (int, float)) else tuple(rotation)
        self.shear = (-shear, shear) if isinstance(shear, (int, float)) else tuple(shear)
        self.translate = (translate, translate) if isinstance(translate, (int, float)) else tuple(translate)
        self.scale = (scale, scale) if isinstance(scale, (int, float)) else tuple(scale)
        self.color = float(color)
        self.blur = float(blur)          # T.GaussianBlur(high=blur): radius ~ U(0, blur) per sample (`--blur_stu / --blur_tea`)
        # the strong view (no flag of the reference): strong_ops ops per sample from STRONG_OPS at RandAugment magnitude strong_magnitude of
        # STRONG_BINS bins; erase = RandomErasing's probability, erase_value its fill (the class's default `mean`, written as is)
        self.strong_ops, self.strong_magnitude = int(strong_ops), int(strong_magnitude)
        self.erase, self.erase_value = float(erase), tuple(float(v) for v in erase_value)
        if self.strong_ops < 0 or not 0 <= self.strong_magnitude < STRONG_BINS:
            raise ValueError(f"strong_ops must be >= 0 and strong_magnitude in 0..{STRONG_BINS - 1}")
        if not 0.0 <= self.erase <= 1.0 or len(self.erase_value) != 3:
            raise ValueError("erase is a probability and erase_value has one value per channel")
        self.flip = float(flip)          # the probability, per sample, of a mirrored view (horizontal flip with left / right joint swap)
        if not 0.0 <= self.flip <= 1.0:
            raise ValueError("flip is a probability")

    def draw_blur(self, rng):
        """GaussianBlur.__call__ (keypoint_detection.py:221-223): one uniform radius per sample (the reference draws from np.random)."""
        return rng.uniform(0.0, self.blur)

    def draw_affine(self, rng, img_size):
        """RandomAffineRotation.get_params (lib/transforms/keypoint_detection.py:396-412), same draws in the same order from
        `rng` (the reference uses the global `random` module)."""
        angle = rng.uniform(self.degrees[0], self.degrees[1])
        shear_x, shear_y = rng.uniform(self.shear[0], self.shear[1]), 0.0
        if len(self.shear) == 4:
            shear_y = rng.uniform(self.shear[2], self.shear[3])
        max_dx, max_dy = float(self.translate[0] * img_size[0]), float(self.translate[1] * img_size[1])
        trans_x = int(round(rng.uniform(-max_dx, max_dx)))
        trans_y = int(round(rng.uniform(-max_dy, max_dy)))
        scale = rng.uniform(self.scale[0], self.scale[1])
        return angle, shear_x, shear_y, trans_x, trans_y, scale

    def draw_jitter(self, rng):
        """ColorJitter(brightness=c, contrast=c, saturation=c): a random order of the three steps and one factor U(1-c, 1+c)
        each.  (torchvision draws these from torch's RNG in a version-dependent way; any order / factors are valid samples of
        the same distribution.)  -> ([op codes], [factors]) with op 1 brightness, 2 contrast, 3 saturation."""
        ops = [1, 2, 3]
        rng.shuffle(ops)
        c = self.color
        return ops, [rng.uniform(max(0.0, 1 - c), 1 + c) for _ in ops]

    def draw_strong(self, rng):
        """RandAugment: strong_ops ops, each uniform over STRONG_OPS, all at magnitude m = strong_magnitude of the published table
        (Cubuk et al. 2020, 31 bins).  Draw order, per op: one `rng.randrange(9)` for the code; then, for codes 1 / 2 / 3 / 8 only, one
        `rng.random()` whose value below 0.5 turns the factor 1 + 0.9 m / 30 into 1 - 0.9 m / 30.  Posterize keeps
        bits = 8 - round(m / 7.5), solarize the threshold 255 - 255 m / 30; codes 0, 4, 5 have no parameter (0.0 stands in) and, like 6 and 7,
        draw nothing further.  -> ([codes], [parameters])"""
        m = self.strong_magnitude
        codes, params = [], []
        for _ in range(self.strong_ops):
            code = STRONG_OPS[rng.randrange(len(STRONG_OPS))]
            if code in (1, 2, 3, 8):
                d = 0.9 * m / (STRONG_BINS - 1)
                p = 1.0 - d if rng.random() < 0.5 else 1.0 + d
            elif code == 6:
                p = 8 - int(round(m / 7.5))
            elif code == 7:
                p = 255.0 - 255.0 * m / (STRONG_BINS - 1)
            else:
                p = 0.0
            codes.append(code)
            params.append(p)
        return codes, params

    def draw_erase(self, rng, H, W, sl=0.02, sh=0.4, r1=0.3):
        """RandomErasing.__call__ (lib/transforms/__init__.py:156-177), same draws in the same order from `rng` (the reference uses the global
        `random` module): one uniform against the probability `erase`; then up to 100 attempts of an area U(sl, sh) x H W and an aspect
        ratio U(r1, 1 / r1), the first box that is smaller than the image on both sides is placed by two `randint`s (row, then column: the
        reference's x1 is the row).  -> (top, left, h, w); (0, 0, 0, 0) when nothing is erased."""
        if rng.uniform(0, 1) >= self.erase:
            return 0, 0, 0, 0
        for _ in range(100):
            area = H * W
            target_area = rng.uniform(sl, sh) * area
            aspect_ratio = rng.uniform(r1, 1 / r1)
            h = int(round(math.sqrt(target_area * aspect_ratio)))
            w = int(round(math.sqrt(target_area / aspect_ratio)))
            if w < W and h < H:
                top = rng.randint(0, H - h)
                left = rng.randint(0, W - w)
                return top, left, h, w
        return 0, 0, 0, 0


    def draw_flip(self, rng):
        """One `rng.random() < flip` per sample -> 0 / 1; drawn after every other draw of the view, and not at all when flip == 0."""
        return int(rng.random() < self.flip)


class TargetViewPipeline:
    """Batched device pipeline for the `_mt` datasets' student / teacher views."""

    # mirrored views: the left / right joint pairs (a sequence of pairs, possibly empty, or a key of lib.keypoint_detection.FLIP_PAIRS), set
    # as an attribute after construction like MeanTeacherTrainer.flip_pairs; a view with flip > 0 needs it (ValueError before anything is drawn)
    flip_pairs = None

    def __init__(self, image_size=256, heatmap_size=64, sigma=2, k=1, student=None, teacher=None, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 rng=None, resize_scale=(0.6, 1.3), np_rng=None, subpixel_labels=False):
        self.image_size, self.heatmap_size, self.sigma, self.k = int(image_size), int(heatmap_size), sigma, int(k)
        # labels(): False = generate_target's Gaussian on the rounded position (the reference); True = on the position itself, the encoding
        # that lib.keypoint_detection.dark_decode inverts (no counterpart in the reference)
        self.subpixel_labels = bool(subpixel_labels)
        self.stu, self.tea = student or ViewConfig(), teacher or ViewConfig()
        self.mean, self.std = tuple(mean), tuple(std)
        self.rng = rng if rng is not None else random
        # the reference draws the blur radius from the GLOBAL np.random (lib/transforms/keypoint_detection.py:221), everything else of a view
        # from python's `random`: two generators, so a seeded pipeline consumes each stream as the reference does
        self.np_rng = np_rng if np_rng is not None else np.random
        self.resize_scale = tuple(resize_scale)          # `--resize-scale` (train_human.py:523)
        self._dev = {}
        self._coef_cache = {}
        self._inv_scale = {}          # per device: autocontrast's 255.0 / d, d = 1 .. 255, divided here (strong_)

    # ------------------------------------------------------------------ device constants
    def _consts(self, device):
        c = self._dev.get(device)
        if c is None:
            tmp = self.sigma * 3
            size = 2 * tmp + 1
            if float(size) != int(size):
                raise NotImplementedError("label patch needs an integer 3*sigma")
            x = np.arange(0, size, 1, np.float32)
            y = x[:, np.newaxis]
            x0 = y0 = size // 2
            g = np.exp(-((x - x0) ** 2 + (y - y0) ** 2) / (2 * self.sigma ** 2)).astype(np.float32)      # util.py:48-53
            c = dict(mean=torch.tensor(self.mean, dtype=torch.float32, device=device), std=torch.tensor(self.std, dtype=torch.float32, device=device),
                     patch=torch.from_numpy(np.ascontiguousarray(g)).to(device), rad=int(tmp))
            self._dev[device] = c
        return c

    # ------------------------------------------------------------------ building blocks (each = one kernel family)
    def warp_images(self, base_u8, params):
        """F.affine on the whole batch: base_u8 [N,H,W,3] uint8 CUDA, params = list of (angle, shear_x, shear_y, tx, ty, scale)."""
        _hip.require_cuda(base_u8)
        N, H, W, C3 = base_u8.shape
        assert C3 == 3 and base_u8.dtype == torch.uint8 and base_u8.is_contiguous()
        coef = [pil_fixed_coefficients(inverse_affine_matrix_pil((W * 0.5, H * 0.5), a, (tx, ty), sc, (shx, shy)))
                for (a, shx, shy, tx, ty, sc) in params]
        cdev = torch.tensor(coef, dtype=torch.int64).to(base_u8.device, non_blocking=True)
        out = torch.empty_like(base_u8)
        check(lib().udapose_aug_affine_u8(_hip.stream(), ptr(base_u8), ptr(out), ptr(cdev), N, H, W), "aug_affine_u8")
        return out

    def hflip(self, base_u8, flips):
        """The mirrored base crops of the flagged samples (udapose_aug_hflip_u8, out of place): base_u8 [N,H,W,3] uint8 CUDA, flips = N
        values 0 / 1.  No flag set: base_u8 itself, no launch."""
        _hip.require_cuda(base_u8)
        N, H, W, C3 = base_u8.shape
        assert C3 == 3 and base_u8.dtype == torch.uint8 and base_u8.is_contiguous()
        flips = [int(f) for f in flips]
        if len(flips) != N or any(f not in (0, 1) for f in flips):
            raise ValueError(f"flips: {N} values 0 / 1 expected, got {flips}")
        if not any(flips):
            return base_u8
        fdev = torch.tensor(flips, dtype=torch.uint8).to(base_u8.device, non_blocking=True)
        out = torch.empty_like(base_u8)
        check(lib().udapose_aug_hflip_u8(_hip.stream(), ptr(base_u8), ptr(out), ptr(fdev), N, H, W), "aug_hflip_u8")
        return out

    def resized_crop(self, raw_u8, keypoints, boxes=None):
        """T.RandomResizedCrop(size=image_size, scale=resize_scale) on the whole batch (train_human.py:55,64): raw_u8 [N,Hs,Ws,3] uint8 CUDA
        (the decoded dataset images; the `_mt` datasets hold square crops, `resize` asserts it), keypoints [N,K,2] pixels;
        boxes = per-sample (top, left, h, w), drawn like the reference when None -> (base_u8 [N,S,S,3], key points [N,K,2])."""
        _hip.require_cuda(raw_u8)
        N, Hs, Ws, C3 = raw_u8.shape
        assert C3 == 3 and raw_u8.dtype == torch.uint8 and raw_u8.is_contiguous()
        S = self.image_size
        if boxes is None:
            boxes = [draw_resized_crop(self.rng, Ws, Hs, self.resize_scale) for _ in range(N)]
        tabs, ksize = [], 1
        for (top, left, h, w) in boxes:
            if not (0 <= top and 0 <= left and 0 < h and 0 < w and top + h <= Hs and left + w <= Ws):
                raise ValueError(f"crop box {(top, left, h, w)} outside a {Hs}x{Ws} image")
            if w != h:
                raise AssertionError("resize() asserts width == height (lib/transforms/keypoint_detection.py:47)")
            key = (w, S)
            if key not in self._coef_cache:
                self._coef_cache[key] = pil_resample_coeffs(w, S)
            tabs.append(self._coef_cache[key])
            ksize = max(ksize, tabs[-1][2])
        bounds = np.zeros((N, 2, S, 2), np.int32)
        coef = np.zeros((N, 2, S, ksize), np.int32)
        for n, (b, c, ks) in enumerate(tabs):
            bounds[n, 0] = bounds[n, 1] = b        # square crop to a square image: both axes share one table
            coef[n, :, :, :ks] = c
        dev = raw_u8.device
        box_d = torch.tensor(boxes, dtype=torch.int32).to(dev, non_blocking=True)
        bounds_d = torch.from_numpy(bounds).to(dev, non_blocking=True)
        coef_d = torch.from_numpy(coef).to(dev, non_blocking=True)
        tmp = torch.empty(N, Hs, S, 3, dtype=torch.uint8, device=dev)
        out = torch.empty(N, S, S, 3, dtype=torch.uint8, device=dev)
        check(lib().udapose_aug_resized_crop_u8(_hip.stream(), ptr(raw_u8), ptr(out), ptr(tmp), ptr(box_d), ptr(bounds_d), ptr(coef_d), N, Hs, Ws,
                                                S, ksize), "aug_resized_crop_u8")
        # key points: crop() shifts them, resize() scales them by size / width (keypoint_detection.py:47-49, 59-64)
        kp = np.array(keypoints, dtype=np.float64, copy=True)
        for n, (top, left, h, w) in enumerate(boxes):
            kp[n, :, 0] -= left
            kp[n, :, 1] -= top
            kp[n] *= float(S) / float(w)
        return out, kp

    def box_crop(self, frames_u8, keypoints, boxes, frame_idx=None):
        """The padded / rotated counterpart of `resized_crop`, ready for `view()`: boxes [M,5] = (cx, cy, bw, bh, rot_deg) on the host
        (lib.keypoint_detection.boxes_from_keypoints / boxes_from_center_scale make them; checked, ValueError naming a bad row) cut from
        frames_u8 [F,Hs,Ws,3] uint8 CUDA (frame_idx [M]: the frame of every box, None: box m crops frame m) and resized to image_size by
        `data_gpu.box_crop` - its own area filter, not PIL's; a box may leave the frame or be non-square.  keypoints [M,K,2] in pixels of
        the frames -> (base_u8 [M,S,S,3], key points [M,K,2] in the crop, lib.keypoint_detection.to_crop_coords)."""
        from .lib import keypoint_detection as kd
        S = self.image_size
        hb = kd.check_boxes(boxes)
        kp = kd.to_crop_coords(keypoints, hb, (S, S))
        return box_crop(frames_u8, hb, (S, S), frame_idx=frame_idx, out="u8"), kp

    def jitter_(self, img_u8, ops, factors):
        """ColorJitter in place: ops / factors = per-sample lists of three op codes / factors (applied in list order)."""
        N, H, W, _ = img_u8.shape
        dev = img_u8.device
        op_t = torch.tensor(ops, dtype=torch.int32).t().contiguous().to(dev, non_blocking=True)          # [3][N]
        f_t = torch.tensor(factors, dtype=torch.float32).t().contiguous().to(dev, non_blocking=True)
        scratch = torch.empty(N, dtype=torch.int32, device=dev)
        for i in range(op_t.shape[0]):
            check(lib().udapose_aug_color_op(_hip.stream(), ptr(img_u8), ptr(op_t[i]), ptr(f_t[i]), ptr(scratch), N, H * W), "aug_color_op")
        return img_u8

    def blur_(self, img_u8, radii):
        """T.GaussianBlur in place: radii = one Gaussian radius per sample (0: unchanged, like PIL's copy)."""
        N, H, W, _ = img_u8.shape
        prm = [pil_box_blur_params(float(r)) or (0xFFFFFFFF, 0, 0) for r in radii]
        if all(p[0] == 0xFFFFFFFF for p in prm):
            return img_u8
        pdev = torch.from_numpy(np.asarray(prm, dtype=np.uint32).view(np.int32)).to(img_u8.device, non_blocking=True)
        tmp = torch.empty_like(img_u8)
        check(lib().udapose_aug_gaussian_blur_u8(_hip.stream(), ptr(img_u8), ptr(tmp), ptr(pdev), N, H, W), "aug_gaussian_blur_u8")
        return img_u8

    def strong_(self, img_u8, ops, params):
        """The strong view's ops in place: ops / params = per-sample lists of equally many codes of STRONG_OPS / their parameters (applied
        in list order): the factor for 1 brightness, 2 contrast, 3 colour and 8 sharpness, `bits` (1..8) for 6 posterize, the threshold for
        7 solarize (PIL compares `i < threshold`; the device gets the integer cut ceil(threshold) clipped to [0, 256]); ignored for 0, 4
        autocontrast and 5 equalize.  Per list position only the launches whose codes occur in the batch are issued; nothing is read back."""
        _hip.require_cuda(img_u8)
        N, H, W, C3 = img_u8.shape
        assert C3 == 3 and img_u8.dtype == torch.uint8 and img_u8.is_contiguous()
        code, color, fpar, ipar = strong_op_arrays(ops, params, N)
        L = code.shape[0]
        if L == 0 or not code.any():
            return img_u8
        dev = img_u8.device
        up = lambda a: torch.from_numpy(a).to(dev, non_blocking=True)
        code_d, fpar_d = up(code), up(fpar)
        has = lambda j, lo, hi: bool(((code[j] >= lo) & (code[j] <= hi)).any())
        if color.any():
            color_d, mean_scratch = up(color), torch.empty(N, dtype=torch.int32, device=dev)
        if any(has(j, 4, 7) for j in range(L)):
            ipar_d, lut = up(ipar), torch.empty(N, 768, dtype=torch.uint8, device=dev)
            inv = self._inv_scale.get(dev)
            if inv is None:
                inv = self._inv_scale[dev] = torch.tensor(AUTOCONTRAST_SCALES, dtype=torch.float64).to(dev)
        tmp = torch.empty_like(img_u8) if any(has(j, 8, 8) for j in range(L)) else None
        for j in range(L):
            if has(j, 1, 3):
                check(lib().udapose_aug_color_op(_hip.stream(), ptr(img_u8), ptr(color_d[j]), ptr(fpar_d[j]), ptr(mean_scratch), N, H * W),
                      "aug_color_op")
            if has(j, 4, 7):
                check(lib().udapose_aug_point_op(_hip.stream(), ptr(img_u8), ptr(code_d[j]), ptr(ipar_d[j]), ptr(inv), ptr(lut), N, H * W),
                      "aug_point_op")
            if has(j, 8, 8):
                check(lib().udapose_aug_sharpness_u8(_hip.stream(), ptr(img_u8), ptr(tmp), ptr(code_d[j]), ptr(fpar_d[j]), N, H, W),
                      "aug_sharpness_u8")
        return img_u8

    def erase_(self, x, boxes, value):
        """RandomErasing's write in place on the normalised tensor x [N,3,H,W] fp32 (the reference applies it after ToTensor and writes
        `mean` as it is): boxes = one (top, left, h, w) per sample, an empty box (h or w 0) leaves its sample alone; value = the three fills."""
        _hip.require_cuda(x)
        N, C3, H, W = x.shape
        assert C3 == 3 and x.dtype == torch.float32 and x.is_contiguous()
        if len(boxes) != N or len(value) != 3:
            raise ValueError(f"erase_: {len(boxes)} boxes for a batch of {N}, {len(value)} fill values for 3 channels")
        for (top, left, h, w) in boxes:
            if h < 0 or w < 0 or (h > 0 and w > 0 and not (0 <= top and 0 <= left and top + h <= H and left + w <= W)):
                raise ValueError(f"erase box {(top, left, h, w)} outside a {H}x{W} image")
        if not any(h > 0 and w > 0 for (_, _, h, w) in boxes):
            return x
        box_d = torch.tensor(boxes, dtype=torch.int32).to(x.device, non_blocking=True)
        check(lib().udapose_aug_erase_f32(_hip.stream(), ptr(x), ptr(box_d), float(value[0]), float(value[1]), float(value[2]), N, H, W),
              "aug_erase_f32")
        return x

    def to_tensor(self, img_u8):
        N, H, W, _ = img_u8.shape
        c = self._consts(img_u8.device)
        out = torch.empty(N, 3, H, W, dtype=torch.float32, device=img_u8.device)
        check(lib().udapose_aug_to_tensor(_hip.stream(), ptr(img_u8), ptr(out), N, H * W, ptr(c["mean"]), ptr(c["std"])), "aug_to_tensor")
        return out

    def labels(self, keypoints, visible, device):
        """generate_target for [N,K,2] key points (numpy float64, image pixels) -> (target [N,K,Hh,Wh], weight [N,K,1]) on device.
        With subpixel_labels the Gaussian is evaluated round keypoint / stride itself (udapose_gaussian_labels_subpixel): same window, same
        weights, no half-pixel rounding of the position."""
        c = self._consts(device)
        N, K, _ = keypoints.shape
        kp = torch.from_numpy(np.ascontiguousarray(keypoints, dtype=np.float64)).to(device, non_blocking=True)
        vis = torch.from_numpy(np.ascontiguousarray(visible, dtype=np.float32).reshape(N * K)).to(device, non_blocking=True)
        Hh = Wh = self.heatmap_size
        target = torch.empty(N, K, Hh, Wh, dtype=torch.float32, device=device)
        weight = torch.empty(N, K, 1, dtype=torch.float32, device=device)
        stride = self.image_size / self.heatmap_size
        if self.subpixel_labels:
            check(lib().udapose_gaussian_labels_subpixel(_hip.stream(), ptr(kp), ptr(vis), ptr(target), ptr(weight), N * K, Hh, Wh, float(stride),
                                                         float(stride), float(self.sigma), c["rad"]), "gaussian_labels_subpixel")
            return target, weight
        check(lib().udapose_gaussian_labels(_hip.stream(), ptr(kp), ptr(vis), ptr(target), ptr(weight), N * K, Hh, Wh, float(stride), float(stride),
                                            ptr(c["patch"]), c["rad"]), "gaussian_labels")
        return target, weight

    def labels_animal(self, tpts, visible, gate, device, sigma=None, label_type="Gaussian", out_res=None):
        """The animal `_mt` datasets' label loop (lib/datasets/real_animal_all_mt.py:274-283 -> draw_labelmap_ori, lib/datasets/util.py:326-363)
        for a batch: tpts [N,K,2+] float32 = the transformed key points as `transform(pts + 1, ...)` returns them (1-based; the datasets pass
        `tpts - 1`), visible [N,K] = pts[:, 2], gate [N,K] bool = `tpts[i, 1] > 0` of the UN-transformed points
        -> (target [N,K,R,R], weight [N,K,1]) on the device.  The stamp is built as the reference builds it (float64, Gaussian or Cauchy)."""
        sigma = self.sigma if sigma is None else sigma
        R = int(out_res or self.heatmap_size)
        tp = np.ascontiguousarray(np.asarray(tpts, dtype=np.float32)[..., :2])
        N, K, _ = tp.shape
        size = 6 * sigma + 1
        x = np.arange(0, size, 1, float)
        y = x[:, np.newaxis]
        x0 = y0 = size // 2
        if label_type == "Gaussian":
            g = np.exp(-((x - x0) ** 2 + (y - y0) ** 2) / (2 * sigma ** 2))
        elif label_type == "Cauchy":
            g = sigma / (((x - x0) ** 2 + (y - y0) ** 2 + sigma ** 2) ** 1.5)
        else:
            raise ValueError("label_type must be 'Gaussian' or 'Cauchy' (lib/datasets/util.py:349-352)")
        patch = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).to(device, non_blocking=True)
        pt = torch.from_numpy(tp - np.float32(1)).to(device, non_blocking=True)
        vis = torch.from_numpy(np.ascontiguousarray(visible, dtype=np.float32).reshape(N * K)).to(device, non_blocking=True)
        gt = torch.from_numpy(np.ascontiguousarray(np.asarray(gate).reshape(N * K), dtype=np.uint8)).to(device, non_blocking=True)
        target = torch.empty(N, K, R, R, dtype=torch.float32, device=device)
        weight = torch.empty(N, K, 1, dtype=torch.float32, device=device)
        check(lib().udapose_draw_labelmap_ori(_hip.stream(), ptr(pt), ptr(vis), ptr(gt), ptr(target), ptr(weight), N * K, R, R,
                                              float(np.float32(3 * sigma)), ptr(patch), int(g.shape[0])), "draw_labelmap_ori")
        return target, weight

    # ------------------------------------------------------------------ one view of the whole batch
    def view(self, base_u8, keypoints, cfg, params=None, jitter=None, blur=None, strong=None, erase=None):
        """One view of the whole batch, every draw not given made here (`view_with_flips` states the result and the order of the draws; the
        flips of a configuration with flip > 0 are drawn)."""
        return self.view_with_flips(base_u8, keypoints, cfg, None, params, jitter, blur, strong, erase)

    def view_with_flips(self, base_u8, keypoints, cfg, flips, params=None, jitter=None, blur=None, strong=None, erase=None):
        """-> (image [N,3,H,W] fp32 normalised, key points [N,K,2], aug_param collated, target, weight)
        strong = per-sample (codes, parameters) as `draw_strong` returns them, erase = per-sample boxes as `draw_erase` does; both are drawn
        when None and the configuration has them on - after every other draw of the view (affine for every sample, jitter for every
        sample, blur), strong for every sample first, then erase: a seeded pipeline draws the same affine / jitter / blur values with the
        strong view on as with it off.  Neither touches key points, aug_param, labels or weights (an erased key point stays labelled).
        flips = per-sample 0 / 1 (`draw_flip`), drawn last of all when None and cfg.flip > 0: a flagged sample's base crop is mirrored ahead
        of the warp and its key points (and visibility) go through `mirror_keypoints` ahead of `transform_keypoints`: the returned key
        points, labels and weights are the mirrored person's.  aug_param gets `flip` (int64 [N]) as a 5th entry when, and only when,
        cfg.flip > 0 (flips for a configuration without: ValueError - the flags would be lost)."""
        N, H, W, _ = base_u8.shape
        if cfg.flip > 0 and self.flip_pairs is None:
            raise ValueError("a view with flip > 0 needs the pipeline's flip_pairs (pipe.flip_pairs = the left / right joint pairs, possibly "
                             "empty, or a key of FLIP_PAIRS): a mirrored person's left joints are its right ones")
        if cfg.flip == 0 and flips is not None:
            raise ValueError("flips were given for a view whose configuration has flip = 0: its aug_param could not carry them")
        if params is None:
            params = [cfg.draw_affine(self.rng, (W, H)) for _ in range(N)]
        if jitter is None:
            jitter = [cfg.draw_jitter(self.rng) for _ in range(N)]
        if blur is None and cfg.blur > 0:
            blur = [cfg.draw_blur(self.np_rng) for _ in range(N)]
        if strong is None and cfg.strong_ops > 0:
            strong = [cfg.draw_strong(self.rng) for _ in range(N)]
        if erase is None and cfg.erase > 0:
            erase = [cfg.draw_erase(self.rng, H, W) for _ in range(N)]
        if flips is None and cfg.flip > 0:
            flips = [cfg.draw_flip(self.rng) for _ in range(N)]
        vis = np.ones((N, keypoints.shape[1], 1), np.float32)
        if flips is not None:
            base_u8 = self.hflip(base_u8, flips)
            keypoints, vis = np.array(keypoints, dtype=np.float64, copy=True), vis.copy()
            for i in range(N):
                if int(flips[i]):
                    keypoints[i], vis[i] = mirror_keypoints(keypoints[i], vis[i], W, self.flip_pairs)
        img = self.warp_images(base_u8, params)
        self.jitter_(img, [j[0] for j in jitter], [j[1] for j in jitter])
        if strong is not None:
            self.strong_(img, [s[0] for s in strong], [s[1] for s in strong])
        if blur is not None:
            self.blur_(img, blur)                     # (after the colour jitter, before ToTensor: train_human.py:67-71)
        x = self.to_tensor(img)
        if erase is not None:
            self.erase_(x, erase, cfg.erase_value)    # (RandomErasing works on the tensor: lib/transforms/__init__.py:154-177)
        kp = np.stack([transform_keypoints(keypoints[i], *params[i], W, H) for i in range(N)])
        # aug_param = the INVERSE augmentation (keypoint_detection.py:139), collated like default_collate does
        aug = [torch.tensor([-p[0] for p in params], dtype=torch.float64),
               [torch.tensor([-p[3] for p in params], dtype=torch.int64), torch.tensor([-p[4] for p in params], dtype=torch.int64)],
               [torch.tensor([-p[1] for p in params], dtype=torch.float64), torch.tensor([-p[2] for p in params], dtype=torch.float64)],
               torch.tensor([1.0 / p[5] for p in params], dtype=torch.float64)]
        if flips is not None:
            aug.append(torch.tensor([int(f) for f in flips], dtype=torch.int64))
        target, weight = self.labels(kp, vis, base_u8.device)
        return x, kp, aug, target, weight

    def __call__(self, base_u8, keypoints, raw=False):
        """The collated 8-tuple of the `_mt` datasets (human36m_mt.py:161): (x_t_stu, target_stu, weight_stu, meta_stu, x_t_teas,
        targets_tea, weights_tea, metas_tea) with the meta fields the loop reads (train_human.py:330-345).  raw=True: `base_u8` are the
        decoded dataset images and the base transform (RandomResizedCrop, human36m_mt.py:86) runs here first."""
        keypoints = np.asarray(keypoints, dtype=np.float64)
        if raw:
            base_u8, keypoints = self.resized_crop(base_u8, keypoints)
        x_s, kp_s, aug_s, t_s, w_s = self.view(base_u8, keypoints, self.stu)
        vis = np.ones((keypoints.shape[0], keypoints.shape[1], 1), np.float32)
        t_ori, w_ori = self.labels(keypoints, vis, base_u8.device)
        meta_stu = {"aug_param_stu": aug_s, "keypoint2d_stu": kp_s, "keypoint2d_ori": keypoints, "target_ori": t_ori, "target_weight_ori": w_ori}
        xs, ts, ws, metas = [], [], [], []
        for _ in range(self.k):
            x_t, kp_t, aug_t, t_t, w_t = self.view(base_u8, keypoints, self.tea)
            xs.append(x_t); ts.append(t_t); ws.append(w_t)
            metas.append({"aug_param_tea": aug_t, "keypoint2d_tea": kp_t})
        return x_s, t_s, w_s, meta_stu, xs, ts, ws, metas
