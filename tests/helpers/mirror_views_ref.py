"""Reference statements of the mirrored views that tests/test_mirror_views_cpu.py and tests/test_gpu_mirror_*.py share.

A mirrored view is A(M(base)): M reverses the columns of the base crop, A is the view's affine.  Everything here is the COMPOSITION the
device forms must reproduce bit for bit - torch.flip(., [-1]), a channel index_select by the flip permutation and a plain (un-mirrored) warp
handed in by the caller - or the semantics themselves on the CPU (the round trip of label maps through oracle/affine_ref.py)."""
import random

import numpy as np
import torch

MIRROR_OUT, MIRROR_IN = 1, 2


def flip_back_ref(y, perm):
    """Un-mirror heat-maps [N,C,H,W]: columns reversed, channel c taken from channel perm[c] (perm: a [C] integer tensor, or None)."""
    out = torch.flip(y, [-1])
    return out if perm is None else out.index_select(1, perm.to(device=y.device, dtype=torch.long))


def _swap(t, bits, perm):
    return t if perm is None or bits not in (MIRROR_OUT, MIRROR_IN) else t.index_select(1, perm.to(device=t.device, dtype=torch.long))


def compose_forward(plain, x, theta, bits, perm=None):
    """The mirrored forward as a composition, sample by sample: plain(x [1,C,H,W], theta [1,S,6]) is the un-mirrored warp; bits = one int
    per sample (MIRROR_OUT | MIRROR_IN); perm applies to the samples with exactly one bit set."""
    outs = []
    for n, m in enumerate(bits):
        xin = _swap(x[n:n + 1], m, perm)
        if m & MIRROR_IN:
            xin = torch.flip(xin, [-1])
        out = plain(xin.contiguous(), theta[n:n + 1].contiguous())
        outs.append(torch.flip(out, [-1]) if m & MIRROR_OUT else out)
    return torch.cat(outs, 0)


def compose_backward(plain_bwd, g, theta, bits, perm=None):
    """The exact transpose: dx = plain_bwd(M_perm(g)) for MIRROR_OUT, dx = M(plain_bwd(g)) for MIRROR_IN (M with perm is an involution);
    plain_bwd(g [1,C,H,W], theta [1,S,6]) is the un-mirrored warp's backward."""
    outs = []
    for n, m in enumerate(bits):
        gin = _swap(g[n:n + 1], m, perm)
        if m & MIRROR_OUT:
            gin = torch.flip(gin, [-1])
        dx = plain_bwd(gin.contiguous(), theta[n:n + 1].contiguous())
        outs.append(torch.flip(dx, [-1]) if m & MIRROR_IN else dx)
    return torch.cat(outs, 0)


def autograd_backward(warp_chain, mode):
    """plain_bwd for compose_backward out of a differentiable plain warp_chain(x, theta, mode)."""
    def bwd(g, theta):
        x = torch.zeros_like(g, requires_grad=True)
        warp_chain(x, theta, mode).backward(g)
        return x.grad
    return bwd


def mirror_keypoints_ref(kp, width, perm):
    """The formula of the contract: x -> W - 1 - x, then row j = the mirrored row perm[j]."""
    out = np.array(kp, dtype=np.float64, copy=True)
    out[:, 0] = width - 1 - out[:, 0]
    return out[np.asarray(perm, dtype=np.int64)]


# ---------------------------------------------------------------- the semantics on the CPU: label maps through the un-warp
S, HM, SIGMA = 128, 32, 2          # image pixels, heat-map pixels, label sigma


def label_maps(kp, heatmap=HM, image=S, sigma=SIGMA):
    """generate_target's Gaussian (lib/datasets/util.py:12-70) for key points [K,2] in image pixels -> [K,h,h] fp32; a joint whose centre
    lies outside the map gets zeros."""
    from uda_poseestimation_amd.synthetic import gaussian_labels
    t, _ = gaussian_labels(np.asarray(kp, np.float32), np.ones((len(kp), 1), np.float32), (heatmap, heatmap), sigma, (image, image))
    return torch.from_numpy(t)


def paired_keypoints(rs, flip_pairs, K, image=S):
    """K key points in the central box of the image; the two joints of a pair lie at least 32 image pixels (8 heat-map pixels) apart in x:
    one in the box's left band, one in its right band - a missing or misplaced swap misses by at least that."""
    lo, hi = 0.25 * image, 0.75 * image
    kp = np.stack([rs.uniform(lo, hi, K), rs.uniform(lo, hi, K)], 1)
    for i, j in flip_pairs:
        kp[i, 0] = rs.uniform(lo, lo + 0.125 * image)
        kp[j, 0] = rs.uniform(hi - 0.125 * image, hi)
    return kp


def unwarp_cpu(labels_view, params, ratio):
    """The loop's three nearest warps (oracle/affine_ref.warp3_ref) with the INVERSE of a view's draw `params` = (angle, shear_x, shear_y,
    tx, ty, scale), as the collated aug_param states it."""
    from oracle.affine_ref import warp3_ref
    a, shx, shy, tx, ty, sc = params
    return warp3_ref(labels_view, -a, -tx, -ty, -shx, -shy, 1.0 / sc, ratio)


def argmax_xy(maps):
    K, h, w = maps.shape
    idx = maps.reshape(K, -1).argmax(1)
    return torch.stack([idx % w, idx // w], 1).double()


def inside_view(kp_view, image=S, margin=S // HM):
    """Joints that stay inside the view: the key point at least one heat-map pixel from every border, so that its label's peak pixel exists."""
    kp_view = np.asarray(kp_view)
    return (kp_view[:, 0] >= margin) & (kp_view[:, 0] < image - margin) & (kp_view[:, 1] >= margin) & (kp_view[:, 1] < image - margin)


def round_trip_cpu(seed, flip_pairs, K, mirrored, draws=8):
    """`draws` seeded affine draws: base key points -> (mirrored and swapped when `mirrored`) -> the view's key points -> label maps in the
    view -> un-warped (and flipped back) -> arg-max against the arg-max of the base labels.
    -> (largest deviation in heat-map pixels over the joints inside the view, share of joints inside the view)."""
    from uda_poseestimation_amd.data_gpu import ViewConfig, mirror_keypoints, transform_keypoints
    from uda_poseestimation_amd.lib.keypoint_detection import flip_perm
    rng, rs = random.Random(seed), np.random.RandomState(seed)
    cfg = ViewConfig()          # the reference's ranges: rotation 180, shear 30, translation 5 %, scale 0.6 .. 1.3
    perm = flip_perm(flip_pairs, K)
    worst, inside_n, total = 0.0, 0, 0
    for _ in range(draws):
        kp = paired_keypoints(rs, flip_pairs if not isinstance(flip_pairs, str) else _table(flip_pairs), K)
        params = cfg.draw_affine(rng, (S, S))
        kp_in = mirror_keypoints(kp, None, S, flip_pairs)[0] if mirrored else kp
        kp_view = transform_keypoints(kp_in, *params, S, S)
        recon = unwarp_cpu(label_maps(kp_view), params, S / HM)
        if mirrored:
            recon = flip_back_ref(recon[None], perm)[0]
        # row j of the view's arrays is joint perm[j] of the base: after flip_back, channel j is the base's joint j again
        ok = inside_view(kp_view)
        ok = ok[perm.numpy()] if mirrored else ok
        d = (argmax_xy(recon) - argmax_xy(label_maps(kp))).norm(dim=1).numpy()
        if ok.any():
            worst = max(worst, float(d[ok].max()))
        inside_n, total = inside_n + int(ok.sum()), total + K
    return worst, inside_n / total


def _table(name):
    from uda_poseestimation_amd.lib.keypoint_detection import FLIP_PAIRS
    return FLIP_PAIRS[name]


def occlude_device_ref(x, y_t_tea_recon, theta_fwd, theta_back, u, ratio, image_size, rate, thresh, size, flags):
    """warp.occlude_keypoints_device for mirrored views as a composition: the package's own decision and paste launches, the PLAIN
    warp_chain, and torch.flip where the mirrored warps fold it in - after the warp to the canonical frame, ahead of the warp back."""
    from uda_poseestimation_amd import _hip, warp
    from uda_poseestimation_amd import heatmap_args as ha
    from uda_poseestimation_amd._hip import check, lib, ptr
    B, K, h, w = y_t_tea_recon.shape
    peak = ha.heatmap_argmax(ha.f32c(y_t_tea_recon), maxv=True, idx=True)
    boxes = torch.empty(B, 6, dtype=torch.int32, device=x.device)
    apply = torch.empty(B, dtype=torch.uint8, device=x.device)
    uu = u.float().contiguous()
    check(lib().udapose_occlusion_pick(_hip.stream(), ptr(peak.maxv), ptr(peak.idx), ptr(uu), B, K, w, float(ratio), int(image_size), float(rate),
                                       float(thresh), int(size), ptr(boxes), ptr(apply)), "occlusion_pick")
    f = torch.as_tensor(flags, device=x.device).bool().view(B, 1, 1, 1)
    temp = warp.warp_chain(x.float().contiguous(), theta_fwd)
    temp = torch.where(f, torch.flip(temp, [-1]), temp).contiguous()
    C = temp.shape[1]
    check(lib().udapose_patch_paste(_hip.stream(), ptr(temp), ptr(boxes), B, C, temp.shape[2], temp.shape[3], 4 * size * size * C), "patch_paste")
    back = warp.warp_chain(torch.where(f, torch.flip(temp, [-1]), temp).contiguous(), theta_back)
    return torch.where(apply.bool().view(B, 1, 1, 1), back, x.float()), apply
