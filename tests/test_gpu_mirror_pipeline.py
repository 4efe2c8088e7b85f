"""Mirrored views through the device data pipeline and the occlusion path on the MI355X: udapose_aug_hflip_u8 ahead of the
u8 affine warp, a whole TargetViewPipeline.view() with flips against the same view of a pre-mirrored base with pre-swapped key points, the
round trip of its labels through warp.recon_heatmaps(flip_pairs=), and warp.occlude_keypoints_device(mirror=) against its composition."""
import random

import numpy as np
import pytest
import torch

from helpers import mirror_views_ref as R

pytestmark = pytest.mark.gpu


def _pipe(size, flip_pairs=None):
    from uda_poseestimation_amd.data_gpu import TargetViewPipeline
    pipe = TargetViewPipeline(image_size=size, heatmap_size=size // 4, rng=random.Random(3), np_rng=np.random.RandomState(3))
    pipe.flip_pairs = flip_pairs
    return pipe


def _bytes(n, size, seed):
    return torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).cuda()


def test_u8_mirror_ahead_of_the_affine_warp():
    from uda_poseestimation_amd.data_gpu import ViewConfig
    pipe = _pipe(64, flip_pairs="body16")
    base = _bytes(3, 64, 1)
    rng = random.Random(2)
    params = [ViewConfig().draw_affine(rng, (64, 64)) for _ in range(3)]
    flips = [1, 0, 1]
    mirrored = pipe.hflip(base, flips)
    assert mirrored.data_ptr() != base.data_ptr()
    got = pipe.warp_images(mirrored, params)
    want_flipped = pipe.warp_images(torch.flip(base, [2]).contiguous(), params)
    want_plain = pipe.warp_images(base, params)
    for n, f in enumerate(flips):
        assert torch.equal(got[n], (want_flipped if f else want_plain)[n]), n
        assert torch.equal(mirrored[n], torch.flip(base[n], [1]) if f else base[n])
    assert not torch.equal(want_flipped[0], want_plain[0])
    assert pipe.hflip(base, [0, 0, 0]) is base          # (no flag: no launch)
    with pytest.raises(ValueError):
        pipe.hflip(base, [0, 2, 0])
    with pytest.raises(ValueError):
        pipe.hflip(base, [0, 1])


def _view_inputs(seed=4, n=4):
    from uda_poseestimation_amd.data_gpu import ViewConfig
    from uda_poseestimation_amd.lib.keypoint_detection import FLIP_PAIRS
    rs, rng = np.random.RandomState(seed), random.Random(seed)
    kps = np.stack([R.paired_keypoints(rs, FLIP_PAIRS["body16"], 16) for _ in range(n)])
    cfg = ViewConfig(flip=0.5)
    params = [cfg.draw_affine(rng, (R.S, R.S)) for _ in range(n)]
    jitter = [cfg.draw_jitter(rng) for _ in range(n)]
    return kps, params, jitter


def test_view_with_flips_is_the_view_of_the_mirrored_base():
    from uda_poseestimation_amd import warp
    from uda_poseestimation_amd.data_gpu import ViewConfig
    from uda_poseestimation_amd.lib.keypoint_detection import flip_perm
    pipe = _pipe(R.S, flip_pairs="body16")
    base = _bytes(4, R.S, 5)
    kps, params, jitter = _view_inputs()
    flips = [1, 0, 1, 1]
    perm = flip_perm("body16", 16)
    x, kp, aug, target, weight = pipe.view_with_flips(base, kps, ViewConfig(flip=0.5), flips, params=params, jitter=jitter)
    # the same view of a base mirrored beforehand, with key points mirrored and swapped beforehand, and no flips
    base_m, kps_m = base.clone(), kps.copy()
    for n, f in enumerate(flips):
        if f:
            base_m[n] = torch.flip(base[n], [1])
            kps_m[n] = R.mirror_keypoints_ref(kps[n], R.S, perm.tolist())
    x2, kp2, aug2, target2, weight2 = pipe.view(base_m, kps_m, ViewConfig(), params=params, jitter=jitter)
    assert torch.equal(x, x2) and torch.equal(target, target2) and torch.equal(weight, weight2) and np.array_equal(kp, kp2)
    assert len(aug) == 5 and len(aug2) == 4
    assert aug[4].dtype == torch.int64 and aug[4].tolist() == flips
    assert torch.equal(warp.pack_aug_param(aug, 4), warp.pack_aug_param(aug2, 4))
    assert float(weight.sum()) > 0
    # flips for a configuration without them would be lost: refused
    with pytest.raises(ValueError):
        pipe.view_with_flips(base, kps, ViewConfig(), flips, params=params, jitter=jitter)
    with pytest.raises(ValueError):       # a flipped view and no pair table: refused before anything is drawn
        _pipe(R.S).view(base, kps, ViewConfig(flip=0.5))
    # drawn when not given; the 5th entry is there even when nothing was flagged
    aug3 = pipe.view(base, kps, ViewConfig(flip=0.5), params=params, jitter=jitter)[2]
    assert len(aug3) == 5 and set(aug3[4].tolist()) <= {0, 1}
    assert len(pipe.view_with_flips(base, kps, ViewConfig(flip=0.5), [0, 0, 0, 0], params=params, jitter=jitter)[2]) == 5

    # the round trip on the device: the mirrored view's labels, un-warped and flipped back, against the base labels; the bound is the
    # un-mirrored view's own largest deviation plus 1 px (tests/test_mirror_views_cpu.py states the rule)
    base_lab = pipe.labels(kps, np.ones((4, 16, 1), np.float32), "cuda")[0]
    x0, kp0, aug0, target0, _ = pipe.view(base, kps, ViewConfig(), params=params, jitter=jitter)

    def deviation(recon, kp_view, flagged):
        worst, inside = 0.0, 0
        for n in range(4):
            ok = R.inside_view(kp_view[n])
            ok = ok[perm.numpy()] if flagged[n] else ok
            d = (R.argmax_xy(recon[n].cpu()) - R.argmax_xy(base_lab[n].cpu())).norm(dim=1).numpy()
            worst, inside = max(worst, float(d[ok].max()) if ok.any() else 0.0), inside + int(ok.sum())
        return worst, inside / (4 * 16)
    d0, share0 = deviation(warp.recon_heatmaps(target0, aug0, 4.0), kp0, [0] * 4)
    d1, share1 = deviation(warp.recon_heatmaps(target, aug, 4.0, flip_pairs="body16"), kp, flips)
    print(f"largest arg-max deviation: un-mirrored {d0:.3f} px, mirrored {d1:.3f} px; joints inside the view {share0:.3f} / {share1:.3f}")
    assert share1 >= 0.5 and d0 + 1.0 < 8.0
    assert d1 <= d0 + 1.0


def test_device_occlusion_with_mirror_is_the_composition():
    from uda_poseestimation_amd import synthetic, warp
    n, S = 4, R.S
    x = synthetic.images(n, S, 21).cuda()
    kps, _, _ = _view_inputs(seed=6)
    y = torch.stack([R.label_maps(kps[i]) for i in range(n)]).cuda()              # confident peaks: every sample qualifies
    ap = synthetic.aug_params(n, np.random.RandomState(22))
    th_f, th_b = warp.recon_thetas(ap, n, 4.0, "cuda"), warp.occlusion_back_thetas(ap, n, 4.0, "cuda")
    u = torch.rand(n, 4, generator=torch.Generator().manual_seed(23)).cuda()
    u[:, 0] = torch.tensor([0.1, 0.2, 0.3, 2.0])                                   # sample 3 fails the rate test: returned as it came
    flips = [1, 0, 1, 1]
    args = (4.0, S, 0.9, 0.5, 10)
    mirror = torch.tensor(flips, dtype=torch.uint8, device="cuda")
    got, apply = warp.occlude_keypoints_device(x, y, th_f, th_b, u, *args, mirror=mirror)
    want, apply_ref = R.occlude_device_ref(x, y, th_f, th_b, u, *args, flips)
    assert apply.tolist() == apply_ref.tolist() == [1, 1, 1, 0]
    assert torch.equal(got, want)
    plain, apply_plain = warp.occlude_keypoints_device(x, y, th_f, th_b, u, *args)
    assert apply_plain.tolist() == apply.tolist()
    assert torch.equal(got[1], plain[1]) and torch.equal(got[3], x[3])            # flag 0: today's result; not selected: untouched
    assert not torch.equal(got[0], plain[0])
    # all flags zero, and no mirror at all: the un-mirrored function
    zero = warp.occlude_keypoints_device(x, y, th_f, th_b, u, *args, mirror=torch.zeros(n, dtype=torch.uint8, device="cuda"))[0]
    assert torch.equal(zero, plain)
