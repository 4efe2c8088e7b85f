"""Mirrored views without a GPU: the draw order of ViewConfig(flip=), the parsing of the 5-entry aug_param, the key-point
algebra of a flip, and the semantics themselves - label maps of the mirrored and swapped key points, un-warped and flipped back with
oracle/affine_ref.py on the CPU, land where the base labels are."""
import random

import numpy as np
import pytest
import torch

from helpers import mirror_views_ref as R


def _draws(cfg, seed, n=6):
    """Every draw of a view in view()'s order, through the draw_* methods alone."""
    rng, nrng = random.Random(seed), np.random.RandomState(seed)
    out = {"affine": [cfg.draw_affine(rng, (128, 128)) for _ in range(n)], "jitter": [cfg.draw_jitter(rng) for _ in range(n)],
           "blur": [cfg.draw_blur(nrng) for _ in range(n)], "strong": [cfg.draw_strong(rng) for _ in range(n)],
           "erase": [cfg.draw_erase(rng, 128, 128) for _ in range(n)]}
    if cfg.flip > 0:
        out["flip"] = [cfg.draw_flip(rng) for _ in range(n)]
    return out, rng.getstate(), nrng.get_state()


def test_flip_is_drawn_last_and_not_at_all_when_off():
    from uda_poseestimation_amd.data_gpu import ViewConfig
    kw = dict(blur=1.5, strong_ops=2, erase=0.5)
    off, on = ViewConfig(flip=0.0, **kw), ViewConfig(flip=0.5, **kw)
    d_off, state_off, nstate_off = _draws(off, 11)
    d_on, state_on, nstate_on = _draws(on, 11)
    for name in ("affine", "jitter", "blur", "strong", "erase"):
        assert d_on[name] == d_off[name], name
    assert "flip" not in d_off and set(d_on["flip"]) <= {0, 1} and len(set(d_on["flip"])) == 2
    # flip = 0 consumes nothing beyond the other draws: the generator stands where a configuration without the argument leaves it
    d_ref, state_ref, nstate_ref = _draws(ViewConfig(**kw), 11)
    assert state_off == state_ref and all(np.array_equal(a, b) for a, b in zip(nstate_off, nstate_ref))
    assert state_on != state_off                        # (the flips come out of python's generator, after everything else)
    assert all(np.array_equal(a, b) for a, b in zip(nstate_on, nstate_off))
    # one rng.random() < flip per sample
    rng, twin = random.Random(5), random.Random(5)
    assert [on.draw_flip(rng) for _ in range(32)] == [int(twin.random() < 0.5) for _ in range(32)]
    with pytest.raises(ValueError):
        ViewConfig(flip=1.5)


def test_pipeline_needs_flip_pairs_for_a_flipped_view():
    """Refused before anything is drawn or launched (the base crop is never looked at: a host tensor does here)."""
    from uda_poseestimation_amd.data_gpu import TargetViewPipeline, ViewConfig
    rng = random.Random(1)
    pipe = TargetViewPipeline(image_size=128, heatmap_size=32, rng=rng)
    assert pipe.flip_pairs is None
    base, kps = torch.zeros(2, 128, 128, 3, dtype=torch.uint8), np.zeros((2, 16, 2))
    with pytest.raises(ValueError, match="flip_pairs"):
        pipe.view(base, kps, ViewConfig(flip=0.5))
    with pytest.raises(ValueError, match="flip = 0"):
        pipe.view_with_flips(base, kps, ViewConfig(), [1, 0])
    assert rng.getstate() == random.Random(1).getstate()


def test_aug_mirror_parsing():
    from uda_poseestimation_amd.warp import aug_mirror, pack_aug_param
    n = 3
    four = [torch.zeros(n, dtype=torch.float64), [torch.zeros(n, dtype=torch.int64)] * 2, [torch.zeros(n, dtype=torch.float64)] * 2,
            torch.ones(n, dtype=torch.float64)]
    assert aug_mirror(four, n) is None
    got = aug_mirror(four + [torch.tensor([1, 0, 1])], n)
    assert got.dtype == torch.uint8 and got.tolist() == [1, 0, 1] and not got.is_cuda
    assert aug_mirror(four + [[0, 1, 0]], n).tolist() == [0, 1, 0]
    for bad in (torch.tensor([0, 2, 1]), torch.tensor([0, -1, 1]), torch.tensor([0, 1]), torch.tensor([0, 1, 0, 1]), torch.tensor([[0, 1, 0]])):
        with pytest.raises(ValueError):
            aug_mirror(four + [bad], n)
    with pytest.raises(ValueError):
        aug_mirror(four[:3], n)
    with pytest.raises(ValueError):
        aug_mirror(four + [torch.tensor([0, 1, 0]), 1], n)
    # the four affine entries of a 5-entry structure are packed as before
    assert torch.equal(pack_aug_param(four + [torch.tensor([1, 0, 1])], n), pack_aug_param(four, n))


@pytest.mark.parametrize("table,K", [("body16", 16), ("animal18", 18), ((), 21), (((1, 3),), 5)])
def test_keypoint_algebra_of_a_flip(table, K):
    from uda_poseestimation_amd.data_gpu import mirror_keypoints
    from uda_poseestimation_amd.lib.keypoint_detection import FLIP_PAIRS, flip_perm
    W = 128
    rs = np.random.RandomState(K)
    kp = rs.uniform(0, W, (K, 2))
    vis = (rs.uniform(size=(K, 1)) > 0.4).astype(np.float32)
    pairs = FLIP_PAIRS[table] if isinstance(table, str) else table
    perm = list(range(K))
    for i, j in pairs:
        perm[i], perm[j] = j, i
    assert flip_perm(table, K).tolist() == perm
    got, gvis = mirror_keypoints(kp, vis, W, table)
    want = R.mirror_keypoints_ref(kp, W, perm)
    assert np.array_equal(got, want) and np.array_equal(gvis, vis[perm])
    for i, j in pairs:      # channel i of a mirrored person is the base's joint j, seen at W - 1 - x
        assert got[i, 0] == W - 1 - kp[j, 0] and got[i, 1] == kp[j, 1] and got[j, 0] == W - 1 - kp[i, 0]
    for k in set(range(K)) - {v for p in pairs for v in p}:
        assert got[k, 0] == W - 1 - kp[k, 0] and got[k, 1] == kp[k, 1]
    back, bvis = mirror_keypoints(got, gvis, W, table)          # an involution
    assert np.allclose(back, kp, rtol=0, atol=1e-12) and np.array_equal(bvis, vis)
    assert kp is not got and np.array_equal(kp, np.random.RandomState(K).uniform(0, W, (K, 2)))      # (the input is left alone)


SEED = 3        # chosen so that at least 75 % of the joints stay inside the view over the 8 draws (asserted below)


def test_mirrored_labels_unwarp_onto_the_base_labels():
    """8 seeded draws at 128 px / 32 x 32 maps, "body16": flip_back o chain of the mirrored view's labels against the base labels.  The bound
    is the un-mirrored run's own largest deviation (nearest resampling, the labels' half-pixel rounding, the loop's three-warp inverse) plus
    1 px for the mirror's W - 1 - x on image pixels against the flip of whole heat-map pixels; paired joints lie >= 8 px apart."""
    plain, share_plain = R.round_trip_cpu(SEED, "body16", 16, mirrored=False)
    mirrored, share = R.round_trip_cpu(SEED, "body16", 16, mirrored=True)
    print(f"largest arg-max deviation: un-mirrored {plain:.3f} px, mirrored {mirrored:.3f} px; joints inside the view: {share_plain:.3f} / {share:.3f}")
    assert share >= 0.75 and share_plain >= 0.75
    assert plain + 1.0 < 8.0          # (the bound separates a correct round trip from a missing swap)
    assert mirrored <= plain + 1.0


def test_round_trip_notices_inverted_semantics():
    """The same round trip with the swap left out, or the mirror taken on the wrong side of the chain, misses by far more than the bound."""
    from uda_poseestimation_amd.data_gpu import ViewConfig, mirror_keypoints, transform_keypoints
    from uda_poseestimation_amd.lib.keypoint_detection import flip_perm
    rng, rs = random.Random(SEED), np.random.RandomState(SEED)
    perm = flip_perm("body16", 16)
    kp = R.paired_keypoints(rs, R._table("body16"), 16)
    params = ViewConfig().draw_affine(rng, (R.S, R.S))
    view = R.label_maps(transform_keypoints(mirror_keypoints(kp, None, R.S, "body16")[0], *params, R.S, R.S))
    base = R.argmax_xy(R.label_maps(kp))
    no_swap = torch.flip(R.unwarp_cpu(view, params, R.S / R.HM), [-1])
    wrong_end = R.unwarp_cpu(R.flip_back_ref(view[None], perm)[0], params, R.S / R.HM)
    right = R.flip_back_ref(R.unwarp_cpu(view, params, R.S / R.HM)[None], perm)[0]
    dev = lambda t: float((R.argmax_xy(t) - base).norm(dim=1).max())
    print(f"right {dev(right):.2f} px, no swap {dev(no_swap):.2f} px, mirror ahead of the chain {dev(wrong_end):.2f} px")
    assert dev(right) < 8.0 <= dev(no_swap) and dev(wrong_end) >= 8.0
