"""The strong student view on the device (csrc/strong_aug.hip through data_gpu.TargetViewPipeline.strong_ / erase_ / view) against PIL
itself, byte for byte: ImageOps.autocontrast / equalize / posterize / solarize and ImageEnhance.Sharpness alone at sizes from 1x1 to
128x128 on random and crafted contents, autocontrast for every (lo, hi) pair in one batch against the numpy restatement that
tests/test_strong_view_cpu.py ties to PIL, mixed batches and chains of ops, the erase, and a whole view with the feature on and off."""
import random

import numpy as np
import pytest
import torch

from helpers import strong_view_ref as R

pytestmark = pytest.mark.gpu

# H*W no multiple of the block and below 255 (equalize's step is 0) ... the lut == 256 image's size ... more than one block per image
SHAPES = [(1, 1), (1, 7), (2, 9), (3, 3), (17, 23), (16, 32), (64, 64), (128, 128)]
SINGLE_OPS = ([(4, 0.0), (5, 0.0)] + [(6, bits) for bits in range(1, 9)] + [(7, thr) for thr in (0, 128, 255, 256, 127.5)] +
              [(8, f) for f in (0.0, 0.1, 1.0, 1.9)])


def content_cases(H, W, seed):
    rs = np.random.RandomState(seed)
    rnd = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    one_const = rnd.copy(); one_const[..., 1] = 77
    two = np.where(rs.rand(H, W, 3) < 0.3, 40, 200).astype(np.uint8)
    full = rnd.copy(); full.reshape(-1, 3)[0] = 0; full.reshape(-1, 3)[-1] = 255
    cases = {"random": rnd, "constant": np.full((H, W, 3), 93, np.uint8), "one constant channel": one_const, "two-valued": two,
             "full range": full, "dark": (rnd // 3).astype(np.uint8)}
    if (H, W) == (16, 32):
        cases["lut 256"] = R.lut256_image()
    return cases


def pipeline(S=8):
    from uda_poseestimation_amd import data_gpu as D
    return D.TargetViewPipeline(image_size=S, heatmap_size=max(S // 4, 1), sigma=2, rng=random.Random(0))


@pytest.mark.parametrize("H,W", SHAPES)
def test_each_op_alone_is_pil_byte_for_byte(H, W):
    """One batch per size: every content x every op and parameter of SINGLE_OPS, one op per image."""
    imgs, ops, names = [], [], []
    for name, img in content_cases(H, W, seed=31 * H + W).items():
        for (code, prm) in SINGLE_OPS:
            imgs.append(img); ops.append((code, prm)); names.append(name)
    base = np.stack(imgs)
    out = pipeline().strong_(torch.from_numpy(base).cuda(), [[o[0]] for o in ops], [[o[1]] for o in ops]).cpu().numpy()
    changed = 0
    for i, (code, prm) in enumerate(ops):
        ref = R.pil_op(base[i], code, prm)
        assert np.array_equal(out[i], ref), f"{H}x{W} {names[i]} op {code} param {prm}: {(out[i] != ref).sum()} of {ref.size} bytes differ from PIL"
        changed += int((ref != base[i]).any())
    assert changed > (10 if H * W > 1 else 0)          # (the batch is not a batch of identities)
    if (H, W) == (16, 32):
        assert out[[i for i, (n, o) in enumerate(zip(names, ops)) if n == "lut 256" and o[0] == 5][0]][15, 31].tolist() == [255, 255, 255]


def test_autocontrast_for_every_lo_hi_pair():
    """32 640 pairs, one per channel of 10 880 images of 16x16 holding every value lo..hi, one batch; against the numpy restatement of the
    table (tests/test_strong_view_cpu.py holds it to PIL's formula for every pair and entry), and against PIL for a sample of the images."""
    pairs = [(lo, hi) for lo in range(256) for hi in range(lo + 1, 256)]
    assert len(pairs) == 32640
    k = np.arange(256)
    chans = np.stack([(lo + k % (hi - lo + 1)) for (lo, hi) in pairs]).astype(np.uint8)          # [32640][256]
    want = np.stack([R.autocontrast_table_lo_hi(lo, hi)[chans[j]] for j, (lo, hi) in enumerate(pairs)]).astype(np.uint8)
    to_img = lambda a: np.ascontiguousarray(a.reshape(10880, 3, 16, 16).transpose(0, 2, 3, 1))
    base, ref = to_img(chans), to_img(want)
    out = pipeline().strong_(torch.from_numpy(base).cuda(), [[4]] * 10880, [[0.0]] * 10880).cpu().numpy()
    bad = np.nonzero((out != ref).reshape(10880, -1).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} images differ, first: image {bad[0]} = pairs {pairs[3 * bad[0]:3 * bad[0] + 3]}"
    for i in (0, 1, 84, 5000, 10879):
        assert np.array_equal(out[i], R.pil_op(base[i], 4)), i


def test_a_batch_with_a_different_op_per_sample_and_chains_of_ops():
    """Codes 0 and 1-3 beside the new ones in one batch; one, two and three ops in sequence (0 = none fills the shorter lists): every image
    equals its own PIL chain, an image with no op keeps its bits."""
    rs = np.random.RandomState(3)
    H, W = 40, 56
    chains = [([0, 0, 0], [0.0, 0.0, 0.0]), ([1, 0, 0], [1.27, 0.0, 0.0]), ([2, 0, 0], [0.73, 0.0, 0.0]), ([3, 0, 0], [1.6, 0.0, 0.0]),
              ([4, 0, 0], [0.0, 0.0, 0.0]), ([5, 0, 0], [0.0, 0.0, 0.0]), ([6, 0, 0], [3, 0.0, 0.0]), ([7, 0, 0], [178.5, 0.0, 0.0]),
              ([8, 0, 0], [1.9, 0.0, 0.0]), ([0, 5, 0], [0.0, 0.0, 0.0]), ([0, 0, 8], [0.0, 0.0, 0.1]),
              ([4, 8, 0], [0.0, 1.27, 0.0]), ([8, 4, 0], [0.1, 0.0, 0.0]), ([5, 7, 0], [0.0, 100.0, 0.0]), ([2, 5, 0], [1.5, 0.0, 0.0]),
              ([6, 4, 0], [2, 0.0, 0.0]), ([7, 6, 8], [64.0, 4, 1.73]), ([5, 4, 5], [0.0, 0.0, 0.0]), ([8, 8, 8], [1.9, 1.9, 0.0]),
              ([3, 8, 1], [0.2, 0.5, 1.4]), ([4, 2, 6], [0.0, 1.3, 5]), ([1, 7, 5], [0.6, 128, 0.0]), ([0, 0, 0], [0.0, 0.0, 0.0])]
    N = len(chains)
    base = rs.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    base[4] = 30 + base[4] // 2; base[11] = 30 + base[11] // 2; base[17] = base[17] // 3          # (autocontrast / equalize have work to do)
    out = pipeline().strong_(torch.from_numpy(base).cuda(), [c[0] for c in chains], [c[1] for c in chains]).cpu().numpy()
    for i, (codes, prm) in enumerate(chains):
        ref = R.pil_chain(base[i], codes, prm)
        assert np.array_equal(out[i], ref), f"sample {i} chain {codes} {prm}: {(out[i] != ref).sum()} bytes differ from PIL"
    assert np.array_equal(out[0], base[0]) and np.array_equal(out[-1], base[-1])
    assert sum(int((out[i] != base[i]).any()) for i in range(N)) == N - 2
    # only code 0 anywhere: the tensor comes back as it is
    t = torch.from_numpy(base).cuda()
    assert pipeline().strong_(t, [[0, 0]] * N, [[0.0, 0.0]] * N) is t and np.array_equal(t.cpu().numpy(), base)


def test_strong_refuses_bad_arguments_before_it_launches():
    t = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device="cuda")
    pipe = pipeline()
    for ops, prm in (([[6], [6]], [[0], [4]]), ([[6], [6]], [[9], [4]]), ([[8], [0]], [[float("nan")], [0.0]]), ([[9], [0]], [[0.0], [0.0]]),
                     ([[4]], [[0.0]]), ([[4], [4, 5]], [[0.0], [0.0, 0.0]]), ([[4], [4]], [[0.0]])):
        with pytest.raises(ValueError):
            pipe.strong_(t, ops, prm)
    with pytest.raises(ValueError):
        pipe.erase_(torch.zeros(2, 3, 8, 8, device="cuda"), [(0, 0, 2, 2)], (0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        pipe.erase_(torch.zeros(2, 3, 8, 8, device="cuda"), [(0, 0, 2, 2), (7, 7, 2, 2)], (0.0, 0.0, 0.0))
    assert int(t.sum()) == 0


def test_erase_fills_its_box_and_nothing_else():
    from uda_poseestimation_amd import data_gpu as D
    H, W = 37, 53
    boxes = [(0, 0, 5, 7), (0, W - 7, 5, 7), (H - 5, 0, 5, 7), (H - 5, W - 7, 5, 7), (0, 11, H, 9), (20, 30, 1, 1), (3, 4, 0, 0), (5, 6, 0, 9),
             (7, 8, 9, 0), (0, 0, H, W), (10, 0, 3, W), (13, 17, 19, 23)]
    x = torch.randn(len(boxes), 3, H, W, generator=torch.Generator().manual_seed(1))
    value = D.ViewConfig().erase_value
    out = pipeline().erase_(x.cuda(), boxes, value).cpu().numpy()
    for i, box in enumerate(boxes):
        ref = R.erase_np(x[i].numpy(), box, value)
        assert np.array_equal(out[i].view(np.uint32), ref.view(np.uint32)), (i, box)          # the box's values and every bit outside it
    assert np.array_equal(out[6], x[6].numpy()) and (out[9] == np.float32(value[1]))[1].all()
    # boxes drawn like the reference draws them, at another size and with other fills
    cfg = D.ViewConfig(erase=0.8, erase_value=(-1.5, 0.0, 2.25))
    rng = random.Random(5)
    drawn = [cfg.draw_erase(rng, 64, 48) for _ in range(16)]
    assert any(b[2] * b[3] == 0 for b in drawn) and any(b[2] * b[3] > 0 for b in drawn)
    y = torch.randn(16, 3, 64, 48, generator=torch.Generator().manual_seed(2))
    out = pipeline().erase_(y.cuda(), drawn, cfg.erase_value).cpu().numpy()
    for i, box in enumerate(drawn):
        assert np.array_equal(out[i].view(np.uint32), R.erase_np(y[i].numpy(), box, cfg.erase_value).view(np.uint32)), (i, box)


def test_a_view_with_the_strong_ops_and_the_erase_is_the_pil_chain_and_leaves_the_rest_alone():
    """view() twice from the same seeds, once with strong_ops = 2, erase = 1.0 and once off: aug_param, key points, labels and weights are
    identical; the image of the strong view is warp -> jitter -> the two ops -> blur -> ToTensor + Normalize by PIL, then the erase."""
    from oracle import transforms_ref as T
    from uda_poseestimation_amd import data_gpu as D
    rs = np.random.RandomState(9)
    N, S, K = 8, 64, 16
    base = rs.randint(0, 256, (N, S, S, 3)).astype(np.uint8)
    base[1] = 40 + base[1] // 2
    kps = rs.uniform(5, S - 5, (N, K, 2))
    res = {}
    for mode, extra in (("off", {}), ("on", dict(strong_ops=2, strong_magnitude=12, erase=1.0))):
        cfg = D.ViewConfig(rotation=40, color=0.25, blur=0.8, **extra)
        pipe = D.TargetViewPipeline(image_size=S, heatmap_size=S // 4, sigma=2, rng=random.Random(12), np_rng=random.Random(13))
        res[mode] = (cfg, pipe.view(torch.from_numpy(base).cuda(), kps, cfg))
    (cfg, (x, kp, aug, target, weight)), (_, (x0, kp0, aug0, target0, weight0)) = res["on"], res["off"]
    assert np.array_equal(kp, kp0) and torch.equal(target, target0) and torch.equal(weight, weight0)
    flat = lambda a: [t for e in a for t in (e if isinstance(e, list) else [e])]
    assert all(torch.equal(u, v) for u, v in zip(flat(aug), flat(aug0)))
    # the draws, in view()'s order
    r, rn = random.Random(12), random.Random(13)
    prm = [cfg.draw_affine(r, (S, S)) for _ in range(N)]
    jit = [cfg.draw_jitter(r) for _ in range(N)]
    blur = [cfg.draw_blur(rn) for _ in range(N)]
    strong = [cfg.draw_strong(r) for _ in range(N)]
    boxes = [cfg.draw_erase(r, S, S) for _ in range(N)]
    assert {4, 5, 7, 8} <= {c for s in strong for c in s[0]} and all(b[2] * b[3] > 0 for b in boxes)
    differs = 0
    for i in range(N):
        w_ref = T.affine_view_ref(base[i], kps[i], *prm[i])[0]
        j_ref = T.color_jitter_ref(w_ref, *jit[i])
        weak = T.to_tensor_normalize_ref(T.gaussian_blur_ref(j_ref, blur[i]), D.IMAGENET_MEAN, D.IMAGENET_STD)
        assert torch.equal(x0[i].cpu(), weak), f"view {i} without the feature differs from the PIL chain"
        t_ref = T.to_tensor_normalize_ref(T.gaussian_blur_ref(R.pil_chain(j_ref, *strong[i]), blur[i]), D.IMAGENET_MEAN, D.IMAGENET_STD)
        ref = R.erase_np(t_ref.numpy(), boxes[i], cfg.erase_value)
        assert np.array_equal(x[i].cpu().numpy().view(np.uint32), ref.view(np.uint32)), f"strong view {i} {strong[i]} {boxes[i]} differs from PIL + erase"
        differs += int(not torch.equal(x[i], x0[i]))
    assert differs == N
