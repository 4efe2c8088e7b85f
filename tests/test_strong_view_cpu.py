"""The strong student view, the part that needs no GPU: the numpy restatements of the device's arithmetic (tests/helpers/strong_view_ref.py)
against PIL itself on random and crafted images, the autocontrast table with the host's scale table against PIL's formula for every
(lo, hi) pair, the draws of ViewConfig.draw_strong / draw_erase, the unchanged draw stream of a view with the feature off, and the public
surface: defaults, refusals, the C ABI's declarations and argument checks."""
import ctypes
import inspect
import math
import os
import random

import numpy as np
import pytest
import torch

from helpers import strong_view_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("udapose_aug_point_op", "udapose_aug_sharpness_u8", "udapose_aug_erase_f32")


def content_cases(H, W, seed=0):
    """name -> [H,W,3] uint8: the contents the device tests use too"""
    rs = np.random.RandomState(seed)
    rnd = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    one_const = rnd.copy(); one_const[..., 1] = 77
    two = np.where(rs.rand(H, W, 3) < 0.3, 40, 200).astype(np.uint8)
    full = rnd.copy(); full.reshape(-1, 3)[0] = 0; full.reshape(-1, 3)[-1] = 255
    return {"random": rnd, "constant": np.full((H, W, 3), 93, np.uint8), "one constant channel": one_const, "two-valued": two,
            "full range": full, "dark": (rnd // 3).astype(np.uint8), "narrow": (100 + rnd % 29).astype(np.uint8)}


SHAPES = [(1, 1), (1, 7), (2, 9), (3, 3), (17, 23), (16, 32), (64, 64)]


def test_point_op_restatements_equal_pil():
    for (H, W) in SHAPES:
        cases = content_cases(H, W, seed=H * 100 + W)
        if (H, W) == (16, 32):
            cases["lut 256"] = R.lut256_image()
        for name, img in cases.items():
            for code in (4, 5):
                assert np.array_equal(R.point_op_np(img, code), R.pil_op(img, code)), (H, W, name, code)
            for bits in range(1, 9):
                assert np.array_equal(R.point_op_np(img, 6, bits), R.pil_op(img, 6, bits)), (H, W, name, bits)
            for thr in (0, 0.3, 127.5, 128, 178.5, 254.01, 255, 256):
                assert np.array_equal(R.point_op_np(img, 7, thr), R.pil_op(img, 7, thr)), (H, W, name, thr)
    assert [R.solarize_cut(t) for t in (-3, 0, 0.3, 127.5, 128, 255, 255.5, 256, 300)] == [0, 0, 1, 128, 128, 255, 256, 256, 256]


def test_equalize_entry_256_is_clipped_as_pil_clips_it():
    img = R.lut256_image()
    h = R.histograms(img)
    for c in range(3):
        nz = h[c][h[c] != 0]
        step = (int(nz.sum()) - int(nz[-1])) // 255
        assert step == 2 and (step // 2 + int(h[c][:255].sum())) // step == 256          # the un-clipped entry of 255
        assert R.equalize_table(h[c])[255] == 255
    out = R.pil_op(img, 5)
    assert tuple(out[15, 31]) == (255, 255, 255) and np.array_equal(R.point_op_np(img, 5), out)
    # H*W < 255: step is 0 and the image comes back
    small = content_cases(17, 23)["random"][:15, :16]
    assert np.array_equal(R.pil_op(small, 5), small) and np.array_equal(R.point_op_np(small, 5), small)


def test_autocontrast_table_with_the_host_scale_table_equals_pils_formula_for_every_pair():
    from uda_poseestimation_amd import data_gpu as D
    assert np.array_equal(np.array(D.AUTOCONTRAST_SCALES), R.SCALE_TABLE) and len(D.AUTOCONTRAST_SCALES) == 255
    ix = np.arange(256, dtype=np.float64)
    pairs = 0
    for lo in range(256):
        his = np.arange(lo + 1, 256)
        if len(his) == 0:
            continue
        # PIL's statements for all hi at once: scale = 255.0 / (hi - lo); offset = -lo * scale; int(ix * scale + offset); clip
        scale = 255.0 / (his - lo).astype(np.float64)
        offset = -float(lo) * scale
        want = np.clip(np.trunc(ix[None, :] * scale[:, None] + offset[:, None]), 0, 255).astype(np.int64)
        got = np.stack([R.autocontrast_table_lo_hi(lo, int(hi), D.AUTOCONTRAST_SCALES) for hi in his])
        assert np.array_equal(got, want), lo
        pairs += len(his)
    assert pairs == 32640
    # ... and PIL's own Python statements, float by float, for a sample of pairs, with the pre-clip range the header states
    rs = np.random.RandomState(1)
    ext = 0.0
    for lo, hi in [(0, 1), (254, 255), (0, 255), (127, 128)] + [tuple(sorted(rs.choice(256, 2, replace=False))) for _ in range(300)]:
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        lut = []
        for i in range(256):
            v = i * scale + offset
            ext = max(ext, abs(v))
            lut.append(min(255, max(0, int(v))))
        assert lut == list(R.autocontrast_table_lo_hi(int(lo), int(hi))), (lo, hi)
    assert ext == 65025.0          # (lo, hi) = (0, 1), entry 255
    # through PIL itself: one channel holding every value lo..hi
    for lo, hi in [(0, 1), (3, 250), (100, 101), (17, 200), (254, 255), (0, 255), (200, 200)]:
        img = np.zeros((16, 16, 3), np.uint8)
        img[..., 0] = (lo + np.arange(256) % (hi - lo + 1)).reshape(16, 16)
        img[..., 1] = lo
        img[..., 2] = np.where(np.arange(256).reshape(16, 16) % 2 == 0, lo, hi)
        assert np.array_equal(R.point_op_np(img, 4), R.pil_op(img, 4)), (lo, hi)


def test_smooth_and_sharpness_restatements_equal_pil():
    total = 0
    for (H, W) in SHAPES + [(128, 128)]:
        for name, img in content_cases(H, W, seed=7 + H).items():
            sm = R.smooth_np(img)
            assert np.array_equal(sm, R.pil_smooth(img)), (H, W, name)
            assert np.array_equal(R.smooth_np(img, bottom_up=True), sm), (H, W, name)          # the row order never showed
            if H < 3 or W < 3:
                assert np.array_equal(sm, img)
            for f in (0.0, 0.1, 0.73, 1.0, 1.27, 1.9):
                assert np.array_equal(R.sharpness_np(img, f), R.pil_op(img, 8, f)), (H, W, name, f)
            total += img.size
    assert total > 100000


def test_draw_strong_follows_the_magnitude_table_and_documents_its_draws():
    from uda_poseestimation_amd import data_gpu as D
    assert D.STRONG_OPS == (0, 1, 2, 3, 4, 5, 6, 7, 8) and D.STRONG_BINS == 31
    seen = set()
    for m in (0, 9, 15, 30):
        cfg = D.ViewConfig(strong_ops=4, strong_magnitude=m)
        rng, twin = random.Random(100 + m), random.Random(100 + m)
        for _ in range(200):
            codes, params = cfg.draw_strong(rng)
            assert len(codes) == len(params) == 4
            for c, p in zip(codes, params):
                assert c == D.STRONG_OPS[twin.randrange(9)]
                seen.add(c)
                if c in (1, 2, 3, 8):
                    minus = twin.random() < 0.5
                    assert p == (1.0 - 0.9 * m / 30 if minus else 1.0 + 0.9 * m / 30) and 0.1 - 1e-12 <= p <= 1.9 + 1e-12
                elif c == 6:
                    assert p == 8 - int(round(m / 7.5)) and isinstance(p, int) and 4 <= p <= 8
                elif c == 7:
                    assert p == 255.0 - 255.0 * m / 30 and 0.0 <= p <= 255.0
                else:
                    assert p == 0.0
        assert rng.getstate() == twin.getstate()          # nothing else was drawn
    assert seen == set(D.STRONG_OPS)
    assert [8 - int(round(m / 7.5)) for m in (0, 9, 15, 30)] == [8, 7, 6, 4]
    assert D.ViewConfig().draw_strong(random.Random(0)) == ([], [])
    for bad in (dict(strong_magnitude=31), dict(strong_magnitude=-1), dict(strong_ops=-1), dict(erase=1.5), dict(erase_value=(0.5,))):
        with pytest.raises(ValueError):
            D.ViewConfig(**bad)


def test_draw_erase_makes_the_reference_classes_draws():
    """RandomErasing.__call__ (lib/transforms/__init__.py:156-177) restated here statement by statement on a generator with the same seed."""
    from uda_poseestimation_amd import data_gpu as D
    mean = (0.4914, 0.4822, 0.4465)
    d = {k: v.default for k, v in inspect.signature(D.ViewConfig.draw_erase).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(sl=0.02, sh=0.4, r1=0.3) and D.ViewConfig().erase_value == mean
    erased = skipped = 0
    for (H, W, prob) in ((64, 64, 0.5), (256, 256, 1.0), (17, 40, 0.7), (3, 3, 1.0), (1, 1, 1.0)):
        cfg = D.ViewConfig(erase=prob)
        rng, ref = random.Random(H + W), random.Random(H + W)
        for _ in range(300):
            box = cfg.draw_erase(rng, H, W)
            want = (0, 0, 0, 0)
            if not ref.uniform(0, 1) >= prob:
                for attempt in range(100):
                    area = H * W
                    target_area = ref.uniform(0.02, 0.4) * area
                    aspect_ratio = ref.uniform(0.3, 1 / 0.3)
                    h = int(round(math.sqrt(target_area * aspect_ratio)))
                    w = int(round(math.sqrt(target_area / aspect_ratio)))
                    if w < W and h < H:
                        x1 = ref.randint(0, H - h)
                        y1 = ref.randint(0, W - w)
                        want = (x1, y1, h, w)          # img[c, x1:x1 + h, y1:y1 + w]: x1 is the row
                        break
            assert box == want
            top, left, h, w = box
            assert 0 <= top and 0 <= left and top + h <= H and left + w <= W and h < max(H, 1) and w < max(W, 1)
            if h * w:
                assert 0.02 * H * W / 3.4 <= h * w <= 0.4 * H * W * 1.2 + 2
                erased += 1
            else:
                skipped += 1
        assert rng.getstate() == ref.getstate()
    assert erased > 500 and skipped > 100
    assert D.ViewConfig(erase=0.0).draw_erase(random.Random(0), 64, 64) == (0, 0, 0, 0)


class _Recorder:
    """TargetViewPipeline with every launch replaced by a note of its name: view()'s host side runs without a device."""

    def __new__(cls, **kw):
        from uda_poseestimation_amd import data_gpu as D

        class P(D.TargetViewPipeline):
            def __init__(self, **kw):
                super().__init__(**kw)
                self.calls = []

            def warp_images(self, base, params):
                self.calls.append(("warp", params)); return base.clone()

            def jitter_(self, img, ops, factors):
                self.calls.append(("jitter", ops, factors)); return img

            def strong_(self, img, ops, params):
                self.calls.append(("strong", ops, params)); return img

            def blur_(self, img, radii):
                self.calls.append(("blur", radii)); return img

            def to_tensor(self, img):
                self.calls.append(("to_tensor",)); return torch.zeros(img.shape[0], 3, img.shape[1], img.shape[2])

            def erase_(self, x, boxes, value):
                self.calls.append(("erase", boxes, value)); return x

            def labels(self, kp, vis, device):
                self.calls.append(("labels", kp.copy())); return None, None
        return P(**kw)


def test_a_view_with_the_feature_off_draws_what_it_drew_before_and_new_draws_come_last():
    from uda_poseestimation_amd import data_gpu as D
    N, S = 5, 32
    base = torch.zeros(N, S, S, 3, dtype=torch.uint8)
    kps = np.random.RandomState(0).uniform(0, S, (N, 4, 2))
    for blur in (0.0, 0.8):
        # off: exactly N draw_affine, then N draw_jitter, from rng; the blur from np_rng
        off = D.ViewConfig(rotation=60, blur=blur)
        pipe = _Recorder(image_size=S, heatmap_size=8, rng=random.Random(5), np_rng=random.Random(6))
        out_off = pipe.view(base, kps, off)
        twin, twin_np = random.Random(5), random.Random(6)
        params = [off.draw_affine(twin, (S, S)) for _ in range(N)]
        jit = [off.draw_jitter(twin) for _ in range(N)]
        radii = [off.draw_blur(twin_np) for _ in range(N)] if blur else None
        assert pipe.rng.getstate() == twin.getstate() and pipe.np_rng.getstate() == twin_np.getstate()
        names = [c[0] for c in pipe.calls]
        assert names == ["warp", "jitter"] + (["blur"] if blur else []) + ["to_tensor", "labels"]          # nothing new is launched
        assert pipe.calls[0][1] == params and pipe.calls[1][1] == [j[0] for j in jit] and pipe.calls[1][2] == [j[1] for j in jit]
        # on: the same affine / jitter / blur values, then strong for every sample, then erase for every sample
        on = D.ViewConfig(rotation=60, blur=blur, strong_ops=2, strong_magnitude=12, erase=1.0)
        pipe2 = _Recorder(image_size=S, heatmap_size=8, rng=random.Random(5), np_rng=random.Random(6))
        out_on = pipe2.view(base, kps, on)
        strong = [on.draw_strong(twin) for _ in range(N)]
        boxes = [on.draw_erase(twin, S, S) for _ in range(N)]
        assert pipe2.rng.getstate() == twin.getstate() and pipe2.np_rng.getstate() == twin_np.getstate()
        calls = {c[0]: c for c in pipe2.calls}
        assert [c[0] for c in pipe2.calls] == ["warp", "jitter", "strong"] + (["blur"] if blur else []) + ["to_tensor", "erase", "labels"]
        assert calls["warp"][1] == params and calls["jitter"][2] == [j[1] for j in jit] and (not blur or calls["blur"][1] == radii)
        assert calls["strong"][1] == [s[0] for s in strong] and calls["strong"][2] == [s[1] for s in strong]
        assert calls["erase"][1] == boxes and calls["erase"][2] == on.erase_value
        # key points, aug_param and the labels' input are those of the view without the feature
        assert np.array_equal(out_on[1], out_off[1]) and np.array_equal(calls["labels"][1], pipe.calls[-1][1])
        for a, b in zip(out_on[2], out_off[2]):
            for u, v in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
                assert torch.equal(u, v)
    # given lists are used as they are, and nothing is drawn for them
    pipe3 = _Recorder(image_size=S, heatmap_size=8, rng=random.Random(5))
    given = [([4, 8], [0.0, 1.5])] * N
    pipe3.view(base, kps, D.ViewConfig(), params=params, jitter=jit, strong=given, erase=[(1, 2, 3, 4)] * N)
    assert pipe3.rng.getstate() == random.Random(5).getstate()
    calls = {c[0]: c for c in pipe3.calls}
    assert calls["strong"][1] == [[4, 8]] * N and calls["erase"][1] == [(1, 2, 3, 4)] * N


def test_defaults_signatures_and_refusals():
    from uda_poseestimation_amd import data_gpu as D
    d = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}
    assert list(inspect.signature(D.TargetViewPipeline.__init__).parameters) == [
        "self", "image_size", "heatmap_size", "sigma", "k", "student", "teacher", "mean", "std", "rng", "resize_scale", "np_rng", "subpixel_labels"]
    cd = d(D.ViewConfig.__init__)
    assert list(cd)[-4:] == ["strong_ops", "strong_magnitude", "erase", "erase_value"]
    assert (cd["strong_ops"], cd["strong_magnitude"], cd["erase"], cd["erase_value"]) == (0, 9, 0.0, (0.4914, 0.4822, 0.4465))
    assert list(inspect.signature(D.TargetViewPipeline.view).parameters)[-2:] == ["strong", "erase"]
    assert d(D.TargetViewPipeline.view) == dict(params=None, jitter=None, blur=None, strong=None, erase=None)
    cfg = D.ViewConfig()
    assert (cfg.strong_ops, cfg.erase) == (0, 0.0)
    pipe = D.TargetViewPipeline(image_size=8, heatmap_size=2)
    img = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="MI355X.*no CPU fallback"):
        pipe.strong_(img, [[4], [8]], [[0.0], [1.5]])
    with pytest.raises(RuntimeError, match="MI355X.*no CPU fallback"):
        pipe.erase_(torch.zeros(2, 3, 8, 8), [(0, 0, 2, 2)] * 2, cfg.erase_value)
    # the argument check of strong_
    code, color, fpar, ipar = D.strong_op_arrays([[1, 6, 0], [7, 8, 4]], [[1.2, 4, 0.0], [127.5, 0.3, None]], 2)
    assert code.tolist() == [[1, 7], [6, 8], [0, 4]] and color.tolist() == [[1, 0], [0, 0], [0, 0]]
    assert ipar.tolist() == [[0, 128], [4, 0], [0, 0]] and fpar[0, 0] == np.float32(1.2) and fpar[1, 1] == np.float32(0.3)
    assert D.strong_op_arrays([[7], [7], [7]], [[-5], [255.5], [1e9]], 3)[3].tolist() == [[0, 256, 256]]
    for ops, prm, n in (([[6]], [[0]], 1), ([[6]], [[9]], 1), ([[6]], [[2.5]], 1), ([[6]], [[float("nan")]], 1), ([[9]], [[0]], 1), ([[-1]], [[0]], 1),
                        ([[8]], [[float("inf")]], 1), ([[2]], [[float("nan")]], 1), ([[7]], [[float("nan")]], 1), ([[1, 2]], [[1.0]], 1),
                        ([[1], [2, 3]], [[1.0], [1.0, 1.0]], 2), ([[1]], [[1.0]], 2), ([[1], [1]], [[1.0]], 2)):
        with pytest.raises(ValueError):
            D.strong_op_arrays(ops, prm, n)


def test_the_abi_declares_the_three_exports_and_checks_its_arguments_on_the_host():
    from uda_poseestimation_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "udapose.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    mk = open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "Makefile")).read()
    assert "strong_aug.hip" in mk
    for name in EXPORTS:
        assert name in _hip._SIGS and f"int {name}(" in hdr and f"`{name}`" in doc, name
    assert "UDAPOSE_AUG_MAX_HW (1 << 30)" in hdr and "### 4.20 The strong student view" in open(os.path.join(ROOT, "DESIGN.md")).read()
    buf = ctypes.create_string_buffer(64)          # a non-null address; the checks below return before anything is launched or read
    a = ctypes.addressof(buf)
    big = (1 << 30) + 1
    for kind in ("bf16", "fp16"):
        L = _hip.lib(kind)
        assert L.udapose_aug_point_op(None, None, a, a, a, a, 1, 4) == -1 and L.udapose_aug_point_op(None, a, a, a, None, a, 1, 4) == -1
        assert L.udapose_aug_point_op(None, a, a, a, a, a, 0, 4) == -1 and L.udapose_aug_point_op(None, a, a, a, a, a, 1, 0) == -1
        assert L.udapose_aug_point_op(None, a, a, a, a, a, 1, big) == -3
        assert L.udapose_aug_sharpness_u8(None, a, None, a, a, 1, 4, 4) == -1 and L.udapose_aug_sharpness_u8(None, a, a, a, a, 1, 0, 4) == -1
        assert L.udapose_aug_sharpness_u8(None, a, a, a, a, 1, 1 << 15, (1 << 15) + 1) == -3
        assert L.udapose_aug_sharpness_u8(None, a, a, a, a, 1, 2, 100) == 0          # below 3 on a side: PIL's copy, nothing to launch
        assert L.udapose_aug_erase_f32(None, None, a, 0.0, 0.0, 0.0, 1, 4, 4) == -1 and L.udapose_aug_erase_f32(None, a, a, 0.0, 0.0, 0.0, 1, 4, -1) == -1
        assert L.udapose_aug_erase_f32(None, a, a, 0.0, 0.0, 0.0, 1, 1 << 15, (1 << 15) + 1) == -3
