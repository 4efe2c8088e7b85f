"""The distribution-aware decode, the quarter-pixel decode and the sub-pixel labels, the part that needs no GPU: the plain-numpy restatement
(tests/helpers/dark_fp64.py, the oracle of tests/test_gpu_dark.py) against independent forms - an explicit 2-D sum for the blur,
numpy.linalg.solve for the Newton step - the recovery experiment that motivates the feature, and the public surface: names, defaults,
refusals, the C ABI's declarations, the unchanged signatures."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

from helpers import dark_fp64 as D64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_taps_are_a_normalised_gaussian_and_the_default_sigma_is_2_at_11():
    assert D64.default_sigma(11) == 2.0 and abs(D64.default_sigma(5) - 1.1) < 1e-15
    for k, s in ((3, None), (5, None), (11, None), (11, 0.0), (17, 3.0), (31, None)):
        t = D64.taps(k, s)
        sg = s if s else D64.default_sigma(k)
        assert t.dtype == np.float32 and t.shape == (k,) and abs(float(t.astype(np.float64).sum()) - 1.0) < 1e-6
        assert np.array_equal(t, t[::-1]) and t.argmax() == k // 2
        np.testing.assert_allclose(t[k // 2 + 1] / t[k // 2], np.exp(-1.0 / (2 * sg * sg)), rtol=1e-6)
    for bad in (1, 2, 4, 33, 0, -3):
        with pytest.raises(ValueError):
            D64.taps(bad)


@pytest.mark.parametrize("H,W,k", [(5, 5, 3), (7, 9, 5), (9, 6, 11), (24, 40, 11), (4, 4, 31)])
def test_separable_blur_is_the_explicit_2d_sum_over_the_zero_padded_map(H, W, k):
    rng = np.random.RandomState(H * 100 + W)
    hm = rng.randn(2, H, W)
    t = D64.taps(k).astype(np.float64)
    c = k // 2
    pad = np.zeros((2, H + 2 * c, W + 2 * c))
    pad[:, c:c + H, c:c + W] = hm
    want = np.zeros_like(hm)
    for y in range(H):
        for x in range(W):
            want[:, y, x] = (pad[:, y:y + k, x:x + k] * np.outer(t, t)).sum((1, 2))
    got = D64.blur(hm, D64.taps(k))
    assert got.dtype == np.float64 and float(np.abs(got - want).max()) < 1e-14
    got32 = D64.blur(hm.astype(np.float32), D64.taps(k))
    assert got32.dtype == np.float32 and float(np.abs(got32 - want).max()) < 1e-5


def test_taylor_step_is_linalg_solve_on_the_same_hessian_and_the_guards_return_none():
    rng = np.random.RandomState(1)
    for _ in range(20):
        g = rng.randn(7, 9)
        x, y = rng.randint(2, 7), rng.randint(2, 5)
        dx, dy, dxx, dyy, dxy = D64.derivatives(g, x, y)
        assert dx == 0.5 * (g[y, x + 1] - g[y, x - 1]) and dyy == 0.25 * (g[y + 2, x] - 2 * g[y, x] + g[y - 2, x])
        want = -np.linalg.solve(np.array([[dxx, dxy], [dxy, dyy]]), np.array([dx, dy]))
        np.testing.assert_allclose(D64.taylor_step(dx, dy, dxx, dyy, dxy), want, rtol=1e-10, atol=1e-12)
    # an exact quadratic log-map: the Newton step lands on the vertex
    ys, xs = np.mgrid[0:9, 0:11].astype(np.float64)
    g = -0.07 * (xs - 5.3) ** 2 - 0.05 * (ys - 3.8) ** 2 + 0.02 * (xs - 5.3) * (ys - 3.8)
    np.testing.assert_allclose(np.array(D64.taylor_step(*D64.derivatives(g, 5, 4))) + (5, 4), (5.3, 3.8), atol=1e-12)
    assert D64.taylor_step(0.1, 0.2, 0.0, 0.0, 0.0) is None and D64.taylor_step(0.1, 0.2, 1.0, 1.0, 1.0) is None       # det == 0
    assert D64.taylor_step(np.float64("nan"), 0.2, -1.0, -1.0, 0.0) is None and D64.taylor_step(0.1, 0.2, np.float64("inf"), -1.0, 0.0) is None


@functools.lru_cache(maxsize=None)
def recovery_experiment(H, W, n=300, sigma=2.0, stride=4.0, seed=0):
    """n seeded centres at least 4 px from every edge of an H x W map, as key points in image pixels (centre * stride)."""
    rng = np.random.RandomState(seed + H)
    centres = np.stack([4 + rng.rand(n) * (W - 1 - 8), 4 + rng.rand(n) * (H - 1 - 8)], -1)
    return centres, centres * stride


@pytest.mark.parametrize("H,W", [(24, 40), (64, 64)])
def test_dark_decode_of_subpixel_labels_recovers_the_position_and_argmax_of_quantised_labels_cannot(H, W):
    centres, kp = recovery_experiment(H, W)
    vis = np.ones(len(kp), dtype=np.float32)
    sub, w = D64.labels(kp, vis, H, W, 4.0, 4.0, 2.0, 6, subpixel=True)
    quant, _ = D64.labels(kp, vis, H, W, 4.0, 4.0, 2.0, 6, subpixel=False)
    assert (w == 1).all()
    dark = D64.dark_decode(sub[None], 11)[0][0]
    hard = D64.argmax_decode(quant[None])[0][0]
    e_dark, e_hard = np.linalg.norm(dark - centres, axis=-1), np.linalg.norm(hard - centres, axis=-1)
    print(f"\n{H}x{W}: sub-pixel labels + DARK max {e_dark.max():.4f} px (mean {e_dark.mean():.4f}); quantised labels + arg-max max "
          f"{e_hard.max():.3f} px (mean {e_hard.mean():.3f})")
    assert e_dark.max() <= 0.01
    assert e_hard.max() > 0.4
    # the quarter-pixel decode of the quantised labels has nothing to go on (the label is symmetric round the rounded position)
    assert np.array_equal(D64.quarter_decode(quant[None])[0][0], hard)
    # and of the sub-pixel labels it moves towards the position
    q = D64.quarter_decode(sub[None])[0][0]
    assert np.linalg.norm(q - centres, axis=-1).mean() < e_hard.mean()


def test_decodes_fixed_cases_zero_rows_borders_ties_and_nan():
    H, W = 8, 10
    hm = np.zeros((1, 6, H, W))
    hm[0, 0] = -1.0                                                      # maximum <= 0: (0, 0)
    hm[0, 1, 3, 4], hm[0, 1, 3, 5], hm[0, 1, 4, 4] = 1.0, 0.5, 0.2       # quarter: +x (right higher), +y (below higher)
    hm[0, 2, 3, 4], hm[0, 2, 3, 3], hm[0, 2, 2, 4] = 1.0, 0.5, 0.2       # quarter: -x, -y
    hm[0, 3, 3, 1] = hm[0, 3, 5, 6] = 1.0                                # a tie: the first flat index, at x = 1 (not refined)
    hm[0, 4, 2, 2], hm[0, 4, 6, 6] = 1.0, np.nan                         # NaN is the maximum
    hm[0, 5, 3, 4] = 1.0                                                 # a symmetric peak: nothing moves
    q, m, idx = D64.quarter_decode(hm)
    assert q[0].tolist() == [[0, 0], [4.25, 3.25], [3.75, 2.75], [1, 3], [0, 0], [4, 3]]
    assert idx[0].tolist() == [0, 34, 34, 31, 66, 34] and np.isnan(m[0, 4, 0]) and m[0, 0, 0] == -1
    d, md, idxd = D64.dark_decode(hm, 5)
    assert np.array_equal(idx, idxd) and d[0, 0].tolist() == [0, 0] and d[0, 3].tolist() == [1, 3] and d[0, 4].tolist() == [0, 0]
    assert d[0, 1, 0] > 4 and d[0, 1, 1] > 3 and d[0, 2, 0] < 4 and d[0, 2, 1] < 3
    np.testing.assert_allclose(d[0, 5], [4, 3], atol=1e-12)


def test_labels_window_weights_and_the_quantised_form():
    kp = np.array([[50.3, 41.9], [2.0, 3.0], [-10.0, 10.0], [161.0, 40.0], [50.3, 41.9], [157.9, 93.9]])
    vis = np.array([1, 1, 1, 1, 0, 1], dtype=np.float32)
    t, w = D64.labels(kp, vis, 24, 40, 4.0, 4.0, 2.0, 6)
    assert w.tolist() == [1, 1, 0, 0, 0, 1] and not t[2].any() and not t[3].any() and not t[4].any()
    cx, cy = int(50.3 / 4 + 0.5), int(41.9 / 4 + 0.5)
    assert (cx, cy) == (13, 10)
    ys, xs = np.nonzero(t[0])
    assert xs.min() == cx - 6 and xs.max() == cx + 6 and ys.min() == cy - 6 and ys.max() == cy + 6
    assert t[0, 10, 13] == np.exp(-((13 - 50.3 / 4) ** 2 + (10 - 41.9 / 4) ** 2) / 8.0)
    # int() truncates towards zero, as in the reference: -3 / 4 + 0.5 = -0.25 -> 0, a centre INSIDE the map
    t2, w2 = D64.labels(np.array([[-3.0, 10.0]]), np.ones(1, np.float32), 24, 40, 4.0, 4.0, 2.0, 6)
    assert w2.tolist() == [1] and t2[0].any()
    tq, wq = D64.labels(kp, vis, 24, 40, 4.0, 4.0, 2.0, 6, subpixel=False)
    assert np.array_equal(wq, w) and tq[0, 10, 13] == 1.0 and tq[5].max() == 1.0


def test_names_defaults_and_refusals():
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    from uda_poseestimation_amd.data_gpu import TargetViewPipeline
    d = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}
    assert list(inspect.signature(kd.dark_decode).parameters) == ["batch_heatmaps", "kernel", "sigma"] and d(kd.dark_decode) == dict(kernel=11, sigma=None)
    assert list(inspect.signature(kd.quarter_decode).parameters) == ["batch_heatmaps"]
    assert d(kd.accuracy) == dict(hm_type="gaussian", thr=0.5, decode="argmax") and d(kd.accuracy_device) == dict(thr=0.5, decode="argmax")
    ps = inspect.signature(TargetViewPipeline.__init__).parameters
    assert list(ps)[-1] == "subpixel_labels" and ps["subpixel_labels"].default is False
    assert TargetViewPipeline().subpixel_labels is False and TargetViewPipeline(subpixel_labels=True).subpixel_labels is True
    x = torch.rand(2, 3, 8, 8)
    for call in (lambda: kd.dark_decode(x), lambda: kd.quarter_decode(x), lambda: kd.dark_decode(x, 5, 1.0), lambda: kd.accuracy(x, x, decode="dark"),
                 lambda: kd.accuracy_device(x, x, decode="quarter")):
        with pytest.raises(RuntimeError, match="MI355X") as e:
            call()
        assert "no CPU fallback" in str(e.value)
    big = torch.empty(1, 1, 91, 211)                       # DARK_MAX_PIXELS + 1 pixels
    assert kd.DARK_MAX_PIXELS + 1 == 91 * 211
    for bad in (lambda: kd.dark_decode(x, 4), lambda: kd.dark_decode(x, 1), lambda: kd.dark_decode(x, 33), lambda: kd.dark_decode(x, 5.5),
                lambda: kd.dark_decode(x, 11, float("inf")), lambda: kd.dark_decode(x, 11, float("nan")), lambda: kd.dark_decode(big),
                lambda: kd.dark_decode(big.numpy()), lambda: kd._decode_pred(x, "hard"), lambda: kd._decode_pred(x, "DARK")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="'quarter', 'dark'"):       # (the choice is judged before the device is touched)
        kd._decode_pred(x, "hard")


def test_the_header_declares_both_exports_and_states_the_bound_and_the_source_is_built():
    """(The prototypes against the ctypes rows: test_host_cpu.py::test_ctypes_signatures_and_policy_fields_match_the_header.)"""
    from uda_poseestimation_amd import _hip
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    hdr = open(os.path.join(ROOT, "include", "udapose.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"^int udapose_refine_decode\(void\* stream, const float\* hm, int R, int H, int W, int mode, int kernel, float sigma,\s*"
                     r"float\* coords, float\* maxvals,\s*int\* flat_idx\);", code, flags=re.M)
    assert re.search(r"^int udapose_gaussian_labels_subpixel\(void\* stream, const double\* kp, const float\* vis, float\* target, float\* weight, "
                     r"int R, int Hh, int Wh,\s*double stride_x, double stride_y, double sigma, int rad\);", code, flags=re.M)
    assert "udapose_refine_decode" in _hip.EXPORTS and "udapose_gaussian_labels_subpixel" in _hip.EXPORTS
    m = re.search(r"^#define UDAPOSE_REFINE_MAX_PIXELS (\d+)$", code, flags=re.M)
    assert m and int(m.group(1)) == kd.DARK_MAX_PIXELS and 2 * 4 * int(m.group(1)) <= 150 * 1024
    assert kd.DARK_MAX_PIXELS >= 96 * 96                    # 64x64 and 96x96 at every kernel size (the budget does not depend on it)
    for guard in ("max(g) > 0 is false", "det Hess == 0", "not finite"):
        assert guard in hdr, guard
    assert "refine.hip" in open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "Makefile")).read()
    losses_h = open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "losses.h")).read()
    assert losses_h.count("int refine_decode(") == 1
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`udapose_refine_decode`" in doc and "`udapose_gaussian_labels_subpixel`" in doc


def test_validate_and_the_trainer_keep_their_signatures():
    from uda_poseestimation_amd.engine import MeanTeacherTrainer, validate, validate_flip
    ps = inspect.signature(validate).parameters
    assert list(ps) == ["batches", "model", "criterion", "decode"] and ps["decode"].default == "argmax"
    pf = inspect.signature(validate_flip).parameters
    assert list(pf) == ["batches", "model", "flip_pairs", "criterion", "decode", "shift_heatmap"] and pf["decode"].default == "argmax"
    assert list(inspect.signature(MeanTeacherTrainer.__init__).parameters) == [
        "self", "student", "teacher", "lr", "teacher_alpha", "lambda_c", "mask_ratio", "sigma", "image_size", "heatmap_size", "use_sgd", "style_net",
        "recover", "s2t_freq", "t2s_freq", "s2t_alpha", "t2s_alpha", "rng", "occlude_rate", "occlude_thresh", "occlude_size", "image_px", "precision",
        "loss_scale_init", "loss_scale_interval", "grad_comm", "criterion", "con_criterion", "ent_criterion", "lambda_ent", "params", "warp_mode"]
