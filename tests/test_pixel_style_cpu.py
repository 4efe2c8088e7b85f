"""Histogram-matching and colour-statistics style nets, the parts that need no GPU: the numpy helper's integer statement of histogram matching
against the float recipe of scikit-image, its mean / std form against the oracle's calc_mean_std AdaIN, level recovery through the project's
normalisation, the three statements of the C ABI, and the refusals that are decided on the host."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import pixel_style_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NEW = ("udapose_pixel_summary_bytes", "udapose_pixel_summary", "udapose_pixel_transfer")


def _planes():
    """(name, content levels, style levels) of one plane each: random with few and many levels, one level, two levels, content == style."""
    rng = np.random.RandomState(11)
    out = []
    for i in range(40):
        nc, ns = rng.choice([3, 17, 256]), rng.choice([3, 40, 256])
        lc, ls = rng.choice(256, nc, replace=False), rng.choice(256, ns, replace=False)
        out.append((f"random{i}", lc[rng.randint(0, nc, (13, 11))], ls[rng.randint(0, ns, (13, 11))]))
    some = rng.randint(0, 256, (13, 11))
    out.append(("one-level content", np.full((13, 11), 7), some))
    out.append(("one-level style", some, np.full((13, 11), 200)))
    out.append(("one-level both", np.full((13, 11), 0), np.full((13, 11), 255)))
    out.append(("two-level style", some, np.where(rng.rand(13, 11) < 0.3, 10, 240)))
    out.append(("two-level content", np.where(rng.rand(13, 11) < 0.6, 0, 255), some))
    out.append(("content == style", some, some.copy()))
    return out


def test_integer_histogram_matching_equals_the_float_recipe():
    """The integer statement (cumulative counts decide the segment) against np.unique / cumsum / size / np.interp, from the histograms and from the
    pixels; float64 rounding of the quantiles is all that separates them."""
    for name, c, s in _planes():
        hc, hs = np.bincount(c.ravel(), minlength=256), np.bincount(s.ravel(), minlength=256)
        t_int, t_flt = R.hist_targets_int(hc, hs), R.hist_targets_interp(hc, hs)
        assert np.array_equal(np.isnan(t_int), hc == 0) and np.array_equal(np.isnan(t_flt), hc == 0), name
        assert np.nanmax(np.abs(t_int - t_flt)) <= 1e-12, name
        assert np.abs(t_int[c] - R.match_histograms_plane(c, s)).max() <= 1e-12, name
        occ = t_int[hc > 0]
        assert np.all(np.diff(occ) >= 0), name                                  # the table is non-decreasing
        assert occ.min() >= np.flatnonzero(hs)[0] and occ.max() <= np.flatnonzero(hs)[-1], name


def test_self_matching_is_the_identity_on_occupied_levels():
    rng = np.random.RandomState(3)
    for levels in (1, 2, 50, 256):
        lv = rng.choice(256, levels, replace=False)
        h = np.bincount(lv[rng.randint(0, levels, 500)], minlength=256)
        t = R.hist_targets_int(h, h)
        assert np.array_equal(t[h > 0], np.flatnonzero(h).astype(np.float64))     # exactly: (q - Cs[v_j]) == 0


def test_cdf_step_property_holds_for_the_helper_itself():
    for name, c, s in _planes():
        hc, hs = np.bincount(c.ravel(), minlength=256), np.bincount(s.ravel(), minlength=256)
        out = np.rint(R.hist_targets_int(hc, hs)[c]).astype(np.int64)
        assert R.cdf_step_violations(out, hc, hs) == 0, name


def test_meanstd_equals_the_oracles_adain_on_an_image():
    """oracle/style_ref.py's calc_mean_std-based AdaIN, given a [N, C, H, W] image of raw levels / 255 in float64 (used as data only)."""
    from oracle import style_ref
    rng = np.random.RandomState(5)
    lc, ls = rng.randint(0, 256, (2, 3, 9, 14)), rng.randint(40, 120, (2, 3, 9, 14))
    want = style_ref.adain_ref(torch.from_numpy(lc / 255.0), torch.from_numpy(ls / 255.0)).numpy() * 255.0 - lc
    got, mag = R.shift(lc, ls, "meanstd", eps=1e-5)
    assert np.abs(got - want).max() <= 1e-10 and np.all(mag >= np.abs(got) - 1e-10)
    same, _ = R.shift(lc, lc, "meanstd")
    assert np.abs(same).max() <= 1e-10
    got3, mag3 = R.shift(lc, lc, "cholesky")
    assert np.abs(got3).max() <= 1e-8                                           # L L^-1 = I
    # the Cholesky form moves the whole covariance: the transferred levels have the style's mean and covariance (eps aside)
    d3, _ = R.shift(lc, ls, "cholesky")
    for n in range(2):
        mu_t, S_t = R._moments(lc[n] + d3[n])
        mu_s, S_s = R._moments(ls[n])
        assert np.abs(mu_t - mu_s).max() <= 1e-9 and np.abs(S_t - S_s).max() <= 2e-4 * np.abs(S_s).max() + 2e-5


def test_levels_recover_every_byte_through_the_normalisation():
    b = np.tile(np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16), (1, 3, 1, 1))
    for mean, std in ((MEAN, STD), (None, None)):
        x = R.from_bytes(b, mean, std)
        R.assert_clear_of_ties(x, mean, std)
        assert np.array_equal(R.levels(x, mean, std), b)
        mu, sd = R.norm(3, mean, std)
        v = (x.astype(np.float64) * sd + mu) * 255.0
        assert np.abs(v - b).max() <= 1.6e-5
    wild = np.array([[[[np.inf, -np.inf, np.nan, 1e30, -1e30, 2.0, -0.3, 0.5]]]], np.float32)
    assert R.levels(wild).ravel().tolist() == [255, 0, 0, 255, 0, 255, 0, 128]
    with pytest.raises(AssertionError, match="half level"):
        R.assert_clear_of_ties(np.array([[[[0.5 / 255.0]]]], np.float32))
    s = R.summary(R.from_bytes(b, MEAN, STD), MEAN, STD)
    assert s.dtype == np.int32 and s.shape == (1, 776) and np.all(s[:, :768] == 1) and np.all(s[:, 774:] == 0)
    assert s[:, 768:774].copy().view(np.int64).ravel().tolist() == [int((np.arange(256) ** 2).sum())] * 3


def test_abi_is_declared_defined_and_bound():
    from uda_poseestimation_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "udapose.h")).read()
    capi = open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "capi.hip")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert re.search(r"\b" + name + r"\s*\(", capi), name
        assert name in _hip._SIGS and name in _hip.EXPORTS
        for kind in ("bf16", "fp16"):
            assert hasattr(_hip.lib(kind), name)
    assert "UDAPOSE_PIXEL_SHARE" in hdr and "low word first" in hdr and "rint(" in hdr          # the layout and the level rule are stated
    from uda_poseestimation_amd.lib.models import pixel_style as ps
    share = int(re.search(r"#define\s+UDAPOSE_PIXEL_SHARE\s+(\d+)", hdr).group(1))
    max_hw = int(re.search(r"#define\s+UDAPOSE_PIXEL_MAX_HW\s+(\d+)", hdr).group(1))
    assert (ps.SHARE, ps.MAX_HW) == (share, max_hw) and max_hw == 2 ** 24
    for mode, code_ in ps.MODES.items():
        assert int(re.search(r"#define\s+UDAPOSE_PIXEL_" + mode.upper() + r"\s+(\d+)", hdr).group(1)) == code_


def test_bad_arguments_are_refused_by_the_library():
    """Every refusal is decided on the host before anything is enqueued: the calls below never touch a device (the pointers are not even mapped)."""
    from uda_poseestimation_amd import _hip
    lib = _hip.lib()
    ARG, UNSUP = -1, -3
    P = 4096                                                                    # a non-null, 8-byte aligned, never dereferenced pointer
    assert lib.udapose_pixel_summary_bytes(32, 3) == 32 * 776 * 4 and lib.udapose_pixel_summary_bytes(2, 4) == 2 * 1024 * 4
    assert lib.udapose_pixel_summary_bytes(0, 3) == ARG and lib.udapose_pixel_summary_bytes(1, 0) == ARG
    summ = lambda *a: lib.udapose_pixel_summary(None, *a)
    assert summ(None, 1, 3, 4, 4, None, None, P) == ARG and summ(P, 1, 3, 4, 4, None, None, None) == ARG
    assert summ(P, 0, 3, 4, 4, None, None, P) == ARG and summ(P, 1, 0, 4, 4, None, None, P) == ARG and summ(P, 1, 3, 0, 4, None, None, P) == ARG
    assert summ(P, 1, 3, 4096, 4097, None, None, P) == UNSUP                  # H W > 2^24
    assert summ(P, 1, 3, 4, 4, P, None, P) == ARG                              # mean without std
    assert summ(P, 1, 3, 4, 4, None, None, P + 4) == ARG                       # the summary holds 64-bit sums
    tr = lambda c, sc, ss, o, N, C, H, W, mode, eps=1e-5, lo=None, hi=None: lib.udapose_pixel_transfer(None, c, sc, ss, o, N, C, H, W, mode, eps, 1.0, None, lo,
                                                                                                      hi, None, None)
    for args in ((None, P, P, P), (P, None, P, P), (P, P, None, P), (P, P, P, None)):
        assert tr(*args, 1, 3, 4, 4, 0) == ARG
    assert tr(P, P, P, P, 0, 3, 4, 4, 0) == ARG and tr(P, P, P, P, 1, 3, 4, 0, 0) == ARG
    assert tr(P, P, P, P, 1, 3, 4096, 4097, 0) == UNSUP
    assert tr(P, P, P, P, 1, 4, 4, 4, 2) == ARG and tr(P, P, P, P, 1, 1, 4, 4, 2) == ARG       # cholesky with C != 3
    assert tr(P, P, P, P, 1, 3, 4, 4, 3) == ARG and tr(P, P, P, P, 1, 3, 4, 4, -1) == ARG      # unknown mode
    assert tr(P, P, P, P, 1, 3, 1, 1, 1) == ARG and tr(P, P, P, P, 1, 3, 1, 1, 2) == ARG       # no unbiased variance of one pixel
    assert tr(P, P, P, P, 1, 3, 4, 4, 1, eps=0.0) == ARG and tr(P, P, P, P, 1, 3, 4, 4, 2, eps=float("nan")) == ARG
    assert tr(P, P, P, P, 1, 3, 4, 4, 0, lo=P) == ARG                          # lo without hi


def test_module_refuses_cpu_tensors_and_bad_arguments():
    import uda_poseestimation_amd.lib.models as models
    from uda_poseestimation_amd.lib.models import pixel_style as ps
    x = torch.rand(1, 3, 8, 8)
    net = ps.PixelStyleNet("hist", MEAN, STD)
    assert len(list(net.parameters())) == 0 and len(list(net.buffers())) == 0 and ps.PixelStyleNet.spectrum is ps.PixelStyleNet.summary
    with pytest.raises(RuntimeError, match="MI355X"):
        net(x, x)
    with pytest.raises(RuntimeError, match="MI355X"):
        net.summary(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        ps.level_histograms(x, MEAN, STD)
    with pytest.raises(RuntimeError, match="MI355X"):
        ps.pixel_style_transfer(x, x, mode="meanstd")
    with pytest.raises(TypeError, match="tensor"):
        net.summary(x.numpy())
    with pytest.raises(ValueError, match="one of"):
        ps.PixelStyleNet("pca")
    with pytest.raises(ValueError, match="go together"):
        ps.PixelStyleNet("hist", mean=MEAN)
    with pytest.raises(ValueError, match="positive"):
        ps.PixelStyleNet("hist", MEAN, (0.2, 0.0, 0.2))
    with pytest.raises(ValueError, match="positive"):
        ps.PixelStyleNet("meanstd", eps=0.0)
    assert ps.summary_words(3) == 776 and ps.summary_words(4) == 1024 and ps.summary_words(1) == 256
    # the architecture list that train_human.py discovers in lib.models stays as it was
    names = sorted(n for n in models.__dict__ if n.islower() and not n.startswith("__") and callable(models.__dict__[n]))
    assert names == ["pose_resnet101", "pose_resnet50"]
