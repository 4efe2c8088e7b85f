"""The merge of teacher views by agreement, without a GPU: the numpy restatement (tests/helpers/view_merge_ref.py) against planes worked by
hand, the declaration in every place the ABI lives, the trainer's switches and the refusals that need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from helpers import view_merge_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 8


def _one(name, k=3, **kw):
    """The restatement on one constructed plane -> Merged with the plane dimension dropped."""
    m = REF.merge(list(REF.constructed_plane(name, k, H, W)[:, None]), REF.CONSTRUCTED_RADIUS, **kw)
    return m, [tuple(int(c) for c in m.peaks[v, 0]) for v in range(k)]


def test_three_views_with_one_outlier():
    planes = REF.constructed_plane("outlier", 3, H, W)
    m, peaks = _one("outlier", mode="trimmed", min_views=2, want_energy=True)
    assert peaks == [(2, 3), (2, 3), (7, 7)] and m.maxvals[:, 0].tolist() == [1.0, 1.125, 0.75]
    # d2 = 41 between the pair and the outlier: sums 41, 41, 82 - views 0 and 1 tie and view 0 is the medoid; 41 > 2 * 2
    assert (int(m.inliers[0]), int(m.n_inliers[0]), int(m.spread2[0]), float(m.agree[0])) == (0b011, 2, 41, 1.0)
    assert m.mean[0, 3, 2] == np.float32(1.0625) and m.mean[0, 7, 7] == 0.0           # the outlier's bump is gone
    assert float(_one("outlier", mode="trimmed")[0].agree[0]) == 0.0                   # min_views defaults to k = 3
    plain = _one("outlier", mode="mean")[0]
    assert plain.mean[0, 3, 2] == (np.float32(1.0) + np.float32(1.125)) / np.float32(3) and plain.mean[0, 7, 7] == np.float32(0.25)
    assert int(plain.inliers[0]) == 0b011                                              # the decision does not depend on the mode
    # energy: the fp64 population variance over the three views, averaged over the 64 pixels (two pixels are not constant)
    want = (np.var([1.0, 1.125, 0.0]) + np.var([0.0, 0.0, 0.75])) / 64
    assert abs(float(m.energy[0]) - want) <= 1e-15 and float(m.energy_abs[0]) > 0
    assert np.array_equal(m.mean[0], ((planes[0] + planes[1]) / np.float32(2)))


def test_equal_maxima_resolve_to_the_first_flat_index():
    m, peaks = _one("first_index_tie")
    # view 0 holds 0.5 at (y, x) = (1, 4), (2, 3) and (7, 1): flat index 12 is the first
    assert peaks == [(4, 1), (3, 2), (3, 2)] and m.maxvals[:, 0].tolist() == [0.5, 0.5, 0.5]
    # d2(0, 1) = 2: sums 4, 2, 2 - view 1 is the medoid (the lower of the tied pair), all within the radius
    assert (int(m.inliers[0]), int(m.n_inliers[0]), int(m.spread2[0]), float(m.agree[0])) == (0b111, 3, 2, 1.0)


def test_a_medoid_tie_resolves_to_the_lowest_view():
    m, peaks = _one("medoid_tie", mode="trimmed")
    assert peaks == [(0, 0), (2, 0), (1, 3)]
    # d2: (0,1) = 4, (0,2) = 10, (1,2) = 10: sums 14, 14, 20 - view 0; view 1 is exactly on the radius, view 2 outside
    assert (int(m.inliers[0]), int(m.n_inliers[0]), int(m.spread2[0]), float(m.agree[0])) == (0b011, 2, 10, 0.0)
    # had view 1 been the medoid the mask would be the same here; the spread tells the planes apart from a two-view case
    two, peaks2 = _one("medoid_tie", k=2)
    assert peaks2 == [(0, 0), (2, 0)] and (int(two.inliers[0]), int(two.spread2[0])) == (0b11, 4)      # sums 4, 4: view 0


def test_a_pair_exactly_on_the_radius_is_inside():
    m, peaks = _one("on_radius")
    assert peaks == [(2, 1), (4, 1), (2, 1)]
    assert (int(m.inliers[0]), int(m.n_inliers[0]), int(m.spread2[0]), float(m.agree[0])) == (0b111, 3, 4, 1.0)      # (float)4 <= 2.f * 2.f
    planes = list(REF.constructed_plane("on_radius", 3, H, W)[:, None])
    below = REF.merge(planes, np.nextafter(np.float32(2.0), np.float32(0.0)))
    assert (int(below.inliers[0]), float(below.agree[0])) == (0b101, 0.0)
    assert int(REF.merge(planes, float("inf")).inliers[0]) == 0b111 and int(REF.merge(planes, 0.0).inliers[0]) == 0b101
    pair = REF.merge(list(REF.constructed_plane("on_radius", 2, H, W)[:, None]), 2.0)
    assert (int(pair.inliers[0]), int(pair.spread2[0])) == (0b11, 4)


def test_an_all_non_positive_view_is_invalid():
    m, peaks = _one("invalid_view", mode="trimmed")
    assert peaks == [(1, 1), (3, 3), (3, 3)] and m.maxvals[:, 0].tolist() == [0.0, 1.0, 1.0]           # the raw peak is still reported
    assert (int(m.inliers[0]), int(m.n_inliers[0]), int(m.spread2[0]), float(m.agree[0])) == (0b110, 2, 0, 0.0)
    assert float(_one("invalid_view", min_views=2)[0].agree[0]) == 1.0
    assert m.mean[0, 3, 3] == 1.0 and m.mean[0, 0, 0] == 0.0                                            # view 0's floor of -1 is not averaged in
    assert _one("invalid_view", mode="mean")[0].mean[0, 0, 0] == np.float32(-1.0) / np.float32(3)


def test_no_valid_view_gives_the_plain_mean_and_no_agreement():
    m, peaks = _one("none_valid", mode="trimmed", min_views=1)
    assert peaks == [(0, 0), (1, 0), (2, 0)] and m.maxvals[:, 0].tolist() == [0.0, -0.25, 0.0]          # maxima of 0 and below: no view is valid
    assert (int(m.inliers[0]), int(m.n_inliers[0]), int(m.spread2[0]), float(m.agree[0])) == (0, 0, 0, 0.0)
    assert np.array_equal(m.mean, _one("none_valid", mode="mean", min_views=1)[0].mean)
    k1 = REF.merge([np.full((2, 1, 1), -1.0, np.float32)], 2.0)                                         # k = 1, 1 x 1 planes
    assert k1.agree.tolist() == [0.0, 0.0] and np.array_equal(k1.mean, np.full((2, 1, 1), -1.0, np.float32))
    ok = REF.merge([np.full((1, 1, 1), 0.5, np.float32)], 0.0)
    assert (ok.agree.tolist(), ok.inliers.tolist(), ok.peaks.tolist()) == ([1.0], [1], [[[0, 0]]])     # k = 1: agree is the view's validity


def test_the_mean_is_the_fp32_sequence_in_view_order():
    rng = np.random.RandomState(0)
    vs = [rng.uniform(0.1, 1.0, (2, 3, 4, 4)).astype(np.float32) * np.float32(10.0 ** rng.randint(-3, 3)) for _ in range(5)]
    m = REF.merge(vs, float("inf"), mode="trimmed")            # every view is valid and inside: trimmed == mean
    want = ((((vs[0] + vs[1]) + vs[2]) + vs[3]) + vs[4]) / np.float32(5)
    assert m.mean.dtype == np.float32 and np.array_equal(m.mean, want) and np.array_equal(m.mean, REF.merge(vs, 0.0, mode="mean").mean)
    t = torch.stack([torch.from_numpy(v) for v in vs]).mean(0).numpy()          # ATen's mean over a handful of rows: the same bits
    assert np.array_equal(m.mean, t)
    assert m.peaks.shape == (5, 2, 3, 2) and m.maxvals.shape == (5, 2, 3) and m.agree.shape == (2, 3)


def test_the_call_is_declared_bound_built_and_documented():
    from uda_poseestimation_amd import _hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "udapose.h")).read(), flags=re.S)
    assert re.search(r"^int udapose_view_merge\(void\* stream, const float\* const\* h_views, int k, int R, int H, int W, int mode, "
                     r"const float\* radius_dev, int min_views,\s+float\* mean, int\* peaks, float\* maxvals, int\* inliers, int\* n_inliers, "
                     r"int\* spread2, float\* agree, float\* energy\);", hdr, flags=re.M)
    assert re.search(r"^#define UDAPOSE_MERGE_MEAN 0$", hdr, flags=re.M) and re.search(r"^#define UDAPOSE_MERGE_TRIMMED 1$", hdr, flags=re.M)
    vp, ci = C.c_void_p, C.c_int
    assert _hip._SIGS["udapose_view_merge"] == (ci, [vp, vp, ci, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp])
    assert "udapose_view_merge" in _hip.EXPORTS
    csrc = os.path.join(ROOT, "uda_poseestimation_amd", "csrc")
    assert "int udapose_view_merge(" in open(os.path.join(csrc, "capi.hip")).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "view_merge.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "-DUDAPOSE_ELEM_F16" in mk and "$(SRCS:%.hip=build_f16/%.o)" in mk          # (both element-type builds compile every source)
    for kind in ("bf16", "fp16"):
        if os.path.exists(_hip.LIB_PATHS[kind]):
            assert hasattr(C.CDLL(_hip.LIB_PATHS[kind]), "udapose_view_merge"), kind
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.17" in design and "udapose_view_merge" in design and "GraphedTrainStep" in design.split("4.17", 1)[1]
    assert "view_merge" in open(os.path.join(ROOT, "README.md")).read()
    assert "`udapose_view_merge`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_trainer_switch_defaults_and_unchanged_constructor():
    from uda_poseestimation_amd import warp
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    src = inspect.getsource(MeanTeacherTrainer.__init__)
    assert "self.view_merge, self.view_radius, self.view_min = None, 2.0, None" in src
    params = list(inspect.signature(MeanTeacherTrainer.__init__).parameters)
    assert not {"view_merge", "view_radius", "view_min"} & set(params)
    assert params == ["self", "student", "teacher", "lr", "teacher_alpha", "lambda_c", "mask_ratio", "sigma", "image_size", "heatmap_size", "use_sgd",
                      "style_net", "recover", "s2t_freq", "t2s_freq", "s2t_alpha", "t2s_alpha", "rng", "occlude_rate", "occlude_thresh",
                      "occlude_size", "image_px", "precision", "loss_scale_init", "loss_scale_interval", "grad_comm", "criterion", "con_criterion",
                      "ent_criterion", "lambda_ent", "params", "warp_mode"]
    assert warp.MERGE_MODES == {"mean": 0, "trimmed": 1}
    assert list(inspect.signature(warp.merge_views).parameters) == ["views", "radius", "mode", "min_views", "want_energy"]
    assert warp.MergedViews._fields == ("mean", "peaks", "maxvals", "inliers", "n_inliers", "spread2", "agree", "energy")
    assert "view_merge" in inspect.getsource(GraphedTrainStep._refuse_uncapturable) and "ValueError" in inspect.getsource(GraphedTrainStep._refuse_uncapturable)
    # the step-time checks need no device: a mode the merge does not know, and fewer than two views
    tr = MeanTeacherTrainer.__new__(MeanTeacherTrainer)
    tr.view_merge = None
    tr._check_view_merge(1)
    tr.view_merge = "trimmed"
    tr._check_view_merge(2)
    with pytest.raises(ValueError, match="at least two"):
        tr._check_view_merge(1)
    tr.view_merge = "median"
    with pytest.raises(ValueError, match="view_merge"):
        tr._check_view_merge(3)


def test_cpu_tensors_and_bad_arguments_are_refused_before_any_launch():
    from uda_poseestimation_amd import warp
    v = torch.zeros(1, 2, 4, 4)
    with pytest.raises(RuntimeError, match="MI355X"):
        warp.merge_views([v, v])
    with pytest.raises(RuntimeError, match="MI355X"):
        warp.merge_views([v])
    with pytest.raises(NotImplementedError, match="at most 8"):
        warp.merge_views([v] * 9)
    with pytest.raises(ValueError, match="mode"):
        warp.merge_views([v, v], mode="median")
    with pytest.raises(ValueError, match="min_views"):
        warp.merge_views([v, v], min_views=3)
    with pytest.raises(ValueError, match="min_views"):
        warp.merge_views([v, v], min_views=0)
    with pytest.raises(ValueError, match="no views"):
        warp.merge_views([])
