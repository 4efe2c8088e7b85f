"""Evaluation report, host side (no GPU): the fp32 restatement the device tests compare with (tests/helpers/pck_curve_ref.py) against
the reference's own accuracy() recorded in tests/golden/pck_curve.npz, its batch-split invariance, PCKMeter.report on hand-made states,
the group tables against the fixture recorded from the reference's dataset classes, threshold validation, the refusal of CPU tensors
and the declarations."""
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import pck_curve_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _kd():
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    return kd


# ---------------------------------------------------------------------------------------------- the restatement against the reference
def test_default_curve_is_the_recorded_one():
    kd = _kd()
    g = np.load(os.path.join(GOLD, "pck_curve.npz"))
    assert len(kd.PCK_THRESHOLDS) == 20 and kd.PCK_THRESHOLDS[9] == 0.5
    assert np.array_equal(np.asarray(kd.PCK_THRESHOLDS), g["thresholds"])
    assert [str(n) for n in g["names"]] == [c[0] for c in R.GOLDEN_CASES]


@pytest.mark.parametrize("case", R.GOLDEN_CASES, ids=lambda c: c[0])
def test_restatement_reproduces_the_reference_accuracy(case):
    """acc, avg_acc and cnt of the reference's accuracy() for all 20 thresholds, from the fp32 state: ratios of the same integers."""
    kd = _kd()
    name, shape, seed = case
    g = np.load(os.path.join(GOLD, "pck_curve.npz"))
    out, tgt = g[name + "/output"], g[name + "/target"]
    assert out.shape == shape and np.array_equal(out, R.golden_inputs(shape, seed)[0]) and np.array_equal(tgt, R.golden_inputs(shape, seed)[1])
    T = len(kd.PCK_THRESHOLDS)
    s = R.state_fp32_heatmaps(out, tgt, np.asarray(kd.PCK_THRESHOLDS, dtype=np.float32))
    count = s[:, T]
    assert (count == 0).any() and ((count > 0) & (count < shape[0])).any()      # hidden everywhere / in some samples
    rep = kd.PCKMeter.report(torch.from_numpy(s), kd.PCK_THRESHOLDS)
    acc = np.where(np.isnan(rep["pck"]), -1.0, rep["pck"]).T                     # the reference writes -1 for an absent joint
    assert np.abs(acc - g[name + "/acc"]).max() <= 1e-12
    assert np.abs(rep["pck_mean"] - g[name + "/avg_acc"]).max() <= 1e-12
    assert np.array_equal(np.full(T, (count > 0).sum()), g[name + "/cnt"])


def test_12x20_pins_the_tie_and_the_size_pairing():
    """dy = 1 and dy = 2 with dx = 0 on a 12 x 20 map: d = 0.5 and 1.0 exactly (y over nw = W / 10 = 2), a miss at the equal threshold."""
    thr = np.asarray(_kd().PCK_THRESHOLDS, dtype=np.float32)
    gt = np.array([[[5, 5], [5, 5]]], dtype=np.float32)
    pred = np.array([[[5, 6], [5, 7]]], dtype=np.float32)
    s = R.state_fp32(pred, gt, thr, 12 / 10.0, 20 / 10.0)
    assert s[0, :20].tolist() == [0] * 10 + [1] * 10 and s[1, :20].tolist() == [0] * 20      # 0.5 < thr[j] from j = 10; 1.0 < nothing
    s = R.state_fp32(pred[..., ::-1].copy(), gt, thr, 12 / 10.0, 20 / 10.0)                    # x over nh = 1.2: 0.8333, 1.6667
    assert s[0, :20].tolist() == [0] * 16 + [1] * 4 and s[1, :20].sum() == 0


def test_restatement_is_invariant_to_the_batch_split():
    rs = np.random.RandomState(3)
    pred = rs.uniform(0, 32, (12, 7, 2)).astype(np.float32)
    gt = rs.uniform(0, 32, (12, 7, 2)).astype(np.float32)
    gt[rs.rand(12, 7) < 0.2] = 0
    pred[3, 2], gt[3, 2] = np.nan, 5
    thr = np.asarray(_kd().PCK_THRESHOLDS, dtype=np.float32)
    whole = R.state_fp32(pred, gt, thr, 3.2, 3.2)
    parts = sum(R.state_fp32(pred[a:b], gt[a:b], thr, 3.2, 3.2) for a, b in ((0, 5), (5, 9), (9, 12)))
    assert np.array_equal(whole, parts) and whole[:, 20].sum() > 0 and whole[2, 22] == 1
    n = rs.uniform(2, 9, 12).astype(np.float32)
    whole = R.state_fp32(pred, gt, thr, 3.2, 3.2, norm=n)
    parts = sum(R.state_fp32(pred[a:b], gt[a:b], thr, 3.2, 3.2, norm=n[a:b]) for a, b in ((0, 5), (5, 9), (9, 12)))
    assert np.array_equal(whole, parts)


def test_hits_equal_independent_compares_with_a_bisection():
    """The device finds the first hit by bisection: on an ascending table that is the T independent compares the restatement makes."""
    rs = np.random.RandomState(4)
    thr = np.sort(rs.uniform(0.01, 2, 64).astype(np.float32))
    d = np.concatenate([rs.uniform(0, 2.2, 500).astype(np.float32), thr[:8], [np.float32(np.nan), np.float32(np.inf), np.float32(0)]])
    for T in (1, 7, 64):
        t = thr[:T]
        for v in d:
            lo, hi = 0, T
            while lo < hi:
                mid = (lo + hi) >> 1
                lo, hi = (lo, mid) if v < t[mid] else (mid + 1, hi)
            assert np.array_equal(np.arange(T) >= lo, v < t)


# ---------------------------------------------------------------------------------------------- report() on hand-made states
def _state(rows):
    return torch.tensor(rows, dtype=torch.int64)


def test_report_leaves_an_unseen_joint_out():
    kd = _kd()
    rep = kd.PCKMeter.report(_state([[1, 2, 4, 3 * 65536, 0], [0, 0, 0, 0, 0], [3, 3, 4, 65536 // 2, 0]]), [0.1, 0.3])
    assert rep["thresholds"] == (0.1, 0.3) and rep["count"].tolist() == [4, 0, 4] and rep["nonfinite"].tolist() == [0, 0, 0]
    assert np.array_equal(rep["pck"][[0, 2]], [[0.25, 0.5], [0.75, 0.75]]) and np.isnan(rep["pck"][1]).all()
    assert np.array_equal(rep["pck_mean"], [0.5, 0.625])                         # joints 0 and 2 only: the reference's avg_acc
    assert np.array_equal(rep["pck_micro"], [0.5, 0.625])
    assert rep["epe"][0] == 0.75 and np.isnan(rep["epe"][1]) and rep["epe"][2] == 0.125 and rep["epe_mean"] == 0.4375
    assert np.isnan(rep["auc_per_joint"][1]) and "groups" not in rep
    empty = kd.PCKMeter.report(_state([[0, 0, 0, 0, 0]]), [0.1, 0.3])
    assert empty["pck_mean"].tolist() == [0.0, 0.0] and np.isnan(empty["pck_micro"]).all() and np.isnan(empty["epe_mean"])


def test_report_micro_and_macro_means_differ_with_unequal_counts():
    rep = _kd().PCKMeter.report(_state([[1, 1, 0, 0], [6, 8, 0, 0]]), [0.5])
    assert rep["pck_mean"].tolist() == [0.875] and rep["pck_micro"].tolist() == [7 / 9]


def test_report_auc_of_a_staircase():
    kd = _kd()
    # pck = 0, 0.5, 0.5, 1 at thresholds 0.1, 0.2, 0.4, 0.5: trapezoids 0.025 + 0.1 + 0.075 = 0.2 over a range of 0.4
    rep = kd.PCKMeter.report(_state([[0, 2, 2, 4, 4, 0, 0]]), [0.1, 0.2, 0.4, 0.5])
    assert rep["auc"] == pytest.approx(0.5, abs=1e-15) and rep["auc_per_joint"][0] == pytest.approx(0.5, abs=1e-15)
    one = kd.PCKMeter.report(_state([[2, 4, 0, 0]]), [0.5])
    assert one["auc"] is None and one["auc_per_joint"] is None and one["pck"].tolist() == [[0.5]]
    full = kd.PCKMeter.report(_state([[4, 4, 4, 0, 0]]), [0.05, 1.0])
    assert full["auc"] == 1.0


def test_report_epe_skips_nonfinite_pairs_and_scales_pixels():
    kd = _kd()
    s = _state([[0, 5, 6 * 65536, 2], [0, 2, 0, 2]])                              # joint 0: 3 finite pairs, 6 px in all; joint 1: none finite
    rep = kd.PCKMeter.report(s, [0.5])
    assert rep["epe"][0] == 2.0 and np.isnan(rep["epe"][1]) and rep["epe_mean"] == 2.0 and rep["nonfinite"].tolist() == [2, 2]
    assert kd.PCKMeter.report(s, [0.5], pixel_scale=4.0)["epe"][0] == 8.0
    assert kd.PCKMeter.report(_state([[0, 1, 1, 0]]), [0.5])["epe"][0] == 2.0 ** -16


def test_report_groups_are_plain_means():
    kd = _kd()
    s = _state([[1, 2, 4, 4 * 65536, 0], [2, 4, 4, 8 * 65536, 0], [0, 0, 0, 0, 0]])
    rep = kd.PCKMeter.report(s, [0.1, 0.3], groups={"a": (0, 1), "b": (1,), "c": (0, 2)})
    assert list(rep["groups"]) == ["a", "b", "c"]
    assert np.array_equal(rep["groups"]["a"]["pck"], [0.375, 0.75]) and rep["groups"]["a"]["epe"] == 1.5
    assert rep["groups"]["a"]["auc"] == pytest.approx((0.375 + 0.75) / 2)
    assert np.array_equal(rep["groups"]["b"]["pck"], [0.5, 1.0]) and rep["groups"]["b"]["epe"] == 2.0
    assert np.isnan(rep["groups"]["c"]["pck"]).all() and np.isnan(rep["groups"]["c"]["epe"])      # an unseen joint has no value to average
    named = kd.PCKMeter.report(torch.zeros(16, 5, dtype=torch.int64), [0.1, 0.3], groups="body16")
    assert list(named["groups"]) == list(kd.JOINT_GROUPS["body16"])
    with pytest.raises(ValueError):
        kd.PCKMeter.report(s, [0.1, 0.3], groups="body17")
    with pytest.raises(ValueError):
        kd.PCKMeter.report(s, [0.1, 0.3], groups={"a": (3,)})
    with pytest.raises(ValueError):
        kd.PCKMeter.report(s, [0.1, 0.3, 0.5])                                   # the state's width does not fit the thresholds
    with pytest.raises(ValueError):
        kd.PCKMeter.report(s.to(torch.int32), [0.1, 0.3])


# ---------------------------------------------------------------------------------------------- tables
def test_group_tables_equal_the_fixture():
    kd = _kd()
    with open(os.path.join(GOLD, "joint_groups.json")) as fh:
        fix = json.load(fh)
    assert set(kd.JOINT_GROUPS) == set(kd.FLIP_PAIRS) == set(fix)
    for layout, table in fix.items():
        assert list(kd.JOINT_GROUPS[layout]) == list(table), layout             # the reference's order of names
        for name, idx in table.items():
            assert kd.JOINT_GROUPS[layout][name] == tuple(idx), (layout, name)


def test_group_accuracy_is_the_reference_rule():
    kd = _kd()
    acc = [float(i) for i in range(16)]
    got = kd.group_accuracy(acc, "body16")
    assert list(got) == ["head", "shoulder", "elbow", "wrist", "hip", "knee", "ankle", "all"]
    assert got["head"] == 9.0 and got["shoulder"] == 12.5 and got["ankle"] == 2.5 and got["all"] == sum((12, 13, 11, 14, 10, 15, 2, 3, 1, 4, 0, 5)) / 12
    assert kd.group_accuracy([0.5, -1.0, 1.0], {"x": (0, 1), "y": [2]}) == {"x": -0.25, "y": 1.0}      # a plain mean: a -1 is averaged in
    with pytest.raises(ValueError):
        kd.group_accuracy(acc, "body17")
    with pytest.raises(ValueError):
        kd.group_accuracy(acc, {"x": ()})


# ---------------------------------------------------------------------------------------------- construction and refusals
@pytest.mark.parametrize("bad", [
    [0.5, 0.25], [0.1, 0.1], [0.1, 0.1 + 1e-10], [0.0, 0.5], [-0.1, 0.5], [0.1, float("nan")], [0.1, float("inf")], [1e-50, 0.5], [0.1, 1e39], [],
    [0.01 * j for j in range(1, 66)]], ids=["unsorted", "duplicate", "duplicate-as-fp32", "zero", "negative", "nan", "inf", "zero-as-fp32",
                                            "inf-as-fp32", "none", "65"])
def test_bad_thresholds_are_refused_at_construction(bad):
    with pytest.raises(ValueError):
        _kd().PCKMeter(16, bad)


def test_good_thresholds_and_key_point_counts():
    kd = _kd()
    assert np.array_equal(kd._check_thresholds([0.01 * j for j in range(1, 65)]), np.asarray([0.01 * j for j in range(1, 65)], dtype=np.float32))
    assert kd._check_thresholds((0.5,)).dtype == np.float32
    for K in (0, 257):
        with pytest.raises(ValueError):
            kd.PCKMeter(K)


def test_meter_refuses_cpu_tensors():
    """With or without a GPU (without one the meter is made without device memory, and has no state to show)."""
    kd = _kd()
    m = kd.PCKMeter(2, [0.5])
    hm = torch.zeros(1, 2, 4, 4)
    with pytest.raises(RuntimeError, match="MI355X"):
        m.update(hm, hm)
    with pytest.raises(RuntimeError, match="MI355X"):
        m.update(hm, target_coords=torch.zeros(1, 2, 2), decode="dark")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="MI355X"):
            m.state()
    with pytest.raises(RuntimeError, match="MI355X"):
        kd.PCKMeter(2, [0.5], device="cpu")


def test_update_checks_its_arguments_before_the_device(monkeypatch):
    """Argument errors and CPU tensors are refused before anything is launched: the library is never asked for."""
    kd = _kd()
    monkeypatch.setattr(kd, "lib", lambda *a, **k: pytest.fail("a launch was attempted"))
    m = kd.PCKMeter.__new__(kd.PCKMeter)
    m.num_keypoints, m._thr32, m.thresholds, m._state, m._thr = 2, kd._check_thresholds([0.5]), (0.5,), None, None
    hm = torch.zeros(1, 2, 4, 4)
    with pytest.raises(ValueError):
        m.update(hm)                                                             # neither target nor target_coords
    with pytest.raises(ValueError):
        m.update(hm, hm, target_coords=torch.zeros(1, 2, 2))                     # both
    with pytest.raises(ValueError):
        m.update(hm, hm, visible=torch.ones(1, 2))                               # visible without coordinates
    with pytest.raises(RuntimeError, match="MI355X"):
        m.update(hm, hm)


# ---------------------------------------------------------------------------------------------- declarations
def test_exports_are_declared_defined_and_bound():
    from uda_poseestimation_amd import _hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "udapose.h")).read(), flags=re.S)
    capi = open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "capi.hip")).read()
    vp, ci, cf = _hip.vp, _hip.ci, _hip.cf
    want = {"udapose_pck_accumulate": [vp, vp, vp, vp, vp, ci, ci, cf, cf, vp, ci, vp],
            "udapose_pck_accumulate_heatmaps": [vp, vp, vp, vp, ci, ci, ci, ci, vp, ci, vp, vp]}
    for name, args in want.items():
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, flags=re.M), f"{name} is not declared in include/udapose.h"
        assert f"int {name}(" in capi, f"capi.hip does not define 'int {name}('"
        assert name in _hip.EXPORTS and _hip._SIGS[name] == (ci, args)
        assert hasattr(_hip.lib("bf16"), name) and hasattr(_hip.lib("fp16"), name)
    assert "long long* state" in hdr
    for macro, value in (("UDAPOSE_PCK_MAX_THRESHOLDS", 64), ("UDAPOSE_PCK_MAX_KEYPOINTS", 256), ("UDAPOSE_PCK_EPE_SCALE", 65536)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", hdr)
    kd = _kd()
    assert (kd.PCK_MAX_THRESHOLDS, kd.PCK_EPE_SCALE) == (64, 65536)
