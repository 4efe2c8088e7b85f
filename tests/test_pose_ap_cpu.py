"""The key-point AP meter without a GPU: the numpy restatement (tests/helpers/pose_ap_ref.py) on hand-worked cases, the
report's names, what the Python layer refuses on the host, and the four exports declared, bound, built and documented."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import pose_ap_ref as ap
from helpers import pose_nms_ref as ref
from uda_poseestimation_amd.lib.keypoint_detection import APMeter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("udapose_ap_match_ws_bytes", "udapose_ap_match", "udapose_ap_curve_ws_bytes", "udapose_ap_curve")
K = 17
SIG = (ref.SIGMA,) * K
AREA = ref.SIDE * ref.SIDE
ALL = {"all": (0, 1e10)}
ONE = 1.0 / (1.0 + np.spacing(1))      # precision without a false positive: tp / (fp + tp + np.spacing(1))


def _meter(**kw):
    kw.setdefault("thresholds", (0.5,))
    kw.setdefault("area_ranges", ALL)
    return ap.APRef(K, SIG, **kw)


def _feed(meter, dets, scores, labels, areas=None, visible=None, **kw):
    G = len(labels)
    meter.update(np.stack(dets), np.asarray(scores, np.float32), np.zeros(len(dets), np.int32), np.stack(labels),
                 np.ones((G, K), np.float32) if visible is None else visible, np.full(G, AREA, np.float32) if areas is None else areas,
                 np.zeros(G, np.int32), num_frames=1, **kw)
    return meter


def _bits(meter):
    s, m, g = meter.records()
    return [int(v) for v in m], [int(v) for v in g]


def test_hand_check_to_the_last_digit():
    """Two labels, three detections in score order: matched, unmatched, matched.  rc = [.5, .5, 1], the envelope [1, 2/3, 2/3]: 51 recall
    points read 1 and 50 read 2/3."""
    a, b, far = ref.base_pose(0, K), ref.base_pose(1, K), ref.base_pose(5, K)
    m = _feed(_meter(), [a, far, b], [0.9, 0.8, 0.7], [a, b])
    assert _bits(m) == ([1, 0, 1], [0, 0, 0]) and m.npig.tolist() == [2]
    p, s, r = m.tables()
    assert p[0, :51, 0].tolist() == [ONE] * 51 and p[0, 51:, 0].tolist() == [2.0 / (3.0 + np.spacing(1))] * 50 and r[0, 0] == 1.0
    assert s[0, :51, 0].tolist() == [np.float32(0.9)] * 51 and s[0, 51:, 0].tolist() == [np.float32(0.7)] * 50
    rep = APMeter.report(p, r, s, m.npig, m.counters()[:6], thresholds=(0.5,), area_ranges=("all",))
    assert float(f"{rep['AP']:.15g}") == 0.834983498349835 and rep["AP"] == np.mean([ONE] * 51 + [2.0 / 3.0] * 50)
    assert rep["AP50"] == rep["AP"] and rep["AR"] == 1.0 and "AP75" not in rep


def test_equal_oks_takes_the_later_label():
    """Both labels have oks 1 with the first detection: it takes the later one, so the second detection, which only label 0 fits, is matched."""
    a = ref.base_pose(0, K)
    vis = np.ones((2, K), np.float32)
    vis[0, 1:] = 0                                   # label 0 counts joint 0 alone
    other = a.copy()
    other[1:] += 400.0                               # right in joint 0, far off elsewhere: oks 1 with label 0, ~1 / K with label 1
    m = _feed(_meter(), [a, other], [0.9, 0.8], [a, a], visible=vis)
    assert _bits(m) == ([1, 1], [0, 0])
    # the other way round (label 1 counts joint 0 alone): the first detection takes label 1 again, and nothing is left for the second
    m = _feed(_meter(), [a, other], [0.9, 0.8], [a, a], visible=vis[::-1].copy())
    assert _bits(m) == ([1, 0], [0, 0])


def test_a_counted_label_goes_before_an_ignored_one():
    """A detection that reaches a counted label at 0.6 and an ignored one at 1.0 takes the counted one; a detection matched to the ignored
    label is neither tp nor fp."""
    a = ref.base_pose(0, K)
    near = ref.duplicate(a, 0.6)
    m = _feed(_meter(), [near, near], [0.9, 0.8], [near, a], gt_ignore=np.asarray([1, 0], np.uint8))
    assert _bits(m) == ([1, 1], [0, 1]) and m.npig.tolist() == [1]
    p, s, r = m.tables()
    assert r[0, 0] == 1.0 and (p[0, :, 0] == ONE).all()                                     # tp = [1, 1], fp = [0, 0]
    # without the flag the same detection takes the better label
    m = _feed(_meter(), [near], [0.9], [near, a])
    p, s, r = m.tables()
    assert r[0, 0] == 0.5
    # a label without a visible joint is ignored and matches nothing (the stated deviation from cocoapi's box fallback)
    vis = np.ones((2, K), np.float32)
    vis[0] = 0
    m = _feed(_meter(), [a], [0.9], [a, ref.base_pose(1, K)], visible=vis)
    assert _bits(m) == ([0], [0]) and m.npig.tolist() == [1]


def test_an_unmatched_detection_outside_the_range_is_ignored():
    a, far = ref.base_pose(0, K), ref.base_pose(5, K)
    rng = {"all": (0, 1e10), "medium": (32 ** 2, 96 ** 2)}
    m = _feed(_meter(area_ranges=rng), [a, far], [0.9, 0.8], [a], areas=np.asarray([50.0 ** 2], np.float32),
              area=np.asarray([50.0 ** 2, 200.0 ** 2], np.float32))
    assert _bits(m) == ([0b11, 0], [0, 0b10])
    # the area from the key points' extent: 60 x 60 or so for the layout's radius of 30 - inside medium
    assert 32 ** 2 < ap.det_area_ref(np.stack([a]).astype(np.float32))[0] < 96 ** 2
    m = _feed(_meter(area_ranges=rng), [a, far], [0.9, 0.8], [a], areas=np.asarray([50.0 ** 2], np.float32))
    assert _bits(m) == ([0b11, 0], [0, 0])


def test_max_dets_capacity_refusals_and_overflow():
    a, b, far = ref.base_pose(0, K), ref.base_pose(1, K), ref.base_pose(5, K)
    m = _feed(_meter(max_dets=2), [b, a, far], [0.7, 0.9, 0.8], [a, b])
    assert m.counts["cut"] == 1 and m.counts["records"] == 2 and _bits(m)[0] == [1, 0]
    m = _feed(_meter(capacity=2), [a, far, b], [0.9, 0.8, 0.7], [a, b])
    assert m.counts["dropped"] == 1 and m.counts["records"] == 2
    bad = a.copy()
    bad[3, 0] = np.inf
    m = _meter()
    m.update(np.stack([a, bad, a, a, b]).astype(np.float32), np.asarray([0.9, 0.8, np.nan, 0.6, 0.5], np.float32), np.asarray([0, 0, 0, 1, 0]),
             np.stack([a, b]), np.ones((2, K)), np.full(2, AREA), np.asarray([0, -1]), num_frames=1, valid=np.asarray([1, 1, 1, 1, 0]))
    assert m.counts["refused"] == 4 and m.counts["bad_labels"] == 1 and m.counts["records"] == 1 and m.npig.tolist() == [1]
    m = _feed(_meter(), [a], [0.9], [ref.base_pose(g, K) for g in range(65)])
    assert m.counts["overflow_frames"] == 1 and m.counts["records"] == 0 and m.npig.tolist() == [0]


def test_no_counted_label_gives_minus_one_and_no_record_gives_zero():
    a = ref.base_pose(0, K)
    rng = {"all": (0, 1e10), "large": (96 ** 2, 1e10)}
    m = _feed(_meter(area_ranges=rng), [a], [0.9], [a], areas=np.asarray([50.0 ** 2], np.float32))
    p, s, r = m.tables()
    assert (p[:, :, 1] == -1).all() and (s[:, :, 1] == -1).all() and r[0, 1] == -1 and (p[:, :, 0] == ONE).all()
    rep = APMeter.report(p, r, s, m.npig, m.counters()[:6], thresholds=(0.5,), area_ranges=tuple(rng))
    assert rep["AP_large"] == -1.0 and rep["APL"] == -1.0 and rep["AR_large"] == -1.0 and abs(rep["AP"] - 1.0) < 1e-15
    m = _feed(_meter(), [a], [0.9], [a], valid=np.asarray([0]))
    p, s, r = m.tables()
    assert (p == 0).all() and (s == 0).all() and (r == 0).all() and m.counts["records"] == 0 and m.npig.tolist() == [1]


def test_report_names():
    T, R, A = 10, 101, 3
    rep = APMeter.report(np.full((T, R, A), 0.5), np.full((T, A), 0.25), np.zeros((T, R, A), np.float32), [3, 2, 1], [6, 0, 1, 2, 0, 0])
    for name in ("AP", "AP50", "AP75", "APM", "APL", "AR", "AR50", "AR75", "AP_all", "AP_medium", "AP_large", "AR_all", "AR_medium", "AR_large",
                 "precision", "recall", "scores", "npig", "counts"):
        assert name in rep, name
    assert rep["AP"] == 0.5 and rep["AR"] == 0.25 and rep["APM"] == rep["AP_medium"] and rep["npig"].tolist() == [3, 2, 1]
    assert rep["counts"] == {"records": 6, "dropped": 0, "refused": 1, "cut": 2, "overflow_frames": 0, "bad_labels": 0}
    with pytest.raises(ValueError):
        APMeter.report(np.zeros((9, R, A)), np.zeros((T, A)), np.zeros((9, R, A)), [0, 0, 0], [0] * 6)


def test_defaults_are_cocoapi_params():
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    assert np.array_equal(np.asarray(kd.AP_OKS_THRESHOLDS), ap.THRESHOLDS) and np.array_equal(np.asarray(kd.AP_RECALL_POINTS), ap.RECALL_POINTS)
    assert kd.AP_AREA_RANGES == ap.AREA_RANGES and list(kd.AP_AREA_RANGES) == ["all", "medium", "large"] and kd.AP_COUNTS == ap.COUNT_NAMES


def test_host_side_refusals():
    from uda_poseestimation_amd import engine
    m = APMeter(17)
    kp, sc, fi = torch.zeros(3, 17, 2), torch.ones(3), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        m.update(kp, sc, fi, kp, torch.ones(3, 17), torch.ones(3), fi, num_frames=1)
    with pytest.raises(ValueError, match="65"):
        APMeter(17, thresholds=np.linspace(0.3, 0.9, 13), area_ranges={str(i): (0, 1e10) for i in range(5)})          # T * A = 65
    APMeter(17, thresholds=np.linspace(0.2, 0.9, 16), area_ranges={str(i): (0, 1e10) for i in range(4)}, device=None)   # T * A = 64
    with pytest.raises(ValueError, match="max_dets"):
        APMeter(17, max_dets=65)
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        APMeter(17, thresholds=(0.5, 1.0))
    with pytest.raises(ValueError, match="ascending"):
        APMeter(17, thresholds=(0.5, 0.5))
    with pytest.raises(ValueError, match="capacity"):
        APMeter(17, capacity=(1 << 18) + 1)
    with pytest.raises(ValueError, match="recall points"):
        APMeter(17, recall_points=np.linspace(0, 1, 129))
    with pytest.raises(ValueError, match="key points"):
        APMeter(65)
    with pytest.raises(ValueError, match="nms"):
        engine.evaluate_ap([], None, nms=None)


def test_exports_declared_bound_built_and_documented():
    from uda_poseestimation_amd import _hip
    text = open(os.path.join(ROOT, "include", "udapose.h")).read()
    docs = open(os.path.join(ROOT, "INTEGRATION.md")).read() + open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in NAMES:
        m = re.search(r"\b(?:int|long long)\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/udapose.h"
        assert name in _hip.EXPORTS and len(m.group(1).split(",")) == len(_hip._SIGS[name][1]), name
        assert name in docs, f"{name} is not documented"
    for line in ("UDAPOSE_AP_MAX_COMBOS 64", "UDAPOSE_AP_MAX_DETS 64", "UDAPOSE_AP_MAX_RECALL_POINTS 128", "UDAPOSE_AP_MAX_CAPACITY 262144",
                 "UDAPOSE_AP_MAX_FRAMES 4096", "UDAPOSE_AP_MAX_LABELS_PER_FRAME 64", "UDAPOSE_AP_COUNTERS 6"):
        assert line in text, line
    csrc = os.path.join(ROOT, "uda_poseestimation_amd", "csrc")
    assert "pose_ap.hip" in open(os.path.join(csrc, "Makefile")).read()
    # the per-pair expression is stated once, in the header both files include
    for src in ("pose_ap.hip", "pose_nms.hip"):
        body = open(os.path.join(csrc, src)).read()
        assert '#include "pose_pair.h"' in body and "oks_term(" in body, src
    if os.path.exists(_hip.LIB_PATH):
        lib = _hip.lib()
        assert lib.udapose_ap_match_ws_bytes(4096, 4096, 4096) == 4 * 4 * 4096 and lib.udapose_ap_match_ws_bytes(4097, 1, 1) == 0
        assert lib.udapose_ap_curve_ws_bytes(8, 10, 3) == 8 * 4 + 2 * 8 * 8 + 2 * 30 * 8 * 4 and lib.udapose_ap_curve_ws_bytes(8, 13, 5) == 0
