"""The instance layer without a GPU: the numpy restatement on hand-worked cases, the C ABI's prototypes against the ctypes
table, and what the Python layer refuses on the host."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import pose_nms_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("udapose_pose_rescore", "udapose_oks_matrix", "udapose_pose_nms_sweep", "udapose_pose_nms_ws_bytes", "udapose_pose_nms")


def _poses(list_of_kp, conf):
    kp = np.stack(list_of_kp).astype(np.float32)
    M, K = kp.shape[:2]
    boxes = np.tile(np.asarray([0, 0, ref.SIDE, ref.SIDE, 0], np.float32), (M, 1))
    return kp, np.broadcast_to(np.asarray(conf, np.float32)[:, None], (M, K)).copy(), boxes


def test_rescore_by_hand():
    conf = np.asarray([[0.9, 0.1, 0.5, 0.3], [0.1, 0.2, 0.15, 0.0], [0.25, 0.25, 0.25, 0.25]], np.float32)
    s = ref.rescore_ref(conf, None, 0.2)
    want0 = np.float32(np.float32(np.float32(np.float32(0.9) + np.float32(0.5)) + np.float32(0.3)) / np.float32(3))
    assert s[0] == want0 and s[1] == 0 and s[2] == np.float32(0.25)      # (0.2 itself is not above the threshold)
    s = ref.rescore_ref(conf, np.asarray([0.5, 1.0, 2.0], np.float32), 0.2)
    assert s[0] == np.float32(want0 * np.float32(0.5)) and s[1] == 0 and s[2] == np.float32(0.5)


def test_order_by_hand():
    score = np.asarray([0.5, 0.9, 0.5, np.nan, 0.0, 0.9, -0.0], np.float32)
    refused = np.asarray([False, False, False, True, False, True, False])
    assert ref.order_ref(score, refused).tolist() == [1, 0, 2, 4, 6, 3, 5]


def test_designed_oks_values():
    """A duplicate made for 0.95 has oks 0.95, two bases are far below 0.05, and the chain's ends are at 0.95^4."""
    K = 17
    a = ref.base_pose(0, K)
    b = ref.duplicate(a, 0.95)
    c = b + (b - a)
    kp, conf, boxes = _poses([a, b, c, ref.base_pose(1, K), ref.duplicate(a, 0.80, 0.4)], [0.9, 0.8, 0.7, 0.6, 0.5])
    o = ref.oks_self_ref(kp, ref.area_ref(boxes), (ref.SIGMA,) * K)
    assert abs(o[0, 1] - 0.95) < 1e-5 and abs(o[1, 2] - 0.95) < 1e-5 and abs(o[0, 2] - 0.95 ** 4) < 1e-5 and abs(o[0, 4] - 0.80) < 1e-5
    assert o[0, 3] < 0.05 and o[4, 3] < 0.05 and np.array_equal(o, o.T) and np.allclose(np.diag(o), 1.0)


def test_greedy_chain_by_hand():
    """A > B > C, oks(A, B) = oks(B, C) = 0.95, oks(A, C) = 0.81: A removes B, and B, removed, removes nothing: C stays."""
    K = 17
    a = ref.base_pose(0, K)
    b = ref.duplicate(a, 0.95)
    kp, conf, boxes = _poses([a, b, b + (b - a)], [0.9, 0.8, 0.7])
    r = ref.nms_ref(kp, conf, boxes, sigmas=(ref.SIGMA,) * K, oks_thr=0.9)
    assert r["order"].tolist() == [0, 1, 2] and r["keep"].tolist() == [1, 0, 1] and r["n_keep"] == 2
    assert r["suppressed_by"].tolist() == [-1, 0, -1] and r["margin"] > 0.04


def test_frames_ties_and_refusals_by_hand():
    K = 16
    a = ref.base_pose(0, K)
    b = ref.duplicate(a, 0.95)
    sig = (ref.SIGMA,) * K
    kp, conf, boxes = _poses([a, b], [0.6, 0.6])
    one = ref.nms_ref(kp, conf, boxes, frame=[0, 0], sigmas=sig)
    assert one["keep"].tolist() == [1, 0] and one["suppressed_by"].tolist() == [-1, 0]            # equal scores: the lower index leads
    two = ref.nms_ref(kp, conf, boxes, frame=[0, 1], sigmas=sig)
    assert two["keep"].tolist() == [1, 1] and two["n_keep"] == 2                                    # other frames never interact
    # a refused leader removes nothing: by status, by a NaN coordinate, by an empty box
    kp, conf, boxes = _poses([a, b], [0.9, 0.6])
    assert ref.nms_ref(kp, conf, boxes, status=[1, 0], sigmas=sig)["keep"].tolist() == [0, 1]
    bad = kp.copy()
    bad[0, 3, 1] = np.nan
    r = ref.nms_ref(bad, conf, boxes, sigmas=sig)
    assert r["keep"].tolist() == [0, 1] and r["order"].tolist() == [1, 0] and r["suppressed_by"].tolist() == [-1, -1]
    flat = boxes.copy()
    flat[0, 2] = 0
    assert ref.nms_ref(kp, conf, flat, sigmas=sig)["keep"].tolist() == [0, 1]
    # no confidence above vis_thr: score 0, still a pose
    r = ref.nms_ref(kp, np.full_like(conf, 0.1), boxes, sigmas=sig)
    assert r["score"].tolist() == [0, 0] and r["keep"].tolist() == [1, 0]


def test_rect_form_by_hand():
    K = 4
    a = ref.base_pose(0, K)
    vis = np.asarray([[1, 1, 0, 0], [0, 0, 0, 0]], np.float32)
    b = a.copy()
    b[2:] += 500.0                                                                                  # hidden joints, far off: they do not count
    o = ref.oks_rect_ref(np.stack([a]), np.stack([b, a]), np.asarray([1e4, 1e4], np.float32), vis, (ref.SIGMA,) * K)
    assert o.shape == (1, 2) and o[0, 0] == 1.0 and o[0, 1] == 0.0


def test_tolerance_is_what_the_derivation_says():
    assert ref.oks_tolerance(17) == 20 * 2.0 ** -24 and ref.oks_tolerance(64) == 43.5 * 2.0 ** -24


def test_grouped_case_keeps_its_margins():
    for M, K in ((65, 17), (130, 16)):
        kp, conf, boxes, frame = ref.grouped_case(M, K)
        assert np.abs(conf - np.float32(0.2)).min() >= 0.05
        for thr in (0.9, 0.7):
            r = ref.nms_ref(kp, conf, boxes, frame=frame, sigmas=(ref.SIGMA,) * K, oks_thr=thr)
            assert r["margin"] >= 1e-3 and 0 < r["n_keep"] < M


def test_header_declares_what_the_bindings_call():
    from uda_poseestimation_amd import _hip
    text = open(os.path.join(ROOT, "include", "udapose.h")).read()
    for name in NAMES:
        m = re.search(r"\b(?:int|long long)\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/udapose.h"
        assert name in _hip.EXPORTS
        assert len(m.group(1).split(",")) == len(_hip._SIGS[name][1]), name
    assert "UDAPOSE_NMS_MAX_POSES 4096" in text and "UDAPOSE_NMS_MAX_KEYPOINTS 64" in text
    src = open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "Makefile")).read()
    assert "pose_nms.hip" in src


def test_host_side_refusals():
    from uda_poseestimation_amd import engine
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    assert kd.OKS_SIGMAS["coco17"][0] == 0.026 and len(kd.OKS_SIGMAS["coco17"]) == 17 and kd.oks_sigmas(17) == kd.OKS_SIGMAS["coco17"]
    assert kd.oks_sigmas(16) == (kd.OKS_UNIFORM_SIGMA,) * 16 and kd.OKS_UNIFORM_SIGMA == ref.SIGMA
    for K in (0, 65, 2.5):
        with pytest.raises(ValueError):
            kd.oks_sigmas(K)
    kp, conf, boxes = torch.zeros(3, 17, 2), torch.ones(3, 17), torch.ones(3, 5)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        kd.oks_nms(kp, conf, boxes)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        kd.rescore(conf)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        kd.oks_matrix(kp, torch.ones(3))
    with pytest.raises(ValueError, match="CUDA tensor"):
        kd.oks_nms(kp.numpy(), conf, boxes)
    with pytest.raises(ValueError, match="thresholds are"):
        kd.nms_threshold("iou_thr", 0.5, "cpu")
    with pytest.raises(ValueError, match="finite"):
        kd.nms_threshold("oks_thr", float("nan"), "cpu")
    # predict(): refused ahead of any device work
    with pytest.raises(ValueError, match="box_scores"):
        engine.predict(None, None, None, box_scores=[1.0])
    with pytest.raises(ValueError, match="iou"):
        engine.predict(None, None, None, nms={"iou": 0.5})
