"""The instance layer on the MI355X (csrc/pose_nms.hip): rescoring, the OKS matrix and greedy OKS-NMS against the numpy
restatement of tests/helpers/pose_nms_ref.py (checked on the CPU by tests/test_pose_nms_cpu.py).

Scores and the order are compared bit for bit; keep, n_keep and suppressed_by must equal the float64 walk's exactly, on inputs constructed
so that every same-frame pair is at least 1e-3 from the threshold (asserted here in float64 for every case: none is left out); the matrix
is within the tolerance the helper derives from the expression."""
import numpy as np
import pytest
import torch

from helpers import pose_nms_ref as ref

pytestmark = pytest.mark.gpu


def _kd():
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    return kd


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _uniform(K):
    return (ref.SIGMA,) * K


def _same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def _run_and_check(kp, conf, boxes, frame=None, status=None, box_score=None, oks_thr=0.9, vis_thr=0.2, want_matrix=False):
    """oks_nms on the device against nms_ref: the margin asserted first, then every output."""
    K = kp.shape[1]
    r = ref.nms_ref(kp, conf, boxes, frame, status, box_score, _uniform(K), oks_thr, vis_thr)
    assert r["margin"] >= 1e-3, r["margin"]
    out = _kd().oks_nms(_dev(kp), _dev(conf), _dev(boxes), frame_idx=_dev(frame, np.int32), status=_dev(status, np.uint8),
                        box_scores=_dev(box_score, np.float32), sigmas=_uniform(K), oks_thr=oks_thr, vis_thr=vis_thr, want_matrix=want_matrix)
    assert all(v.is_cuda for v in out.values())
    _compare(out, r)
    return out, r


def _compare(out, r):
    assert _same_bits(out["score"].cpu().numpy(), r["score"])
    assert out["order"].cpu().numpy().tolist() == r["order"].tolist()
    assert out["keep"].cpu().numpy().tolist() == r["keep"].tolist()
    assert int(out["n_keep"].item()) == r["n_keep"]
    assert out["suppressed_by"].cpu().numpy().tolist() == r["suppressed_by"].tolist()


def _poses(list_of_kp, conf):
    kp = np.stack(list_of_kp).astype(np.float32)
    M, K = kp.shape[:2]
    boxes = np.tile(np.asarray([0, 0, ref.SIDE, ref.SIDE, 0], np.float32), (M, 1))
    return kp, np.broadcast_to(np.asarray(conf, np.float32)[:, None], (M, K)).copy(), boxes


def test_greedy_chain():
    """A > B > C with oks(A, B) = oks(B, C) = 0.95 and oks(A, C) = 0.81: A and C stay, B is removed by A.  (Suppressing whatever a
    higher-scored pose overlaps would remove C as well.)"""
    a = ref.base_pose(0, 17)
    b = ref.duplicate(a, 0.95)
    kp, conf, boxes = _poses([a, b, b + (b - a)], [0.9, 0.8, 0.7])
    out, r = _run_and_check(kp, conf, boxes)
    assert r["keep"].tolist() == [1, 0, 1] and r["suppressed_by"].tolist() == [-1, 0, -1]
    # the same chain met in another order of indices
    out, r = _run_and_check(kp[::-1].copy(), conf[::-1].copy(), boxes)
    assert r["keep"].tolist() == [1, 0, 1] and r["suppressed_by"].tolist() == [-1, 2, -1]


def test_frames_and_ties():
    a = ref.base_pose(0, 16)
    b = ref.duplicate(a, 0.95)
    kp, conf, boxes = _poses([a], [0.7])
    out, r = _run_and_check(kp, conf, boxes)                                             # M = 1
    assert r["keep"].tolist() == [1] and r["n_keep"] == 1
    kp, conf, boxes = _poses([a, b], [0.6, 0.8])
    out, r = _run_and_check(kp, conf, boxes, frame=np.asarray([0, 0]))
    assert r["keep"].tolist() == [0, 1]
    out, r = _run_and_check(kp, conf, boxes)                                             # frame_idx None: one frame
    assert r["keep"].tolist() == [0, 1]
    out, r = _run_and_check(kp, conf, boxes, frame=np.asarray([0, 1]))                   # other frames: both stay
    assert r["keep"].tolist() == [1, 1]
    kp, conf, boxes = _poses([a, b, ref.base_pose(1, 16), ref.duplicate(ref.base_pose(1, 16), 0.95)], [0.6, 0.6, 0.6, 0.6])
    out, r = _run_and_check(kp, conf, boxes)                                             # equal scores: the lower index leads
    assert r["order"].tolist() == [0, 1, 2, 3] and r["keep"].tolist() == [1, 0, 1, 0]
    out, r = _run_and_check(kp, conf, boxes, box_score=np.asarray([0.5, 1.0, 1.0, 0.5], np.float32))
    assert r["order"].tolist() == [1, 2, 0, 3] and r["keep"].tolist() == [0, 1, 1, 0]


@pytest.mark.parametrize("M", [65, 130])
def test_three_interleaved_frames(M):
    """Groups whose members are more than 64 indices apart: the bits of a row lie in several mask words."""
    kp, conf, boxes, frame = ref.grouped_case(M, 17)
    out, r = _run_and_check(kp, conf, boxes, frame=frame, want_matrix=True)
    assert 0 < r["n_keep"] < M and (r["suppressed_by"] >= 0).any()
    out, r = _run_and_check(kp, conf, boxes, frame=frame, oks_thr=0.7)                   # now the 0.80 duplicates go as well
    assert r["n_keep"] == (M + 2) // 3


@pytest.mark.parametrize("K", [1, 16, 17, 21])
def test_key_point_counts(K):
    kp, conf, boxes, frame = ref.grouped_case(65, K)
    _run_and_check(kp, conf, boxes, frame=frame)


@pytest.mark.parametrize("M", [17, 257])
def test_rank_across_the_group_boundary_and_the_padding(M):
    """Distinct poses on one frame, scores from three levels: the index decides nearly every place of the order.  M = 17 ranks beside 15
    padding keys (the keys are padded to 32); M = 257 spans two 256-pose work-groups, with equal keys on both sides of the boundary."""
    K = 17
    level = np.asarray([0.5, 0.7, 0.9], np.float32)[np.arange(M) % 3]
    kp, conf, boxes = _poses([ref.base_pose(i, K) for i in range(M)], level)
    out, r = _run_and_check(kp, conf, boxes)
    assert len(set(r["score"].tolist())) == 3 and r["n_keep"] == M
    assert sorted(r["order"].tolist()) == list(range(M)) and r["order"].tolist()[:3] == [2, 5, 8]
    if M > 256:
        assert set(r["score"][256:].tolist()) <= set(r["score"][:256].tolist())


def test_full_size_without_the_matrix():
    kp, conf, boxes, frame = ref.grouped_case(4096, 17)
    out, r = _run_and_check(kp, conf, boxes, frame=frame)
    assert "oks" not in out and 1366 <= r["n_keep"] < 4096


def test_too_many_poses_writes_nothing():
    kd = _kd()
    from uda_poseestimation_amd import _hip
    L, M, K = _hip.lib(), 4097, 17
    kp, conf, boxes, frame = ref.grouped_case(M, K)
    d = [_dev(kp), _dev(conf), _dev(boxes), _dev(frame)]
    sg = torch.full((K,), ref.SIGMA, device="cuda")
    thr = torch.tensor([0.2, 0.9], device="cuda")
    assert L.udapose_pose_nms_ws_bytes(M) == 0 and L.udapose_pose_nms_ws_bytes(4096) == 4096 * (64 * 8 + 5)
    ws = torch.zeros(1024, dtype=torch.int64, device="cuda")
    score = torch.full((M,), -7.0, device="cuda")
    order, sby = torch.full((M,), -7, dtype=torch.int32, device="cuda"), torch.full((M,), -7, dtype=torch.int32, device="cuda")
    keep, n_keep = torch.full((M,), 7, dtype=torch.uint8, device="cuda"), torch.full((1,), -7, dtype=torch.int32, device="cuda")
    p = _hip.ptr

    def call(M, K, kp_ptr=p(d[0])):
        return L.udapose_pose_nms(_hip.stream(), kp_ptr, p(d[1]), p(d[2]), p(d[3]), None, None, p(sg), p(thr[:1]), p(thr[1:]), M, K, p(ws), p(score),
                                  p(order), p(keep), p(n_keep), p(sby), None)
    for args in ((4097, K), (0, K), (64, 0), (64, 65)):
        assert call(*args) == -1
    assert call(64, K, None) == -1
    torch.cuda.synchronize()
    assert bool((score == -7).all()) and bool((order == -7).all()) and bool((sby == -7).all()) and bool((keep == 7).all())
    assert int(n_keep.item()) == -7 and not bool(ws.any())
    with pytest.raises(ValueError, match="4096"):
        kd.oks_nms(*d[:3])


def test_refused_poses():
    """A refused leader removes nothing and is not kept; a pose without a confidence above vis_thr scores 0 and is a pose like any other."""
    a, c = ref.base_pose(0, 17), ref.base_pose(1, 17)
    kp, conf, boxes = _poses([a, ref.duplicate(a, 0.95), c, ref.duplicate(c, 0.95), ref.base_pose(2, 17)], [0.9, 0.6, 0.8, 0.7, 0.5])
    out, r = _run_and_check(kp, conf, boxes, status=np.asarray([1, 0, 0, 0, 0], np.uint8))
    assert r["keep"].tolist() == [0, 1, 1, 0, 1] and r["order"].tolist() == [2, 3, 1, 4, 0]
    bad = kp.copy()
    bad[2, 5, 0] = np.nan
    bad[4, 0, 1] = np.inf
    out, r = _run_and_check(bad, conf, boxes)
    assert r["keep"].tolist() == [1, 0, 0, 1, 0] and r["order"].tolist() == [0, 3, 1, 2, 4]
    flat = boxes.copy()
    flat[0, 2] = 0.0                 # zero area
    flat[2, 3] = -3.0                # negative area
    flat[4, 2] = np.nan
    out, r = _run_and_check(kp, conf, flat)
    assert r["keep"].tolist() == [0, 1, 0, 1, 0]
    out, r = _run_and_check(kp, conf, boxes, box_score=np.asarray([np.inf, 1, 1, 1, 1], np.float32))      # a score that is not finite
    assert r["keep"].tolist() == [0, 1, 1, 0, 1]
    low = conf.copy()
    low[0] = 0.1                     # the leader of the first pair has no visible joint: score 0, last of the order, removed by its duplicate
    low[4] = 0.15
    out, r = _run_and_check(kp, low, boxes)
    assert r["score"][[0, 4]].tolist() == [0, 0] and r["order"].tolist() == [2, 3, 1, 0, 4] and r["keep"].tolist() == [0, 1, 1, 0, 1]


def test_rescore_function():
    kd = _kd()
    _, conf, _, _ = ref.grouped_case(130, 17)
    bs = (0.5 + 0.5 * ((np.arange(130) * 0.37) % 1.0)).astype(np.float32)
    assert _same_bits(kd.rescore(_dev(conf)).cpu().numpy(), ref.rescore_ref(conf, None, 0.2))
    assert _same_bits(kd.rescore(_dev(conf), _dev(bs), vis_thr=0.5).cpu().numpy(), ref.rescore_ref(conf, bs, 0.5))


@pytest.fixture(scope="module")
def matrix_case():
    """130 poses of the grouped construction under COCO's own table and unequal areas: values, not decisions."""
    kp, conf, boxes, frame = ref.grouped_case(130, 17)
    area = (ref.SIDE * ref.SIDE * (0.5 + (np.arange(130) * 0.29) % 1.0)).astype(np.float32)
    return kp, area, frame, _kd().OKS_SIGMAS["coco17"]


def test_matrix_values_and_symmetry(matrix_case):
    kd = _kd()
    kp, area, frame, sig = matrix_case
    o = kd.oks_matrix(_dev(kp), _dev(area), sigmas="coco17")
    want = ref.oks_self_ref(kp, area, sig)
    err = np.abs(o.cpu().numpy().astype(np.float64) - want).max()
    print(f"self form, M = 130, K = 17: max error {err:.3e}, tolerance {ref.oks_tolerance(17):.3e}")
    assert err <= ref.oks_tolerance(17)
    assert torch.equal(o, o.t())                                                        # oks(i, j) and oks(j, i): the same bits
    for K in (1, 21, 64):
        kpk = ref.grouped_case(70, K)[0]
        ok = kd.oks_matrix(_dev(kpk), _dev(area[:70]), sigmas=None)
        errk = np.abs(ok.cpu().numpy().astype(np.float64) - ref.oks_self_ref(kpk, area[:70], kd.oks_sigmas(K))).max()
        print(f"self form, M = 70, K = {K}: max error {errk:.3e}, tolerance {ref.oks_tolerance(K):.3e}")
        assert errk <= ref.oks_tolerance(K) and torch.equal(ok, ok.t())


def test_mask_bits(matrix_case):
    """The exported mask: bit (i, j) = same frame, neither refused, i != j, oks > oks_thr - the diagonal and the bits past M clear."""
    from uda_poseestimation_amd import _hip
    kp, area, frame, sig = matrix_case
    M, K, W = 130, 17, 3
    refused = np.zeros(M, np.uint8)
    refused[[3, 64, 129]] = 1
    thr = 0.8
    want = ref.oks_self_ref(kp, area, sig)
    off = ~np.eye(M, dtype=bool)
    assert np.abs(want[off] - thr).min() >= 1e-3
    mask = torch.full((M, W), -1, dtype=torch.int64, device="cuda")
    p = _hip.ptr
    t = [_dev(kp), _dev(area), _dev(np.asarray(sig, np.float32)), _dev(frame), _dev(refused), torch.tensor([thr], device="cuda")]
    code = _hip.lib().udapose_oks_matrix(_hip.stream(), p(t[0]), p(t[1]), M, None, None, None, M, K, p(t[2]), p(t[3]), p(t[4]), p(t[5]), None, p(mask))
    assert code == 0
    words = mask.cpu().numpy().view(np.uint64)
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).reshape(M, W * 64).astype(bool)
    ok = refused == 0
    expect = (want > thr) & off & (frame[:, None] == frame[None, :]) & ok[:, None] & ok[None, :]
    assert not bits[:, M:].any() and not bits[:, :M][np.eye(M, dtype=bool)].any()
    assert np.array_equal(bits[:, :M], expect) and expect.any()


def test_rectangular_form(matrix_case):
    kd = _kd()
    kp, area, frame, sig = matrix_case
    a, b = kp[:70], kp[60:105] + np.float32(1.5)                                         # 45 labels near some predictions, far from most
    vis = ((np.arange(45)[:, None] * 7 + np.arange(17)[None, :] * 3) % 4 != 0).astype(np.float32)
    vis[11] = 0.0                                                                       # a label without a visible joint
    vis[12] = 1.0
    o = kd.oks_matrix(_dev(a), _dev(area[:70]), _dev(b), _dev(area[60:105]), _dev(vis), sigmas="coco17")
    want = ref.oks_rect_ref(a, b, area[60:105], vis, sig)
    err = np.abs(o.cpu().numpy().astype(np.float64) - want).max()
    print(f"rectangular form, 70 x 45, K = 17: max error {err:.3e}, tolerance {ref.oks_tolerance(17):.3e}")
    assert o.shape == (70, 45) and err <= ref.oks_tolerance(17)
    assert bool((o[:, 11] == 0).all()) and want[:, 12].max() > 0.5
    full = kd.oks_matrix(_dev(a), _dev(area[:70]), _dev(b), _dev(area[60:105]), None, sigmas="coco17")
    assert np.abs(full.cpu().numpy() - ref.oks_rect_ref(a, b, area[60:105], None, sig)).max() <= ref.oks_tolerance(17)


def test_captured_call_follows_threshold_and_boxes():
    """Nothing is read back or uploaded: a captured oks_nms follows nms_threshold() and new values in the boxes tensor."""
    kd = _kd()
    kp, conf, boxes, frame = ref.grouped_case(65, 17)
    empty = boxes.copy()
    empty[:5, 2] = 0.0                                                                  # five poses lose their area: refused
    sig = _uniform(17)
    want = {(thr, name): ref.nms_ref(kp, conf, b, frame, None, None, sig, thr) for thr in (0.9, 0.7) for name, b in (("boxes", boxes), ("empty", empty))}
    assert all(r["margin"] >= 1e-3 for r in want.values())
    assert len({tuple(r["keep"].tolist()) for r in want.values()}) == 4
    d_kp, d_conf, d_boxes, d_frame = _dev(kp), _dev(conf), _dev(boxes), _dev(frame)
    kd.oks_nms(d_kp, d_conf, d_boxes, frame_idx=d_frame, sigmas=sig, oks_thr=0.9)       # (the device scalars and the table exist before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = kd.oks_nms(d_kp, d_conf, d_boxes, frame_idx=d_frame, sigmas=sig, oks_thr=0.9)
    try:
        for thr, name in ((0.9, "boxes"), (0.7, "boxes"), (0.7, "empty"), (0.9, "empty"), (0.9, "boxes")):
            kd.nms_threshold("oks_thr", thr, "cuda")
            d_boxes.copy_(torch.from_numpy(boxes if name == "boxes" else empty))
            out["keep"].fill_(9)
            graph.replay()
            torch.cuda.synchronize()
            _compare(out, want[(thr, name)])
    finally:
        kd.nms_threshold("oks_thr", 0.9, "cuda")


def test_predict_with_nms():
    """predict(nms=True) on a small PoseResNet-50 with repeated and shifted boxes: its instance outputs are oks_nms on its own key points,
    confidences, boxes, frames and status; a box given twice on one frame is one pose; nms=None returns what it returned before."""
    from uda_poseestimation_amd import engine
    import uda_poseestimation_amd.lib.models as models
    kd = _kd()
    torch.manual_seed(0)
    model = models.pose_resnet50(17, pretrained_backbone=False).cuda()
    rs = np.random.RandomState(9)
    frames = torch.from_numpy(rs.randint(0, 256, (2, 96, 128, 3)).astype(np.uint8)).cuda()
    one, two = (64, 48, 96, 96, 0), (30, 30, 80, 100, 20)
    boxes = np.asarray([one, two, one, (65, 48.5, 96, 96, 0), one, (100, 70, 120, 90, -60), two, (64, 48, float("nan"), 96, 0)], np.float32)
    fi = torch.tensor([0, 1, 0, 0, 1, 1, 1, 0], dtype=torch.int32, device="cuda")
    bs = torch.tensor([0.9, 0.8, 0.95, 0.7, 0.6, 0.5, 0.85, 0.99], device="cuda")
    bd = torch.from_numpy(boxes).cuda()
    plain = engine.predict(frames, bd, model, frame_idx=fi, batch=4, input_size=64)
    assert sorted(plain) == ["confidence", "keypoints", "status"]
    out = engine.predict(frames, bd, model, frame_idx=fi, batch=4, input_size=64, box_scores=bs, nms=True)
    assert sorted(out) == ["confidence", "keep", "keypoints", "n_keep", "order", "score", "status", "suppressed_by"]
    for k in ("keypoints", "confidence", "status"):
        assert torch.equal(out[k][:7], plain[k][:7])
    assert out["status"].tolist() == [0] * 7 + [1]
    again = kd.oks_nms(out["keypoints"], out["confidence"], bd, frame_idx=fi, status=out["status"], box_scores=bs)
    for k in ("score", "order", "keep", "n_keep", "suppressed_by"):
        assert torch.equal(out[k], again[k]), k
    keep, sby = out["keep"].tolist(), out["suppressed_by"].tolist()
    assert torch.equal(out["keypoints"][0], out["keypoints"][2]) and torch.equal(out["keypoints"][1], out["keypoints"][6])
    score = out["score"].tolist()
    for i, j in ((0, 2), (1, 6)):                                                       # the same box twice on one frame: oks = 1, never two poses
        lead, other = (j, i) if score[j] > score[i] else (i, j)
        assert keep[other] == 0 and sby[other] >= 0 and (keep[lead] == 0 or sby[other] == lead)
    assert keep[7] == 0 and sby[7] == -1 and out["order"].tolist()[-1] == 7              # the refused box
    assert int(out["n_keep"].item()) == sum(keep) and out["keep"].shape == (8,)
    loose = engine.predict(frames, bd, model, frame_idx=fi, batch=4, input_size=64, box_scores=bs, nms={"oks_thr": 0.0, "want_matrix": True})
    assert loose["oks"].shape == (8, 8) and int(loose["n_keep"].item()) <= int(out["n_keep"].item())
