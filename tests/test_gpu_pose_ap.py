"""The key-point AP meter on the MI355X (csrc/pose_ap.hip) against the numpy restatement of tests/helpers/pose_ap_ref.py
(checked on the CPU by tests/test_pose_ap_cpu.py).

Inputs are constructed from pose_nms_ref.base_pose / offset_length: labels are base poses of a grid (oks of two bases is below e^-12), a
detection is a label's pose with every joint moved by the length that gives a designed oks at the mid-points 0.525, 0.575, ... 0.975 under
the label's own area, or a base pose no label has.  Every case asserts in float64 that every same-frame (detection, label) pair is at
least 1e-3 from every threshold - none is left out - and then the raw record words, the counters and the three tables must be EQUAL to the
helper's (np.array_equal, no tolerance)."""
import numpy as np
import pytest
import torch

from helpers import pose_ap_ref as ap
from helpers import pose_nms_ref as ref

pytestmark = pytest.mark.gpu

MIDS = tuple(0.525 + 0.05 * i for i in range(10))
LABEL_AREAS = (20.0 ** 2, 50.0 ** 2, 90.0 ** 2, 120.0 ** 2, 31.0 ** 2, 33.0 ** 2, 95.0 ** 2, 97.0 ** 2)      # both sides of 32^2 and 96^2


def _kd():
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    return kd


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _moved(pose, q, area, twist):
    """`pose` with every joint moved by the length that gives oks q under the label's area, the direction turning with the joint."""
    k = np.arange(pose.shape[0])
    ang = 0.7 * k + twist
    return pose + ref.offset_length(q, area=area) * np.stack([np.cos(ang), np.sin(ang)], axis=1)


def scene(K, labels_per_frame, dets_per_frame, levels=None, stray_every=4, with_area=False):
    """One update as numpy arrays.  labels_per_frame / dets_per_frame: a count per frame.  Frame f's labels are its own base poses (the grid
    index runs over the whole scene), with areas cycling through LABEL_AREAS, every seventh hidden in some joints and every eleventh flagged
    ignore; its detections go round its labels with designed oks values cycling through MIDS, every `stray_every`-th a base pose of a grid
    cell no label has.  Scores: a fixed scramble of [0.3, 0.9], or one of `levels` equal values.  Detection and label indices interleave
    the frames."""
    F = len(labels_per_frame)
    gkp, gvis, garea, gframe, gign = [], [], [], [], []
    mine = [[] for _ in range(F)]
    for f in range(F):
        for _ in range(labels_per_frame[f]):
            g = len(gkp)
            mine[f].append(g)
            gkp.append(ref.base_pose(g, K))
            v = np.ones(K)
            if g % 7 == 3 and K > 2:
                v[(np.arange(K) + g) % 3 == 0] = 0
            gvis.append(v)
            garea.append(LABEL_AREAS[g % len(LABEL_AREAS)])
            gframe.append(f)
            gign.append(1 if g % 11 == 5 else 0)
    G = len(gkp)
    kp, frame = [], []
    for f in range(F):
        for i in range(dets_per_frame[f]):
            n = len(kp)
            if not mine[f] or (stray_every and n % stray_every == stray_every - 1):
                kp.append(ref.base_pose(G + n, K))
            else:
                g = mine[f][i % len(mine[f])]
                kp.append(_moved(gkp[g], MIDS[(n * 7) % len(MIDS)], garea[g], 0.4 * n))
            frame.append(f)
    M = len(kp)
    frac = (np.arange(M) * 0.6180339887) % 1.0
    score = 0.3 + 0.6 * (np.floor(frac * levels) / levels if levels else frac)
    pd, pg = np.argsort((np.arange(M) * 0.7548776662) % 1.0), np.argsort((np.arange(max(G, 1)) * 0.5698402910) % 1.0)[:G]      # interleave
    out = {"keypoints": np.asarray(kp, np.float32)[pd], "score": score.astype(np.float32)[pd], "frame_idx": np.asarray(frame, np.int32)[pd],
           "gt_keypoints": np.asarray(gkp, np.float32)[pg], "gt_visible": np.asarray(gvis, np.float32)[pg],
           "gt_area": np.asarray(garea, np.float32)[pg], "gt_frame": np.asarray(gframe, np.int32)[pg],
           "gt_ignore": np.asarray(gign, np.uint8)[pg], "num_frames": F}
    if with_area:
        out["area"] = np.asarray([LABEL_AREAS[(3 * m) % len(LABEL_AREAS)] for m in range(M)], np.float32)
    return out


ARRAYS = ("keypoints", "score", "frame_idx", "gt_keypoints", "gt_visible", "gt_area", "gt_frame")
OPTIONAL = ("area", "valid", "gt_ignore")


def _feed(meter, u, on_device):
    conv = _dev if on_device else (lambda a: a)
    meter.update(*[conv(u[k]) for k in ARRAYS], num_frames=u["num_frames"], **{k: conv(u[k]) for k in OPTIONAL if k in u})


def _records(meter):
    st = meter.state()
    cnt = st["counters"].cpu().numpy()
    n = int(cnt[0])
    return st["score"][:n].cpu().numpy(), st["matched"][:n].cpu().numpy().view(np.uint64), st["ignored"][:n].cpu().numpy().view(np.uint64), cnt


def _same(meter, want):
    """The meter's records, counters and tables against the helper's: equal."""
    assert ap.min_margin(want) >= 1e-3, ap.min_margin(want)
    s, m, g, cnt = _records(meter)
    ws, wm, wg = want.records()
    assert np.array_equal(cnt, want.counters()), (cnt, want.counters())
    assert np.array_equal(s.view(np.uint32), ws.view(np.uint32)) and np.array_equal(m, wm) and np.array_equal(g, wg)
    rep = meter.compute()
    p, sc, r = want.tables()
    assert np.array_equal(rep["precision"], p) and np.array_equal(rep["recall"], r)
    assert np.array_equal(rep["scores"].view(np.uint32), sc.view(np.uint32))
    assert np.array_equal(rep["npig"], want.npig) and rep["counts"] == want.counts
    return rep


def _both(K, updates, **kw):
    sig = (ref.SIGMA,) * K
    meter, want = _kd().APMeter(K, sigmas=sig, device="cuda", **kw), ap.APRef(K, sig, **kw)
    for u in updates:
        _feed(meter, u, True)
        _feed(want, u, False)
    return meter, want


def test_three_frames_default_tables():
    u = scene(17, [4, 4, 4], [12, 13, 11])
    meter, want = _both(17, [u])
    rep = _same(meter, want)
    assert want.counts["records"] == 36 and (want.npig > 0).all() and want.npig[0] > want.npig[1] > 0
    assert 0 < rep["AP"] < 1 and 0 < rep["AP50"] <= 1 and rep["AP50"] >= rep["AP75"] and rep["APM"] > -1 and rep["APL"] > -1 and 0 < rep["AR"] <= 1
    # explicit areas on both sides of the ranges: unmatched detections outside a range are ignored there
    meter, want = _both(17, [scene(17, [4, 4, 4], [12, 13, 11], with_area=True)])
    _same(meter, want)
    s, m, g = want.records()
    assert (g & ~m).any()


@pytest.mark.parametrize("K", [1, 16, 17, 64])
def test_key_point_counts(K):
    meter, want = _both(K, [scene(K, [3, 5], [9, 10])])
    _same(meter, want)
    assert want.counts["records"] == 19


def _split(u):
    """The update cut frame by frame, in ascending frames."""
    parts = []
    for f in range(u["num_frames"]):
        d, g = u["frame_idx"] == f, u["gt_frame"] == f
        if d.any() and g.any():
            part = {k: u[k][d] for k in ("keypoints", "score", "frame_idx", "area", "valid") if k in u}
            part.update({k: u[k][g] for k in ("gt_keypoints", "gt_visible", "gt_area", "gt_frame", "gt_ignore")})
            part["num_frames"] = u["num_frames"]
            parts.append(part)
    return parts


def test_one_update_and_frame_by_frame_give_the_same_bits():
    u = scene(17, [4, 3, 5, 2], [10, 12, 9, 7], levels=5)
    whole, want = _both(17, [u])
    rep = _same(whole, want)
    parts, want2 = _both(17, _split(u))
    rep2 = _same(parts, want2)
    for a, b in zip(_records(whole), _records(parts)):
        assert np.array_equal(a, b)
    assert np.array_equal(rep["precision"], rep2["precision"]) and np.array_equal(rep["scores"], rep2["scores"])


@pytest.mark.parametrize("N", [257, 1025])
def test_equal_scores_across_rank_tiles(N):
    """Three score levels: the sequence number decides nearly every place of the sort; 257 and 1025 records cross the 256-record groups."""
    F = 22 if N == 257 else 64
    dets = [N // F + (1 if f < N % F else 0) for f in range(F)]
    meter, want = _both(17, [scene(17, [3] * F, dets, levels=3)], thresholds=(0.5, 0.75), area_ranges={"all": (0, 1e10), "medium": (32 ** 2, 96 ** 2)})
    _same(meter, want)
    assert want.counts["records"] == N and len(set(want.records()[0].tolist())) == 3


def test_sort_across_its_key_tile():
    """4096 + 19 records: the sort streams its keys through LDS 4096 at a time, so the second tile's index base is past zero.  Three score
    levels: equal keys lie on both sides of the tile boundary and the sequence number places them."""
    F = 256
    updates = [scene(17, [4] * F, [16] * F, levels=3), scene(17, [3, 5], [9, 10], levels=3)]
    meter, want = _both(17, updates, thresholds=(0.5, 0.75), area_ranges={"all": (0, 1e10)})
    _same(meter, want)
    s = want.records()[0]
    assert want.counts["records"] == 4096 + 19 and len(set(s.tolist())) == 3 and set(s[4096:].tolist()) == set(s[:4096].tolist())


def test_record_offsets_across_the_waves_of_the_frame_scan():
    """259 frames, one label and one or two detections each: a thread of the frame kernel owns 4 frames, so threads 0 .. 64 hold them and the
    offsets of the last frames take the first wave's sum."""
    F = 259
    meter, want = _both(17, [scene(17, [1] * F, [1 + f % 2 for f in range(F)])])
    _same(meter, want)
    assert want.counts["records"] == F + F // 2


def test_label_and_detection_limits_of_a_frame():
    meter, want = _both(17, [scene(17, [64, 65, 2], [6, 6, 6])], thresholds=(0.5, 0.75))
    with pytest.warns(UserWarning, match="left out"):
        _same(meter, want)
    assert want.counts["overflow_frames"] == 1 and want.counts["records"] == 12 and want.counts["cut"] == 0
    meter, want = _both(17, [scene(17, [4, 4], [20, 25])], thresholds=(0.5, 0.75))
    _same(meter, want)
    assert want.counts["cut"] == 5 and want.counts["records"] == 40
    meter, want = _both(17, [scene(17, [65], [3])], thresholds=(0.5,))      # nothing but a frame that is left out
    with pytest.warns(UserWarning, match="left out"):
        _same(meter, want)


def test_capacity_drops_and_counts():
    u = scene(17, [3, 3], [5, 6])
    meter, want = _both(17, [u, u], capacity=8)
    with pytest.warns(UserWarning, match="dropped"):
        _same(meter, want)
    assert want.counts["records"] == 8 and want.counts["dropped"] == 14


def test_refusals():
    u = scene(17, [3, 3], [6, 6], with_area=True)
    u["valid"] = np.ones(12, np.uint8)
    u["valid"][1] = 0
    u["score"][2] = np.nan
    u["keypoints"][3, 5, 1] = np.inf
    u["area"][4] = np.nan
    u["frame_idx"][5], u["frame_idx"][6] = -1, 2
    u["gt_frame"][0], u["gt_frame"][4] = 2, -3
    meter, want = _both(17, [u])
    _same(meter, want)
    assert want.counts["refused"] == 6 and want.counts["bad_labels"] == 2 and want.counts["records"] == 6


def test_full_size_and_too_many():
    from uda_poseestimation_amd import _hip
    F = 256
    u = scene(17, [4] * F, [16] * F, levels=64)
    assert u["keypoints"].shape[0] == 4096
    meter, want = _both(17, [u], thresholds=(0.5, 0.75), area_ranges={"all": (0, 1e10)})
    _same(meter, want)
    # M = 4097: ERR_ARG, ahead of the first launch - nothing written
    L, p = _hip.lib(), _hip.ptr
    kp = torch.zeros(4097, 17, 2, device="cuda")
    sc, fi = torch.ones(4097, device="cuda"), torch.zeros(4097, dtype=torch.int32, device="cuda")
    g = {k: _dev(u[k][:8]) for k in ("gt_keypoints", "gt_visible", "gt_area", "gt_frame")}
    st = meter._st
    ws = torch.zeros(1 << 14, dtype=torch.int64, device="cuda")
    rs, rm, ri = torch.full((64,), -7.0, device="cuda"), torch.full((64,), -7, dtype=torch.int64, device="cuda"), torch.full((64,), -7, dtype=torch.int64, device="cuda")
    cnt = torch.full((7,), -7, dtype=torch.int64, device="cuda")
    assert L.udapose_ap_match_ws_bytes(4097, 8, 1) == 0

    def call(M, G=8, K=17, F=1, T=2, A=1, max_dets=20, capacity=64, kp_ptr=p(kp)):
        return L.udapose_ap_match(_hip.stream(), kp_ptr, p(sc), p(fi), None, None, M, p(g["gt_keypoints"]), p(g["gt_visible"]), p(g["gt_area"]),
                                  p(g["gt_frame"]), None, G, K, F, p(st["sigmas"]), p(st["thr"]), T, p(st["ranges"]), A, max_dets, p(ws), p(rs),
                                  p(rm), p(ri), capacity, p(cnt))
    for kw in ({"M": 4097}, {"M": 0}, {"M": 8, "G": 4097}, {"M": 8, "F": 4097}, {"M": 8, "K": 65}, {"M": 8, "T": 13, "A": 5}, {"M": 8, "max_dets": 65},
               {"M": 8, "capacity": (1 << 18) + 1}, {"M": 8, "kp_ptr": None}):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((rs == -7).all()) and bool((rm == -7).all()) and bool((ri == -7).all()) and bool((cnt == -7).all()) and not bool(ws.any())
    with pytest.raises(ValueError, match="4096"):
        meter.update(kp, sc, fi, *[g[k] for k in ("gt_keypoints", "gt_visible", "gt_area", "gt_frame")], num_frames=1)


def test_sixty_four_combinations():
    rng = {"all": (0, 1e10), "small": (0, 32 ** 2), "medium": (32 ** 2, 96 ** 2), "large": (96 ** 2, 1e10)}
    meter, want = _both(17, [scene(17, [4, 4, 4], [12, 13, 11], with_area=True)], thresholds=tuple(0.2 + 0.05 * i for i in range(16)), area_ranges=rng)
    rep = _same(meter, want)
    assert rep["precision"].shape == (16, 101, 4) and "AP_small" in rep and (want.records()[1] >> np.uint64(63)).any()


def test_merge_equals_one_meter_fed_both():
    u1, u2 = scene(17, [4, 3], [9, 8], levels=4), scene(17, [2, 5, 3], [7, 9, 6], levels=4)
    one, want = _both(17, [u1, u2])
    a, _ = _both(17, [u1])
    b, _ = _both(17, [u2])
    a.merge(b)
    _same(one, want)
    _same(a, want)
    for x, y in zip(_records(one), _records(a)):
        assert np.array_equal(x, y)
    small, _ = _both(17, [u1], capacity=20)
    small.merge(b)
    cnt = small.state()["counters"].cpu().numpy()
    assert cnt[0] == 20 and cnt[1] == 17 + 22 - 20


def test_captured_update_replayed_on_new_values():
    kd = _kd()
    u1 = scene(17, [4, 4], [10, 11])
    u2 = scene(17, [4, 4], [10, 11], levels=3)
    u2["keypoints"] = u2["keypoints"][::-1].copy()          # other poses under the same frames: other matches
    assert u1["keypoints"].shape == u2["keypoints"].shape
    sig = (ref.SIGMA,) * 17
    meter, want = kd.APMeter(17, sigmas=sig, device="cuda"), ap.APRef(17, sig)
    d = {k: _dev(u1[k]) for k in ARRAYS + ("gt_ignore",)}
    meter.update(*[d[k] for k in ARRAYS], num_frames=2, gt_ignore=d["gt_ignore"])      # (one eager call ahead of the capture)
    meter.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        meter.update(*[d[k] for k in ARRAYS], num_frames=2, gt_ignore=d["gt_ignore"])
    meter.reset()
    for u in (u1, u2, u1):
        for k in d:
            d[k].copy_(torch.from_numpy(u[k]))
        graph.replay()
        _feed(want, u, False)
    torch.cuda.synchronize()
    _same(meter, want)
    assert want.counts["records"] == 63


def test_the_threshold_compares_the_bits_of_oks_matrix():
    """The device's own oks_matrix value of a pair as the single threshold: the pair matches (oks < best is false); the next fp32 above it
    as the threshold: it does not."""
    kd = _kd()
    K = 17
    sig = (ref.SIGMA,) * K
    for q, area in ((0.775, 90.0 ** 2), (0.625, 33.0 ** 2), (0.925, 120.0 ** 2)):
        label = ref.base_pose(2, K)
        det = _moved(label, q, area, 0.3)
        vis = np.ones((1, K), np.float32)
        vis[0, 4] = 0
        t = [_dev(np.stack([det]), np.float32), _dev(np.stack([label]), np.float32), _dev(np.asarray([area], np.float32)), _dev(vis)]
        value = np.float32(kd.oks_matrix(t[0], None, t[1], t[2], t[3], sigmas=sig).item())
        assert abs(float(value) - q) < 1e-4
        for thr, hit in ((value, 1), (np.nextafter(value, np.float32(2)), 0)):
            meter = kd.APMeter(K, sigmas=sig, thresholds=(float(thr),), area_ranges={"all": (0, 1e10)}, device="cuda")
            meter.update(t[0], torch.ones(1, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), t[1], t[3], t[2],
                         torch.zeros(1, dtype=torch.int32, device="cuda"), num_frames=1)
            s, m, g, cnt = _records(meter)
            assert cnt[0] == 1 and int(m[0]) == hit and int(g[0]) == 0


def test_evaluate_ap_on_a_small_network():
    """engine.evaluate_ap over two batches of a small PoseResNet-50: labels made from predict()'s own key points (tiny areas, so that only an
    identical pose reaches a threshold), the report equal to the helper's on predict()'s outputs."""
    from uda_poseestimation_amd import engine
    import uda_poseestimation_amd.lib.models as models
    kd = _kd()
    torch.manual_seed(0)
    model = models.pose_resnet50(17, pretrained_backbone=False).cuda()
    rs = np.random.RandomState(9)
    one, two = (64, 48, 96, 96, 0), (30, 30, 80, 100, 20)
    boxes = np.asarray([one, two, one, (65, 48.5, 96, 96, 0), one, (100, 70, 120, 90, -60), two, (64, 48, float("nan"), 96, 0)], np.float32)
    fi = np.asarray([0, 1, 0, 0, 1, 1, 1, 0], np.int32)
    bs = np.asarray([0.9, 0.8, 0.95, 0.7, 0.6, 0.5, 0.85, 0.99], np.float32)
    batches, outs = [], []
    for b in range(2):
        frames = torch.from_numpy(rs.randint(0, 256, (2, 96, 128, 3)).astype(np.uint8)).cuda()
        res = engine.predict(frames, _dev(boxes), model, frame_idx=_dev(fi), batch=4, input_size=64, box_scores=_dev(bs), nms=True)
        kp = res["keypoints"].cpu().numpy()
        pick = [0, 1, 5] if b == 0 else [3, 4]                                            # labels: some of predict()'s own poses
        gt = {"gt_keypoints": kp[pick].copy(), "gt_visible": np.ones((len(pick), 17), np.float32),
              "gt_area": np.asarray([1.0, 2.0, 1.5][:len(pick)], np.float32), "gt_frame": fi[pick].copy()}
        outs.append((res, gt))
        batches.append(dict({"frames": frames, "boxes": _dev(boxes), "frame_idx": _dev(fi), "box_scores": _dev(bs)}, **{k: _dev(v) for k, v in gt.items()}))
    rep = engine.evaluate_ap(batches, model, batch=4, input_size=64)
    want = ap.APRef(17, kd.OKS_SIGMAS["coco17"])
    for res, gt in outs:
        valid = ((res["keep"] != 0) & (res["status"] == 0)).cpu().numpy()
        want.update(res["keypoints"].cpu().numpy(), res["score"].cpu().numpy(), fi, gt["gt_keypoints"], gt["gt_visible"], gt["gt_area"], gt["gt_frame"],
                    num_frames=2, valid=valid)
    assert ap.min_margin(want) >= 1e-3
    p, sc, r = want.tables()
    assert np.array_equal(rep["precision"], p) and np.array_equal(rep["recall"], r) and np.array_equal(rep["scores"], sc)
    assert rep["counts"] == want.counts and np.array_equal(rep["npig"], want.npig)
    assert rep["counts"]["refused"] >= 2 + 2 and rep["counts"]["records"] >= 4 and rep["AR"] > 0 and rep["AP"] > 0
