"""The evaluation meter on the MI355X (csrc/pck_curve.hip through lib.keypoint_detection.PCKMeter and engine.evaluate) against the numpy
restatement of tests/helpers/pck_curve_ref.py (checked against the reference's own accuracy() by tests/test_pck_curve_cpu.py).

The state is integers, so every comparison with the fp32 restatement is exact (torch.equal); the two comparisons with fp64 carry derived
bounds, stated where they are used.  Shapes are the smallest at which the kernels can go wrong: B*K no multiple of a wave, K above a wave
and at the limit of 256, B above a block's 256 lanes (two blocks per joint), T = 1, 7 and 64, planes whose pixel count is no multiple
of 4 (the element-by-element sweep) and the product's 64x64.
"""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import pck_curve_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 5, 16, 16), (2, 70, 8, 8), (2, 256, 4, 4), (300, 2, 8, 8), (2, 3, 7, 9), (2, 16, 64, 64)]


def _kd():
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    return kd


def thresholds(T, top=1.0):
    """T ascending thresholds up to `top`."""
    return [top * (j + 1) / T for j in range(T)]


@functools.lru_cache(maxsize=None)
def random_maps(B, K, H, W, seed=0):
    """(output, target) CPU heat-maps: the output is the target plus noise, so the two arg-maxes agree on some planes and differ on
    others; every seventh target plane is all -1 (decoded (0, 0): not visible), every fifth output plane all zeros."""
    g = torch.Generator().manual_seed(seed + 1000 * B + 100 * K + 10 * H + W)
    t = torch.randn(B, K, H, W, generator=g)
    o = t + 0.6 * torch.randn(B, K, H, W, generator=g)
    flat_t, flat_o = t.view(B * K, -1), o.view(B * K, -1)
    flat_t[::7] = -1.0
    flat_o[3::5] = 0.0
    return o, t


def top_of(H, W):
    """The largest threshold of the shape tests: half a map side in normalised units (the side is 10), so that far pairs miss it."""
    return 5.0


def accumulate_coords(pred, gt, thr, nh, nw, visible=None, norm=None, state=None):
    """udapose_pck_accumulate on CUDA tensors: (code, state)."""
    from uda_poseestimation_amd import _hip
    B, K = pred.shape[:2]
    thr_d = torch.tensor(thr, dtype=torch.float32, device="cuda")
    if state is None:
        state = torch.zeros(K, len(thr) + 3, dtype=torch.int64, device="cuda")
    code = _hip.lib().udapose_pck_accumulate(_hip.stream(), _hip.ptr(pred), _hip.ptr(gt), _hip.ptr(visible), _hip.ptr(norm), B, K, nh, nw,
                                             _hip.ptr(thr_d), len(thr), _hip.ptr(state))
    torch.cuda.synchronize()
    return code, state


def argmax_of(hm):
    from uda_poseestimation_amd import _hip
    B, K, H, W = hm.shape
    preds = torch.empty(B, K, 2, dtype=torch.float32, device=hm.device)
    _hip.check(_hip.lib().udapose_heatmap_argmax(_hip.stream(), _hip.ptr(hm), B * K, H, W, None, None, _hip.ptr(preds), None, None, 0), "argmax")
    return preds


def _bits(t):
    return t.contiguous().view(torch.int32)


def ref_state(*a, **k):
    return torch.from_numpy(R.state_fp32(*a, **k))


# ---------------------------------------------------------------------------------------------- the golden cases, the old path
@pytest.mark.parametrize("case", R.GOLDEN_CASES, ids=lambda c: c[0])
def test_golden_cases(case):
    kd = _kd()
    name, shape, _ = case
    g = np.load(os.path.join(ROOT, "tests", "golden", "pck_curve.npz"))
    out, tgt = g[name + "/output"], g[name + "/target"]
    m = kd.PCKMeter(shape[1])
    pred = m.update(torch.from_numpy(out).cuda(), torch.from_numpy(tgt).cuda())
    assert torch.equal(m.state().cpu(), torch.from_numpy(R.state_fp32_heatmaps(out, tgt, np.asarray(kd.PCK_THRESHOLDS, dtype=np.float32))))
    assert np.array_equal(pred.cpu().numpy(), R.argmax_preds(out))
    rep = m.compute()
    acc = np.where(np.isnan(rep["pck"]), -1.0, rep["pck"]).T
    assert np.array_equal(acc, g[name + "/acc"])                               # ratios of the same integers, all 20 thresholds
    assert np.abs(rep["pck_mean"] - g[name + "/avg_acc"]).max() <= 1e-12
    assert rep["nonfinite"].sum() == 0 and rep["auc"] is not None


@pytest.mark.parametrize("shape", [(3, 5, 16, 16), (2, 16, 12, 20), (2, 16, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_single_threshold_equals_accuracy_device(shape):
    kd = _kd()
    o, t = (a.clone().cuda() for a in random_maps(*shape))
    t[:, 1] = -1.0                                   # joint 1 is absent from the batch
    acc, avg_cnt, pred_old = kd.accuracy_device(o, t)
    m = kd.PCKMeter(shape[1], thresholds=[0.5])
    pred = m.update(o, t)
    s = m.state()
    hits, count = s[:, 0], s[:, 1]
    present = count > 0
    assert present.any() and (~present).any()
    assert torch.equal(_bits((hits.float() / count.float())[present]), _bits(acc[present]))
    assert (acc[~present] == -1).all() and torch.equal(pred, pred_old)


# ---------------------------------------------------------------------------------------------- shapes, both forms
def check_both_forms(shape, T):
    kd = _kd()
    B, K, H, W = shape
    o, t = random_maps(*shape)
    thr = thresholds(T, top_of(H, W))
    m = kd.PCKMeter(K, thr)
    m.update(o.cuda(), t.cuda())
    exp = torch.from_numpy(R.state_fp32_heatmaps(o.numpy(), t.numpy(), np.asarray(thr, dtype=np.float32)))
    assert torch.equal(m.state().cpu(), exp)
    assert exp[:, T].sum() > 0 and exp[:, :T].sum() > 0 and (exp[:, 0] < exp[:, T]).any()           # visible pairs, hits and misses
    # the coordinate form on sub-pixel predictions with a mask: not what the fused form sees
    g = torch.Generator().manual_seed(B + K)
    pred = torch.from_numpy(R.argmax_preds(o.numpy())) + torch.rand(B, K, 2, generator=g) - 0.5
    gt = torch.from_numpy(R.argmax_preds(t.numpy())) + torch.rand(B, K, 2, generator=g) - 0.5
    vis = (torch.rand(B, K, generator=g) < 0.8).to(torch.uint8)
    nh, nw = H / 10.0, W / 10.0
    for v in (None, vis):
        code, state = accumulate_coords(pred.cuda(), gt.cuda(), thr, nh, nw, visible=None if v is None else v.cuda())
        assert code == 0
        assert torch.equal(state.cpu(), ref_state(pred.numpy(), gt.numpy(), thr, nh, nw, visible=None if v is None else v.numpy())), v is None
    m2 = kd.PCKMeter(K, thr)
    m2.update(o.cuda(), target_coords=gt.cuda(), visible=vis.bool().cuda())
    assert torch.equal(m2.state().cpu(), ref_state(R.argmax_preds(o.numpy()), gt.numpy(), thr, nh, nw, visible=vis.numpy()))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_fused_and_coordinate_forms(shape):
    check_both_forms(shape, 7)


@pytest.mark.parametrize("T", [1, 64])
def test_threshold_counts_fused_and_coordinate_forms(T):
    check_both_forms(SHAPES[0], T)


# ---------------------------------------------------------------------------------------------- fused equals unfused
def test_fused_equals_the_unfused_pieces():
    kd = _kd()
    B, K, H, W = 2, 6, 8, 12
    o, t = (a.clone() for a in random_maps(B, K, H, W))
    o[0, 0] = -1.0                                   # a plane of all -1: the prediction is zeroed
    o[0, 1, 3, 5] = float("nan")                     # a NaN is the maximum
    o[0, 2] = 0.25; o[0, 2, 2, 7] = 0.5; o[0, 2, 5, 1] = 0.5      # a two-way tie: the first flat index
    o[1, 0, 4, 4] = float("nan"); o[1, 0, 1, 2] = float("nan")    # two NaNs: the first
    t[0, 3] = 0.0; t[0, 3, 4, 6] = float("nan")      # a NaN target maximum: decoded (0, 0), not visible
    od, td = o.cuda(), t.cuda()
    m = kd.PCKMeter(K)
    pred = m.update(od, td)
    exp_pred = argmax_of(od)
    assert torch.equal(_bits(pred), _bits(exp_pred))
    assert pred[0, 0].tolist() == [0.0, 0.0] and pred[0, 2].tolist() == [7.0, 2.0]
    assert pred[0, 1].tolist() == pred[1, 0].tolist() == [0.0, 0.0]           # (a NaN maximum is not > 0: zeroed, as get_max_preds does)
    code, state = accumulate_coords(exp_pred, argmax_of(td), list(kd.PCK_THRESHOLDS), H / 10.0, W / 10.0)
    assert code == 0 and torch.equal(state, m.state())
    assert torch.equal(state.cpu(), torch.from_numpy(R.state_fp32_heatmaps(o.numpy(), t.numpy(), np.asarray(kd.PCK_THRESHOLDS, dtype=np.float32))))


# ---------------------------------------------------------------------------------------------- batch split, merge
def test_batch_split_invariance_and_merge():
    kd = _kd()
    B, K, H, W = 12, 5, 16, 16
    o, t = (a.cuda() for a in random_maps(B, K, H, W))
    norm = torch.linspace(2.0, 7.0, B).cuda()
    thr = thresholds(20, top_of(H, W))
    for decode, nrm in (("argmax", None), ("quarter", None), ("argmax", norm)):
        states = []
        for split in ((12,), (5, 4, 3), (1,) * 12):
            m = kd.PCKMeter(K, thr)
            a = 0
            for n in split:
                m.update(o[a:a + n], t[a:a + n], decode=decode, norm=None if nrm is None else nrm[a:a + n])
                a += n
            states.append(m.state().clone())
        assert states[0][:, 20].sum() > 0 and torch.equal(states[0], states[1]) and torch.equal(states[0], states[2]), decode
    m1, m2 = kd.PCKMeter(K, thr), kd.PCKMeter(K, thr)
    m1.update(o[:7], t[:7]); m2.update(o[7:], t[7:])
    m1.merge(m2)
    whole = kd.PCKMeter(K, thr)
    whole.update(o, t)
    assert torch.equal(m1.state(), whole.state())
    m2.merge(m2.state().cpu())                                       # a state tensor from another device
    m3 = kd.PCKMeter(K, thr)
    m3.update(o[7:], t[7:]); m3.update(o[7:], t[7:])
    assert torch.equal(m2.state(), m3.state())
    whole.reset()
    assert int(whole.state().abs().sum()) == 0
    with pytest.raises(ValueError):
        whole.merge(torch.zeros(K, 5, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------- sub-pixel decodes, coordinate targets
@functools.lru_cache(maxsize=None)
def gaussian_case(seed=5):
    """Heat-maps with one Gaussian (sigma 2) per plane at an un-rounded centre well inside a 32 x 32 map, the centres moved by up to
    0.7 px as coordinate targets, and a visibility mask."""
    B, K, H, W = 4, 6, 32, 32
    g = torch.Generator().manual_seed(seed)
    c = 8 + 16 * torch.rand(B, K, 2, generator=g)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    hm = torch.exp(-((xs - c[..., 0, None, None]) ** 2 + (ys - c[..., 1, None, None]) ** 2) / 8.0)
    coords = c + 1.4 * torch.rand(B, K, 2, generator=g) - 0.7
    vis = torch.rand(B, K, generator=g) < 0.85
    return hm, coords, vis


@pytest.mark.parametrize("decode", ["dark", "soft"])
def test_subpixel_decodes_against_coordinate_targets(decode):
    kd = _kd()
    hm, coords, vis = gaussian_case()
    B, K, H, W = hm.shape
    thr = [0.02 * j for j in range(1, 21)]           # d = e / 3.2: up to 1.28 px
    m = kd.PCKMeter(K, thr)
    pred = m.update(hm.cuda(), decode=decode, target_coords=coords.cuda(), visible=vis.cuda()).cpu().numpy()
    nh, nw = H / 10.0, W / 10.0
    state = m.state().cpu()
    assert torch.equal(state, ref_state(pred, coords.numpy(), thr, nh, nw, visible=vis.numpy()))
    # against fp64, with the derived bounds
    d, e, v = R.distances_fp64(pred, coords.numpy(), nh, nw, visible=vis.numpy())
    assert np.array_equal(v, vis.numpy()) and v.sum(0).min() > 0
    rep = m.compute()
    tol = 2.0 ** -17 + 4 * 2.0 ** -24 * e[v].max()  # half a fixed-point quantum + 4 fp32 ulps (the differences, two squares / sum, the root)
    epe64 = np.array([e[:, k][v[:, k]].mean() for k in range(K)])
    err = np.abs(rep["epe"] - epe64).max()
    print(f"{decode}: max |epe - fp64| {err:.3e} (bound {tol:.3e}), epe_mean {rep['epe_mean']:.4f} px")
    assert err <= tol
    t32 = np.asarray(thr, dtype=np.float32).astype(np.float64)
    close = (np.abs(d[..., None] - t32) <= 8 * 2.0 ** -24 * t32) & v[..., None]      # may fall either side: excluded
    print(f"{decode}: {int(close.sum())} of {int(v.sum()) * len(thr)} (pair, threshold) comparisons excluded")
    assert close.sum(axis=(0, 1)).max() <= 0.01 * v.sum() and close.sum() == 0       # (the seed shows none)
    assert np.array_equal(state[:, :20].numpy(), ((d[..., None] < t32) & v[..., None]).sum(0))
    assert 0 < state[:, :20].sum() and (state[:, 0] < state[:, 20]).any()


# ---------------------------------------------------------------------------------------------- norm, NaN coordinates
def test_per_sample_norm():
    kd = _kd()
    B, K, H, W = 6, 5, 16, 16
    o, t = random_maps(B, K, H, W)
    norm = torch.tensor([3.0, float("nan"), 0.0, -2.0, 5.5, float("inf")])
    thr = thresholds(7, 4.0)
    m = kd.PCKMeter(K, thr)
    m.update(o.cuda(), t.cuda(), norm=norm.cuda())
    exp = torch.from_numpy(R.state_fp32_heatmaps(o.numpy(), t.numpy(), np.asarray(thr, dtype=np.float32), norm=norm.numpy()))
    assert torch.equal(m.state().cpu(), exp)
    only = torch.from_numpy(R.state_fp32_heatmaps(o[[0, 4]].numpy(), t[[0, 4]].numpy(), np.asarray(thr, dtype=np.float32), norm=norm[[0, 4]].numpy()))
    assert torch.equal(exp, only) and exp[:, 7].sum() > 0                       # the four bad samples dropped out of every column
    pred, gt = torch.from_numpy(R.argmax_preds(o.numpy())), torch.from_numpy(R.argmax_preds(t.numpy()))
    code, state = accumulate_coords(pred.cuda(), gt.cuda(), thr, H / 10.0, W / 10.0, norm=norm.cuda())
    assert code == 0 and torch.equal(state.cpu(), exp)
    with pytest.raises(ValueError):
        m.update(o.cuda(), t.cuda(), norm=norm[:5].cuda())


def test_nan_prediction_coordinates():
    B, K = 5, 3
    g = torch.Generator().manual_seed(2)
    gt = 2 + 10 * torch.rand(B, K, 2, generator=g)
    pred = gt + torch.rand(B, K, 2, generator=g) - 0.5
    thr = thresholds(7, 1.0)
    _, clean = accumulate_coords(pred.cuda(), gt.cuda(), thr, 1.6, 1.6)
    bad = pred.clone()
    bad[1, 2, 0] = float("nan"); bad[3, 2, 1] = float("inf")
    code, state = accumulate_coords(bad.cuda(), gt.cuda(), thr, 1.6, 1.6)
    assert code == 0 and torch.equal(state.cpu(), ref_state(bad.numpy(), gt.numpy(), thr, 1.6, 1.6))
    assert torch.equal(state[:2], clean[:2])
    assert state[2, 7] == clean[2, 7] == B and state[2, 9] == 2 and clean[2, 9] == 0          # still counted, and flagged
    keep = torch.ones(B, K, dtype=torch.uint8); keep[1, 2] = 0; keep[3, 2] = 0
    _, rest = accumulate_coords(pred.cuda(), gt.cuda(), thr, 1.6, 1.6, visible=keep.cuda())
    assert torch.equal(state[2, :7], rest[2, :7]) and state[2, 8] == rest[2, 8]                 # no hit from them, the others' EPE unchanged


# ---------------------------------------------------------------------------------------------- capture
def test_update_captures_and_replays():
    kd = _kd()
    o, t = (a.cuda() for a in random_maps(3, 5, 16, 16))
    coords = argmax_of(t)
    for kw in ({"target": t}, {"target_coords": coords, "decode": "quarter"}):
        m = kd.PCKMeter(5)
        m.update(o, **kw)
        eager = m.state().clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            m.update(o, **kw)
        m.reset()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        assert eager[:, 20].sum() > 0 and torch.equal(m.state(), 3 * eager)


# ---------------------------------------------------------------------------------------------- engine.evaluate
@functools.lru_cache(maxsize=None)
def tiny_net_and_batches():
    """PoseResNet with one bottleneck per stage, K = 16, eval mode with running statistics of one train-mode forward; three batches of
    four 64x64 images, the second of which hides joint 3 completely."""
    from uda_poseestimation_amd import synthetic
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(0)
    net = pr._pose_resnet("t", 16, pr.Bottleneck_default, [1, 1, 1, 1], False, False)
    torch.nn.init.normal_(net.head.weight, std=0.05)
    net = net.cuda()
    batches = []
    for i in range(3):
        b = synthetic.mean_teacher_batch(4, num_keypoints=16, image_size=64, heatmap_size=16, seed=60 + i)
        label = b["label_s"].clone()
        if i == 1:
            label[:, 3] = 0
        batches.append((b["x_s"], label, b["weight_s"]))
    net.train()
    net.bn_momentum = 1.0
    with torch.no_grad():
        net(torch.cat([b[0] for b in batches]).cuda())
    net.bn_momentum = 0.1
    net.eval()
    return net, batches


def test_engine_evaluate():
    from uda_poseestimation_amd import engine
    kd = _kd()
    net, batches = tiny_net_and_batches()
    thr32 = np.asarray(kd.PCK_THRESHOLDS, dtype=np.float32)
    exp = np.zeros((16, 23), dtype=np.int64)
    for x, label, _ in batches:                      # validate()-style per-batch decodes, counted on the host over the whole set
        with torch.no_grad():
            y = net(x.cuda())
        exp += R.state_fp32(kd._decode(y)[0].cpu().numpy(), kd._decode(label.cuda())[0].cpu().numpy(), thr32, 1.6, 1.6)
    rep = engine.evaluate(batches, net, groups="body16")
    assert rep["n"] == 12 and np.array_equal(rep["count"], exp[:, 20]) and 0 < rep["count"][3] <= 8
    j0 = kd.PCK_THRESHOLDS.index(0.5)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(rep["pck"][:, j0], exp[:, j0] / exp[:, 20], equal_nan=True)
        assert np.array_equal(rep["pck"], exp[:, :20] / exp[:, 20:21], equal_nan=True)
    _, loss = engine.validate(batches, net)
    assert rep["loss"] == loss and not net.training
    assert list(rep["groups"]) == list(kd.JOINT_GROUPS["body16"])
    assert rep["groups"]["wrist"]["pck"][j0] == (rep["pck"][10, j0] + rep["pck"][15, j0]) / 2
    # the flip test: the merge launch's decode through the coordinate form = a meter fed flip_forward's heat-maps
    flip = engine.evaluate(batches, net, flip_pairs="body16")
    m = kd.PCKMeter(16)
    for x, label, _ in batches:
        m.update(engine.flip_forward(net, x.cuda(), "body16"), label.cuda())
    mine = m.compute()
    for key in ("count", "pck", "epe", "nonfinite"):
        assert np.array_equal(flip[key], mine[key], equal_nan=True), key
    assert flip["auc"] == mine["auc"] and not np.array_equal(flip["epe"], rep["epe"], equal_nan=True)
    # coordinate targets in the batch's fourth element, a per-sample length, another decode
    with_coords = [(x, label, w, {"target_coords": kd._decode(label.cuda())[0], "visible": kd._decode(label.cuda())[0].gt(1).all(-1)})
                   for x, label, w in batches]
    again = engine.evaluate(with_coords, net, norm=lambda batch: torch.full((batch[0].shape[0],), 1.6, device="cuda"))
    assert np.array_equal(again["count"], rep["count"]) and again["loss"] == rep["loss"]
    net.train()
    try:
        assert engine.evaluate(batches, net, thresholds=[0.5], decode="quarter")["auc"] is None and net.training      # the mode is restored
    finally:
        net.eval()
    with pytest.raises(ValueError):
        engine.evaluate(batches, net, thresholds=[0.5, 0.5])


# ---------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors():
    from uda_poseestimation_amd import _hip
    L, st = _hip.lib(), _hip.stream()
    B, K, H, W, T = 2, 3, 4, 4, 2
    hm = torch.rand(B, K, H, W, device="cuda")
    xy = torch.rand(B, K, 2, device="cuda")
    thr = torch.tensor([0.5, 1.0], device="cuda")
    state = torch.zeros(K, T + 3, dtype=torch.int64, device="cuda")
    p = _hip.ptr

    def coords(pred=xy, gt=xy, b=B, k=K, t=T, s=state, th=thr):
        return L.udapose_pck_accumulate(st, p(pred), p(gt), None, None, b, k, 0.4, 0.4, p(th), t, p(s))

    def maps(o=hm, g=hm, b=B, k=K, t=T, s=state, th=thr, h=H):
        return L.udapose_pck_accumulate_heatmaps(st, p(o), p(g), None, b, k, h, W, p(th), t, p(s), None)

    for call in (coords, maps):
        assert call() == 0
        assert call(s=None) == -1 and call(th=None) == -1 and call(t=0) == -1 and call(t=65) == -1 and call(b=0) == -1 and call(k=0) == -1
        assert call(k=257) == -3
    assert coords(pred=None) == -1 and coords(gt=None) == -1 and maps(o=None) == -1 and maps(g=None) == -1 and maps(h=0) == -1
    torch.cuda.synchronize()
