"""The merge of teacher views by agreement on the MI355X (csrc/view_merge.hip through warp.merge_views and the mean-teacher step) against the
numpy restatement of its definitions (tests/helpers/view_merge_ref.py).

Everything discrete (peaks, inlier masks, counts, spread2, agree) and the mean are compared BIT FOR BIT: the kernel adds the views in view
order in fp32 and divides once, which is what the restatement does.  Only `energy` has a bar, and it is derived, not measured:
(4k + 8 + ceil(log2(H*W))) * 2^-23 * E_abs against the fp64 value (view_merge_ref.energy_bound).

Shapes: 64x64 and 96x96 (threads loop, 16-byte accesses), 5x7 (a plane smaller than a wave, element accesses), 1x1, 64x63 (H*W % 4 != 0 on a
plane of several quads per thread); k = 1, 2, 3 and the full 8; 1, 3 and 34 planes.  The constructed planes of tests/test_view_merge_cpu.py sit
at planes 0.. of every input (as many as the input has planes)."""
import functools

import numpy as np
import pytest
import torch

from helpers import view_merge_ref as REF

pytestmark = pytest.mark.gpu
SHAPES = [(64, 64), (96, 96), (5, 7), (1, 1), (64, 63)]
KS = [1, 2, 3, 8]
PLANES = {1: (1, 1), 3: (1, 3), 34: (2, 17)}          # R -> (B, K)
RADIUS = REF.CONSTRUCTED_RADIUS
CASES = [pytest.param(s, k, id=f"{s[0]}x{s[1]}-k{k}") for s in SHAPES for k in KS]
FIELDS = ("mean", "peaks", "maxvals", "inliers", "n_inliers", "spread2", "agree", "energy")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _inputs(H, W, k, R):
    """k views [B, K, H, W]: weak noise plus one Gaussian bump per view near a common position per plane; now and then a view far off, or a view
    that is non-positive everywhere.  The constructed planes replace planes 0.."""
    rng = np.random.RandomState(1000 * H + 10 * W + k + 7 * R)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    views = np.empty((k, R, H, W), np.float32)
    for r in range(R):
        cx, cy = rng.randint(0, W), rng.randint(0, H)
        for v in range(k):
            noise = rng.uniform(-0.05, 0.2, (H, W)).astype(np.float32)
            u = rng.rand()
            if u < 0.1:
                views[v, r] = -np.abs(noise)                                   # an invalid view
                continue
            px, py = (rng.randint(0, W), rng.randint(0, H)) if u < 0.25 else (cx + rng.randint(-2, 3), cy + rng.randint(-2, 3))
            amp = np.float32(rng.uniform(0.5, 1.0))
            views[v, r] = noise + amp * np.exp(-((xs - px) ** 2 + (ys - py) ** 2) / np.float32(4.5))
    for r, name in enumerate(REF.CONSTRUCTED[:R]):
        views[:, r] = REF.constructed_plane(name, k, H, W)
    B, K = PLANES[R]
    return tuple(np.ascontiguousarray(views[v].reshape(B, K, H, W)) for v in range(k))


@functools.lru_cache(maxsize=None)
def _ref(H, W, k, R, mode, min_views, want_energy=False):
    return REF.merge(_inputs(H, W, k, R), RADIUS, mode, min_views, want_energy)


@functools.lru_cache(maxsize=None)
def _dev(H, W, k, R, mode, min_views, want_energy=False):
    from uda_poseestimation_amd import warp
    out = warp.merge_views([torch.from_numpy(v).cuda() for v in _inputs(H, W, k, R)], RADIUS, mode, min_views, want_energy)
    torch.cuda.synchronize()
    return warp.MergedViews(*[None if t is None else t.cpu().numpy() for t in out])


def _combos(k):
    return [(R, mode, mv) for R in PLANES for mode in ("mean", "trimmed") for mv in sorted({1, k})]


# ---------------------------------------------------------------------------------------------- 1: everything discrete
@pytest.mark.parametrize("shape,k", CASES)
def test_peaks_inliers_and_agreement_equal_the_restatement_bit_for_bit(shape, k):
    from uda_poseestimation_amd import utils
    H, W = shape
    seen = set()
    for R, mode, mv in _combos(k):
        dev, ref = _dev(H, W, k, R, mode, mv), _ref(H, W, k, R, mode, mv)
        for f in ("peaks", "maxvals", "inliers", "n_inliers", "spread2", "agree"):
            assert _same(getattr(dev, f), getattr(ref, f)), (R, mode, mv, f)
        assert dev.energy is None
        seen |= set(dev.n_inliers.reshape(-1).tolist())
        if mode == "mean" and mv == 1:          # the peaks are the arg-max decode's, view by view
            for v, x in enumerate(_inputs(H, W, k, R)):
                preds, maxv = utils.get_max_preds_torch_raw(torch.from_numpy(x).cuda())
                assert np.array_equal(preds.cpu().numpy().astype(np.int32), dev.peaks[v]) and _same(maxv[..., 0].cpu().numpy(), dev.maxvals[v])
    big = _ref(H, W, k, 34, "mean", k)
    print(f"\n{H}x{W} k={k}: inlier counts seen {sorted(seen)}; 34 planes: agree on {int(big.agree.sum())}, spread2 up to {int(big.spread2.max())}")
    assert 0 in seen and k in seen              # a plane without a valid view and a plane on which every view is inside are among the inputs


# ---------------------------------------------------------------------------------------------- 2: the mean
@pytest.mark.parametrize("shape,k", CASES)
def test_mean_is_the_fp32_sequence_and_mode_mean_is_mean_views(shape, k):
    from uda_poseestimation_amd import warp
    H, W = shape
    differ = 0
    for R, mode, mv in _combos(k):
        dev, ref = _dev(H, W, k, R, mode, mv), _ref(H, W, k, R, mode, mv)
        assert _same(dev.mean, ref.mean), (R, mode, mv)
        if mode == "mean" and mv == 1:
            plain = warp.mean_views([torch.from_numpy(v).cuda() for v in _inputs(H, W, k, R)])
            assert _same(plain.cpu().numpy(), dev.mean), R
        if mode == "trimmed":
            differ += int(not _same(dev.mean, _dev(H, W, k, R, "mean", mv).mean))
    assert differ > 0 or k == 1                 # with k >= 2 the inputs hold outliers: trimming changes the map somewhere


# ---------------------------------------------------------------------------------------------- 3: the energy
@pytest.mark.parametrize("shape,k", CASES)
def test_energy_is_within_the_derived_rounding_bound_of_fp64(shape, k):
    """Worst measured |energy - fp64| / bound over all cases of this file on one MI355X: see profiles/view_merge.txt."""
    H, W = shape
    worst = 0.0
    for R in PLANES:
        for mode in ("mean", "trimmed"):        # (with energy both modes take the two-pass form; the mean must still be the same bits)
            dev, ref = _dev(H, W, k, R, mode, k, True), _ref(H, W, k, R, "mean", k, True)
            assert _same(dev.mean, _ref(H, W, k, R, mode, k).mean) and _same(dev.inliers, ref.inliers)
            err = np.abs(dev.energy.astype(np.float64) - ref.energy)
            bound = REF.energy_bound(k, H, W, ref.energy_abs)
            ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
            worst = max(worst, ratio)
            assert dev.energy.dtype == np.float32 and dev.energy.shape == ref.energy.shape
        assert _same(_dev(H, W, k, R, "mean", k, True).energy, _dev(H, W, k, R, "trimmed", k, True).energy)     # all views count in either mode
    print(f"\n{H}x{W} k={k}: largest |energy - fp64| / bound = {worst:.4f}")
    assert worst <= 1.0
    if k == 1:
        assert all(not _dev(H, W, 1, R, "mean", 1, True).energy.any() for R in PLANES)          # one view has no variance


# ---------------------------------------------------------------------------------------------- 4: reproducible, and the same on both access paths
def test_two_runs_agree_and_an_unaligned_base_takes_the_scalar_path_with_the_same_bits():
    from uda_poseestimation_amd import warp
    H, W, k, R = 64, 64, 3, 34
    B, K = PLANES[R]
    host = _inputs(H, W, k, R)
    aligned = [torch.from_numpy(v).cuda() for v in host]
    shifted = []
    for v in host:
        buf = torch.empty(v.size + 1, device="cuda")
        view = buf[1:].view(B, K, H, W)
        view.copy_(torch.from_numpy(v))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        shifted.append(view)
    for mode in ("mean", "trimmed"):
        for want_energy in (False, True):
            runs = [warp.merge_views(vs, RADIUS, mode, 2, want_energy) for vs in (aligned, aligned, shifted)]
            torch.cuda.synchronize()
            for f in FIELDS:
                a, b, c = (getattr(o, f) for o in runs)
                if a is None:
                    assert f == "energy" and not want_energy
                    continue
                assert _same(a.cpu().numpy(), b.cpu().numpy()), (mode, want_energy, f, "second run")
                assert _same(a.cpu().numpy(), c.cpu().numpy()), (mode, want_energy, f, "base pointer + 4 bytes")
            assert _same(runs[0].mean.cpu().numpy(), _ref(H, W, k, R, mode, 2).mean)


# ---------------------------------------------------------------------------------------------- 5: captured
def test_a_captured_launch_follows_the_radius_on_the_device():
    from uda_poseestimation_amd import warp
    H, W, k, R = 64, 64, 3, 34
    views = [torch.from_numpy(v).cuda() for v in _inputs(H, W, k, R)]
    rad = torch.tensor(0.5, dtype=torch.float32, device="cuda")

    def run(radius):
        return warp.merge_views(views, radius, "trimmed", None, True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(rad)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(rad)
    got = {}
    for value in (0.5, float("inf")):
        rad.fill_(value)
        graph.replay()
        torch.cuda.synchronize()
        got[value] = [t.cpu().numpy().copy() for t in captured]
        eager = run(value)
        torch.cuda.synchronize()
        for f, c, e in zip(FIELDS, got[value], eager):
            assert _same(c, e.cpu().numpy()), (value, f)
        ref = REF.merge(_inputs(H, W, k, R), value, "trimmed", None)
        assert _same(got[value][FIELDS.index("inliers")], ref.inliers) and _same(got[value][0], ref.mean)
    n_small, n_inf = (got[v][FIELDS.index("n_inliers")] for v in (0.5, float("inf")))
    assert (n_inf >= n_small).all() and (n_inf > n_small).any()          # the replay read the new radius
    assert not _same(got[0.5][0], got[float("inf")][0])


# ---------------------------------------------------------------------------------------------- 6: refusals
def test_bad_arguments_return_an_error_code_and_write_nothing():
    import ctypes as C
    from uda_poseestimation_amd import _hip
    lib, st = _hip.lib(), _hip.stream()
    ERR_ARG = -1
    k, R, H, W = 3, 4, 8, 8
    views = [torch.rand(R, H, W, device="cuda") for _ in range(9)]
    rad = torch.tensor(2.0, device="cuda")

    def sentinel(*shape, dtype=torch.int32):
        return torch.full(shape, -1, dtype=torch.int32, device="cuda").view(dtype)         # 0xFF bytes

    outs = [sentinel(R, H, W, dtype=torch.float32), sentinel(k, R, 2), sentinel(k, R, dtype=torch.float32), sentinel(R), sentinel(R), sentinel(R),
            sentinel(R, dtype=torch.float32), sentinel(R, dtype=torch.float32)]
    p = [t.data_ptr() for t in outs]

    def arr(n, null_at=None):
        return (C.c_void_p * n)(*[None if j == null_at else views[j].data_ptr() for j in range(n)])

    r = rad.data_ptr()
    cases = [("k = 0", (arr(1), 0, R, H, W, 0, r, 1, *p)), ("k = 9", (arr(9), 9, R, H, W, 0, r, 1, *p)),
             ("a null view", (arr(k, null_at=1), k, R, H, W, 0, r, 1, *p)), ("a null view array", (None, k, R, H, W, 0, r, 1, *p)),
             ("null mean", (arr(k), k, R, H, W, 0, r, 1, None, *p[1:])), ("null radius", (arr(k), k, R, H, W, 0, None, 1, *p)),
             ("min_views = 0", (arr(k), k, R, H, W, 0, r, 0, *p)), ("min_views = k + 1", (arr(k), k, R, H, W, 0, r, k + 1, *p)),
             ("H = 0", (arr(k), k, R, 0, W, 0, r, 1, *p)), ("W = 0", (arr(k), k, R, H, 0, 0, r, 1, *p)), ("W = -1", (arr(k), k, R, H, -1, 0, r, 1, *p)),
             ("mode = 2", (arr(k), k, R, H, W, 2, r, 1, *p)), ("mode = -1", (arr(k), k, R, H, W, -1, r, 1, *p)),
             ("R = 0", (arr(k), k, 0, H, W, 0, r, 1, *p))]
    for name, args in cases:
        assert lib.udapose_view_merge(st, *args) == ERR_ARG, name
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t.view(torch.int32) == -1).all())
    # and the same call with good arguments runs (every optional output absent, then present)
    assert lib.udapose_view_merge(st, arr(k), k, R, H, W, 1, r, k, p[0], *([None] * 7)) == 0
    assert lib.udapose_view_merge(st, arr(k), k, R, H, W, 1, r, k, *p) == 0
    torch.cuda.synchronize()
    ref = REF.merge([v.cpu().numpy() for v in views[:k]], 2.0, "trimmed", k, True)
    assert _same(outs[0].cpu().numpy(), ref.mean) and _same(outs[3].cpu().numpy(), ref.inliers) and _same(outs[6].cpu().numpy(), ref.agree)


# ---------------------------------------------------------------------------------------------- 7: the step (tiny network, three teacher views)
N_, K_, S = 4, 16, 128
DEFAULT_KEYS = {"loss_all", "loss_s", "loss_c", "y_s", "tea_mask", "y_t_tea_recon", "y_t_stu_recon"}


def _step_inputs():
    from uda_poseestimation_amd import synthetic
    bs = [synthetic.mean_teacher_batch(N_, num_keypoints=K_, image_size=S, heatmap_size=S // 4, seed=s) for s in (71, 72, 73)]
    g = [{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()} for b in bs]
    first = g[0]
    return (first["x_s"], first["label_s"], first["weight_s"], first["x_t_stu"], [b["x_t_tea"] for b in g], first["aug_param_stu"],
            [b["aug_param_tea"] for b in g])


def test_the_step_with_merged_views_gates_the_mask_and_leaves_the_default_step_alone():
    from test_gpu_steps import _tiny
    from uda_poseestimation_amd import warp
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    x_s, label_s, weight_s, x_t_stu, x_t_teas, ap_stu, aps_tea = _step_inputs()
    stu, tea = _tiny(K_, seed=8), _tiny(K_, seed=8)
    with torch.no_grad():
        # a positive head bias (the head's weights are initialised at 1e-3): every re-warped teacher map has a positive maximum, so every plane
        # has a valid view.  On a plane WITHOUT one agree is 0 and the mask kernels compare 0 * confidence instead of the (non-positive)
        # confidence with the threshold - check (a) is about the planes where the gate is 1.
        stu.head.bias.fill_(0.25)
    tr = MeanTeacherTrainer(stu.cuda(), tea.cuda(), lr=1e-4, image_size=S, heatmap_size=S // 4, precision="bf16")
    assert (tr.view_merge, tr.view_radius, tr.view_min) == (None, 2.0, None)
    th_s = warp.recon_thetas(ap_stu, N_, tr.ratio, "cuda")
    th_t = [warp.recon_thetas(ap, N_, tr.ratio, "cuda") for ap in aps_tea]

    def fwd_bwd():
        """One eager forward + backward of the step, no optimizer update: every call starts from the same weights."""
        st = tr._forward_part(x_s, label_s, weight_s, x_t_stu, x_t_teas, th_s, th_t)
        out = tr._loss_backward_part(st, None)
        tr._sync_grads()
        tr.student.finish_grads()
        torch.cuda.synchronize()
        return out, tr.student._flat_grad.clone()

    def rewarped_teacher_views():
        tr.teacher.train()
        with torch.no_grad():
            return [warp.warp_chain(tr.teacher(x), th, tr.warp_mode) for x, th in zip(x_t_teas, th_t)]

    off, g_off = fwd_bwd()
    assert set(off) == DEFAULT_KEYS and tr._view_rad is None
    # (a) the plain mean, every valid view an inlier, one inlier enough: the gate is 1 everywhere and multiplies the confidences by 1.0
    tr.view_merge, tr.view_radius, tr.view_min = "mean", float("inf"), 1
    on, g_on = fwd_bwd()
    assert bool((on["view_n_inliers"] >= 1).all()) and bool((on["view_agree"] == 1).all())
    for key in ("loss_all", "tea_mask", "y_t_tea_recon"):
        assert on[key].dtype == off[key].dtype and _same(on[key].float().cpu().numpy(), off[key].float().cpu().numpy()), key
    assert _same(g_on.cpu().numpy(), g_off.cpu().numpy()) and bool(g_off.any()) and bool(off["tea_mask"].any())
    # (b) radius 0: only views whose peak IS the medoid's are inliers; with view_min = k a joint passes only where all three peaks coincide
    tr.view_radius, tr.view_min, tr.mask_mode = 0.0, None, "per_joint"
    out_b, _ = fwd_bwd()
    ref = REF.merge([v.cpu().numpy() for v in rewarped_teacher_views()], 0.0, "mean", None)
    assert _same(out_b["view_agree"].cpu().numpy(), ref.agree) and _same(out_b["view_n_inliers"].cpu().numpy(), ref.n_inliers)
    assert _same(out_b["view_spread2"].cpu().numpy(), ref.spread2)
    assert not bool((out_b["tea_mask"] & ~out_b["view_agree"].bool()).any())
    print(f"\nradius 0, three views: {int(ref.agree.sum())} of {N_ * K_} joints agree; mask {int(out_b['tea_mask'].sum())}; "
          f"spread2 up to {int(ref.spread2.max())}")
    assert float(tr._view_rad[0]) == 0.0                              # the device scalar followed the host value
    # (c) trimmed at the default radius: the teacher's map is the merge of the three re-warps
    tr.view_merge, tr.view_radius, tr.mask_mode = "trimmed", 2.0, "global"
    out_c, _ = fwd_bwd()
    again = warp.merge_views(rewarped_teacher_views(), 2.0, "trimmed")
    assert torch.equal(out_c["y_t_tea_recon"].view(torch.int32), again.mean.view(torch.int32))
    assert torch.equal(out_c["view_agree"], again.agree) and torch.equal(out_c["view_n_inliers"], again.n_inliers)
    assert set(out_c) == DEFAULT_KEYS | {"view_agree", "view_n_inliers", "view_spread2"}
    assert not bool((out_c["tea_mask"] & ~out_c["view_agree"].bool()).any())
    # (d) what cannot run says so: a captured step stages one teacher view; one view has nothing to agree with
    one_view = (x_s, label_s, weight_s, x_t_stu, x_t_teas[0], ap_stu, aps_tea[0])
    with pytest.raises(ValueError, match="view_merge"):
        GraphedTrainStep(tr, *one_view)
    with pytest.raises(ValueError, match="at least two"):
        tr.train_step(*one_view)
    with pytest.raises(ValueError, match="at least two"):
        tr.train_step(x_s, label_s, weight_s, x_t_stu, x_t_teas[:1], ap_stu, aps_tea[:1])
