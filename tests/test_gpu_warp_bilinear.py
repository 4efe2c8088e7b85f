"""The bilinear re-warp on the MI355X (udapose_affine_bilinear through warp.warp_chain / warp.affine / warp.recon_heatmaps): forward
and backward of every case against tests/helpers/affine_bilinear_fp64.py in fp64, the adjoint identity, and bit-reproducibility.

THE BOUND is measured, not chosen.  For every case the same helper is also evaluated in fp32 on the CPU - torch's own fp32 arithmetic,
which the kernel restates - and its maximum absolute error against fp64 is the yardstick.  The device is allowed 4x that (it contracts the
coordinate expressions into FMAs and adds the four taps in its own order: each worth a few ulp of a coordinate, which a bilinear kernel
passes on continuously - there are no ties to exclude), with a floor of 4 ulp of the input's maximum magnitude for the cases whose
yardstick is 0.  The backward's yardstick is autograd through the fp32 helper.  Every case prints both figures.

BIT-EXACT cases: an identity or integer-translation chain must return the (shifted) input to the bit wherever torchvision's arithmetic
itself is exact, i.e. on planes whose sides are powers of two (16x16, 64x64): there 1 / (0.5 * W) is exact and every sample point is an
integer.  On 12x20 and 160x160 the divisions by 10, 6 and 80 round, and not even the fp64 reference returns its input (it is off by
1e-15 .. 2e-14; the fp32 helper by 4e-7 .. 1e-5): those shapes go by the measured bound, like every other case.

Shapes: [2,3,16,16] and the non-square [2,2,12,20] take the LDS form; [1,1,160,160] (2 x 100 KB > the 150 KB budget) the stage-by-stage
form from global memory; 1, 2 and 3 stages each.
"""
import pytest
import torch

from helpers.affine_bilinear_fp64 import chain_ref

pytestmark = pytest.mark.gpu
MARGIN = 4.0
EPS = float(torch.finfo(torch.float32).eps)

SHAPES = {"lds_16x16": (2, 3, 16, 16), "lds_12x20": (2, 2, 12, 20), "global_160x160": (1, 1, 160, 160)}
KINDS = ("loop", "identity", "int_shift", "half_shift", "out_of_frame", "scale4", "scale025", "zero")
EXACT_KINDS = ("identity", "int_shift")


def _pow2(v):
    return v & (v - 1) == 0


def _inv(angle, translate, scale, shear):
    from uda_poseestimation_amd.warp import inverse_affine_matrix
    return inverse_affine_matrix(angle, translate, scale, shear)


def make_thetas(kind, N, H, W, seed):
    """[N,3,6] fp32 matrices of one kind, different for every sample and stage."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * float(torch.rand((), generator=g))
    if kind == "loop":
        # the loop's own chain (warp.recon_thetas) with parameters over the reference's ranges; translations in image pixels at ratio 4
        from uda_poseestimation_amd.warp import recon_thetas
        ap = [[u(-180, 180) for _ in range(N)], [[u(-12, 12) for _ in range(N)], [u(-12, 12) for _ in range(N)]],
              [[u(-30, 30) for _ in range(N)], [u(-30, 30) for _ in range(N)]], [u(0.6, 1.3) for _ in range(N)]]
        return recon_thetas(ap, N, 4.0)
    th = torch.zeros(N, 3, 6)
    for n in range(N):
        for s in range(3):
            if kind == "identity":
                m = [1, 0, 0, 0, 1, 0]
            elif kind == "int_shift":
                m = [1, 0, int(u(-3, 4)), 0, 1, int(u(-3, 4))]
            elif kind == "half_shift":
                m = [1, 0, int(u(-2, 3)) + 0.5, 0, 1, int(u(-2, 3)) + (0.5 if s == 1 else 0.0)]
            elif kind == "out_of_frame":
                m = [1, 0, 3.0 * W, 0, 1, -2.0 * H] if s == 0 else _inv(u(-20, 20), [u(-1, 1), u(-1, 1)], 1.0, [0.0, 0.0])
            elif kind in ("scale4", "scale025"):
                up = (s % 2 == 0) == (kind == "scale4")
                m = _inv(u(-15, 15), [u(-1.5, 1.5), u(-1.5, 1.5)], 4.0 if up else 0.25, [0.0, 0.0])
            else:
                m = [0.0] * 6
            th[n, s] = torch.tensor(m, dtype=torch.float32)
    return th


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g), torch.randn(*shape, generator=g)


def _bar(yard, floor_of):
    return max(MARGIN * yard, 4.0 * EPS * float(floor_of.abs().max()))


_REFS = {}


def refs(shape_id, kind, S):
    """(x, g, theta, forward fp64, forward fp32, gradient fp64, gradient fp32): computed once per case, shared, never modified."""
    key = (shape_id, kind, S)
    if key not in _REFS:
        shape = SHAPES[shape_id]
        x, g = _inputs(shape, 1000 * list(SHAPES).index(shape_id) + 10 * KINDS.index(kind) + S)
        th = make_thetas(kind, shape[0], shape[2], shape[3], 100 + 7 * KINDS.index(kind) + shape[2])[:, :S].contiguous()
        out = {}
        for dt in (torch.float64, torch.float32):
            xr = x.clone().requires_grad_(True)
            y = chain_ref(xr, th, dt, "bilinear")
            y.backward(g.to(dt))
            out[dt] = (y.detach(), xr.grad.detach())
        _REFS[key] = (x, g, th, out[torch.float64][0], out[torch.float32][0], out[torch.float64][1], out[torch.float32][1])
    return _REFS[key]


def device_run(x, g, th, mode="bilinear"):
    from uda_poseestimation_amd import warp
    xd = x.cuda().requires_grad_(True)
    y = warp.warp_chain(xd, th.cuda(), mode)
    y.backward(g.cuda())
    torch.cuda.synchronize()
    return y.detach().cpu(), xd.grad.detach().cpu()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape_id", list(SHAPES))
def test_forward_backward_adjoint_and_determinism(shape_id, kind):
    N, C, H, W = SHAPES[shape_id]
    for S in (1, 2, 3):
        x, g, th, y64, y32, d64, d32 = refs(shape_id, kind, S)
        y, dx = device_run(x, g, th)
        y_again, dx_again = device_run(x, g, th)
        tag = f"{shape_id} {kind} stages={S}"
        # forward
        yard, err = float((y32.double() - y64).abs().max()), float((y.double() - y64).abs().max())
        bar_f = _bar(yard, x)
        print(f"{tag}: forward  max|device - fp64| {err:.3e}, fp32 helper (yardstick) {yard:.3e}, bar {bar_f:.3e}")
        assert err <= bar_f, f"{tag}: forward error {err:.3e} over the bar {bar_f:.3e} (yardstick {yard:.3e})"
        # backward
        yard_b, err_b = float((d32.double() - d64).abs().max()), float((dx.double() - d64).abs().max())
        bar_b = _bar(yard_b, g)
        print(f"{tag}: backward max|device - fp64| {err_b:.3e}, fp32 autograd (yardstick) {yard_b:.3e}, bar {bar_b:.3e}")
        assert err_b <= bar_b, f"{tag}: backward error {err_b:.3e} over the bar {bar_b:.3e} (yardstick {yard_b:.3e})"
        # <W x, g> == <x, W^T g>, both sides accumulated in fp64 from the device results.  Yardstick: the fp32 helper's own mismatch of the
        # two sides; floor: a sum whose every term carries the per-element floor (4 ulp of max|x| per output, of max|g| per gradient)
        adj = abs(float((y.double() * g.double()).sum() - (x.double() * dx.double()).sum()))
        adj_yard = abs(float((y32.double() * g.double()).sum() - (x.double() * d32.double()).sum()))
        adj_floor = 4.0 * EPS * (float(x.abs().max()) * float(g.abs().sum()) + float(g.abs().max()) * float(x.abs().sum()))
        adj_bar = max(MARGIN * adj_yard, adj_floor)
        print(f"{tag}: adjoint  |<Wx,g> - <x,W'g>| {adj:.3e}, fp32 helper {adj_yard:.3e}, bar {adj_bar:.3e}")
        assert adj <= adj_bar, f"{tag}: adjoint mismatch {adj:.3e} over the bar {adj_bar:.3e}"
        # two runs agree to the bit (no atomics, a fixed order), forward and backward
        assert torch.equal(y, y_again) and torch.equal(dx, dx_again), f"{tag}: two runs differ"
        if kind in EXACT_KINDS and _pow2(H) and _pow2(W):
            assert torch.equal(y.double(), y64), f"{tag}: not bit-exact"
            assert torch.equal(dx.double(), d64), f"{tag}: gradient not bit-exact"
            if kind == "identity":
                assert torch.equal(y, x) and torch.equal(dx, g)
        if kind == "out_of_frame":
            assert not y.any() and not dx.any()


def test_zero_theta_backward_on_a_64x64_plane_has_no_rank_limit():
    """4096 outputs on at most four input pixels, per stage: the gather scans the whole plane and adds them all, the same bits twice."""
    x, g = _inputs((2, 2, 64, 64), 5)
    th = torch.zeros(2, 3, 6)
    for S in (1, 3):
        t = th[:, :S].contiguous()
        xr = {}
        for dt in (torch.float64, torch.float32):
            xr[dt] = x.clone().requires_grad_(True)
            chain_ref(xr[dt], t, dt, "bilinear").backward(g.to(dt))
        d64, d32 = xr[torch.float64].grad, xr[torch.float32].grad
        y, dx = device_run(x, g, t)
        _, dx2 = device_run(x, g, t)
        yard, err = float((d32.double() - d64).abs().max()), float((dx.double() - d64).abs().max())
        bar = _bar(yard, g)
        print(f"zero theta 64x64 stages={S}: backward max|device - fp64| {err:.3e}, fp32 autograd {yard:.3e}, bar {bar:.3e}; "
              f"non-zero gradient pixels per plane {int((dx[0, 0] != 0).sum())}")
        assert err <= bar
        assert torch.equal(dx, dx2)
        assert int((dx[0, 0] != 0).sum()) == 4          # (the plane's 4096 outputs all landed on its four centre pixels)


def test_affine_with_bilinear_interpolation_equals_the_chain_with_its_matrix():
    from uda_poseestimation_amd import warp
    x = torch.rand(3, 5, 16, 24, generator=torch.Generator().manual_seed(2)).cuda()
    args = (33.0, [2.5, -1.25], 0.8, [10.0, -5.0])
    m = torch.tensor(warp.inverse_affine_matrix(args[0], args[1], args[2], args[3]), dtype=torch.float32).reshape(1, 1, 6)
    want = warp.warp_chain(x, m.expand(3, 1, 6).contiguous().cuda(), "bilinear")
    for spelling in ("bilinear", 2):
        assert torch.equal(warp.affine(x, *args, interpolation=spelling), want)
    got3 = warp.affine(x[1], *args, interpolation="bilinear")
    assert got3.shape == x[1].shape and torch.equal(got3, want[1])
    assert not torch.equal(want, warp.affine(x, *args))          # (it is not the nearest result)
    # differentiable through the public call, like the nearest form
    xg = x.clone().requires_grad_(True)
    warp.affine(xg, *args, interpolation="bilinear").sum().backward()
    assert xg.grad is not None and float(xg.grad.abs().sum()) > 0


def test_recon_heatmaps_mode_and_unchanged_nearest_results():
    from uda_poseestimation_amd import synthetic, warp
    b = synthetic.mean_teacher_batch(4, num_keypoints=4, image_size=64, heatmap_size=16, seed=3)
    y = torch.rand(4, 4, 16, 16, generator=torch.Generator().manual_seed(4)).cuda()
    th = warp.recon_thetas(b["aug_param_stu"], 4, 4.0, "cuda")
    assert torch.equal(warp.recon_heatmaps(y, b["aug_param_stu"], 4.0, mode="bilinear"), warp.warp_chain(y, th, "bilinear"))
    # nearest through the new keyword is the call without it, forward and backward
    g = torch.randn(4, 4, 16, 16, generator=torch.Generator().manual_seed(5)).cuda()
    res = []
    for kw in ({}, {"mode": "nearest"}):
        yg = y.clone().requires_grad_(True)
        out = warp.warp_chain(yg, th, **kw)
        out.backward(g)
        res.append((out.detach(), yg.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(warp.recon_heatmaps(y, b["aug_param_stu"], 4.0), warp.recon_heatmaps(y, b["aug_param_stu"], 4.0, mode="nearest"))
    assert torch.equal(warp.affine(y, 20.0, [1, 2], 1.1, [3.0, 0.0]), warp.affine(y, 20.0, [1, 2], 1.1, [3.0, 0.0], interpolation="nearest"))


def test_16bit_input_returns_its_dtype_and_a_gradient():
    from uda_poseestimation_amd import warp
    x = torch.rand(2, 2, 16, 16, generator=torch.Generator().manual_seed(6)).cuda().half().requires_grad_(True)
    th = make_thetas("loop", 2, 16, 16, 9).cuda()
    y = warp.warp_chain(x, th, "bilinear")
    y.float().sum().backward()
    assert y.dtype == torch.float16 and x.grad.dtype == torch.float16
    assert torch.equal(y, warp.warp_chain(x.detach().float(), th, "bilinear").half())
