"""Soft-argmax decode and coordinate losses on the MI355X (csrc/softargmax.hip through lib.keypoint_detection.soft_argmax,
lib.models.loss.JointsSoftArgmaxLoss / ConsSoftArgmaxLoss): values and gradients against fp64 autograd of the plain-torch restatement
(tests/helpers/soft_argmax_fp64.py, checked against independent forms by tests/test_soft_argmax_cpu.py), the fixed cases (ties, constant
rows, non-positive rows, NaN / inf, a temperature at which the decode IS the arg-max), 16-bit inputs, capture and replay, PCK with the
soft decode, and the mean-teacher step with the coordinate criteria.

THE BOUND of the value / gradient comparisons is measured, not chosen: the same restatement is evaluated in fp32
torch on the CPU, its worst error against fp64 over the shapes of a test is the yardstick, and the device is allowed 4x that figure.
Coordinates: max abs error in pixels, with a floor of 4 ulp of max(H, W) (the coordinate is an fp32 number of that magnitude).  Loss
values: relative error.  Gradients: max abs error / max|gradient|.  Every test prints the device | fp32 pairs.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import soft_argmax_fp64 as S64

pytestmark = pytest.mark.gpu
MARGIN = 4.0
MAPS = [(16, 16), (7, 9), (64, 64), (72, 72)]        # registers; HW = 63, element by element; exactly 4096; 5184, re-read
BK = [(2, 3), (1, 33)]
CONFIGS = [(1.0, -1), (10.0, 5), (10.0, 0), (30.0, 3)]


def _kd():
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    return kd


def _losses():
    from uda_poseestimation_amd.lib.models import loss as L
    return L


def _win(window):
    return None if window < 0 else window


def _bits(t):
    return t.contiguous().view(torch.int32)


def bump_centres(R, H, W, g):
    """[R,2] (x, y) sub-pixel centres; row r with r % 9 < 8 sits at a corner / on an edge of the map, the others anywhere."""
    c = torch.rand(R, 2, generator=g, dtype=torch.float64) * torch.tensor([W - 1.0, H - 1.0], dtype=torch.float64)
    forced = [(0.2, 0.3), (W - 1.3, 0.2), (0.3, H - 1.2), (W - 1.2, H - 1.3), (W / 2 + 0.4, 0.1), (W / 2 - 0.3, H - 1.1), (0.2, H / 2 + 0.3),
              (W - 1.1, H / 2 - 0.4)]
    for r in range(R):
        if r % 9 < 8:
            c[r] = torch.tensor(forced[r % 9], dtype=torch.float64)
    return c


def bumps(centres, H, W, sigma, amp=1.0):
    y, x = torch.arange(H, dtype=torch.float64)[:, None], torch.arange(W, dtype=torch.float64)[None, :]
    cx, cy = centres[:, 0, None, None], centres[:, 1, None, None]
    return amp * torch.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma * sigma))


@functools.lru_cache(maxsize=None)
def make_maps(B, K, H, W, seed):
    """fp32 [B,K,H,W] Gaussian bumps at sub-pixel centres plus N(0, 0.02) noise (bump_centres: corners and edges included), and the
    centres [B,K,2]."""
    g = torch.Generator().manual_seed(seed)
    c = bump_centres(B * K, H, W, g)
    hm = bumps(c, H, W, 1.5 if min(H, W) < 10 else 2.0) + 0.02 * torch.randn(B * K, H, W, generator=g, dtype=torch.float64)
    return hm.float().reshape(B, K, H, W), c.reshape(B, K, 2)


def coord_floor(H, W):
    return 4.0 * float(np.spacing(np.float32(max(H, W))))


# ---------------------------------------------------------------------------------------------- decode and its gradient
@functools.lru_cache(maxsize=None)
def reference_decode(B, K, H, W, beta, window, seed):
    """(coords, gradient) of the restatement in fp64 and in fp32 on the CPU, for the upstream gradient `up` [B,K,2]."""
    hm, _ = make_maps(B, K, H, W, seed)
    up = torch.randn(B, K, 2, generator=torch.Generator().manual_seed(seed + 1000))
    out = {}
    for dt in (torch.float64, torch.float32):
        x = hm.to(dt).clone().requires_grad_(True)
        c, m = S64.decode(x, beta, _win(window))
        c.backward(up.to(dt))
        out[dt] = (c.detach(), x.grad.detach(), m)
    return hm, up, out


@pytest.mark.parametrize("beta,window", CONFIGS, ids=[f"beta{b:g}_win{w}" for b, w in CONFIGS])
def test_decode_and_gradient_match_fp64(beta, window):
    kd = _kd()
    res, bad = [], []
    for (H, W) in MAPS:
        for i, (B, K) in enumerate(BK):
            hm, up, ref = reference_decode(B, K, H, W, beta, window, 11 + i)
            (c64, g64, m64), (c32, g32, _) = ref[torch.float64], ref[torch.float32]
            x = hm.cuda().requires_grad_(True)
            c, m = kd.soft_argmax(x, beta, _win(window))
            assert c.shape == (B, K, 2) and m.shape == (B, K, 1) and c.dtype == torch.float32 and not m.requires_grad
            c.backward(up.cuda())
            gd = x.grad.cpu()
            assert torch.equal(m.cpu().double(), m64) and gd.shape == hm.shape and gd.dtype == torch.float32
            assert torch.equal(m, kd.get_max_preds(hm.cuda())[1])
            ec = (float((c.detach().cpu().double() - c64).abs().max()), float((c32.double() - c64).abs().max()))
            gm = float(g64.abs().max())
            if window == 0:
                # the arg-max alone: p = 1 at (cx, cy), every term of the gradient is a product with an exact zero
                assert gm == 0.0 and not gd.any() and torch.equal(c.detach().cpu().double(), c64)
                eg = (0.0, 0.0)
            else:
                assert gm > 0
                eg = (float((gd.double() - g64).abs().max()) / gm, float((g32.double() - g64).abs().max()) / gm)
            res.append(((B, K, H, W), ec, eg))
    yc, yg = max(r[1][1] for r in res), max(r[2][1] for r in res)
    print(f"\nsoft_argmax beta={beta:g} window={window}: error against fp64, device | fp32 torch on the CPU "
          f"(coordinates: max abs, px; gradient: max abs / max|grad|); yardsticks {yc:.2e} px, {yg:.2e}")
    for s, ec, eg in res:
        barc = max(MARGIN * yc, coord_floor(s[2], s[3]))
        print(f"  {str(s):18s} coordinates {ec[0]:.2e} | {ec[1]:.2e} (bar {barc:.2e})   gradient {eg[0]:.2e} | {eg[1]:.2e} (bar {MARGIN * yg:.2e})")
        if ec[0] > barc:
            bad.append((s, "coordinates", ec[0], barc))
        if eg[0] > MARGIN * yg:
            bad.append((s, "gradient", eg[0], MARGIN * yg))
    assert not bad, bad


def test_numpy_in_numpy_out_and_the_decode_of_the_motivating_experiment():
    """The CPU experiment of tests/test_soft_argmax_cpu.py on the device: 0.0036 px against the arg-max's 0.378 px."""
    from test_soft_argmax_cpu import subpixel_experiment
    kd = _kd()
    hm, centres = subpixel_experiment()
    c, m = kd.soft_argmax(hm.numpy().astype(np.float32), 10.0, 5)
    assert isinstance(c, np.ndarray) and c.dtype == np.float32 and c.shape == (8, 16, 2) and isinstance(m, np.ndarray) and m.shape == (8, 16, 1)
    soft = float(np.linalg.norm(c - centres.numpy(), axis=-1).mean())
    hard = float(np.linalg.norm(kd.get_max_preds(hm.numpy().astype(np.float32))[0] - centres.numpy(), axis=-1).mean())
    print(f"\nmean error on the device: soft-argmax(beta=10, window=5) {soft:.4f} px, arg-max {hard:.3f} px")
    assert soft <= 0.01 and hard >= 0.3


def test_fixed_cases_ties_constant_rows_nonpositive_rows_nan_and_bad_beta():
    kd = _kd()
    H, W = 16, 20
    hm = torch.zeros(1, 8, H, W)
    hm[0, 0, 3, 4] = hm[0, 0, 9, 15] = 1.0                      # two equal maxima: the window sits round the first
    hm[0, 1] = 0.25                                              # a constant row: the first pixel is the arg-max
    hm[0, 2] = -1.0 - torch.rand(H, W, generator=torch.Generator().manual_seed(1))      # maximum < 0
    hm[0, 2, 7, 11] = -0.5
    hm[0, 3, 5, 6], hm[0, 3, 12, 2] = 3.0, float("nan")          # a NaN far from the finite peak: NaN is the maximum
    hm[0, 4, 8, 8] = float("inf")
    hm[0, 5] = float("-inf")
    hm[0, 6, 10, 10], hm[0, 6, 10, 11], hm[0, 6, 2, 2] = 1.0, float("-inf"), float("-inf")      # -inf below a finite maximum: weight 0
    hm[0, 7, 0, 0] = 0.5
    for window in (3, None):
        c64, m64 = S64.decode(hm.double(), 10.0, window)
        c, m = kd.soft_argmax(hm.cuda(), 10.0, window)
        c, m = c.cpu(), m.cpu()
        assert torch.equal(torch.isnan(c), torch.isnan(c64)) and torch.isnan(c64[0, 3:6]).all() and not torch.isnan(c64[0, [0, 1, 2, 6, 7]]).any()
        ok = ~torch.isnan(c64)
        assert float((c.double()[ok] - c64[ok]).abs().max()) <= 1e-4
        assert torch.equal(torch.isnan(m), torch.isnan(m64)) and torch.equal(m.double()[~torch.isnan(m64)], m64[~torch.isnan(m64)])
    c, m = (t.cpu() for t in kd.soft_argmax(hm.cuda(), 10.0, 3))
    e = float(np.exp(-10.0))
    assert abs(float(c[0, 0, 0]) - 4.0) < 1e-6 and abs(float(c[0, 0, 1]) - 3.0) < 1e-6          # the second maximum is outside the window
    assert torch.allclose(c[0, 1], torch.tensor([1.5, 1.5]), atol=1e-6, rtol=0)                # the clipped 4x4 window round (0, 0), uniform
    # a row whose maximum is <= 0 keeps its soft coordinates here ...
    assert float(m[0, 2]) == -0.5 and abs(float(c[0, 2, 0]) - 11.0) < 0.2 and abs(float(c[0, 2, 1]) - 7.0) < 0.2 and float(c[0, 2, 0]) != 0.0
    # -inf inside the window weighs nothing: the peak and 47 pixels of weight e round (10, 10), the 48th (x = 11) left out
    assert abs(float(c[0, 6, 0]) - (10 + 469 * e) / (1 + 47 * e)) < 1e-5 and abs(float(c[0, 6, 1]) - 10.0) < 1e-5
    # ... and is zeroed, like the arg-max's, in accuracy(decode="soft")
    tgt = torch.zeros(1, 8, H, W)
    tgt[0, :, 7, 11] = 1.0
    hm_ok = torch.nan_to_num(hm, nan=0.0, posinf=9.0, neginf=-9.0)
    acc, avg, cnt, pred = kd.accuracy(hm_ok.cuda(), tgt.cuda(), decode="soft")
    assert pred[0, 2].tolist() == [0.0, 0.0] and pred[0, 5].tolist() == [0.0, 0.0] and abs(float(pred[0, 7, 0])) < 0.5 and float(pred[0, 0, 0]) > 3.9
    assert acc[2] == 0.0 and cnt == 8
    for beta in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            kd.soft_argmax(hm.cuda(), beta, 3)
    # the entry points themselves return -1 (bad argument)
    from uda_poseestimation_amd import _hip
    x = hm.cuda()
    co, mv = torch.empty(8, 2, device="cuda"), torch.empty(8, device="cuda")
    ix, st = torch.empty(8, dtype=torch.int32, device="cuda"), torch.empty(32, device="cuda")
    for beta in (0.0, -2.0, float("inf"), float("nan")):
        assert _hip.lib().udapose_soft_argmax_fwd(_hip.stream(), x.data_ptr(), 8, H, W, beta, 3, co.data_ptr(), mv.data_ptr(), ix.data_ptr(), st.data_ptr()) == -1
        assert _hip.lib().udapose_coord_loss_fwd(_hip.stream(), x.data_ptr(), co.data_ptr(), None, None, 8, 8, H, W, beta, 3, 0, mv.data_ptr(),
                                                 ix.data_ptr(), st.data_ptr(), mv.data_ptr()) == -1
    assert _hip.lib().udapose_coord_loss_fwd(_hip.stream(), x.data_ptr(), co.data_ptr(), None, None, 8, 3, H, W, 10.0, 3, 0, mv.data_ptr(),
                                             ix.data_ptr(), st.data_ptr(), mv.data_ptr()) == -1      # 8 rows in groups of 3
    assert _hip.lib().udapose_coord_loss_fwd(_hip.stream(), x.data_ptr(), co.data_ptr(), None, None, 8, 8, H, W, 10.0, 3, 2, mv.data_ptr(),
                                             ix.data_ptr(), st.data_ptr(), mv.data_ptr()) == -1      # norm 2
    torch.cuda.synchronize()


@pytest.mark.parametrize("H,W", [(16, 16), (7, 9), (72, 72)])
def test_at_a_huge_beta_the_decode_is_get_max_preds_to_the_bit(H, W):
    """beta = 1e4 on maps whose maximum leads every other pixel by >= 0.05: every other term is exp(-500) = 0 in fp32."""
    kd = _kd()
    g = torch.Generator().manual_seed(H)
    hm = 0.9 * torch.rand(1, 33, H, W, generator=g)
    peaks = bump_centres(33, H, W, g).round().long()
    for r in range(33):
        hm[0, r, peaks[r, 1], peaks[r, 0]] = 1.0
    srt = hm.reshape(33, -1).sort(-1).values
    assert float((srt[:, -1] - srt[:, -2]).min()) >= 0.05
    want, wantm = kd.get_max_preds(hm.cuda())
    assert torch.equal(want.cpu().long().reshape(33, 2), peaks)
    for window in (None, 5):
        c, m = kd.soft_argmax(hm.cuda(), 1e4, window)
        assert torch.equal(_bits(c), _bits(want)) and torch.equal(_bits(m), _bits(wantm))


# ---------------------------------------------------------------------------------------------- the two losses
LOSS_SHAPES = [(2, 3, 16, 16), (2, 3, 7, 9), (1, 33, 64, 64), (2, 3, 72, 72)]


@functools.lru_cache(maxsize=None)
def loss_inputs(B, K, H, W, seed):
    """Student maps, target / teacher maps whose bumps sit within ~2 px of the student's, a 0 / 0.5 / 1 target_weight with zeros, a
    tea_mask with some false, and one all-zero target row."""
    g = torch.Generator().manual_seed(seed)
    stu, c = make_maps(B, K, H, W, seed)
    ct = (c.reshape(-1, 2) + 4 * torch.rand(B * K, 2, generator=g, dtype=torch.float64) - 2).clamp(min=0)
    ct = torch.minimum(ct, torch.tensor([W - 1.0, H - 1.0], dtype=torch.float64))
    tgt = bumps(ct, H, W, 1.5 if min(H, W) < 10 else 2.0).float().reshape(B, K, H, W)
    tgt[tgt < 0.01] = 0.0
    tgt[-1, -1] = 0.0                                           # carries no position
    tea = tgt + 0.02 * torch.randn(B, K, H, W, generator=g)
    weight = torch.tensor([1.0, 0.0, 0.5])[torch.randint(0, 3, (B, K, 1), generator=g)]
    weight[0, 0], weight[-1, -1], weight[0, 1] = 1.0, 1.0, 0.0
    tea_mask = torch.rand(B, K, generator=g) > 0.4
    tea_mask[0, 0], tea_mask[0, 1] = True, False
    return {"stu": stu, "tgt": tgt, "tea": tea, "weight": weight, "tea_mask": tea_mask}


def loss_kinds(beta, window):
    """name -> (device loss, restatement); both take the inputs dict on the student's device / in its dtype."""
    L = _losses()
    w = _win(window)
    J = lambda **kw: L.JointsSoftArgmaxLoss(beta, w, **kw)
    C = lambda **kw: L.ConsSoftArgmaxLoss(beta, w, **kw)
    return {
        "joints_l1_w": (lambda x, d: J()(x, d["tgt"], d["weight"]), lambda x, d: S64.joints_soft_argmax(x, d["tgt"], d["weight"], beta, w, "l1")),
        "joints_l1": (lambda x, d: J()(x, d["tgt"]), lambda x, d: S64.joints_soft_argmax(x, d["tgt"], None, beta, w, "l1")),
        "joints_l2_w": (lambda x, d: J(norm="l2")(x, d["tgt"], d["weight"][..., 0]), lambda x, d: S64.joints_soft_argmax(x, d["tgt"], d["weight"], beta, w, "l2")),
        "joints_l2": (lambda x, d: J(norm="l2")(x, d["tgt"]), lambda x, d: S64.joints_soft_argmax(x, d["tgt"], None, beta, w, "l2")),
        "cons_l1_mask": (lambda x, d: C()(x, d["tea"], tea_mask=d["tea_mask"]), lambda x, d: S64.cons_soft_argmax(x, d["tea"], d["tea_mask"], beta, w, "l1")),
        "cons_l2": (lambda x, d: C(norm="l2")(x, d["tea"]), lambda x, d: S64.cons_soft_argmax(x, d["tea"], None, beta, w, "l2")),
        "cons_l1_soft_mask": (lambda x, d: C(tea_decode="soft")(x, d["tea"], None, d["tea_mask"]),
                              lambda x, d: S64.cons_soft_argmax(x, d["tea"], d["tea_mask"], beta, w, "l1", "soft")),
    }


def _cast(d, dtype=None, device=None):
    out = {}
    for k, v in d.items():
        if v.dtype.is_floating_point and dtype is not None:
            v = v.to(dtype)
        out[k] = v.to(device) if device is not None else v
    return out


def _value_and_grad(fn, x, d):
    x = x.clone().requires_grad_(True)
    loss = fn(x, d)
    loss.backward()
    return loss.detach(), x.grad.detach()


@functools.lru_cache(maxsize=None)
def reference_losses(shape, beta, window, seed):
    d = loss_inputs(*shape, seed)
    d64 = _cast(d, torch.float64)
    out = {}
    for name, (_, ref_fn) in loss_kinds(beta, window).items():
        out[name] = (_value_and_grad(ref_fn, d64["stu"], d64), _value_and_grad(ref_fn, d["stu"], d))
    return out


@pytest.mark.parametrize("beta,window", [(10.0, 5), (30.0, 3)], ids=["beta10_win5", "beta30_win3"])
def test_losses_and_their_gradients_match_fp64(beta, window):
    res = {}
    for i, s in enumerate(LOSS_SHAPES):
        d = loss_inputs(*s, 50 + i)
        dd = _cast(d, None, "cuda")
        ref = reference_losses(s, beta, window, 50 + i)
        for name, (dev_fn, _) in loss_kinds(beta, window).items():
            (l64, g64), (l32, g32) = ref[name]
            ld, gd = (t.cpu() for t in _value_and_grad(dev_fn, dd["stu"], dd))
            assert ld.dtype == torch.float32 and ld.shape == () and gd.dtype == torch.float32 and gd.shape == d["stu"].shape
            assert torch.isfinite(g64).all() and torch.isfinite(gd).all() and float(l64) > 0, name
            gm = float(g64.abs().max())
            assert gm > 0, name
            res[(name, s)] = (abs(float(ld) - float(l64)) / float(l64), abs(float(l32) - float(l64)) / float(l64),
                              float((gd.double() - g64).abs().max()) / gm, float((g32.double() - g64).abs().max()) / gm)
            if name.startswith("joints"):
                # the all-zero target row and the rows of weight 0 get no gradient at all
                w = d["weight"] if name.endswith("_w") else torch.ones_like(d["weight"])
                dead = (w.reshape(s[0], s[1]) == 0) | (d["tgt"].reshape(s[0], s[1], -1).amax(-1) <= 0)
                assert dead.any() and not gd[dead].any() and gd[~dead].any(), name
            if "mask" in name:
                assert not gd[~d["tea_mask"]].any() and gd[d["tea_mask"]].any(), name
    bad = []
    print(f"\ncoordinate losses beta={beta:g} window={window}: error against fp64 autograd, device | fp32 torch on the CPU "
          "(value: relative; gradient: max abs / max|grad|), worst over the shapes")
    for name in loss_kinds(beta, window):
        rs = {s: r for (n, s), r in res.items() if n == name}
        v32, g32 = max(r[1] for r in rs.values()), max(r[3] for r in rs.values())
        print(f"  {name:18s} value {max(r[0] for r in rs.values()):.2e} | {v32:.2e}   gradient {max(r[2] for r in rs.values()):.2e} | {g32:.2e}")
        for s, r in rs.items():
            if r[0] > MARGIN * v32:
                bad.append((name, s, "value", r[0], v32))
            if r[2] > MARGIN * g32:
                bad.append((name, s, "gradient", r[2], g32))
    assert not bad, bad


def test_coordinate_targets_and_heatmap_targets_give_identical_bits_and_none_reduces_per_sample():
    kd, L = _kd(), _losses()
    none_err = []
    for i, s in enumerate(LOSS_SHAPES):
        d = _cast(loss_inputs(*s, 50 + i), None, "cuda")
        B, K = s[:2]
        xy, maxv = kd.get_max_preds(d["tgt"])
        present = (maxv > 0).float()
        assert float(present[-1, -1]) == 0.0 and present.sum() == B * K - 1
        for norm in ("l1", "l2"):
            crit = L.JointsSoftArgmaxLoss(10.0, 5, norm)
            a = _value_and_grad(lambda x, _: crit(x, d["tgt"], d["weight"]), d["stu"], d)
            b = _value_and_grad(lambda x, _: crit(x, xy, d["weight"] * present), d["stu"], d)
            assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
            # the all-zero target row contributes 0: the loss is that of the other rows, over all B*K
            w0 = d["weight"].clone()
            w0[-1, -1] = 0.0
            assert torch.equal(_bits(crit(d["stu"], d["tgt"], w0)), _bits(a[0]))
            # 'none': the per-sample means, [B]
            none = L.JointsSoftArgmaxLoss(10.0, 5, norm, reduction="none")
            x = d["stu"].clone().requires_grad_(True)
            got = none(x, d["tgt"], d["weight"])
            want = S64.joints_soft_argmax(d["stu"].double().cpu(), d["tgt"].double().cpu(), d["weight"].double().cpu(), 10.0, 5, norm, "none")
            want32 = S64.joints_soft_argmax(d["stu"].cpu(), d["tgt"].cpu(), d["weight"].cpu(), 10.0, 5, norm, "none")
            assert got.shape == (B,) and got.dtype == torch.float32
            e, y = float(((got.detach().cpu().double() - want) / want).abs().max()), float(((want32.double() - want) / want).abs().max())
            print(f"{s} {norm} 'none': relative error against fp64, device | fp32 torch on the CPU {e:.2e} | {y:.2e}")
            none_err.append((s, norm, e, y))
            assert abs(float(got.detach().double().mean()) - float(a[0])) <= 1e-6 * float(a[0])
            with pytest.raises(NotImplementedError):
                got.sum().backward()
        with pytest.raises(ValueError):
            L.ConsSoftArgmaxLoss()(d["stu"], d["tea"], valid_mask=torch.ones(B, s[2], s[3], dtype=torch.bool, device="cuda"))
        # masks in other storage select the same rows
        c = L.ConsSoftArgmaxLoss(10.0, 5)
        assert torch.equal(_bits(c(d["stu"], d["tea"], tea_mask=d["tea_mask"])), _bits(c(d["stu"], d["tea"], tea_mask=d["tea_mask"].float())))
    bar = MARGIN * max(y for _, _, _, y in none_err)          # the yardstick: the fp32 restatement's worst over the shapes of this test
    assert all(e <= bar for _, _, e, _ in none_err), (bar, none_err)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_16bit_inputs_return_gradients_in_the_input_dtype(dtype):
    kd = _kd()
    d = loss_inputs(2, 3, 16, 16, 50)
    d16 = _cast({k: (v.to(dtype) if k in ("stu", "tgt", "tea") else v) for k, v in d.items()}, None, "cuda")
    d32 = {k: (v.float() if v.dtype == dtype else v) for k, v in d16.items()}
    up = torch.randn(2, 3, 2, generator=torch.Generator().manual_seed(5)).cuda()
    kinds = dict(loss_kinds(10.0, 5))
    kinds["soft_argmax"] = (lambda x, _: (kd.soft_argmax(x, 10.0, 5)[0] * up).sum(), None)
    for name, (dev_fn, _) in kinds.items():
        l16, g16 = _value_and_grad(dev_fn, d16["stu"], d16)
        l32, g32 = _value_and_grad(dev_fn, d32["stu"], d32)
        assert g16.dtype == dtype and l16.dtype == torch.float32, name
        # the operands are taken as fp32 rows: the same numbers as the fp32 call on the widened inputs, the gradient rounded once
        assert torch.equal(g16, g32.to(dtype)) and torch.equal(l16, l32) and g32.any(), name
    c16, m16 = kd.soft_argmax(d16["stu"], 10.0, 5)
    assert c16.dtype == torch.float32 and torch.equal(c16, kd.soft_argmax(d32["stu"], 10.0, 5)[0])


def test_loss_forward_and_backward_replayed_from_a_graph_equal_eager_bit_for_bit():
    """Loss + backward alone, captured into a hipGraph and replayed on fresh inputs: the same kernels in the same order and no atomics, so
    the results are the eager run's bits.  Two eager runs of one backward are bit-identical for the same reason."""
    kd = _kd()
    B, K, H, W = 4, 16, 32, 32
    static = _cast(loss_inputs(B, K, H, W, 70), None, "cuda")
    static = {k: v.clone() for k, v in static.items()}
    ks = loss_kinds(10.0, 5)
    x = static["stu"].clone().requires_grad_(True)
    scale = torch.tensor(3.0, device="cuda")
    up = torch.randn(B, K, 2, generator=torch.Generator().manual_seed(6)).cuda()

    def run(xx, dd):
        outs = []
        for name in ("joints_l1_w", "joints_l2", "cons_l1_mask", "cons_l1_soft_mask"):
            loss = ks[name][0](xx, dd)
            (g,) = torch.autograd.grad(loss * scale, xx)
            outs += [loss, g]
        c, m = kd.soft_argmax(xx, 30.0, 3)
        (g,) = torch.autograd.grad(c, xx, up)
        return outs + [c.detach(), m, g]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(x, static)
        run(x, static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(x, static)
    for i in range(3):
        fresh = _cast(loss_inputs(B, K, H, W, 71 + i), None, "cuda")
        for k, v in fresh.items():
            static[k].copy_(v)
        with torch.no_grad():
            x.copy_(fresh["stu"])
        graph.replay()
        xe = fresh["stu"].clone().requires_grad_(True)
        eager = run(xe, fresh)
        again = run(xe, fresh)
        torch.cuda.synchronize()
        assert len(captured) == len(eager) == 11
        for j, (c, e, a) in enumerate(zip(captured, eager, again)):
            assert torch.equal(_bits(c), _bits(e)), (i, j)
            assert torch.equal(_bits(e), _bits(a)), (i, j)
        assert all(torch.isfinite(e).all() for e in eager) and all(e.any() for e in eager)


# ---------------------------------------------------------------------------------------------- PCK with the soft decode
class _Identity(torch.nn.Module):
    """A 'model' whose output is its input: validate() is fed heat-maps."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return x


def test_accuracy_with_the_soft_decode_is_the_oracles_pck_of_the_helpers_coordinates():
    """accuracy / accuracy_device / validate with decode="soft" (and a callable) against the PCK restatement (helpers.pck, checked against
    oracle.keypoints_ref.accuracy_ref on the CPU) fed with the fp64 helper's soft coordinates, zeroed where the maximum is <= 0; the target
    keeps the arg-max.  No normalised distance lies within 1e-4 of the threshold - asserted for every joint - so the fp32 kernel cannot
    fall on the other side."""
    from uda_poseestimation_amd.engine import validate
    kd = _kd()
    B, K, H, W, thr = 6, 7, 24, 40, 0.5
    g = torch.Generator().manual_seed(3)
    ct = torch.stack([torch.randint(2, W - 2, (B * K,), generator=g), torch.randint(2, H - 2, (B * K,), generator=g)], -1).double()
    off = (torch.rand(B * K, 2, generator=g, dtype=torch.double) - 0.5) * torch.tensor([3.5, 6.0], dtype=torch.double)
    cp = torch.minimum((ct + off).clamp(min=0), torch.tensor([W - 1.0, H - 1.0], dtype=torch.double))
    out = (bumps(cp, H, W, 2.0) + 0.02 * torch.randn(B * K, H, W, generator=g, dtype=torch.double)).float().reshape(B, K, H, W)
    tgt = bumps(ct, H, W, 2.0).float().reshape(B, K, H, W)
    tgt[:, 3] = 0.0                                  # a key point absent from the whole batch: -1
    tgt[0, 1] = 0.0
    out[1, 2] = -out[1, 2] - 0.5                     # a prediction without a positive maximum: decoded as (0, 0)
    c64, m64 = S64.decode(out.double(), 10.0, 5)
    c64 = c64 * (m64 > 0)
    assert c64[1, 2].tolist() == [0.0, 0.0]
    gt = S64.argmax_decode(tgt.double())[0]
    acc, avg, cnt, dist = S64.pck(c64.numpy(), gt.numpy(), H, W, thr)
    counted = ~np.isnan(dist)
    assert counted.sum() == B * (K - 1) - 1 and (np.abs(dist[counted] - thr) > 1e-4).all(), np.abs(dist[counted] - thr).min()
    assert acc[3] == -1 and cnt == K - 1 and 0.2 < avg < 0.9, (acc, avg)
    hard = S64.pck(S64.argmax_decode(out.double())[0].numpy(), gt.numpy(), H, W, thr)
    print(f"\nPCK@{thr / 10:g}: soft decode {avg:.4f}, arg-max decode {hard[1]:.4f}; nearest distance to the threshold {np.abs(dist[counted] - thr).min():.2e}")
    o, t = out.cuda(), tgt.cuda()
    for decode in ("soft", lambda h: kd.soft_argmax(h, 10.0, 5), lambda h: tuple(a.cpu().numpy() for a in kd.soft_argmax(h, 10.0, 5))):
        a1, avg1, cnt1, pred1 = kd.accuracy(o, t, thr=thr, decode=decode)
        assert np.array_equal(a1, acc.astype(np.float32).astype(np.float64)) and abs(avg1 - avg) < 1e-6 and cnt1 == cnt
        assert pred1.shape == (B, K, 2) and float((pred1.cpu().double() - c64).abs().max()) < 1e-4 and pred1[1, 2].tolist() == [0.0, 0.0]
        a2, ac2, pred2 = kd.accuracy_device(o, t, thr, decode=decode)
        assert a2.is_cuda and np.array_equal(a2.cpu().numpy().astype(np.float64), a1) and torch.equal(pred2, pred1) and int(ac2[1]) == cnt
    an, avgn, cntn, predn = kd.accuracy(out.numpy(), tgt.numpy(), thr=thr, decode="soft")
    assert isinstance(predn, np.ndarray) and np.array_equal(an, a1) and avgn == avg1 and cntn == cnt1
    # the default decode is the arg-max path, as before
    ah, avgh, cnth, predh = kd.accuracy(o, t, thr=thr)
    assert torch.equal(predh, kd.get_max_preds(o)[0]) and predh[1, 2].tolist() == [0.0, 0.0] and cnth == cnt
    with pytest.raises(ValueError):
        kd.accuracy(o, t, decode="hard")
    # validate(): two batches of three samples, batch-size weighted means of the per-batch PCK, -1 entries skipped
    model = _Identity().cuda()
    wt = torch.ones(3, K, 1, device="cuda")
    batches = [(o[:3], t[:3], wt), (o[3:], t[3:], wt)]
    for decode in ("soft", "argmax"):
        accs, loss = validate(batches, model, decode=decode)
        want, den = np.zeros(K), np.zeros(K)
        for (ob, tb, _) in batches:
            cb = S64.decode(ob.double().cpu(), 10.0, 5) if decode == "soft" else S64.argmax_decode(ob.double().cpu())
            cb = cb[0] * (cb[1] > 0)
            acc_b = S64.pck(cb.numpy(), S64.argmax_decode(tb.double().cpu())[0].numpy(), H, W, 0.5)[0]
            want += np.where(acc_b >= 0, acc_b, 0) * 3
            den += (acc_b >= 0) * 3
        assert den[3] == 0 and den[1] == 6
        np.testing.assert_allclose(accs, np.where(den > 0, want / np.maximum(den, 1), 0), atol=1e-6)
        assert np.isfinite(loss)
    assert validate(batches, model) == validate(batches, model, decode="argmax")


# ---------------------------------------------------------------------------------------------- the step with the coordinate criteria
N, K_, S = 4, 16, 128


def _coord_criteria():
    L = _losses()
    mse, sa = L.JointsMSELoss(), L.JointsSoftArgmaxLoss(window=5)
    return dict(criterion=lambda y, l, w: mse(y, l, w) + 0.1 * sa(y, l, w), con_criterion=L.ConsSoftArgmaxLoss(window=5))


def _batches(seeds):
    from uda_poseestimation_amd import synthetic
    out = []
    for s in seeds:
        b = synthetic.mean_teacher_batch(N, num_keypoints=K_, image_size=S, heatmap_size=S // 4, seed=s)
        g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
        out.append((g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"]))
    return out


def test_captured_steps_with_the_coordinate_criteria_equal_eager_steps():
    """test_captured_steps_with_the_new_criteria_equal_eager_steps (tests/test_gpu_softmax_losses.py) with
    JointsMSELoss + 0.1 * JointsSoftArgmaxLoss(window=5) and ConsSoftArgmaxLoss(window=5) as the step's criteria, precision 'bf16':
    its assertions and bars (there is no entropy term here), with the split and the unsplit capture."""
    from test_gpu_steps import _tiny
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    precision = "bf16"
    batches = _batches((31, 32, 33, 34))
    base = _tiny(K_, seed=8)
    for split in (False, True):
        nets = []
        for _ in range(2):
            s_, t_ = _tiny(K_, seed=8), _tiny(K_, seed=8)
            s_.load_state_dict(base.state_dict())
            nets.append((s_.cuda(), t_.cuda()))
        tr_g = MeanTeacherTrainer(*nets[0], lr=1e-4, image_size=S, heatmap_size=S // 4, precision=precision, **_coord_criteria())
        tr_e = MeanTeacherTrainer(*nets[1], lr=1e-4, image_size=S, heatmap_size=S // 4, precision=precision, **_coord_criteria())
        p0 = [p.detach().clone() for p in nets[0][0].parameters()]
        gs = GraphedTrainStep(tr_g, *batches[0], warmup=1, split=split)       # the warm-up step IS step 1 (on batch 0)
        tr_e.train_step(*batches[0])
        for bt in batches[1:]:
            og = gs.step(*bt)
            oe = tr_e.train_step(*bt)
            print(f"{precision} split={split}: loss_all {float(og['loss_all']):.6e} / {float(oe['loss_all']):.6e}  loss_s {float(og['loss_s']):.6e}  "
                  f"loss_c {float(og['loss_c']):.4e} / {float(oe['loss_c']):.4e}")
            assert abs(float(og["loss_all"]) - float(oe["loss_all"])) <= 2e-3 * abs(float(oe["loss_all"]))
            assert abs(float(og["loss_c"]) - float(oe["loss_c"])) <= 5e-3 * abs(float(oe["loss_c"])) + 1e-7
            want = float(oe["loss_s"]) + float(oe["loss_c"])
            assert abs(float(oe["loss_all"]) - want) <= 1e-5 * abs(want)
            assert "loss_ent" not in og and float(oe["loss_c"]) > 0
        sg, se, tg, te = nets[0][0], nets[1][0], nets[0][1], nets[1][1]
        num = den = 0.0
        for pg, pe, q0 in zip(sg.parameters(), se.parameters(), p0):
            num += float(((pg.detach() - pe.detach()) ** 2).sum())
            den += float(((pe.detach() - q0) ** 2).sum())
        rel = (num / max(den, 1e-30)) ** 0.5
        print(f"{precision} split={split}: ||student(graph) - student(eager)|| / ||student(eager) - start|| = {rel:.3e} after {len(batches)} steps")
        assert den > 0 and rel < 0.2
        tn = sum(float(((a.detach() - c.detach()) ** 2).sum()) for a, c in zip(tg.parameters(), te.parameters()))
        td = sum(float(((c.detach() - q0) ** 2).sum()) for c, q0 in zip(te.parameters(), p0))
        assert (tn / max(td, 1e-30)) ** 0.5 < 0.1
        gs.release()


def test_two_captured_steps_with_the_coordinate_criteria_agree_to_the_bit_after_three_steps():
    from test_gpu_steps import _tiny
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    batches = _batches(range(40, 44))
    base = _tiny(K_, seed=9)
    runs = []
    for _ in range(2):
        s_, t_ = _tiny(K_, seed=9), _tiny(K_, seed=9)
        s_.load_state_dict(base.state_dict())
        s_, t_ = s_.cuda(), t_.cuda()
        tr = MeanTeacherTrainer(s_, t_, lr=1e-4, image_size=S, heatmap_size=S // 4, precision="bf16", **_coord_criteria())
        gs = GraphedTrainStep(tr, *batches[0], warmup=1)
        losses = []
        for bt in batches[1:]:
            o = gs.step(*bt)
            losses.append(torch.stack([o[k].detach().float().reshape(()) for k in ("loss_all", "loss_s", "loss_c")]).clone())
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), [p.detach().cpu().clone() for p in s_.parameters()], [p.detach().cpu().clone() for p in t_.parameters()]))
        gs.release()
    (la, sa, ta), (lb, sb, tb) = runs
    print("losses of the third step [all, s, c]:", la[-1].tolist())
    assert torch.isfinite(la).all() and torch.equal(_bits(la), _bits(lb))
    assert all(torch.equal(a, b) for a, b in zip(sa, sb)) and all(torch.equal(a, b) for a, b in zip(ta, tb))
    assert any(not torch.equal(a, p.detach()) for a, p in zip(sa, base.parameters()))          # it trained
