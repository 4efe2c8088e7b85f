"""Histogram-matching and colour-statistics style nets on the MI355X (csrc/pixel_style.hip, lib.models.pixel_style): the integer summaries
bit for bit against numpy, every transferred element against float64 within the bar DERIVED in helpers/pixel_style_ref.py, the exact properties,
a captured launch, the refusals, and the trainer's style protocol, eager and captured.

MEASURED on an MI355X (printed by every run; DESIGN.md 4.21 keeps the table): see the docstring of test_transfers_against_fp64."""
import numpy as np
import pytest
import torch

from helpers import pixel_style_ref as R

pytestmark = pytest.mark.gpu

MEAN4, STD4 = (0.485, 0.456, 0.406, 0.45), (0.229, 0.224, 0.225, 0.226)
MEAN, STD = MEAN4[:3], STD4[:3]
LO, HI = (-2.1179, -2.0357, -1.8044), (2.2489, 2.4285, 2.64)
# ragged tails and unaligned planes; two pixels; four channels (no Cholesky); several samples; a plane of more than one work-group's share
SHAPES = [(2, 3, 17, 23), (1, 1, 1, 2), (1, 4, 8, 200), (3, 3, 64, 64), (2, 3, 96, 160)]
CASES = ("random", "constant content", "constant style", "two-level style", "content == style", "levels 0 and 255")
ALPHAS = (0.0, 0.3, 1.0)


@pytest.fixture(autouse=True)
def _bf16_unless_stated(monkeypatch):
    from uda_poseestimation_amd.lib.models.pose_resnet import PoseResNet
    monkeypatch.setattr(PoseResNet, "default_precision", "bf16")


@pytest.fixture(autouse=True)
def _device_still_sound():
    """Nothing is started on a device that an earlier test left in an error state."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reports an error before this test: {e}", returncode=3)
    yield


def _ps():
    from uda_poseestimation_amd.lib.models import pixel_style
    return pixel_style


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                     # (a copy: the shared inputs are read-only)


def _norm(C, normed):
    return (MEAN4[:C], STD4[:C]) if normed else (None, None)


def _clamp(C, normed):
    """bounds that bind: the trainer's `recover` for normalised images, an inner band for raw ones"""
    if normed:
        return (LO + (2.0,))[:C], (HI + (2.3,))[:C]
    return (0.2, 0.3, 0.1, 0.25)[:C], (0.7, 0.6, 0.8, 0.75)[:C]


def _bytes(case, shape, seed):
    """(content, style) uint8 images of one case"""
    rng = np.random.RandomState(seed)
    c = rng.randint(0, 256, shape).astype(np.uint8)
    s = np.clip(rng.normal(150, 30, shape), 0, 255).astype(np.uint8)       # another distribution, so that every mode moves the content
    if case == "constant content":
        c = np.broadcast_to(rng.randint(0, 256, shape[:2] + (1, 1)), shape).astype(np.uint8)
    elif case == "constant style":
        s = np.broadcast_to(rng.randint(0, 256, shape[:2] + (1, 1)), shape).astype(np.uint8)
    elif case == "two-level style":
        s = np.where(rng.rand(*shape) < 0.3, 10, 240).astype(np.uint8)
    elif case == "content == style":
        s = c.copy()
    elif case == "levels 0 and 255":
        c = np.where(rng.rand(*shape) < 0.6, 0, 255).astype(np.uint8)
        s = np.where(rng.rand(*shape) < 0.2, 0, 255).astype(np.uint8)
    return c, s


_INPUTS = {}


def _inputs(case, shape, normed):
    """(content, style) float32 through the normalisation, made once per case and left unchanged"""
    key = (case, shape, normed)
    if key not in _INPUTS:
        mean, std = _norm(shape[1], normed)
        bc, bs = _bytes(case, shape, 100 + CASES.index(case))
        xc, xs = R.from_bytes(bc, mean, std), R.from_bytes(bs, mean, std)
        R.assert_clear_of_ties(xc, mean, std)
        R.assert_clear_of_ties(xs, mean, std)
        assert np.array_equal(R.levels(xc, mean, std), bc) and np.array_equal(R.levels(xs, mean, std), bs)
        xc.setflags(write=False)
        xs.setflags(write=False)
        _INPUTS[key] = (xc, xs)
    return _INPUTS[key]


def _wild(shape, normed):
    """the random content with a third of its pixels far out of range, infinite or NaN"""
    mean, std = _norm(shape[1], normed)
    wild = np.array(_inputs("random", shape, normed)[0])
    flat = wild.reshape(-1)
    vals = np.array([np.inf, -np.inf, np.nan, 1e30, -1e30, 3.71, -2.23, 77.13], np.float32)
    pos = np.random.RandomState(9).permutation(flat.size)[:flat.size // 3]
    flat[pos] = vals[np.arange(pos.size) % vals.size]
    R.assert_clear_of_ties(wild, mean, std)
    return wild


def _modes(shape):
    return ("hist", "meanstd", "cholesky") if shape[1] == 3 else ("hist", "meanstd")


@pytest.mark.parametrize("normed", (True, False), ids=("normalised", "raw"))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_summaries_equal_the_integers(shape, normed):
    """Every word of the summary against numpy's integers; two runs agree; sample i of a batch equals the same sample alone; the functional
    histogram view; a tensor with values far out of range, infinities and NaN (the levels clamp)."""
    ps = _ps()
    mean, std = _norm(shape[1], normed)
    net = ps.PixelStyleNet("hist", mean, std)
    N, C = shape[:2]
    wild = _wild(shape, normed)
    for name, x in [(c, _inputs(c, shape, normed)[0]) for c in CASES] + [("constant style (style)", _inputs("constant style", shape, normed)[1]), ("wild", wild)]:
        want = torch.from_numpy(R.summary(x, mean, std))
        xd = _dev(x)
        got = net.summary(xd)
        assert got.dtype == torch.int32 and tuple(got.shape) == (N, ps.summary_words(C)) and got.is_contiguous()
        assert torch.equal(got.cpu(), want), name
        assert torch.equal(net.summary(xd), got) and net.spectrum(xd).equal(got), name
        buf = torch.full_like(got, -1)
        assert net.summary(xd, out=buf) is buf and torch.equal(buf, got), name
        for i in range(N):
            assert torch.equal(net.summary(xd[i:i + 1].contiguous()), got[i:i + 1]), (name, i)
        hist, cross = ps.split_summary(got, C)
        assert torch.equal(ps.level_histograms(xd, mean, std), hist) and int(hist.sum()) == int(np.prod(shape))
        assert (cross is None) == (C != 3)
        if C == 3:
            assert torch.equal(cross.cpu(), torch.from_numpy(R.cross_sums(R.levels(x, mean, std)))), name


@pytest.mark.parametrize("normed", (True, False), ids=("normalised", "raw"))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_transfers_against_fp64(shape, normed):
    """Every element of every case, mode, alpha in {0, 0.3, 1} (as a float and as a device tensor), with and without the clamp, against float64
    within the bar of helpers/pixel_style_ref.py: u = 2^-24 times the number of fp32 roundings of the stated formula (the once-rounded
    coefficient, its products, the final add), each weighted by the magnitude of the terms it rounds BEFORE they cancel:
        bar = u (k_d alpha inv_c Mag + 3 |alpha (T - l) inv_c| + |x|) (1 + 2^-20) + alpha inv_c (2^-32 Mag + 2^-40)
        k_d, Mag = 1, |T - l| (hist: the table entry is rounded once);  2, |A l| + |B| (meanstd: two rounded coefficients, one fmaf);
                   4, sum_b |K_ab l_b| + |K_a3| (cholesky: four rounded coefficients, three fmaf whose partial sums are at most Mag)
    The last term is the float64 side (the derivation is in the helper's docstring).  alpha == 0 must be exact.

    Measured on an MI355X, worst error / bar over all shapes, cases, alphas and clamps (normalised / raw inputs):
        hist 0.894 / 0.933;  meanstd 0.891 / 0.838;  cholesky 0.861 / 0.738   (the bar is tight by construction)."""
    ps = _ps()
    C = shape[1]
    mean, std = _norm(C, normed)
    clamp = _clamp(C, normed)
    clamp_dev = (torch.tensor(clamp[0]).cuda(), torch.tensor(clamp[1]).cuda())
    worst = {}
    for mode in _modes(shape):
        net = ps.PixelStyleNet(mode, mean, std)
        for case in CASES:
            xc, xs = _inputs(case, shape, normed)
            d, mag = R.shift(R.levels(xc, mean, std), R.levels(xs, mean, std), mode)
            dc, ds = _dev(xc), _dev(xs)
            sc, ss = net.summary(dc), net.summary(ds)
            moved = 0.0
            for alpha in ALPHAS:
                a_dev = torch.tensor([alpha], dtype=torch.float32).cuda()
                for cl, cl_dev in ((None, None), (clamp, clamp_dev)):
                    ref, bar = R.finish(xc, d, mag, mode, alpha, cl, std)
                    got = net.transfer(dc, sc, ss, alpha, cl_dev)
                    assert torch.equal(net.transfer(dc, sc, ss, a_dev, cl_dev), got), (mode, case, alpha)
                    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
                    assert np.all(np.isfinite(err))
                    ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bar, np.finfo(np.float64).tiny))))
                    worst[mode] = max(worst.get(mode, 0.0), ratio)
                    assert ratio <= 1.0, (mode, case, alpha, cl is not None, ratio, float(err.max()))
                    if alpha == 0.0:
                        assert float(err.max()) == 0.0 or cl is not None
                    if cl is None:
                        moved = max(moved, float(np.abs(ref - xc).max()))
            assert (moved > 0.01) == (case != "content == style"), (mode, case, moved)     # (the transfer does something)
    print(f"\n[pixel_style] {shape} {'normalised' if normed else 'raw'}: worst error / bar " + ", ".join(f"{m} {r:.3f}" for m, r in worst.items()))


def test_exact_properties():
    ps = _ps()
    shape = (3, 3, 64, 64)
    xc, xs = _inputs("random", shape, True)
    dc, ds = _dev(xc), _dev(xs)
    lo, hi = torch.tensor(LO).cuda(), torch.tensor(HI).cuda()
    tight_lo, tight_hi = torch.tensor([-0.5, -0.4, -0.3]).cuda(), torch.tensor([0.5, 0.6, 0.7]).cuda()
    for mode in ("hist", "meanstd", "cholesky"):
        net = ps.PixelStyleNet(mode, MEAN, STD)
        # alpha = 0 -> the content to the bit (compared as integers: the sign of a zero counts)
        for alpha in (0.0, torch.zeros(1, device="cuda")):
            assert torch.equal(net(dc, ds, alpha)[2].view(torch.int32), dc.view(torch.int32)), mode
        clamped = torch.maximum(torch.minimum(dc, tight_hi.view(1, 3, 1, 1)), tight_lo.view(1, 3, 1, 1))
        assert torch.equal(net(dc, ds, 0.0, clamp=(tight_lo, tight_hi))[2], clamped) and not torch.equal(clamped, dc)
        # the fused clamp holds everywhere and is the clamp of the plain result
        plain = net(dc, ds, 0.8)[2]
        got = net(dc, ds, 0.8, clamp=(tight_lo, tight_hi))[2]
        assert torch.equal(got, torch.maximum(torch.minimum(plain, tight_hi.view(1, 3, 1, 1)), tight_lo.view(1, 3, 1, 1)))
        assert bool((got >= tight_lo.view(1, 3, 1, 1)).all()) and bool((got <= tight_hi.view(1, 3, 1, 1)).all()) and not torch.equal(plain, dc)
        # forward == transfer(summary, summary); the three-tuple; out= is written in place; two runs give the same bits
        r = net(dc, ds, 0.8)
        assert r[0] is None and r[1] is None and torch.equal(r[2], plain)
        assert torch.equal(net.transfer(dc, net.summary(dc), net.spectrum(ds), 0.8), plain)
        out = torch.full_like(dc, float("nan"))
        assert net.transfer(dc, net.summary(dc), net.summary(ds), 0.8, out=out) is out and torch.equal(out, plain)
        assert torch.equal(ps.pixel_style_transfer(dc, ds, mode=mode, alpha=0.8, mean=MEAN, std=STD), plain)
        # sample i of a batch == the same sample alone
        for i in range(3):
            assert torch.equal(net(dc[i:i + 1].contiguous(), ds[i:i + 1].contiguous(), 0.8)[2], plain[i:i + 1])
    # content == style returns the content to the bit in "hist", for every alpha
    net = ps.PixelStyleNet("hist", MEAN, STD)
    for alpha in (1.0, 0.3):
        assert torch.equal(net(dc, dc.clone(), alpha)[2].view(torch.int32), dc.view(torch.int32))
    assert not torch.equal(net(dc, ds, 1.0)[2], dc)


@pytest.mark.parametrize("case", ("random", "two-level style", "constant content", "levels 0 and 255"))
def test_matched_histogram_follows_the_styles(case):
    """alpha = 1, "hist": the levels of the OUTPUT have a cumulative histogram within one occupied style level of the style's
    (helpers/pixel_style_ref.py: cdf_step_violations states the two inequalities), per plane."""
    ps = _ps()
    shape = (2, 3, 96, 160)
    for normed in (True, False):
        mean, std = _norm(3, normed)
        xc, xs = _inputs(case, shape, normed)
        out = ps.pixel_style_transfer(_dev(xc), _dev(xs), mode="hist", alpha=1.0, mean=mean, std=std).cpu().numpy()
        lo_, lc, ls = R.levels(out, mean, std), R.levels(xc, mean, std), R.levels(xs, mean, std)
        hc, hs = R.histograms(lc), R.histograms(ls)
        for n in range(2):
            for c in range(3):
                # (the property allows either neighbour for a target at a half level, so a tie in `out` cannot break it)
                assert R.cdf_step_violations(lo_[n, c], hc[n, c], hs[n, c]) == 0, (case, normed, n, c)
                assert lo_[n, c].min() >= np.flatnonzero(hs[n, c])[0] and lo_[n, c].max() <= np.flatnonzero(hs[n, c])[-1]


def test_captured_launch_follows_alpha_and_the_static_images():
    ps = _ps()
    shape = (2, 3, 96, 160)
    lo, hi = torch.tensor(LO).cuda(), torch.tensor(HI).cuda()
    first = _inputs("random", shape, True)
    for mode in ("hist", "meanstd", "cholesky"):
        net = ps.PixelStyleNet(mode, MEAN, STD)
        xc, xs = _dev(first[0]), _dev(first[1])
        alpha = torch.tensor([0.3], dtype=torch.float32).cuda()
        sc, ss, out = net.summary(xc).clone(), net.summary(xs).clone(), torch.empty_like(xc)

        def run():
            net.summary(xc, out=sc)
            net.summary(xs, out=ss)
            return net.transfer(xc, sc, ss, alpha, (lo, hi), out=out)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run()
        seen = []
        for a, case in ((0.3, "random"), (0.9, "random"), (0.9, "two-level style"), (0.0, "levels 0 and 255"), (1.0, "constant content")):
            nc, ns = _inputs(case, shape, True)
            xc.copy_(_dev(nc))
            xs.copy_(_dev(ns))
            alpha.fill_(a)
            out.fill_(float("nan"))
            graph.replay()
            want = net(xc.clone(), xs.clone(), a, clamp=(lo, hi))[2]
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (mode, a, case)
            assert torch.equal(sc, net.summary(xc)) and torch.equal(ss, net.summary(xs))
            seen.append(out.clone())
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_refusals_write_nothing():
    from uda_poseestimation_amd import _hip
    ps = _ps()
    lib = _hip.lib()
    st = _hip.stream()
    x = torch.rand(1, 3, 16, 16, device="cuda")
    x4 = torch.rand(1, 4, 16, 16, device="cuda")

    def sentinel(nbytes):
        return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")

    def untouched(t):
        return bool((t.view(torch.uint8) == 0xFF).all())

    summ, out = sentinel(4 * 1024 * 4), sentinel(4 * 16 * 16 * 4)
    good = ps.PixelStyleNet("hist").summary(x)
    p = lambda t: t.data_ptr()
    codes = [
        lib.udapose_pixel_summary(st, p(x), 0, 3, 16, 16, None, None, p(summ)),                # no planes
        lib.udapose_pixel_summary(st, p(x), 1, 3, 4096, 4097, None, None, p(summ)),            # H W > 2^24
        lib.udapose_pixel_summary(st, None, 1, 3, 16, 16, None, None, p(summ)),
        lib.udapose_pixel_summary(st, p(x), 1, 3, 16, 16, p(x), None, p(summ)),                # mean without std
        lib.udapose_pixel_transfer(st, p(x4), p(good), p(good), p(out), 1, 4, 16, 16, 2, 1e-5, 1.0, None, None, None, None, None),   # cholesky, C = 4
        lib.udapose_pixel_transfer(st, p(x), p(good), p(good), p(out), 1, 3, 16, 16, 5, 1e-5, 1.0, None, None, None, None, None),    # unknown mode
        lib.udapose_pixel_transfer(st, p(x), p(good), p(good), p(out), 1, 3, 1, 1, 1, 1e-5, 1.0, None, None, None, None, None),      # H W < 2
        lib.udapose_pixel_transfer(st, p(x), p(good), p(good), p(out), 1, 3, 1, 1, 2, 1e-5, 1.0, None, None, None, None, None),
        lib.udapose_pixel_transfer(st, p(x), p(good), p(good), p(out), 1, 3, 4096, 4097, 0, 1e-5, 1.0, None, None, None, None, None),
        lib.udapose_pixel_transfer(st, p(x), None, p(good), p(out), 1, 3, 16, 16, 0, 1e-5, 1.0, None, None, None, None, None),
        lib.udapose_pixel_transfer(st, p(x), p(good), p(good), p(out), 0, 3, 16, 16, 0, 1e-5, 1.0, None, None, None, None, None),
        lib.udapose_pixel_transfer(st, p(x), p(good), p(good), p(out), 1, 3, 16, 16, 1, 0.0, 1.0, None, None, None, None, None),     # eps = 0
        lib.udapose_pixel_transfer(st, p(x), p(good), p(good), p(out), 1, 3, 16, 16, 0, 1e-5, 1.0, None, p(x), None, None, None),    # lo without hi
    ]
    torch.cuda.synchronize()
    assert all(c in (-1, -3) for c in codes), codes
    assert codes[1] == -3 and codes[8] == -3 and untouched(summ) and untouched(out)
    # the module's refusals: nothing is launched, `out` stays as it was
    o32 = out[:3 * 16 * 16 * 4].view(torch.float32).view(1, 3, 16, 16)
    o4 = out.view(torch.float32).view(1, 4, 16, 16)
    net = ps.PixelStyleNet("hist")
    with pytest.raises(ValueError, match="same shape"):
        net(x, torch.rand(1, 3, 16, 32, device="cuda"))
    with pytest.raises(ValueError, match="same shape"):
        net(x, torch.rand(2, 3, 16, 16, device="cuda"))
    with pytest.raises(TypeError, match="float32"):
        net(x.half(), x.half())
    with pytest.raises(TypeError, match="float32"):
        net.transfer(x.half(), good, good, 1.0, out=o32)
    nc = torch.rand(1, 3, 16, 32, device="cuda")[:, :, :, ::2]
    with pytest.raises(ValueError, match="contiguous"):
        net.transfer(nc, good, good, 1.0, out=o32)
    with pytest.raises(ValueError, match="summary"):
        net.transfer(x, good[:, :768], good, 1.0, out=o32)
    with pytest.raises(ValueError, match="summary"):
        net.transfer(x, good, good.float(), 1.0, out=o32)
    with pytest.raises(ValueError, match="alpha"):
        net.transfer(x, good, good, 1.5, out=o32)
    with pytest.raises(ValueError, match="alpha"):
        net.transfer(x, good, good, torch.ones(2, device="cuda"), out=o32)
    with pytest.raises(ValueError, match="out must be"):
        net.transfer(x, good, good, 1.0, out=o4)
    with pytest.raises(ValueError, match="3 channels"):
        ps.PixelStyleNet("cholesky").transfer(x4, ps.PixelStyleNet("hist").summary(x4), ps.PixelStyleNet("hist").summary(x4), 1.0, out=o4)
    one = torch.rand(1, 3, 1, 1, device="cuda")
    s1 = net.summary(one)
    with pytest.raises(ValueError, match=">= 2"):
        ps.PixelStyleNet("meanstd").transfer(one, s1, s1, 1.0, out=out[:12].view(torch.float32).view(1, 3, 1, 1))
    with pytest.raises(ValueError, match="channels"):
        ps.PixelStyleNet("hist", MEAN, STD).summary(x4)
    torch.cuda.synchronize()
    assert untouched(out)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------

def _tiny(K=16, seed=0):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(seed)
    return pr._pose_resnet("t", K, pr.Bottleneck_default, [1, 1, 1, 1], False, False)


def _batch(seed, N=4, K=16, S=64):
    from uda_poseestimation_amd import synthetic
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=seed)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    return (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])


def _trainer(base, style_net, rng_seed, **kw):
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    s_, t_ = _tiny(seed=8), _tiny(seed=8)
    s_.load_state_dict(base.state_dict())
    s_, t_ = s_.cuda(), t_.cuda()
    lo, hi = torch.tensor(LO).cuda(), torch.tensor(HI).cuda()
    tr = MeanTeacherTrainer(s_, t_, lr=1e-4, image_size=64, heatmap_size=16, style_net=style_net, recover=(lo, hi),
                            rng=np.random.RandomState(rng_seed), **kw)
    return s_, t_, tr


@pytest.mark.parametrize("mode", ("hist", "cholesky"))
def test_trainer_eager_step_feeds_the_transferred_images(mode):
    ps = _ps()
    base = _tiny(seed=8)
    args = _batch(41)
    net = ps.PixelStyleNet(mode, MEAN, STD)
    stu, tea, tr = _trainer(base, net, 7, s2t_freq=1.0, t2s_freq=1.0)
    seen = []
    inner = tr._forward_backward
    tr._forward_backward = lambda *a, **k: (seen.append((a[0], a[4])), inner(*a, **k))[1]
    out = tr.train_step(*args)
    probe = np.random.RandomState(7)
    probe.rand(); a_s2t = probe.uniform(0.0, 1.0)
    probe.rand(); a_t2s = probe.uniform(0.0, 1.0)
    lo, hi = tr.recover
    x_s, x_t = args[0], args[4]
    want_s = ps.pixel_style_transfer(x_s, x_t, mode, a_s2t, clamp=(lo, hi), mean=MEAN, std=STD)
    want_t = ps.pixel_style_transfer(x_t, x_s, mode, a_t2s, clamp=(lo, hi), mean=MEAN, std=STD)
    assert len(seen) == 1 and torch.equal(seen[0][0], want_s) and len(seen[0][1]) == 1 and torch.equal(seen[0][1][0], want_t)
    assert not torch.equal(want_s, x_s) and not torch.equal(want_t, x_t)
    assert all(bool(torch.isfinite(out[k])) for k in ("loss_all", "loss_s", "loss_c"))


def test_trainer_captured_step_equals_its_eager_twin():
    """GraphedTrainStep with a PixelStyleNet against an eager twin with the same host draws from identical state, over steps whose drawn
    directions and alphas differ: losses and student weights bit for bit; then a replay of the t2s graph against the eager call."""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    ps = _ps()
    base = _tiny(seed=8)
    batches = [_batch(s) for s in (41, 42, 43, 44, 45)]
    nets, trs = [], []
    for _ in range(2):
        s_, t_, tr = _trainer(base, ps.PixelStyleNet("hist", MEAN, STD), 123, s2t_freq=0.5, t2s_freq=0.5, s2t_alpha=(0.0, 1.0), t2s_alpha=(0.0, 1.0))
        nets.append((s_, t_))
        trs.append(tr)
    tr_g, tr_e = trs
    probe, seen = np.random.RandomState(123), []
    for _ in batches:
        a = probe.rand() < 0.5
        if a:
            probe.uniform(0, 1)
        b_ = probe.rand() < 0.5
        if b_:
            probe.uniform(0, 1)
        seen.append((a, b_))
    assert len(set(seen)) >= 3, seen                                # (the steps draw different directions)
    gs = GraphedTrainStep(tr_g, *batches[0], warmup=1)             # the warm-up step IS step 1 (on batch 0, with step 1's draws)
    assert set(gs.g_style) == {"enc", "s2t", "t2s"} and gs.static["sp_s"].dtype == torch.int32
    assert tuple(gs.static["sp_s"].shape) == (4, ps.summary_words(3))
    tr_e.train_step(*batches[0])
    for i, bt in enumerate(batches[1:]):
        og = gs.step(*bt)
        oe = tr_e.train_step(*bt)
        for k in ("loss_all", "loss_s", "loss_c"):
            assert torch.isfinite(og[k]) and float(og[k]) == float(oe[k]), (i, k, float(og[k]), float(oe[k]))
    for (n, pg), (_, pe), q0 in zip(nets[0][0].named_parameters(), nets[1][0].named_parameters(), base.parameters()):
        assert torch.equal(pg.detach(), pe.detach()), n
    assert any(not torch.equal(p.detach().cpu(), q0.detach()) for p, q0 in zip(nets[0][0].parameters(), base.parameters()))
    sa, sb = tr_g.rng.get_state(), tr_e.rng.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]           # both consumed exactly the same host draws
    st = gs.static
    st["alpha_t2s"].fill_(0.625)
    gs.g_style["enc"].replay()
    gs.g_style["t2s"].replay()
    want = ps.pixel_style_transfer(st["x_t_tea"], st["x_s"], "hist", 0.625, clamp=tr_g.recover, mean=MEAN, std=STD)
    assert torch.equal(st["x_t_tea_in"], want) and not torch.equal(want, st["x_t_tea"])
