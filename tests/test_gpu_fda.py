"""Fourier-domain style transfer on the MI355X (csrc/fda.hip, lib.models.fda): spectrum and transferred image per element against float64
within the derived bars of helpers/fda_fp64.py, the exactness properties bit for bit, the raw-space DC variant, the refusals, and the trainer's
third style protocol, eager and captured.

MEASURED on an MI355X (printed by every run; DESIGN.md 4.13 keeps the table): see the docstring of test_spectrum_and_transfer_against_fp64."""
import numpy as np
import pytest
import torch

from helpers import fda_fp64 as ff

pytestmark = pytest.mark.gpu

# (shape, b)
CASES = [((2, 3, 16, 16), 1), ((1, 3, 16, 16), 0), ((1, 3, 16, 16), 7), ((1, 3, 12, 20), 1), ((1, 1, 15, 17), 2), ((1, 3, 64, 64), 5),
         ((1, 3, 256, 256), 23), ((1, 3, 384, 384), 34)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
LO, HI = (-2.1179, -2.0357, -1.8044), (2.2489, 2.4285, 2.64)


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


def _fda():
    from uda_poseestimation_amd.lib.models import fda
    return fda


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ratio(got, ref, bar):
    """worst |got - ref| / bar over the elements (0 / 0 counts as 0)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert np.all(np.isfinite(err))
    return float(np.max(np.where(err == 0, 0.0, err / np.where(bar == 0, np.finfo(np.float64).tiny, bar)))), float(err.max())


@pytest.mark.parametrize("shape,b", CASES)
def test_spectrum_and_transfer_against_fp64(shape, b):
    """Every coefficient (real and imaginary part) and every output element within the helper's bar, alpha 1.0 and 0.37.

    Measured (worst error / bar; worst absolute error of the output, the numpy complex64 emulation's beside it): DESIGN.md 4.13."""
    fda = _fda()
    seed = ff.pick_seed(shape, b)
    c, s = ff.inputs(shape, seed)
    cond = min(ff.condition(c, b), ff.condition(s, b))
    assert cond >= ff.MIN_CONDITION, cond                          # (otherwise the phase term makes the bar meaningless)
    xc, xs = _dev(c), _dev(s)
    g = fda.low_freq_spectrum(xc, b)
    assert g.dtype == torch.complex64 and tuple(g.shape) == (shape[0], shape[1], 2 * b + 1, b + 1)
    gref, gbar = ff.spectrum(c, b), np.broadcast_to(ff.spectrum_bar(c, b), (shape[0], shape[1], 2 * b + 1, b + 1))
    gh = g.cpu().numpy()
    r_re, _ = _ratio(gh.real, gref.real, gbar)
    r_im, _ = _ratio(gh.imag, gref.imag, gbar)
    emu_g, _ = ff.emulate_c64(c, s, b, 1.0)
    print(f"\n[fda] {shape} b={b} seed={seed} condition {cond:.1e}: spectrum error / bar {max(r_re, r_im):.3e}; "
          f"max |dG| / sum|x| device {np.abs(gh - gref).max() / np.abs(c).sum(axis=(2, 3)).min():.2e} "
          f"complex64 emulation {np.abs(emu_g - gref).max() / np.abs(c).sum(axis=(2, 3)).min():.2e}")
    assert max(r_re, r_im) <= 1.0
    H, W = shape[-2:]
    for alpha in (1.0, 0.37):
        out = fda.fda_transfer(xc, xs, beta=(b + 0.5) / min(H, W), alpha=alpha)
        assert fda.window(H, W, (b + 0.5) / min(H, W)) == b
        ref, bar = ff.low_rank(c, s, b, alpha), ff.transfer_bar(c, s, b, alpha)
        r, e = _ratio(out.cpu().numpy(), ref, bar)
        e_emu = float(np.abs(ff.emulate_c64(c, s, b, alpha)[1].astype(np.float64) - ref).max())
        print(f"[fda] {shape} b={b} alpha={alpha}: output error / bar {r:.3e}; max error device {e:.2e}, complex64 emulation {e_emu:.2e}; "
              f"moved by {np.abs(ref - c).max():.2f}")
        assert r <= 1.0
        assert np.abs(ref - c).max() > 0.01                       # (the transfer does something at this shape)


def test_exact_properties():
    fda = _fda()
    shape, b = (4, 3, 16, 16), 2
    c, s = ff.inputs(shape, 1)
    xc, xs = _dev(c), _dev(s)
    lo, hi = torch.tensor([0.2, 0.3, 0.1]).cuda(), torch.tensor([0.7, 0.6, 0.8]).cuda()
    net = fda.FDANet(2.5 / 16)
    assert net.window_of(xc) == b
    # alpha = 0 -> the (clamped) content
    assert torch.equal(net(xc, xs, 0.0)[2], xc)
    clamped = torch.maximum(torch.minimum(xc, hi.view(1, 3, 1, 1)), lo.view(1, 3, 1, 1))
    assert torch.equal(net(xc, xs, 0.0, clamp=(lo, hi))[2], clamped) and not torch.equal(clamped, xc)
    # style is content -> the content
    assert torch.equal(net(xc, xc, 1.0)[2], xc)
    # the fused clamp
    plain = net(xc, xs, 0.8)[2]
    assert torch.equal(net(xc, xs, 0.8, clamp=(lo, hi))[2], torch.maximum(torch.minimum(plain, hi.view(1, 3, 1, 1)), lo.view(1, 3, 1, 1)))
    assert not torch.equal(plain, xc)
    # alpha as a device scalar == the same float; the forward's three-tuple
    a = torch.tensor([0.8], dtype=torch.float32).cuda()
    r = net(xc, xs, a)
    assert r[0] is None and r[1] is None and torch.equal(r[2], plain)
    assert torch.equal(net(xc, xs, a.reshape(()))[2], plain)
    # two runs give the same bits, spectrum and image
    assert torch.equal(torch.view_as_real(net.spectrum(xc)), torch.view_as_real(net.spectrum(xc)))
    assert torch.equal(net(xc, xs, 0.8)[2], plain)
    # plane i in a batch of 4 == plane i alone
    for i in range(4):
        assert torch.equal(torch.view_as_real(net.spectrum(xc[i:i + 1].contiguous())), torch.view_as_real(net.spectrum(xc))[i:i + 1])
        assert torch.equal(net(xc[i:i + 1].contiguous(), xs[i:i + 1].contiguous(), 0.8)[2], plain[i:i + 1])
    # spectrum() / transfer() are forward()'s two halves
    assert torch.equal(net.transfer(xc, net.spectrum(xc), net.spectrum(xs), 0.8), plain)


def test_all_zero_content_takes_the_unit_phase():
    fda = _fda()
    shape, b = (1, 3, 16, 16), 2
    _, s = ff.inputs(shape, 2)
    z = np.zeros(shape, dtype=np.float32)
    out = fda.fda_transfer(_dev(z), _dev(s), beta=2.5 / 16, alpha=1.0)
    ref, bar = ff.low_rank(z, s, b, 1.0), ff.transfer_bar(z, s, b, 1.0)
    r, e = _ratio(out.cpu().numpy(), ref, bar)
    print(f"\n[fda] all-zero content: error / bar {r:.3e}, max error {e:.2e}, output up to {np.abs(ref).max():.2f}")
    assert r <= 1.0 and np.abs(ref).max() > 0.5


def test_raw_space_dc_variant():
    fda = _fda()
    shape, b = (2, 3, 16, 16), 1
    rng = np.random.RandomState(5)
    m, sd = np.reshape(MEAN, (1, 3, 1, 1)), np.reshape(STD, (1, 3, 1, 1))
    c = (((0.30 + 0.1 * rng.standard_normal(shape)) - m) / sd).astype(np.float32)     # raw means on either side of the dataset mean
    s = (((0.65 + 0.1 * rng.standard_normal(shape)) - m) / sd).astype(np.float32)
    assert min(ff.condition(c, b), ff.condition(s, b)) >= ff.MIN_CONDITION
    xc, xs = _dev(c), _dev(s)
    for alpha in (1.0, 0.37):
        out = fda.fda_transfer(xc, xs, beta=0.1, alpha=alpha, mean=MEAN, std=STD)
        ref, bar = ff.low_rank(c, s, b, alpha, MEAN, STD), ff.transfer_bar(c, s, b, alpha, MEAN, STD)
        r, e = _ratio(out.cpu().numpy(), ref, bar)
        print(f"\n[fda] raw-space DC alpha={alpha}: error / bar {r:.3e}, max error {e:.2e}")
        assert r <= 1.0
        assert np.abs(ref - ff.raw_reference(c, s, b, alpha, MEAN, STD)).max() <= 1e-12
        plain = fda.fda_transfer(xc, xs, beta=0.1, alpha=alpha)
        assert float((out - plain).abs().max()) > 0.1
    net = fda.FDANet(0.1, torch.tensor(MEAN), torch.tensor(STD))
    assert torch.equal(net(xc, xs, 0.37)[2], out)


def test_refusals_write_nothing():
    from uda_poseestimation_amd import _hip
    fda = _fda()
    lib = _hip.lib()
    x = torch.rand(1, 3, 16, 16, device="cuda")
    st = _hip.stream()

    def untouched(t):
        return bool((t.view(torch.uint8) == 0xFF).all())

    for b in (8, fda.MAX_B + 1, -1):                                # 2b + 1 > min(H, W); b > UDAPOSE_FDA_MAX_B; b < 0
        nb = max(b, 0)
        spec = torch.full((1, 3, 2 * nb + 1, nb + 1, 2), float("nan"), device="cuda").view(torch.uint8).fill_(0xFF).view(torch.float32)
        ws = torch.full((4096,), 0xFF, dtype=torch.uint8, device="cuda")
        out = torch.full((1 * 3 * 16 * 16 * 4,), 0xFF, dtype=torch.uint8, device="cuda")
        assert lib.udapose_fda_ws_bytes(3, 16, 16, b) in (-1, -3)
        assert lib.udapose_fda_spectrum(st, x.data_ptr(), 3, 16, 16, b, ws.data_ptr(), spec.data_ptr()) in (-1, -3)
        assert lib.udapose_fda_apply(st, x.data_ptr(), spec.data_ptr(), spec.data_ptr(), out.data_ptr(), 3, 3, 16, 16, b, 1.0, None, None, None,
                                     None, None) in (-1, -3)
        torch.cuda.synchronize()
        assert untouched(spec) and untouched(ws) and untouched(out), b
    big = torch.rand(1, 1, 256, 256, device="cuda")
    with pytest.raises(NotImplementedError, match="b <= "):
        fda.low_freq_spectrum(big, fda.MAX_B + 1)
    with pytest.raises(ValueError, match="Nyquist"):
        fda.low_freq_spectrum(x, 8)
    with pytest.raises(ValueError, match="Nyquist"):
        fda.fda_transfer(x, x, beta=0.6)
    # the module's refusals: shape mismatch, fp16 input, non-contiguous input - nothing is launched, `out` stays as it was
    net = fda.FDANet(0.1)
    sp = net.spectrum(x)
    out = torch.full((1 * 3 * 16 * 16 * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    o32 = out.view(torch.float32).view(1, 3, 16, 16)
    with pytest.raises(ValueError, match="same shape"):
        net(x, torch.rand(1, 3, 16, 32, device="cuda"))
    with pytest.raises(ValueError, match="same shape"):
        net(x, torch.rand(2, 3, 16, 16, device="cuda"))
    with pytest.raises(TypeError, match="float32"):
        net(x.half(), x.half())
    with pytest.raises(TypeError, match="float32"):
        net.transfer(x.half(), sp, sp, 1.0, out=o32)
    nc = torch.rand(1, 3, 16, 32, device="cuda")[:, :, :, ::2]
    assert not nc.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        net.transfer(nc, sp, sp, 1.0, out=o32)
    with pytest.raises(ValueError, match="contiguous"):
        net(x, nc)
    with pytest.raises(ValueError, match="spectrum"):
        net.transfer(x, sp[:, :, :, :1], sp, 1.0, out=o32)
    with pytest.raises(ValueError, match="alpha"):
        net.transfer(x, sp, sp, 1.5, out=o32)
    torch.cuda.synchronize()
    assert untouched(out)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------

def _tiny(K=16, seed=0):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(seed)
    return pr._pose_resnet("t", K, pr.Bottleneck_default, [1, 1, 1, 1], False, False)


def _batch(seed, N=4, K=16, S=128):
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
    tr = MeanTeacherTrainer(s_, t_, lr=1e-4, image_size=128, heatmap_size=32, style_net=style_net, recover=(lo, hi),
                            rng=np.random.RandomState(rng_seed), **kw)
    return s_, t_, tr


def test_trainer_eager_step_feeds_the_transferred_images():
    fda = _fda()
    base = _tiny(seed=8)
    args = _batch(41)
    net = fda.FDANet(0.05, MEAN, STD)
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
    want_s = fda.fda_transfer(x_s, x_t, 0.05, a_s2t, clamp=(lo, hi), mean=MEAN, std=STD)
    want_t = fda.fda_transfer(x_t, x_s, 0.05, a_t2s, clamp=(lo, hi), mean=MEAN, std=STD)
    assert len(seen) == 1 and torch.equal(seen[0][0], want_s) and len(seen[0][1]) == 1 and torch.equal(seen[0][1][0], want_t)
    assert not torch.equal(want_s, x_s) and not torch.equal(want_t, x_t)
    assert all(bool(torch.isfinite(out[k])) for k in ("loss_all", "loss_s", "loss_c"))
    # the draws forced off: the step of style_net=None, bit for bit
    stu_a, tea_a, tr_a = _trainer(base, net, 7, s2t_freq=0.0, t2s_freq=0.0)
    stu_b, tea_b, tr_b = _trainer(base, None, 7)
    oa, ob = tr_a.train_step(*args), tr_b.train_step(*args)
    assert torch.equal(oa["loss_all"], ob["loss_all"])
    for pa, pb in zip(list(stu_a.parameters()) + list(tea_a.parameters()), list(stu_b.parameters()) + list(tea_b.parameters())):
        assert torch.equal(pa.detach(), pb.detach())
    assert not all(torch.equal(pa.detach(), pb.detach()) for pa, pb in zip(stu_a.parameters(), stu.parameters()))      # (the styled step went elsewhere)


def test_trainer_captured_step_equals_its_eager_twin():
    """GraphedTrainStep with an FDANet against an eager twin with the same host draws from identical state, over steps whose style decisions
    differ (the seeded mix of test_config2_step_with_style_and_occlusion_captured_equals_eager_twin), occlusion decided on the device: losses
    and student weights bit for bit."""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    fda = _fda()
    base = _tiny(seed=8)
    batches = [_batch(s) for s in (41, 42, 43, 44, 45)]
    nets, trs = [], []
    for _ in range(2):
        s_, t_, tr = _trainer(base, fda.FDANet(0.05, MEAN, STD), 123, s2t_freq=0.5, t2s_freq=0.5, s2t_alpha=(0.0, 1.0), t2s_alpha=(0.0, 1.0),
                              occlude_rate=0.5, occlude_thresh=-1e9, occlude_size=10)
        tr.device_occlusion = True
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
        probe.rand(4, 4)
        seen.append((a, b_))
    assert seen[0] == (False, True) and (False, False) in seen[1:] and (True, False) in seen[1:], seen
    gs = GraphedTrainStep(tr_g, *batches[0], warmup=1)             # the warm-up step IS step 1 (on batch 0, with step 1's draws)
    assert set(gs.g_style) == {"enc", "s2t", "t2s"} and gs.static["sp_s"].dtype == torch.complex64
    tr_e.train_step(*batches[0])
    for i, bt in enumerate(batches[1:]):
        og = gs.step(*bt)
        oe = tr_e.train_step(*bt)
        for k in ("loss_all", "loss_s", "loss_c"):
            assert torch.isfinite(og[k]) and float(og[k]) == float(oe[k]), (i, k, float(og[k]), float(oe[k]))
        assert int(tr_e.occluded.sum()) == int(tr_g.occluded.sum())
    for (n, pg), (_, pe), q0 in zip(nets[0][0].named_parameters(), nets[1][0].named_parameters(), base.parameters()):
        assert torch.equal(pg.detach(), pe.detach()), n
    assert any(not torch.equal(p.detach().cpu(), q0.detach()) for p, q0 in zip(nets[0][0].parameters(), base.parameters()))
    sa, sb = tr_g.rng.get_state(), tr_e.rng.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]           # both consumed exactly the same host draws
    # the t2s graph follows the device alpha: a replay against the eager call
    st = gs.static
    st["alpha_t2s"].fill_(0.625)
    gs.g_style["enc"].replay()
    gs.g_style["t2s"].replay()
    want = fda.fda_transfer(st["x_t_tea"], st["x_s"], 0.05, 0.625, clamp=tr_g.recover, mean=MEAN, std=STD)
    assert torch.equal(st["x_t_tea_in"], want) and not torch.equal(want, st["x_t_tea"])
