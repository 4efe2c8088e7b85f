"""The AdaIN decoder's training step (uda_poseestimation_amd.adain, reference adain/net.py:102-162) on the MI355X: the backward kernels one
by one against torch-CPU fp32 autograd on the same 16-bit-rounded inputs, the whole step against the CPU oracle, determinism, and a
short Adam run with the reference's call forms."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from uda_poseestimation_amd import _hip, ops  # noqa: E402

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _nhwc(x_nchw, dt):
    return x_nchw.permute(0, 2, 3, 1).contiguous().to(dt).cuda()


def _r(x, dt):
    """round to the 16-bit type and back to fp32 (CPU)"""
    return x.to(dt).float()


# ------------------------------------------------------------------ per kernel
# (N, H, W, Ci, Co, upsample, relu mask): decoder and encoder geometries at reduced maps, odd sizes included
GEOMS = [(2, 8, 8, 512, 256, True, True), (2, 16, 16, 256, 256, False, True), (2, 9, 7, 256, 128, False, True), (2, 16, 16, 128, 128, True, True),
         (1, 13, 11, 128, 64, False, True), (2, 16, 16, 64, 64, True, True), (2, 33, 31, 64, 64, False, False), (2, 20, 20, 64, 128, False, True),
         (2, 5, 6, 256, 512, False, True), (2, 4, 4, 512, 512, False, True), (1, 2, 3, 64, 64, False, True)]


def _ref_conv(x, w, b, up):
    if up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("geom", GEOMS)
def test_reflect_conv_dgrad_wgrad_bias(geom, prec):
    N, H, W, Ci, Co, up, mask = geom
    dt = DT[prec]
    g = torch.Generator().manual_seed(hash(geom) & 0xffff)
    x = _r(torch.randn(N, Ci, H, W, generator=g), dt)
    if mask:
        x = _r(F.relu(x), dt)           # the producer's ReLU output (the mask source)
    w = _r(torch.randn(Co, Ci, 3, 3, generator=g) * (2.0 / (9 * Ci)) ** 0.5, dt)
    b = torch.randn(Co, generator=g) * 0.1
    Hl, Wl = H << int(up), W << int(up)
    dy = _r(torch.randn(N, Co, Hl, Wl, generator=g), dt)
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    _ref_conv(xr, wr, br, up).backward(dy)
    dx_ref = xr.grad * (x > 0) if mask else xr.grad
    d = ops.conv_desc(N, H, W, Ci, Co, 3, 1, 1, reflect=True, upsample=up)
    ops.conv_bwd_prepare(d, dt)
    ws = torch.empty(ops.conv_bwd_ws_bytes(d), dtype=torch.uint8, device="cuda")
    w_bwd = ops.pack_weight(w.cuda(), d, "bwd", dtype=dt)
    dyn, xn = _nhwc(dy, dt), _nhwc(x, dt)
    dx = ops.conv2d_bwd_data_reflect(dyn, w_bwd, d, ws, relu_src=xn if mask else None)
    dx = dx.float().permute(0, 3, 1, 2).cpu()
    err = (dx - dx_ref).abs().max().item()
    assert err <= 1.2e-2 * dx_ref.abs().max().item(), (err, dx_ref.abs().max().item())
    dw = ops.conv2d_bwd_weight_reflect(dyn, xn, d, ws).cpu()
    err = (dw - wr.grad).abs().max().item()
    assert err <= 2e-3 * wr.grad.abs().max().item(), (err, wr.grad.abs().max().item())
    bws = torch.empty(ops.bias_grad_ws_bytes(N * Hl * Wl, Co), dtype=torch.uint8, device="cuda")
    db = ops.bias_grad(dyn, bws).cpu()
    assert (db - br.grad).abs().max().item() <= 2e-3 * br.grad.abs().max().item()
    # bit-reproducible
    dw2 = ops.conv2d_bwd_weight_reflect(dyn, xn, d, ws).cpu()
    db2 = ops.bias_grad(dyn, bws).cpu()
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def test_reflect_dgrad_unsupported_today_is_supported():
    """the pre-existing per-layer calls keep refusing reflect geometries; the new ones accept them"""
    d = ops.conv_desc(1, 8, 8, 64, 64, 3, 1, 1, reflect=True)
    assert ops.conv_bwd_ws_bytes(d) > 0
    dy = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(64, 9, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.conv2d_bwd_data(dy, w, d)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("HW", [(16, 16), (9, 7)])
def test_end_layers(prec, HW):
    """the two odd end layers alone: the encoder stem's data gradient into the 3-channel image (1x1 colour conv folded in, Ci 3 zero-padded
    to 64: channels 3..63 of the result exactly zero) and the decoder's 64 -> 3 layer (Co zero-padded to 64, co_valid = 3)"""
    from uda_poseestimation_amd.adain.net import Net
    from uda_poseestimation_amd.lib.models.Style_net import _compile
    dt = DT[prec]
    H, W = HW
    N = 2
    g = torch.Generator().manual_seed(H * 100 + W)
    # ---- stem: y = conv3x3(reflect(conv1x1(x)))
    c1, c3 = nn.Conv2d(3, 3, 1), nn.Conv2d(3, 64, 3)
    x = torch.rand(N, 3, H, W, generator=g)
    dz = _r(torch.randn(N, 64, H, W, generator=g), dt)
    xr = x.clone().requires_grad_(True)
    c3(F.pad(c1(xr), (1, 1, 1, 1), mode="reflect")).backward(dz)
    st = _compile([c1, nn.ReflectionPad2d(1), c3, nn.ReLU()])[0]
    w, _ = Net._folded(st)
    wp = torch.zeros(64, 64, 3, 3)
    wp[:, :3] = w
    d = ops.conv_desc(N, H, W, 64, 64, 3, 1, 1, reflect=True)
    ops.conv_bwd_prepare(d, dt)
    ws = torch.empty(ops.conv_bwd_ws_bytes(d), dtype=torch.uint8, device="cuda")
    dP = ops.conv2d_bwd_data_reflect_padded(_nhwc(dz, dt), ops.pack_weight(wp.cuda(), d, "bwd", dtype=dt), d,
                                            torch.empty(N, H + 2, W + 2, 64, dtype=dt, device="cuda"))
    dx = ops.reflect_fold(torch.empty(N, H, W, 64, dtype=dt, device="cuda"), dP=dP).float().cpu()
    assert torch.count_nonzero(dx[..., 3:]) == 0
    ref = xr.grad.permute(0, 2, 3, 1)
    assert (dx[..., :3] - ref).abs().max().item() <= 1.2e-2 * ref.abs().max().item()
    # ---- decoder's last layer: 64 -> 3, no ReLU after it; its input is a ReLU output
    conv = nn.Conv2d(64, 3, 3)
    conv.weight.data = _r(conv.weight.data, dt)
    xin = _r(F.relu(torch.randn(N, 64, H, W, generator=g)), dt)
    dy = _r(torch.randn(N, 3, H, W, generator=g), dt)
    xr = xin.clone().requires_grad_(True)
    conv(F.pad(xr, (1, 1, 1, 1), mode="reflect")).backward(dy)
    dyp = torch.zeros(N, 64, H, W)
    dyp[:, :3] = dy
    wp = torch.zeros(64, 64, 3, 3)
    wp[:3] = conv.weight.detach()
    dyn, xn = _nhwc(dyp, dt), _nhwc(xin, dt)
    dxd = ops.conv2d_bwd_data_reflect(dyn, ops.pack_weight(wp.cuda(), d, "bwd", dtype=dt), d, ws, relu_src=xn).float().permute(0, 3, 1, 2).cpu()
    refx = xr.grad * (xin > 0)
    assert (dxd - refx).abs().max().item() <= 1.2e-2 * refx.abs().max().item()
    dw = ops.conv2d_bwd_weight_reflect(dyn, xn, d, ws, co_valid=3).cpu()
    assert dw.shape == (3, 64, 3, 3)
    assert (dw - conv.weight.grad).abs().max().item() <= 2e-3 * conv.weight.grad.abs().max().item()
    bws = torch.empty(ops.bias_grad_ws_bytes(N * H * W, 64), dtype=torch.uint8, device="cuda")
    db = ops.bias_grad(dyn, bws, c_valid=3).cpu()
    assert (db - conv.bias.grad).abs().max().item() <= 2e-3 * conv.bias.grad.abs().max().item()


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(2, 8, 8, 64), (2, 7, 9, 128), (1, 1, 5, 64), (3, 5, 1, 64)])
def test_maxpool_bwd_bit_exact_ties(shape, prec):
    dt = DT[prec]
    N, H, W, C = shape
    g = torch.Generator().manual_seed(3)
    x = F.relu(torch.randint(-3, 4, (N, C, H, W), generator=g).float())     # many ties (zeros and small integers after ReLU)
    dy = torch.randn(N, C, (H + 1) // 2, (W + 1) // 2, generator=g).to(dt).float()
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(xr, 2, 2, 0, ceil_mode=True).backward(dy)
    for mask in (False, True):
        ref = xr.grad * (x > 0) if mask else xr.grad
        out = ops.maxpool2x2_ceil_bwd(_nhwc(x, dt), _nhwc(dy, dt), relu_mask=mask).float().permute(0, 3, 1, 2).cpu()
        assert torch.equal(out, ref.to(dt).float())


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_style_stat_loss_and_grad_fp64(prec):
    dt = DT[prec]
    N, C, H, W = 2, 64, 7, 9
    g = torch.Generator().manual_seed(5)
    x = F.relu(torch.randn(N, C, H, W, generator=g)).to(dt).double()
    s = torch.randn(N, C, H, W, generator=g).abs().to(dt).double()
    xr = x.clone().requires_grad_(True)

    def ms(f):
        v = f.reshape(N, C, -1).var(dim=2) + 1e-5
        return f.reshape(N, C, -1).mean(dim=2), v.sqrt()
    (m, sd), (mt, sdt) = ms(xr), ms(s)
    loss = F.mse_loss(m, mt) + F.mse_loss(sd, sdt)
    sw = 0.7
    (sw * loss).backward()
    xn, sn = _nhwc(x.float(), dt), _nhwc(s.float(), dt)
    stats = ops.adain(xn, sn, stats_only=True)
    out = torch.empty((), dtype=torch.float32, device="cuda")
    ops.style_stat_loss(stats, out)
    assert abs(out.item() - loss.item()) <= 1e-4 * abs(loss.item())
    gs = torch.tensor(sw, device="cuda")
    dx = ops.reflect_fold(torch.empty_like(xn), x=xn, stats=stats, gscale_s=gs).float().permute(0, 3, 1, 2).cpu().double()
    ref = xr.grad
    assert (dx - ref).abs().max().item() <= 1e-2 * ref.abs().max().item()
    # content MSE forward
    mws = torch.empty(ops.feat_mse_ws_bytes(), dtype=torch.uint8, device="cuda")
    mse = ops.feat_mse(xn, sn, mws).item()
    assert abs(mse - F.mse_loss(x, s).item()) <= 1e-4 * F.mse_loss(x, s).item()


# ------------------------------------------------------------------ whole step
def _nets(prec):
    from helpers.adain_oracle import make_nets
    from uda_poseestimation_amd.adain import net as anet
    vgg_r, dec_r = make_nets()
    vgg = copy.deepcopy(anet.vgg)
    dec = copy.deepcopy(anet.decoder)
    vgg.load_state_dict(vgg_r.state_dict())
    dec.load_state_dict(dec_r.state_dict())
    vgg31 = nn.Sequential(*list(vgg.children())[:31])
    n = anet.Net(vgg31, dec.cuda()).cuda()
    n.precision = prec
    return vgg_r, dec_r, n, dec


def _images(N, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, 3, S, S, generator=g), torch.rand(N, 3, S, S, generator=g)


BARS = {"bf16": (2e-2, 0.995, 0.1), "fp16": (2e-3, 0.999, 0.05)}


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("N,S", [(2, 64), (4, 256)])
def test_step_against_oracle(prec, N, S, capsys):
    from helpers.adain_oracle import step_ref
    vgg_r, dec_r, net, dec = _nets(prec)
    c, s = _images(N, S, 7)
    lc_r, ls_r, g_r = step_ref(nn.Sequential(*list(vgg_r.children())[:31]), dec_r, c, s)
    (lc_r + 0.1 * ls_r).backward()
    lc, ls, g_t = net(c.cuda(), s.cuda())
    (lc + 0.1 * ls).backward()
    lerr, cmin, nerr = BARS[prec]
    rows = []
    assert abs(lc.item() - lc_r.item()) <= lerr * abs(lc_r.item()), (lc.item(), lc_r.item())
    assert abs(ls.item() - ls_r.item()) <= lerr * abs(ls_r.item()), (ls.item(), ls_r.item())
    bad = []
    for (name, p), (_, pr) in zip(dec.named_parameters(), dec_r.named_parameters()):
        a, b = p.grad.detach().cpu().double().flatten(), pr.grad.double().flatten()
        cos = (a @ b / (a.norm() * b.norm())).item()
        rn = ((a.norm() - b.norm()).abs() / b.norm()).item()
        rows.append(f"{name}: cos {cos:.5f} rel-norm {rn:.4f}")
        if cos < cmin or rn > nerr:
            bad.append(rows[-1])
    with capsys.disabled():
        print(f"\n[{prec} N={N} {S}x{S}] loss_c {lc.item():.5g} (ref {lc_r.item():.5g}) loss_s {ls.item():.5g} (ref {ls_r.item():.5g})")
        print("\n".join(rows))
    assert not bad, bad
    # only the decoder receives gradients
    assert all(p.grad is None for p in net.enc_1.parameters())


def test_step_deterministic():
    _, _, net, dec = _nets("bf16")
    c, s = _images(2, 64, 9)
    out = []
    for _ in range(2):
        dec.zero_grad(set_to_none=True)
        lc, ls, _ = net(c.cuda(), s.cuda())
        (lc + 0.1 * ls).backward()
        out.append([p.grad.clone() for p in dec.parameters()] + [lc.detach().clone(), ls.detach().clone()])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_gt_gradient_is_added():
    _, _, net, dec = _nets("bf16")
    c, s = _images(2, 64, 10)
    lc, ls, g = net(c.cuda(), s.cuda())
    (lc + 0.1 * ls).backward()
    g0 = [p.grad.clone() for p in dec.parameters()]
    dec.zero_grad(set_to_none=True)
    lc, ls, g = net(c.cuda(), s.cuda())
    (lc + 0.1 * ls + 1e-3 * g.square().sum()).backward()
    assert any(not torch.equal(a, p.grad) for a, p in zip(g0, dec.parameters()))


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("opt", ["adam", "fused"])
def test_training_loss_falls_and_tracks_oracle(opt, prec, capsys):
    """20 steps on fixed synthetic pairs in the reference's loop form (random content/style swap, Adam on the decoder's parameters at the
    reference's lr 1e-5), device against the CPU oracle stepped alongside: every step's loss within 5 %, the 20th within 3 %.  The loss at
    ONE fixed pair order falls (this needs training: with lr 0 it stays put).
    (At lr 1e-4 the first Adam step sends this seeded network's loss from 0.97 to ~22 and the 16-bit and fp32 trajectories separate from
    there, with the oracle's gradient at the device's weights still at cosine >= 0.999 in fp16: DESIGN.md section 4.1.)"""
    from helpers.adain_oracle import step_ref
    from uda_poseestimation_amd.optim import FusedAdam
    vgg_r, dec_r, net, dec = _nets(prec)
    vgg31r = nn.Sequential(*list(vgg_r.children())[:31])
    src, tgt = _images(2, 64, 21)
    lr = 1e-5
    o = torch.optim.Adam(net.decoder.parameters(), lr=lr) if opt == "adam" else FusedAdam(net.decoder.parameters(), lr=lr)
    o_r = torch.optim.Adam(dec_r.parameters(), lr=lr)

    def fixed_pair_loss():
        with torch.no_grad():
            lc, ls, _ = net(src.cuda(), tgt.cuda())
        return (lc + 0.1 * ls).item()
    before = fixed_pair_loss()
    rs = np.random.RandomState(0)
    hist, hist_r = [], []
    for _ in range(20):
        if rs.rand() > 0.5:
            c, s = src, tgt
        else:
            c, s = tgt, src
        lc, ls, _ = net(c.cuda(), s.cuda())
        loss = lc + 0.1 * ls
        o.zero_grad()
        loss.backward()
        o.step()
        hist.append(loss.item())
        lcr, lsr, _ = step_ref(vgg31r, dec_r, c, s)
        lr_ = lcr + 0.1 * lsr
        o_r.zero_grad()
        lr_.backward()
        o_r.step()
        hist_r.append(lr_.item())
    after = fixed_pair_loss()
    gaps = [abs(a - b) / b for a, b in zip(hist, hist_r)]
    with capsys.disabled():
        print(f"\n[{opt} {prec}] per step: device / oracle / gap")
        for k, (a, b, e) in enumerate(zip(hist, hist_r, gaps)):
            print(f"  {k + 1:2d} {a:.5f} {b:.5f} {e:.4f}")
        print(f"  fixed pair order: {before:.5f} -> {after:.5f}")
    assert after < 0.8 * before
    assert max(gaps) <= 0.05, gaps
    assert gaps[-1] <= 0.03, gaps


def test_trained_decoder_loads_into_style_net():
    from oracle.style_ref import style_forward_ref
    from uda_poseestimation_amd.lib.models import Style_net
    vgg_r, dec_r, net, dec = _nets("bf16")
    o = torch.optim.Adam(net.decoder.parameters(), lr=1e-4)
    c, s = _images(2, 64, 30)
    for _ in range(2):
        lc, ls, _ = net(c.cuda(), s.cuda())
        o.zero_grad()
        (lc + 0.1 * ls).backward()
        o.step()
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    sn_dec = copy.deepcopy(Style_net.decoder)
    sn_dec.load_state_dict(sd)
    dec_r.load_state_dict(sd)
    vgg31 = nn.Sequential(*list(copy.deepcopy(Style_net.vgg).children())[:31])
    vgg31.load_state_dict(nn.Sequential(*list(vgg_r.children())[:31]).state_dict())
    sn = Style_net.Net(vgg31.cuda(), sn_dec.cuda())
    g = sn(c.cuda(), s.cuda())[2].cpu()
    with torch.no_grad():
        g_r = style_forward_ref(nn.Sequential(*list(vgg_r.children())[:31]), dec_r, c, s)
    assert (g - g_r).abs().max().item() <= 5e-5 * g_r.abs().max().item() + 1e-6


# ------------------------------------------------------------------ against the reference's own adain/net.py (tests/golden/adain_train.npz)
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_step_against_reference_golden(prec, golden_dir):
    import os
    z = np.load(os.path.join(golden_dir, "adain_train.npz"))
    _, _, net, dec = _nets(prec)          # the same seeds as the fixture (vgg 11, decoder 12)
    c, s = torch.from_numpy(z["content"]).cuda(), torch.from_numpy(z["style"]).cuda()
    lc, ls, g_t = net(c, s)
    (lc + float(z["style_weight"]) * ls).backward()
    lerr, cmin, nerr = BARS[prec]
    assert abs(lc.item() - z["losses"][0, 0]) <= lerr * z["losses"][0, 0]
    assert abs(ls.item() - z["losses"][0, 1]) <= lerr * z["losses"][0, 1]
    assert (g_t.detach().cpu().numpy() - z["g_t"]).std() <= 0.05 * z["g_t"].std()
    for name, p in dec.named_parameters():
        g = p.grad.detach().cpu().double().flatten().numpy()
        ref = z[f"step0/{name}/values"].astype(np.float64)
        got = g[z[f"step0/{name}/idx"]] if f"step0/{name}/idx" in z else g
        cos = got @ ref / (np.linalg.norm(got) * np.linalg.norm(ref))
        rn = abs(np.linalg.norm(g) - float(z[f"step0/{name}/norm"])) / float(z[f"step0/{name}/norm"])
        assert cos >= cmin and rn <= nerr, (name, cos, rn)


# ------------------------------------------------------------------ capture
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_captured_step_equals_eager_to_the_bit(prec):
    """5 Adam steps, eager against one captured step replayed: losses, parameters and both moments bit-identical.  The replays must re-pack
    the decoder weights their own optimizer step wrote (a host-side pack cache would replay stale packs and diverge at step 2).  Runs in a
    fresh interpreter (tests/helpers/adain_capture_check.py): a stream capture re-registers the CUDA generator's state with the graph, which
    later tests of this session that draw from it must not see."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "helpers", "adain_capture_check.py"), prec], cwd=root, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "CAPTURE_EQUALS_EAGER" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
