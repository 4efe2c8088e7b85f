"""The fp64 BatchNorm / max-pool references and their bars (tests/helpers/fp64_bn.py) on the CPU: the references equal torch's float64
BatchNorm2d (train mode, autograd, residual and ReLU) and max_pool2d at ragged shapes; an fp32 emulation of each kernel form's order of
operations passes at the bars the GPU tests use (tests/test_gpu_bn_pool_forms.py); and each planted fault of the kind a wrong kernel
makes - one pixel dropped from a sum of 32768, a neighbouring channel group's coefficients, one skipped 32-pixel range, one flipped mask
element, a tap index off by one, zero instead of -inf padding - fails them."""
import pytest
import torch
import torch.nn.functional as F

from helpers import fp64_bn as fb
from helpers import fp64_conv as fc

BF = torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _params(C, seed):
    g = _gen(seed)
    return torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3


def _slab64(y, rows):
    """[rows][2][C] partial sums (float64) of y [M, C] over `rows` ragged pixel ranges."""
    parts = torch.tensor_split(y.double(), rows, 0)
    return torch.stack([torch.stack([p.sum(0), (p * p).sum(0)]) for p in parts])


# ---- the references equal torch --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,res,relu", [((3, 5, 7, 24), True, True), ((2, 1, 9, 8), False, True), ((1, 7, 3, 40), True, False),
                                            ((5, 3, 3, 16), False, False)])
def test_batchnorm_reference_equals_torch_float64(shape, res, relu):
    N, H, W, C = shape
    g = _gen(C + H)
    y = (torch.randn(shape, generator=g) * 1.5 + 0.3).double()
    r = torch.randn(shape, generator=g).double() if res else None
    dz = torch.randn(shape, generator=g).double()
    gamma, beta = (t.double() for t in _params(C, 3))
    bn = torch.nn.BatchNorm2d(C).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
        bn.running_mean.normal_(generator=g); bn.running_var.uniform_(0.5, 2, generator=g)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    yt = y.permute(0, 3, 1, 2).clone().requires_grad_(True)
    z = bn(yt)
    if res:
        z = z + r.permute(0, 3, 1, 2)
    if relu:
        z = torch.relu(z)
    z.backward(dz.permute(0, 3, 1, 2))
    M = N * H * W
    fin = fb.finalize(_slab64(y.reshape(M, C), 5), M, gamma, beta, momentum=0.1, eps=1e-5, running_mean=rm0, running_var=rv0)
    eps32 = float(torch.tensor(1e-5, dtype=torch.float32))       # (the reference takes eps and momentum as the fp32 values the kernel is passed)
    close = dict(rtol=1e-6, atol=1e-9)
    torch.testing.assert_close(fin["mean"][0], y.reshape(M, C).mean(0), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(fin["invstd"][0], 1 / torch.sqrt(y.reshape(M, C).var(0, unbiased=False) + eps32), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(fin["unbiased_var"][0], y.reshape(M, C).var(0, unbiased=True), rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(fin["running_mean"][0], bn.running_mean, **close)      # (momentum 0.1 against fp32(0.1): 1.5e-8 relative)
    torch.testing.assert_close(fin["running_var"][0], bn.running_var, **close)
    zr, absref = fb.apply(y.reshape(M, C), fin["scale"][0], fin["shift"][0], r.reshape(M, C) if res else None, relu)
    torch.testing.assert_close(zr, z.detach().permute(0, 2, 3, 1).reshape(M, C), rtol=1e-9, atol=1e-9)     # (eps against fp32(eps))
    assert bool((absref >= zr.abs() - 1e-12).all())
    keep = (zr > 0) if relu else None
    if relu and not res:        # the mask recomputed from y is the mask of z
        k2, und = fb.relu_mask_from_y(y.reshape(M, C), fin["mean"][0], fin["invstd"][0], gamma, beta)
        assert und == 0 and torch.equal(k2, keep)
    b = fb.backward(dz.reshape(M, C), y.reshape(M, C), fin["mean"][0], fin["invstd"][0], gamma, keep)
    torch.testing.assert_close(b["dy"][0], yt.grad.permute(0, 2, 3, 1).reshape(M, C), rtol=1e-8, atol=1e-10)
    torch.testing.assert_close(b["dgamma"][0], bn.weight.grad, rtol=1e-8, atol=1e-10)
    torch.testing.assert_close(b["dbeta"][0], bn.bias.grad, rtol=1e-10, atol=1e-10)
    assert bool((b["dy"][1] >= b["dy"][0].abs() - 1e-12).all())
    # the pre-reduced form on the slab of the masked gradient's own sums is the same backward
    gx = torch.stack([b["g"].sum(0), (b["g"] * b["xhat"]).sum(0)])[None]
    p = fb.backward_pre(b["g"], y.reshape(M, C), fin["mean"][0], fin["invstd"][0], gamma, gx)
    torch.testing.assert_close(p["dy"][0], b["dy"][0], rtol=1e-12, atol=1e-12)


def test_finalize_reference_clamp_count_one_and_pre_bias():
    C = 8
    gamma, beta = _params(C, 1)
    slab = torch.zeros(3, 2, C)
    k = torch.tensor([5.0, 2.0, 9.0])
    slab[:, 0] = 0.5 * k[:, None]
    slab[:, 1] = 0.25 * k[:, None] * (1 - 2.0 ** -20)       # sum of squares below count * mean^2: a negative variance, clamped
    fin = fb.finalize(slab, 16, gamma, beta, eps=1e-5)
    eps32 = float(torch.tensor(1e-5, dtype=torch.float32))
    torch.testing.assert_close(fin["invstd"][0], torch.full((C,), eps32 ** -0.5, dtype=torch.float64), rtol=1e-15, atol=0)
    assert torch.equal(fin["unbiased_var"][0], torch.zeros(C, dtype=torch.float64))
    one = torch.tensor([[[3.0] * C, [9.5] * C]])            # count == 1: the variance stays biased (no division by zero)
    f1 = fb.finalize(one, 1, gamma, beta)
    assert torch.equal(f1["unbiased_var"][0], torch.full((C,), 0.5, dtype=torch.float64))
    pb = torch.arange(C, dtype=torch.float32)
    f2 = fb.finalize(one, 1, gamma, beta, pre_bias=pb)     # the bias shifts the mean, not the variance
    assert torch.equal(f2["mean"][0], 3.0 + pb.double()) and torch.equal(f2["invstd"][0], f1["invstd"][0])


def _special_maps(shape, seed):
    g = _gen(seed)
    x = torch.randn(shape, generator=g).to(BF).float()
    out = {"random": x, "all_negative": -x.abs() - 0.5, "post_relu": torch.relu(x), "all_equal": torch.full(shape, 1.25)}
    xi = x.clone()
    xi[torch.rand(shape, generator=g) < 0.3] = float("-inf")
    out["neg_inf"] = xi
    xn = x.clone()
    xn[torch.rand(shape, generator=g) < 0.15] = float("nan")
    out["nan"] = xn
    return out


@pytest.mark.parametrize("shape", [(2, 1, 1, 8), (1, 1, 7, 8), (2, 2, 2, 16), (2, 7, 9, 24), (1, 8, 8, 8), (1, 18, 20, 8)])
def test_maxpool_reference_equals_torch(shape):
    N, H, W, C = shape
    for name, x in _special_maps(shape, H * W).items():
        xt = x.double().permute(0, 3, 1, 2)
        for kind in ("3x3", "2x2"):
            if kind == "3x3":
                val, tap = fb.maxpool3x3s2(x)
                tv, ti = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
                ho = torch.arange(val.shape[1])[:, None] * 2 - 1
                wo = torch.arange(val.shape[2])[None, :] * 2 - 1
                K = 3
            else:
                val, tap = fb.maxpool2x2_ceil(x)
                tv, ti = F.max_pool2d(xt, 2, 2, 0, ceil_mode=True, return_indices=True)
                ho = torch.arange(val.shape[1])[:, None] * 2
                wo = torch.arange(val.shape[2])[None, :] * 2
                K = 2
            fb.check_exact(val, tv.permute(0, 2, 3, 1), f"{name} {kind} value")
            ti = ti.permute(0, 2, 3, 1)
            ttap = (ti // W - ho[None, :, :, None]) * K + (ti % W - wo[None, :, :, None])
            fb.check_exact(tap, ttap, f"{name} {kind} tap")
        if name in ("nan", "neg_inf"):
            continue
        dy = torch.randn(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, generator=_gen(5)).double()
        xa = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        F.max_pool2d(xa, 3, 2, 1).backward(dy.permute(0, 3, 1, 2))
        _, tap = fb.maxpool3x3s2(x)
        ref, absref = fb.maxpool3x3s2_bwd(dy, tap, H, W)
        torch.testing.assert_close(ref, xa.grad.permute(0, 2, 3, 1), rtol=1e-13, atol=1e-13)
        assert bool((absref >= ref.abs()).all())
        dy2 = torch.randn(N, (H + 1) // 2, (W + 1) // 2, C, generator=_gen(6)).double()
        for mask in (False, True):
            xa = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
            F.max_pool2d(torch.relu(xa) if mask else xa, 2, 2, 0, ceil_mode=True).backward(dy2.permute(0, 3, 1, 2))
            if mask and name != "random":
                continue        # (relu'(0) = 0 in autograd sends a window of zeros nowhere; the library masks by x > 0 after pooling x itself)
            r2, _ = fb.maxpool2x2_ceil_bwd(torch.relu(x) if mask else x, dy2, relu_mask=mask)
            torch.testing.assert_close(r2, xa.grad.permute(0, 2, 3, 1), rtol=1e-13, atol=1e-13)


# ---- fp32 emulations of the kernels' order of operations --------------------------------------------------------------------------

def _seq_sum(t, dim):
    acc = torch.zeros_like(t.select(dim, 0))
    for k in range(t.shape[dim]):
        acc = acc + t.select(dim, k)
    return acc


def _emulate_bwd(dz, y, mean, invstd, gamma, keep, ppb, pstep, out_dtype, drop_pixel=None, skip_range=None, flip=None):
    """bn_bwd_reduce[_chunk]_k + finalize + apply in fp32: work-groups of ppb pixels, thread prow adds pixels prow, prow + pstep, ...
    in order, one thread adds the pstep LDS rows in order, the slab is summed in fp64, the apply is fp32.  Faults: a pixel left out of
    the sums, a pixel range the reduce skipped, one mask element flipped in the apply."""
    M, C = y.shape
    yf, gf = y.float(), torch.where(keep, dz.float(), torch.zeros(())) if keep is not None else dz.float()
    xh = (yf - mean) * invstd
    t1, t2 = gf.clone(), gf * xh
    if drop_pixel is not None:
        t1[drop_pixel], t2[drop_pixel] = 0, 0
    if skip_range is not None:
        t1[skip_range:skip_range + 32], t2[skip_range:skip_range + 32] = 0, 0
    rows = -(-M // ppb)
    J = -(-ppb // pstep)

    def red(t):
        # block b covers [b*ppb, (b+1)*ppb); inside, pixel j*pstep + prow belongs to thread prow
        tb = torch.zeros(rows, J * pstep, C)
        src = torch.cat([t, torch.zeros(rows * ppb - M, C)]).reshape(rows, ppb, C)
        tb[:, :ppb] = src
        return _seq_sum(_seq_sum(tb.reshape(rows, J, pstep, C), 1), 1)          # [rows, C] fp32 partials
    s1, s2 = red(t1).double().sum(0), red(t2).double().sum(0)
    ca = gamma * invstd
    cb, cc = (s1 / M).float(), (s2 / M).float()
    ga = gf.clone()
    if flip is not None:
        ga[flip] = dz.float()[flip] if ga[flip] == 0 else 0.0
    dy = (ca * (ga - cb - xh * cc)).to(out_dtype)
    return dy, s1.float(), s2.float()


def _bwd_case(M, C, seed, relu=True):
    g = _gen(seed)
    y = (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(BF)
    dz = torch.randn(M, C, generator=g).to(BF)
    dz[dz == 0] = 1.0
    mean = torch.randn(C, generator=g) * 0.2 + 0.3
    invstd = torch.rand(C, generator=g) * 0.5 + 0.4
    gamma, beta = _params(C, seed + 1)
    keep = fb.relu_mask_from_y(y, mean, invstd, gamma, beta)[0] if relu else None
    return y, dz, mean, invstd, gamma, keep


def _check_bwd(out, ref, L, dtype, what):
    dy, s1, s2 = out
    tau = fb.tau_of(L)
    worst = [fc.check(dy, *ref["dy"], dtype, tau, tau, what + " dy")]
    worst.append(fb.check_sums(s1, *ref["dbeta"], tau, what + " dbeta"))
    worst.append(fb.check_sums(s2, *ref["dgamma"], tau, what + " dgamma"))
    return max(w[0] for w in worst)


@pytest.mark.parametrize("M,C,chunked", [(1031, 8, False), (1031, 64, False), (31, 128, False), (32768, 64, False), (1200, 256, True),
                                         (32768, 256, True)])
def test_fp32_backward_emulation_passes_the_bars(M, C, chunked):
    y, dz, mean, invstd, gamma, keep = _bwd_case(M, C, M + C)
    ref = fb.backward(dz, y, mean, invstd, gamma, keep)
    if chunked:
        ppb, pstep, L = fb.chunk_P(M, C), 32, fb.chunk_chain(M, C)
    else:
        pstep = 256 // (C // 8)
        rows = max(1, min(1024, -(-M // pstep)))
        ppb, L = -(-M // rows), fb.stream_chain(M, C)
    for dt in (BF, torch.float32):
        t = _check_bwd(_emulate_bwd(dz, y, mean, invstd, gamma, keep, ppb, pstep, dt), ref, L, dt, f"M {M} C {C}")
        assert t < 0.5 * fb.tau_of(L), (t, fb.tau_of(L))


def test_planted_backward_faults_fail():
    M, C = 32768, 64
    y, dz, mean, invstd, gamma, keep = _bwd_case(M, C, 7)
    ref = fb.backward(dz, y, mean, invstd, gamma, keep)
    L = fb.stream_chain(M, C)
    pix = int(keep[:, 5].nonzero()[100])          # a pixel whose gradient survives the mask in channel 5
    # the measured tau a dropped pixel leaves in dy: far above the bar
    dy, _, _ = _emulate_bwd(dz, y, mean, invstd, gamma, keep, 32, 32, torch.float32, drop_pixel=pix)
    t_drop, _ = fc.measure(dy, *ref["dy"], torch.float32)
    assert t_drop > 20 * fb.tau_of(L), (t_drop, fb.tau_of(L))
    # (a 16-bit dy hides a sum that is off by one pixel of 32768 under its own rounding: there the fp32 dbeta / dgamma are what shows it,
    # which is why the GPU tests hold them to the same bar; a flipped mask element shows in dy itself in every type)
    for kw, outs in (({"drop_pixel": pix}, ("dy", "dbeta", "dgamma")), ({"skip_range": 4096}, ("dy", "dbeta", "dgamma")), ({"flip": (777, 3)}, ("dy",))):
        for dt in (BF, torch.float32):
            out = _emulate_bwd(dz, y, mean, invstd, gamma, keep, 32, 32, dt, **kw)
            for name, got in zip(("dy", "dbeta", "dgamma"), out):
                if name in outs and not (name == "dy" and dt == BF and "flip" not in kw):
                    with pytest.raises(AssertionError):
                        if name == "dy":
                            fc.check(got, *ref[name], dt, fb.tau_of(L), fb.tau_of(L), name)
                        else:
                            fb.check_sums(got, *ref[name], fb.tau_of(L), name)
    # the sums of the device's own gout: a reduce that masks differently from the apply shows there even in a 16-bit dy
    _, s1, _ = _emulate_bwd(dz, y, mean, invstd, gamma, keep, 32, 32, BF, drop_pixel=pix)
    with pytest.raises(AssertionError):
        fb.check_sums(s1, ref["g"].sum(0), ref["g"].abs().sum(0), fb.tau_of(L), "dbeta against gout")


def test_planted_exact_zero_is_masked_and_a_non_strict_mask_fails():
    """relu == 2 recomputes the mask as y * sc + sh > 0, strictly.  Planted exact zeros - mean 0.5, invstd 2, gamma 1, beta 0, y = 0.5: sc = 2,
    sh = -1, every intermediate exact in fp32, fused or not - are decided, not undecided, and masked out; a kernel whose test read >= 0 would
    pass their gradient, and fails gout, dy and the sums."""
    M, C = 1031, 64
    y, dz, mean, invstd, gamma, _ = _bwd_case(M, C, 31, relu=False)
    beta = _params(C, 32)[1]
    pix = torch.tensor([0, 343, 515, 1030])
    zero = torch.zeros(M, C, dtype=torch.bool)
    for ch in (0, C - 1):
        mean[ch], invstd[ch], gamma[ch], beta[ch] = 0.5, 2.0, 1.0, 0.0
        y[pix, ch] = 0.5
        zero[pix, ch] = True
    sc = gamma * invstd
    sh = beta - mean * sc
    assert bool((y.float()[zero] * sc.expand(M, C)[zero] + sh.expand(M, C)[zero] == 0).all())               # separate multiply and add
    assert bool((torch.addcmul(sh.expand(M, C), y.float(), sc.expand(M, C))[zero] == 0).all())            # one fused operation
    keep, und = fb.relu_mask_from_y(y, mean, invstd, gamma, beta)
    assert und == 0 and not bool(keep[zero].any())
    # the device's gout is not consulted for them: a device that passed them cannot talk the reference round
    keep2, _ = fb.relu_mask_from_y(y, mean, invstd, gamma, beta, gout=dz)
    assert torch.equal(keep2, keep)
    ref = fb.backward(dz, y, mean, invstd, gamma, keep)
    L = fb.stream_chain(M, C)
    pstep = 256 // (C // 8)
    ppb = -(-M // max(1, min(1024, -(-M // pstep))))
    for dt in (BF, torch.float32):
        _check_bwd(_emulate_bwd(dz, y, mean, invstd, gamma, keep, ppb, pstep, dt), ref, L, dt, "strict mask")
        ge = keep | zero                                                                                  # the mask of a kernel that tests >= 0
        dy, s1, s2 = _emulate_bwd(dz, y, mean, invstd, gamma, ge, ppb, pstep, dt)
        with pytest.raises(AssertionError):
            fb.check_exact(torch.where(ge, dz, torch.zeros(()).to(BF)), ref["g"], "gout")
        with pytest.raises(AssertionError):
            fc.check(dy, *ref["dy"], dt, fb.tau_of(L), fb.tau_of(L), "dy")
        with pytest.raises(AssertionError):
            fb.check_sums(s1, *ref["dbeta"], fb.tau_of(L), "dbeta")


def test_fp32_pre_reduced_emulation_passes_and_planted_faults_fail():
    """The pre-reduced backward (bn_bwd_apply_pre[_chunk]_k): the slab of the masked gradient's partial sums is added in fp64, the
    coefficients and the apply are fp32 (L = 0)."""
    M, C = 1200, 64
    y, dz, mean, invstd, gamma, keep = _bwd_case(M, C, 21)
    g = torch.where(keep, dz, torch.zeros(()).to(BF))
    xh64 = (y.double() - mean.double()) * invstd.double()
    parts = torch.tensor_split(torch.arange(M), 57)
    slab = torch.stack([torch.stack([g.double()[i].sum(0), (g.double() * xh64)[i].sum(0)]) for i in parts]).float()
    ref = fb.backward_pre(g, y, mean, invstd, gamma, slab)
    tau = fb.tau_of(0)

    def emulate(slab_, ca):
        s = slab_.double().sum(0)
        cb, cc = (s[0] / M).float(), (s[1] / M).float()
        xh = (y.float() - mean) * invstd
        return (ca * (g.float() - cb - xh * cc)), s[0].float(), s[1].float()
    for dt in (BF, torch.float16, torch.float32):
        dy, s1, s2 = emulate(slab, gamma * invstd)
        t, _ = fc.check(dy.to(dt), *ref["dy"], dt, tau, tau, "pre dy")
        assert t < 0.5 * tau
        fb.check_sums(s1, *ref["dbeta"], tau, "pre dbeta")
        fb.check_sums(s2, *ref["dgamma"], tau, "pre dgamma")
        with pytest.raises(AssertionError):           # one slab row of 57 left out of the prelude
            fc.check(emulate(slab[1:], gamma * invstd)[0].to(dt), *ref["dy"], dt, tau, tau, "pre dy, row skipped")
        with pytest.raises(AssertionError):           # a neighbouring channel group's coefficients
            fc.check(emulate(slab, (gamma * invstd).roll(8))[0].to(dt), *ref["dy"], dt, tau, tau, "pre dy, rolled coefficients")
    with pytest.raises(AssertionError):
        fb.check_sums(emulate(slab[1:], gamma * invstd)[1], *ref["dbeta"], tau, "pre dbeta, row skipped")


def _emulate_apply(y, scale, shift, res, relu, dtype):
    o = y.float() * scale + shift
    if res is not None:
        o = o + res.float()
    return (torch.relu(o) if relu else o).to(dtype)


def test_fp32_forward_emulation_passes_and_planted_faults_fail():
    M, C = 1031, 64
    g = _gen(11)
    y = (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(BF)
    res = torch.randn(M, C, generator=g).to(BF)
    gamma, beta = _params(C, 12)
    slab = _slab64(y, 97).float()
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    fin = fb.finalize(slab, M, gamma, beta, running_mean=rm, running_var=rv)
    # the kernel's finalize: fp64 sums, then fp32
    s = slab.double().sum(0)
    mean = s[0] / M
    var = (s[1] / M - mean * mean).clamp(min=0)
    invstd = (1.0 / torch.sqrt(var + float(torch.tensor(1e-5)))).float()
    sc = gamma * invstd
    sh = beta - mean.float() * sc
    m32 = torch.tensor(0.1)
    got = {"mean": mean.float(), "invstd": invstd, "scale": sc, "shift": sh, "unbiased_var": (var * M / (M - 1)).float(),
           "running_mean": (1 - m32) * rm + m32 * mean.float(), "running_var": (1 - m32) * rv + m32 * (var * M / (M - 1)).float()}
    for k, v in got.items():
        fb.check_ulps(v, *fin[k], 2 if k in ("mean", "invstd", "scale", "unbiased_var") else 3, k)
    with pytest.raises(AssertionError):           # one slab row left out of 97
        fb.check_ulps((slab[1:].double().sum(0)[0] / M).float(), *fin["mean"], 2, "mean")
    tau = fb.tau_of(0)
    for dt in (BF, torch.float16, torch.float32):
        for r_, relu in ((res, True), (None, False)):
            ref = fb.apply(y, sc, sh, r_, relu)
            t, _ = fc.check(_emulate_apply(y, sc, sh, r_, relu, dt), *ref, dt, tau, tau, "apply")
            assert t < 0.5 * tau
            # a neighbouring channel group's coefficients
            with pytest.raises(AssertionError):
                fc.check(_emulate_apply(y, sc.roll(8), sh.roll(8), r_, relu, dt), *ref, dt, tau, tau, "apply, rolled coefficients")
            # one skipped 32-pixel range (the output keeps what it held)
            z = _emulate_apply(y, sc, sh, r_, relu, dt)
            z[992:1024] = 0
            with pytest.raises(AssertionError):
                fc.check(z, *ref, dt, tau, tau, "apply, skipped range")


def test_planted_pool_faults_fail():
    x = _special_maps((2, 7, 9, 8), 3)["all_negative"]
    val, tap = fb.maxpool3x3s2(x)
    zero_pad = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2, 0).permute(0, 2, 3, 1)      # zero instead of -inf padding
    with pytest.raises(AssertionError):
        fb.check_exact(zero_pad, val, "zero padding")
    # a kernel that reports tap 0 for a window of equal values: at a border the first in-range tap is not tap 0
    _, tie = fb.maxpool3x3s2(torch.full((2, 7, 9, 8), 1.25))
    assert int(tie[0, 0, 0, 0]) == 4 and int(tie[0, 0, 1, 0]) == 3 and int(tie[0, 1, 0, 0]) == 1 and int(tie[0, 1, 1, 0]) == 0
    with pytest.raises(AssertionError):
        fb.check_exact(torch.zeros_like(tie), tie, "tap 0 in a border window")
    off = tap.clone()
    off[1, 2, 3, 4] += 1                                                                                  # a tap index off by one: the gradient lands a pixel away
    dy = torch.randn(val.shape, generator=_gen(2)).to(BF)
    ref, absref = fb.maxpool3x3s2_bwd(dy, tap, 7, 9)
    bad, _ = fb.maxpool3x3s2_bwd(dy, off, 7, 9)
    fc.check(ref.to(BF), ref, absref, BF, fb.tau_of(4), fb.tau_of(4), "pool backward")
    with pytest.raises(AssertionError):
        fc.check(bad.to(BF), ref, absref, BF, fb.tau_of(4), fb.tau_of(4), "pool backward, wrong tap")
    nan = _special_maps((1, 4, 4, 8), 4)["nan"]
    v2, _ = fb.maxpool2x2_ceil(nan)
    dropped = torch.nan_to_num(nan, nan=float("-inf")).reshape(1, 2, 2, 2, 2, 8).amax((2, 4))              # fmaxf drops a NaN
    assert bool(torch.isnan(v2).any())
    with pytest.raises(AssertionError):
        fb.check_exact(dropped, v2, "NaN dropped")
