"""Every convolution kernel form against the float64 reference, element by element (tests/helpers/fp64_conv.py: check()).

(A) Forced-form matrix at small, ragged shapes: each igemm tile id (3, 4, 5, 6, 9; 10 / 11 in the 16-bit builds), with the lean 1x1,
    short-LDS and tap0 variants on and off and the 3-stage ring lowered to small K (igemm_ns3_k), in the bf16 and fp16 builds, the
    exact fp32 path and the f16x2 split path; fprop (+ the fused statistics, + residual / bias / ReLU / fp32 output), the data
    gradient, and the data gradient with the consumer BatchNorm's epilogue.  Weight gradients: every wgrad_tile, split counts 1 / 3 / 4,
    the three loaders (wgrad_fastgeo 0 / 1 / 2), the filter-row form on and off, DMA and non-DMA channel counts, transposed, the
    stem, accumulation.
(B) The convolutions of the benchmarked PoseResNet-101 (configs[1]: N = 32, 256x256, bf16; configs[4]: N = 8, 384x384, K = 18, fp16)
    under the default policy and under every tile form eligible there; the default output must be bit-identical to one forced form.
(C) Grouped weight-gradient launches against per-layer launches on the full configs[1] network.

Forms the library refuses (an error code, nothing launched - each return precedes the kernel launch in igemm_launch / wgrad_launch):
  * 16-bit forward with Ci % 64 != 0 (other than the Ci == 8 stem); exact-fp32 / f16x2 forward with Ci % 32 != 0;
  * any data gradient whose conv has Co % 64 != 0 (the data gradient's K is Co) - the executor pads the head's Co to 64 for that reason;
  * data gradients of reflection-padded, upsampling or Ci == 8 convolutions (UDAPOSE_ERR_UNSUPPORTED: the style network's reflect
    gradients go through the padded form, the stem has no data gradient).
A refusal of a form not in this list fails the test."""
import time

import pytest
import torch

from helpers import fp64_conv as fc

pytestmark = pytest.mark.gpu

ELEM = {"bf16": torch.bfloat16, "fp16": torch.float16}
TILES = (3, 4, 5, 6, 9, 10, 11)
WORST = {}          # (kind, op) -> [tau, rho] worst measured over the module (printed at the end of each part)
STATS_WORST = [0.0]  # worst error of the fused statistics, relative to the column sums of |y| (sum) and y^2 (sum of squares)


def _note(kind, op, tr):
    w = WORST.setdefault((kind, op), [0.0, 0.0])
    w[0], w[1] = max(w[0], tr[0]), max(w[1], tr[1])


def _report(part, t0):
    print(f"\n[{part}] wall {time.time() - t0:.1f} s; worst measured (tau, rho) against the bars:")
    for (kind, op), (t, r) in sorted(WORST.items()):
        bt, br = fc.BOUNDS[(kind, op)]
        print(f"  {kind:6s} {op:6s} tau {t:.3g} (bar {bt:g})  rho {r:.3g} (bar {br:g})")
    print(f"  fused statistics: {STATS_WORST[0]:.3g} of the column sums of |y| / y^2 (bar 1e-5)")


def _ops():
    from uda_poseestimation_amd import ops, _hip
    return ops, _hip


def _refused(e):
    return "error -1" in str(e) or "error -3" in str(e)


class Failures:
    def __init__(self):
        self.items = []

    def run(self, what, fn):
        try:
            return fn()
        except (AssertionError, RuntimeError) as e:       # (RuntimeError: a library call returned an error code)
            self.items.append(f"{what}: {e}")
        return None

    def assert_none(self):
        assert not self.items, f"{len(self.items)} failing form(s):\n" + "\n".join(self.items[:40])


class Case:
    """Operands (rounded to the element type) of one geometry and their cached float64 references."""

    def __init__(self, d, dtype, seed, w_scale=None, with_dgrad=True):
        ops, _ = _ops()
        self.d, self.g, self.dtype = d, fc.geom_of(d), dtype
        g = self.g
        gen = torch.Generator(device="cuda").manual_seed(seed)
        cin = 3 if g.Ci == 8 else g.Ci
        wshape = (g.Ci, g.Co, g.KH, g.KW) if g.transposed else (g.Co, cin, g.KH, g.KW)
        fan = (g.Co if g.transposed else cin) * g.KH * g.KW
        self.w = (torch.randn(wshape, device="cuda", generator=gen) * (w_scale or fan ** -0.5)).to(dtype).float()
        x = torch.randn(g.N, g.Hi, g.Wi, g.Ci, device="cuda", generator=gen)
        if g.Ci == 8:
            x[..., 3:] = 0
        self.x = x.to(dtype)
        self.dy = torch.randn(g.N, g.Ho, g.Wo, g.Co, device="cuda", generator=gen).to(dtype)
        self.wp = fc.phys_weight(self.w, g)
        self.wf = ops.pack_weight(self.w, d, "fwd", dtype=dtype)
        self.wb = ops.pack_weight(self.w, d, "bwd", dtype=dtype) if with_dgrad and g.Ci != 8 else None
        self._ref = {}

    def ref(self, op):
        if op not in self._ref:
            if op == "fprop":
                self._ref[op] = fc.fprop(self.g, self.x, self.wp)
            elif op == "dgrad":
                self._ref[op] = fc.dgrad(self.g, self.dy, self.wp)
            else:
                self._ref[op] = fc.wgrad(self.g, self.dy, self.x)
        return self._ref[op]

    def bn_operands(self, seed):
        g = self.g
        gen = torch.Generator(device="cuda").manual_seed(seed)
        bn_y = (torch.randn(g.N, g.Hi, g.Wi, g.Ci, device="cuda", generator=gen) * 1.5 + 0.3).to(self.dtype)
        mean = torch.randn(g.Ci, device="cuda", generator=gen) * 0.2 + 0.3
        invstd = torch.rand(g.Ci, device="cuda", generator=gen) * 0.5 + 0.4
        gamma = torch.rand(g.Ci, device="cuda", generator=gen) + 0.5
        beta = torch.randn(g.Ci, device="cuda", generator=gen) * 0.3
        return bn_y, mean, invstd, gamma, beta


def _check_stats(stats, y, what):
    """Fused statistics = column sums (sum, sum of squares) of the kernel's own stored fp32 output: fp32 partials per m-tile."""
    s = stats.double().sum(0)
    yd = y.double().reshape(-1, y.shape[-1])
    for k, (want, mag) in enumerate(((yd.sum(0), yd.abs().sum(0)), ((yd * yd).sum(0), (yd * yd).sum(0)))):
        err = float(((s[k] - want).abs() / (mag + 1e-30)).max())
        STATS_WORST[0] = max(STATS_WORST[0], err)
        assert err <= 1e-5, f"{what}: statistics row {k} off by {err:.3g} of sum|.| (bar 1e-5)"
    return err


def _check_bn_epilogue(gq, slab, dx0, bn, what):
    """The BN-backward epilogue: g = dz * mask bit for bit where the mask is certain, slab column sums = sums of the stored g."""
    bn_y, mean, invstd, gamma, beta = bn
    sc = gamma * invstd
    t = bn_y.double() * sc.double() + (beta - mean * sc).double()
    keep = t > 0
    sure = t.abs() > 1e-5 * (bn_y.double().abs() * sc.double().abs() + 1.0)
    want = torch.where(keep, dx0, torch.zeros_like(dx0))
    assert torch.equal(gq[sure], want[sure]), f"{what}: masked output differs from mask * plain data gradient"
    xhat = (bn_y.double() - mean.double()) * invstd.double()
    gd = gq.double()
    got = slab.double().sum(0)
    for k, (s_, a_) in enumerate(((gd.sum((0, 1, 2)), gd.abs().sum((0, 1, 2))), ((gd * xhat).sum((0, 1, 2)), (gd * xhat).abs().sum((0, 1, 2))))):
        err = float(((got[k] - s_).abs() / (a_ + 1e-30)).max())
        assert err < 2e-6, f"{what}: BN slab row {k} off by {err:.3g} (bar 2e-6)"


def _igemm_16bit(case, pol, fail, what, outs=None, dgrad=True, epilogues=True):
    """fprop (+ stats, + epilogues), data gradient (plain, fp32 out, BN epilogue) of one 16-bit case under one policy."""
    ops, _hip = _ops()
    d = ops.with_policy(case.d, _hip.policy(**pol))
    dt = case.dtype
    kind = "16bit"
    f32_out = case.g.Co % 8 != 0           # (16-bit outputs need whole 8-channel groups: the K = 18 head stores fp32)
    try:
        y, stats = ops.conv2d_fwd(case.x, case.wf, d, want_stats=True, out_f32=f32_out)
    except RuntimeError as e:
        fail.items.append(f"{what}: forward refused: {e}")
        return
    ref, absref = case.ref("fprop")
    ydt = torch.float32 if f32_out else dt
    tr = fail.run(what + " fprop", lambda: fc.check(y, ref, absref, ydt, *fc.BOUNDS[(kind, "fprop")], what + " fprop"))
    if tr:
        _note(kind, "fprop", tr)
    if outs is not None:
        outs["fprop"] = (y, stats)
    if epilogues:
        yf, st = ops.conv2d_fwd(case.x, case.wf, d, out_f32=True, want_stats=True)
        tr = fail.run(what + " fprop f32-out", lambda: fc.check(yf, ref, absref, torch.float32, *fc.BOUNDS[(kind, "fprop")], what + " fprop f32-out"))
        if tr:
            _note(kind, "fprop", tr)
        fail.run(what + " stats", lambda: _check_stats(st, yf, what + " stats"))
        gen = torch.Generator(device="cuda").manual_seed(5)
        bias = torch.randn(case.g.Co, device="cuda", generator=gen)
        if case.g.Co % 8 == 0:
            res = torch.randn(ref.shape, device="cuda", generator=gen).to(dt)
            ye = ops.conv2d_fwd(case.x, case.wf, d, res=res, bias=bias, relu=True)
            r_e = torch.relu(ref + bias.double() + res.double())
            a_e = absref + bias.double().abs() + res.double().abs()
            tr = fail.run(what + " fprop res+bias+relu", lambda: fc.check(ye, r_e, a_e, dt, *fc.BOUNDS[(kind, "fprop")], what + " fprop res+bias+relu"))
            if tr:
                _note(kind, "fprop", tr)
        yb = ops.conv2d_fwd(case.x, case.wf, d, bias=bias, out_f32=True)
        tr = fail.run(what + " fprop bias f32-out", lambda: fc.check(yb, ref + bias.double(), absref + bias.double().abs(), torch.float32,
                                                                      *fc.BOUNDS[(kind, "fprop")], what + " fprop bias f32-out"))
        if tr:
            _note(kind, "fprop", tr)
    if not dgrad:
        return
    dref, dabs = case.ref("dgrad")
    dx = ops.conv2d_bwd_data(case.dy, case.wb, d)
    tr = fail.run(what + " dgrad", lambda: fc.check(dx, dref, dabs, dt, *fc.BOUNDS[(kind, "dgrad")], what + " dgrad"))
    if tr:
        _note(kind, "dgrad", tr)
    if epilogues:
        dxf = ops.conv2d_bwd_data(case.dy, case.wb, d, out_f32=True)
        tr = fail.run(what + " dgrad f32-out", lambda: fc.check(dxf, dref, dabs, torch.float32, *fc.BOUNDS[(kind, "dgrad")], what + " dgrad f32-out"))
        if tr:
            _note(kind, "dgrad", tr)
    bn = case.bn_operands(9)
    gq, slab = ops.conv2d_bwd_data_bn(case.dy, case.wb, d, bn[0], bn[1], bn[2], bn_gamma=bn[3], bn_beta=bn[4])
    fail.run(what + " dgrad+bn", lambda: _check_bn_epilogue(gq, slab, dx, bn, what + " dgrad+bn"))
    if outs is not None:
        outs["dgrad"] = dx
        outs["dgrad_bn"] = (gq, slab)


def _igemm_fp32(case, pol, fail, what, split):
    """Exact-fp32 (split=False) or f16x2 (split=True) forward of a case's fp32 operands (x, w unrounded): fp32 and split outputs."""
    ops, _hip = _ops()
    d = ops.with_policy(case.d, _hip.policy(**pol))
    g = case.g
    kind = "split" if split else "f32"
    wf = case.wp.float() if not g.transposed else case.wp.float().permute(2, 1, 0).contiguous()
    x, w = case.xf, wf
    if split:
        x, w = ops.f32_to_split(x), ops.f32_to_split(w)
    ref, absref = case.ref32
    y, stats = ops.conv2d_fwd(x, w, d, out_f32=True, want_stats=True)
    tr = fail.run(what, lambda: fc.check(y, ref, absref, torch.float32, *fc.BOUNDS[(kind, "fprop")], what))
    if tr:
        _note(kind, "fprop", tr)
    fail.run(what + " stats", lambda: _check_stats(stats, y, what + " stats"))
    if split and g.Co % 8 == 0:
        ys = ops.split_to_f32(ops.conv2d_fwd(x, w, d))
        tr = fail.run(what + " split-out", lambda: fc.check(ys, ref, absref, torch.float32, *fc.BOUNDS[(kind, "fprop")], what + " split-out"))
        if tr:
            _note(kind, "fprop", tr)
    return y


def _with_fp32_operands(case, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    g = case.g
    case.xf = torch.randn(g.N, g.Hi, g.Wi, g.Ci, device="cuda", generator=gen)
    if g.Ci == 8:
        case.xf[..., 3:] = 0
    case.ref32 = fc.fprop(g, case.xf, case.wp)       # case.wp: the (16-bit-representable) weight in fp64; the fp32 paths take it as is


# ---- (A) forced forms at small, ragged shapes ------------------------------------------------------------------------------------

IGEMM_SHAPES = [
    # name, N, H, W, Ci, Co, K, stride, pad, transposed, reflect, upsample
    ("1x1_s1_odd_m315", 1, 15, 21, 64, 128, 1, 1, 0, False, False, False),
    ("1x1_s1_co96", 2, 9, 11, 128, 96, 1, 1, 0, False, False, False),
    ("1x1_s2_odd", 2, 13, 9, 128, 192, 1, 2, 0, False, False, False),
    ("1x1_co16_head", 2, 10, 7, 256, 16, 1, 1, 0, False, False, False),
    ("1x1_co24", 1, 9, 9, 64, 24, 1, 1, 0, False, False, False),
    ("1x1_co32", 1, 9, 9, 64, 32, 1, 1, 0, False, False, False),
    ("3x3_w12", 2, 12, 12, 64, 64, 3, 1, 1, False, False, False),
    ("3x3_w24", 1, 10, 24, 64, 128, 3, 1, 1, False, False, False),
    ("3x3_w40", 1, 7, 40, 128, 64, 3, 1, 1, False, False, False),
    ("3x3_w64", 1, 5, 64, 64, 64, 3, 1, 1, False, False, False),
    ("3x3_s2_15x9", 2, 15, 9, 128, 128, 3, 2, 1, False, False, False),
    ("deconv4x4_s2_5x7", 2, 5, 7, 128, 64, 4, 2, 1, True, False, False),
    ("stem7x7_s2", 2, 23, 17, 8, 64, 7, 2, 3, False, False, False),
    ("K_one_stage_1x1_c64", 2, 11, 13, 64, 64, 1, 1, 0, False, False, False),
    ("K_over_one_stage_1x1_c128", 2, 11, 13, 128, 64, 1, 1, 0, False, False, False),
    ("K2048_1x1", 1, 9, 14, 2048, 64, 1, 1, 0, False, False, False),
    ("K2304_3x3", 1, 6, 7, 256, 128, 3, 1, 1, False, False, False),
    ("reflect_3x3", 1, 9, 13, 64, 64, 3, 1, 1, False, True, False),
    ("upsample_reflect_3x3", 1, 5, 7, 64, 64, 3, 1, 1, False, True, True),
]


def _variants():
    v = [(f"tile{t}", {"igemm_tile": t}) for t in TILES]
    v += [(f"tile{t}_lean0_short0_tap0", {"igemm_tile": t, "igemm_lean": 0, "igemm_short_lds": 0, "igemm_tap0": 0}) for t in TILES]
    v += [("default", {}), ("lean0", {"igemm_lean": 0}), ("short_lds0", {"igemm_short_lds": 0}), ("tap0_0", {"igemm_tap0": 0}),
          ("ns3_k64", {"igemm_ns3_k": 64}), ("h3_off", {"igemm_h3": 0})]
    return v


@pytest.fixture(scope="module", autouse=True)
def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from uda_poseestimation_amd import _hip
    _hip.lib("bf16"), _hip.lib("fp16")
    yield


def test_igemm_forms_against_fp64():
    """Part A, implicit GEMM: every geometry of IGEMM_SHAPES under every variant of _variants(), both 16-bit builds, and the exact-fp32 and
    f16x2 forwards under every tile id.  Failures are collected over the whole matrix and reported together."""
    ops, _hip = _ops()
    t0 = time.time()
    fail = Failures()
    refusals = set()
    for name, N, H, W, Ci, Co, K, s, p, tr, refl, up in IGEMM_SHAPES:
        d = ops.conv_desc(N, H, W, Ci, Co, K, s, p, transposed=tr, reflect=refl, upsample=up, policy=_hip.policy(patch_conv=0))
        dgrad_ok = Co % 64 == 0 and not (refl or up or Ci == 8)
        for build, dt in ELEM.items():
            case = Case(d, dt, seed=len(name) * 7 + Co)
            for vname, pol in _variants():
                pol = dict(pol, patch_conv=0)
                fail.run(f"{name} {build} {vname}", lambda: _igemm_16bit(case, pol, fail, f"{name} {build} {vname}", dgrad=dgrad_ok))
            if not dgrad_ok:
                # a refused data gradient returns an error code
                try:
                    ops.conv2d_bwd_data(case.dy, case.wb if case.wb is not None else case.wf, d)
                    fail.items.append(f"{name} {build}: data gradient with Co % 64 != 0 / reflect / stem was not refused")
                except RuntimeError as e:
                    assert _refused(e), e
                    refusals.add(f"{name}: data gradient")
            if build == "bf16" and (Ci % 32 == 0 or Ci == 8):
                _with_fp32_operands(case, 3)
                for split in (False, True):
                    for t in TILES[:5]:
                        what = f"{name} {'split' if split else 'f32'} tile{t}"
                        fail.run(what, lambda: _igemm_fp32(case, {"igemm_tile": t, "patch_conv": 0}, fail, what, split))
                    what = f"{name} {'split' if split else 'f32'} default"
                    fail.run(what, lambda: _igemm_fp32(case, {"patch_conv": 0}, fail, what, split))
            del case
        torch.cuda.empty_cache()
    _report("A igemm", t0)
    print("  refusals seen: " + "; ".join(sorted(refusals)))
    fail.assert_none()


WGRAD_SHAPES = [
    # name, N, H, W, Ci, Co, K, stride, pad, transposed
    ("3x3_dma_pow2", 2, 16, 16, 128, 128, 3, 1, 1, False),
    ("3x3_dma_w8_m64", 1, 8, 8, 64, 64, 3, 1, 1, False),
    ("3x3_non_dma_ci96_co40", 2, 9, 11, 96, 40, 3, 1, 1, False),
    ("1x1_dma_m_ragged", 3, 7, 9, 64, 192, 1, 1, 0, False),
    ("1x1_dma_pow2_m_not64", 1, 4, 8, 256, 128, 1, 1, 0, False),
    ("3x3_s2_odd", 2, 15, 9, 128, 64, 3, 2, 1, False),
    ("1x1_s2", 2, 14, 10, 64, 128, 1, 2, 0, False),
    ("3x3_non_pow2_24", 2, 24, 24, 64, 64, 3, 1, 1, False),
    ("deconv4x4_s2", 2, 5, 7, 128, 64, 4, 2, 1, True),
    ("deconv4x4_s2_non_dma", 2, 6, 5, 96, 48, 4, 2, 1, True),
    ("stem7x7_s2", 2, 23, 17, 8, 64, 7, 2, 3, False),
    ("head_co32", 2, 8, 8, 256, 32, 1, 1, 0, False),
]


def _wgrad_variants(stem):
    if stem:
        return [("default", {}), ("ksplit1", {"wgrad_ksplit": 1}), ("ksplit3", {"wgrad_ksplit": 3}), ("ksplit4", {"wgrad_ksplit": 4})]
    v = [("default", {})]
    for t in (-1, 0, 1, 2, 3):
        for ks in (-1, 1, 3, 4):
            v.append((f"tile{t}_ks{ks}", {"wgrad_tile": t, "wgrad_ksplit": ks}))
    for fg in (0, 1, 2):
        for r3 in (0, 1):
            for ks in (1, 4):
                v.append((f"fastgeo{fg}_row3{r3}_ks{ks}", {"wgrad_fastgeo": fg, "wgrad_row3": r3, "wgrad_ksplit": ks}))
    for fg in (0, 1, 2):
        for t in (0, 1):
            v.append((f"fastgeo{fg}_tile{t}_ks1", {"wgrad_fastgeo": fg, "wgrad_tile": t, "wgrad_ksplit": 1}))
    return v


def test_wgrad_forms_against_fp64():
    """Part A, weight gradients: every tile id and split count, the three loaders and the filter-row form, DMA and non-DMA channel
    counts, ragged and non-power-of-two maps, transposed, the stem, accumulation.  The three loaders of one tile at one split run the same
    MFMAs on the same LDS contents: identical bits."""
    ops, _hip = _ops()
    t0 = time.time()
    fail = Failures()
    for name, N, H, W, Ci, Co, K, s, p, tr in WGRAD_SHAPES:
        for build, dt in ELEM.items():
            d = ops.conv_desc(N, H, W, Ci, Co, K, s, p, transposed=tr)
            case = Case(d, dt, seed=len(name) + Ci, with_dgrad=False)
            ref, absref = case.ref("wgrad")
            outs = {}
            for vname, pol in _wgrad_variants(Ci == 8):
                dd = ops.with_policy(d, _hip.policy(**pol))
                what = f"{name} {build} {vname}"
                dw = fail.run(what, lambda: ops.conv2d_bwd_weight(case.dy, case.x, dd))
                if dw is None:
                    continue
                outs[vname] = dw
                tr_ = fail.run(what, lambda: fc.check(dw, ref, absref, torch.float32, *fc.BOUNDS[("16bit", "wgrad")], what, bm=(64, 128), bn=64))
                if tr_:
                    _note("16bit", "wgrad", tr_)
            # accumulate: dw += wgrad (default form and a split one)
            for vname in ("default", "ksplit4" if Ci == 8 else "tile-1_ks4"):
                dd = ops.with_policy(d, _hip.policy(**dict(_wgrad_variants(Ci == 8))[vname]))
                what = f"{name} {build} {vname} accumulate"
                acc = fail.run(what, lambda: ops.conv2d_bwd_weight(case.dy, case.x, dd, dw=outs[vname].clone()))
                if acc is None:
                    continue
                tr_ = fail.run(what, lambda: fc.check(acc, 2 * ref, 2 * absref, torch.float32, *fc.BOUNDS[("16bit", "wgrad")], what))
                if tr_:
                    _note("16bit", "wgrad", tr_)
            if Ci != 8:
                for t in (0, 1):
                    a = outs.get(f"fastgeo0_tile{t}_ks1")
                    for fg in (1, 2):
                        b = outs.get(f"fastgeo{fg}_tile{t}_ks1")
                        if a is not None and b is not None and not torch.equal(a, b):
                            fail.items.append(f"{name} {build}: loader fastgeo {fg} differs in bits from fastgeo 0 (tile {t}, one split)")
            del case, outs
    _report("A wgrad", t0)
    fail.assert_none()


# ---- (B) the benchmarked geometries ---------------------------------------------------------------------------------------------

def _poseresnet101_convs(N, S, K):
    """Every distinct convolution of PoseResNet-101 at N x S x S: (name, N, H, W, Ci, Co, k, stride, pad, transposed)."""
    out = [("stem", N, S, S, 8, 64, 7, 2, 3, False)]
    H = S // 4
    inpl = 64
    for li, (planes, stride) in enumerate(((64, 1), (128, 2), (256, 2), (512, 2)), 1):
        out.append((f"l{li}.c1_first", N, H, H, inpl, planes, 1, 1, 0, False))
        out.append((f"l{li}.c2_first", N, H, H, planes, planes, 3, stride, 1, False))
        Ho = H // stride
        out.append((f"l{li}.c3", N, Ho, Ho, planes, planes * 4, 1, 1, 0, False))
        out.append((f"l{li}.ds", N, H, H, inpl, planes * 4, 1, stride, 0, False))
        if stride == 2 or inpl != planes * 4:
            out.append((f"l{li}.c1", N, Ho, Ho, planes * 4, planes, 1, 1, 0, False))
        if stride == 2:
            out.append((f"l{li}.c2", N, Ho, Ho, planes, planes, 3, 1, 1, False))
        H, inpl = Ho, planes * 4
    for i in range(3):
        out.append((f"deconv{i + 1}", N, H, H, inpl, 256, 4, 2, 1, True))
        H, inpl = H * 2, 256
    out.append(("head", N, H, H, 256, K, 1, 1, 0, False))
    seen, uniq = set(), []
    for c in out:
        if c[1:] not in seen:          # (l1.ds = l1.c3's geometry with Ci = 64: kept once)
            seen.add(c[1:])
            uniq.append(c)
    return uniq


def _bench_geometries(N, S, K, build, fail, matched, t0, with_fp32):
    ops, _hip = _ops()
    dt = ELEM[build]
    for name, n, H, W, Ci, Co, k, s, p, tr in _poseresnet101_convs(N, S, K):
        head = name == "head"
        d = ops.conv_desc(n, H, W, Ci, Co, k, s, p, transposed=tr)
        case = Case(d, dt, seed=sum(map(ord, name)))
        dgrad_ok = not (Ci == 8)
        label = f"{build} N{N} {S} {name}"
        outs = {}
        fail.run(label + " default", lambda: _igemm_16bit(case, {}, fail, label + " default", outs=outs, dgrad=dgrad_ok and not head, epilogues=False))
        forms = {}
        h3 = k == 3 and s == 1 and Ci % 64 == 0 and Co % 64 == 0 and W <= 64
        for t in TILES:
            if t in (10, 11) and not (h3 and (t == 10 or W <= 32)):
                continue
            if Co <= 32 and t != 3:
                continue
            o = {}
            fail.run(label + f" tile{t}", lambda: _igemm_16bit(case, {"igemm_tile": t}, fail, label + f" tile{t}", outs=o, dgrad=dgrad_ok and not head,
                                                                epilogues=False))
            forms[t] = o
        for key in outs:
            same = [t for t, o in forms.items() if key in o and _same(outs[key], o[key])]
            if not same:
                fail.items.append(f"{label}: default {key} matches no forced tile form bit for bit")
            matched.setdefault(label, {})[key] = same
        del forms, outs
        if head:
            # the head's data gradient as the executor runs it: dy channel-padded to 64, fp32 output; its weight gradient on the padded dy
            dh = ops.conv_desc(n, H, W, Ci, 64, 1)
            hc = Case(dh, dt, seed=77)
            hc.dy[..., K:] = 0
            hc.w[K:] = 0
            hc.wp = fc.phys_weight(hc.w, hc.g)
            hc.wb = ops.pack_weight(hc.w, dh, "bwd", dtype=dt)
            dref, dabs = hc.ref("dgrad")
            tr_ = fail.run(label + " dgrad (Co padded to 64, fp32 out)", lambda: fc.check(ops.conv2d_bwd_data(hc.dy, hc.wb, dh, out_f32=True), dref, dabs,
                                                                                          torch.float32, *fc.BOUNDS[("16bit", "dgrad")], label + " dgrad"))
            if tr_:
                _note("16bit", "dgrad", tr_)
            case = hc
        ref, absref = case.ref("wgrad")
        tr_ = fail.run(label + " wgrad", lambda: fc.check(ops.conv2d_bwd_weight(case.dy, case.x, case.d), ref, absref, torch.float32, *fc.BOUNDS[("16bit", "wgrad")], label + " wgrad"))
        if tr_:
            _note("16bit", "wgrad", tr_)
        if with_fp32 and not head:
            _with_fp32_operands(case, 4)
            for split in (False, True):
                what = f"{label} {'split' if split else 'f32'}"
                fail.run(what, lambda: _igemm_fp32(case, {}, fail, what, split))
        del case, ref, absref
        torch.cuda.empty_cache()
        print(f"  {label}: done at {time.time() - t0:.1f} s; default matched tiles {matched.get(label)}")


def _same(a, b):
    if isinstance(a, tuple):
        return all(torch.equal(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


@pytest.mark.parametrize("cfg", [(32, 256, 16, "bf16", True), (8, 384, 18, "fp16", False)], ids=["config1_n32_256_bf16", "config4_n8_384_fp16"])
def test_benchmarked_geometries_against_fp64(cfg):
    """Part B: every distinct convolution of the benchmarked network, default policy and every eligible tile form, against fp64; the
    default output equals one forced form's output bit for bit; the per-layer weight gradient (default split) against fp64; at configs[1]
    also the exact-fp32 and f16x2 forwards (the teacher's, validate()'s and 'strict''s forward)."""
    N, S, K, build, with_fp32 = cfg
    t0 = time.time()
    fail, matched = Failures(), {}
    _bench_geometries(N, S, K, build, fail, matched, t0, with_fp32)
    _report(f"B {build} N={N} {S}x{S}", t0)
    fail.assert_none()


# ---- (C) grouped weight gradients at bench size ----------------------------------------------------------------------------------

def test_grouped_weight_gradients_equal_per_layer_launches_at_bench_size():
    """Part C: PoseResNet-101, K = 16, N = 32, 256x256, bf16: the grouped weight-gradient launches (default policy: deterministic split
    partials, real split counts) against layer-by-layer launches (wgrad_group 0) on the same input and the same output gradient, per
    parameter tensor: the bound of tests/test_gpu_net.py::test_grouped_weight_gradients_equal_per_layer_launches and a relative L2 bound."""
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    t0 = time.time()
    torch.manual_seed(0)
    net = pr._pose_resnet("conv_forms", 16, pr.Bottleneck_default, [3, 4, 23, 3], False, False).cuda()
    net.precision = "bf16"
    x = torch.randn(32, 3, 256, 256, generator=torch.Generator().manual_seed(2)).cuda()
    R = torch.randn(32, 16, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    grads = {}
    for mode, pol in ((0, {"wgrad_group": 0}), (1, {})):
        net.policy, net._handles = pol, {}
        net.zero_grad(set_to_none=True)
        (net(x) * R).sum().backward()
        torch.cuda.synchronize()
        grads[mode] = {n_: p_.grad.clone() for n_, p_ in net.named_parameters() if p_.grad is not None}
        net._handles = {}
        torch.cuda.empty_cache()
    assert len(grads[0]) == len(grads[1]) >= 300
    worst_el, worst_l2 = 0.0, 0.0
    bad = []
    for n_ in grads[0]:
        a, b = grads[1][n_], grads[0][n_]
        el = float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)
        l2 = float((a - b).double().norm() / (b.double().norm() + 1e-30))
        worst_el, worst_l2 = max(worst_el, el), max(worst_l2, l2)
        if not float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()) + 1e-7 or l2 > 1e-5:
            bad.append(f"{n_}: max {el:.3g} of max|g|, rel-L2 {l2:.3g}")
    print(f"\n[C] wall {time.time() - t0:.1f} s; {len(grads[0])} parameter tensors: worst max|grouped - per-layer| {worst_el:.3g} of max|g| "
          f"(bar 2e-5), worst relative L2 {worst_l2:.3g} (bar 1e-5)")
    assert not bad, "\n".join(bad[:20])
