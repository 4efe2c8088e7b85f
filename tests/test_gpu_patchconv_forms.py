"""Every patch-staged convolution form (csrc/patchconv.hip) against the float64 reference, element by element (tests/helpers/fp64_conv.py:
check(), the bars of BOUNDS - the implicit GEMM's, not derived from these kernels), in the bf16 and fp16 builds and in the f16x2 split form.

(A) Forced forms at the smallest shapes that can go wrong: patch3x3_co16_kernel (Ci = 64, Co in 1 / 3 / 13 / 16, fp32 output: one tile whose
    patch reflects at all four borders, tile seams, tile counts with and without an XCD remainder), patch3x3_ci8_kernel (3 of 8 input channels
    -> 64: one tile; 780 and 1560 tiles, so that the persistent work-groups run a second, a third and - split form - a fourth round, with and
    without the prefetch of the next patch), patch3x3_kernel in its six instantiations (split or not x 4 x 32 / 2 x 64 tile x 64 / 128 output
    channels per work-group), each without and with the folded x2 upsample, 8 / 16 channel slices at Ci = 512; and one geometry per refusal of
    patch_conv_ok / patch_trunk_ok a caller can reach, which must take the implicit GEMM (bit-identical to patch_conv = 0).
(B) Every distinct convolution of Style_net's encoder (to relu4_1) and decoder, derived from the modules, at N = 1 / 256 x 256 and
    N = 2 / 128 x 128 under Style_net._SeqRunner.policy_overrides, with bias / ReLU / the fp32 last layer / the folded upsample as the executor
    applies them.

Every image of a batch has its own seed (a stale or foreign patch fails per element).  Outputs live in 0xFF-filled guarded buffers
(helpers.gpu_forms.Guards): an element never written comes back NaN, a write outside the output damages a guard.  Each case also runs the
implicit GEMM (patch_conv = 0) on the same operands, which must pass the same bars; the number of elements whose bits differ between the two
is printed, not asserted.  The CPU twin that shows check() catching these kernels' faults is tests/test_conv_bounds_cpu.py
(test_patch_kernel_faults_fail_the_check).  The library has no query for the form a call took: profiles/patchconv_forms.txt lists the
kernels this module launched in one traced run (all ten instantiations), with call counts."""
import ctypes as C
import time

import pytest
import torch

from helpers import fp64_conv as fc
from helpers.gpu_forms import Failures, Guards

pytestmark = pytest.mark.gpu

ELEM = {"bf16": torch.bfloat16, "fp16": torch.float16}
KINDS = ("bf16", "fp16", "split")
ALL_EPILOGUES = ((False, False), (True, False), (False, True), (True, True))      # (bias, relu)
BIAS_RELU = ((True, True),)


def _ops():
    from uda_poseestimation_amd import ops, _hip
    return ops, _hip


def _bars(kind):
    return fc.BOUNDS[("split" if kind == "split" else "16bit", "fprop")]


class Report:
    """Worst measured (tau, rho) per (kind, form family) and the count of elements whose bits differ from the implicit GEMM's."""

    def __init__(self):
        self.worst, self.diff, self.t0 = {}, {}, time.time()

    def note(self, kind, family, tr):
        w = self.worst.setdefault((kind, family), [0.0, 0.0])
        w[0], w[1] = max(w[0], tr[0]), max(w[1], tr[1])

    def note_diff(self, kind, family, n, total):
        d = self.diff.setdefault((kind, family), [0, 0])
        d[0], d[1] = d[0] + n, d[1] + total

    def print(self, part):
        print(f"\n[{part}] wall {time.time() - self.t0:.1f} s; worst measured (tau, rho) against the bars:")
        for (kind, family), (t, r) in sorted(self.worst.items()):
            bt, br = _bars(kind)
            n, total = self.diff.get((kind, family), (0, 0))
            tail = f"  {n} of {total} elements differ in bits from the igemm's" if family != "igemm" else ""
            print(f"  {kind:5s} {family:8s} tau {t:.3g} (bar {bt:g})  rho {r:.3g} (bar {br:g}){tail}")


def _conv(x, w, d, out_f32, bias, relu, res=None):
    """udapose_conv2d_fwd with the output inside a 0xFF-filled guarded allocation (ops.conv2d_fwd allocates its own): -> (y, guards)."""
    ops, _hip = _ops()
    ho, wo = ops.conv_out_hw(d)
    G = Guards()
    y = G.new((d.N, ho, wo, d.Co), torch.float32 if out_f32 else x.dtype, wo * d.Co)
    flags = (ops.EPI_RELU if relu else 0) | (ops.EPI_OUT_F32 if out_f32 else 0) | (ops.EPI_SPLIT if x.dtype == ops.SPLIT else 0)
    _hip.check(_hip.lib_for(x).udapose_conv2d_fwd(_hip.stream(), C.byref(d), _hip.ptr(x), _hip.ptr(w), _hip.ptr(y), _hip.ptr(res), _hip.ptr(bias),
                                                  None, flags), "conv2d_fwd")
    return y, G


class Operands:
    """The operands of one reflection-padded 3x3 geometry exactly as the kernel sees them - 16-bit: rounded to the element type; split: the
    fp32 values (weights included: both operands have an l part) - and their float64 reference.  Every image has a seed of its own."""

    def __init__(self, kind, N, Hi, Wi, Ci, Co, up, seed):
        ops, _ = _ops()
        self.kind = kind
        self.g = g = fc.Geom(N, Hi, Wi, Ci, Co, 3, 3, 1, 1, False, True, up)
        cin = 3 if Ci == 8 else Ci
        gen = torch.Generator(device="cuda").manual_seed(seed)
        w = torch.randn(Co, cin, 3, 3, device="cuda", generator=gen) * (cin * 9) ** -0.5
        self.bias = torch.randn(Co, device="cuda", generator=gen)
        x = torch.empty(N, Hi, Wi, Ci, device="cuda")
        for n in range(N):
            x[n] = torch.randn(Hi, Wi, Ci, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed * 4096 + n + 1))
        if Ci == 8:
            x[..., 3:] = 0
        if kind == "split":
            self.wp = fc.phys_weight(w, g)
            self.x, self.w = ops.f32_to_split(x), ops.f32_to_split(self.wp.float().contiguous())
            xr = x
        else:
            dt = ELEM[kind]
            w = w.to(dt).float()
            self.wp = fc.phys_weight(w, g)
            self.x = xr = x.to(dt)
            self.w = ops.pack_weight(w, ops.conv_desc(N, Hi, Wi, Ci, Co, 3, 1, 1, reflect=True, upsample=up), "fwd", dtype=dt)
        self.ref, self.absref = fc.fprop(g, xr, self.wp)

    def residual(self):
        """(the residual as the kernel reads it, its values in float64)"""
        ops, _ = _ops()
        g = self.g
        res = torch.randn(g.N, g.Ho, g.Wo, g.Co, device="cuda", generator=torch.Generator(device="cuda").manual_seed(g.Ho + g.Co))
        if self.kind == "split":
            res = ops.f32_to_split(res)
            return res, ops.split_to_f32(res).double()
        res = res.to(ELEM[self.kind])
        return res, res.double()


def _family(g, out_f32, res, pol):
    """The kernel family patch_conv_ok / patch_trunk_ok (csrc/patchconv.hip) route this call to: a label for the report."""
    pc = pol.get("patch_conv", 2)
    Ho, Wo = g.Ho, g.Wo
    if res or not pc:
        return "igemm"
    if pc >= 2 and not out_f32 and g.Ci >= 64 and g.Ci % 64 == 0 and g.Co % 64 == 0 and Wo % 32 == 0 and Ho >= 2 and Ho % 2 == 0 and \
            (Ho % 4 == 0 or Wo % 64 == 0):
        return "trunk"
    if g.upsample or g.Wi % 64 or g.Hi % 4:
        return "igemm"
    if g.Ci == 64 and g.Co <= 16 and out_f32:
        return "co16"
    if g.Ci == 8 and g.Co == 64 and not out_f32:
        return "ci8"
    return "igemm"


def _run(op, pol, rep, fail, what, out_f32=False, epilogues=ALL_EPILOGUES, with_res=False, expect=None):
    """One geometry under policy `pol` and under the same policy with patch_conv = 0, per epilogue: both against fp64 at the same bars,
    guards untouched; expect: the family the call must be routed to by the rules of patch_conv_ok (a check of the case list itself)."""
    ops, _hip = _ops()
    g, kind = op.g, op.kind
    family = _family(g, out_f32, with_res, pol)
    assert expect is None or family == expect, f"{what}: the case list expects the {expect} form, the dispatch rules give {family}"
    descs = [(family, ops.conv_desc(g.N, g.Hi, g.Wi, g.Ci, g.Co, 3, 1, 1, reflect=True, upsample=g.upsample, policy=_hip.policy(**pol))),
             ("igemm", ops.conv_desc(g.N, g.Hi, g.Wi, g.Ci, g.Co, 3, 1, 1, reflect=True, upsample=g.upsample,
                                     policy=_hip.policy(**dict(pol, patch_conv=0))))]
    odt = torch.float32 if (out_f32 or kind == "split") else ELEM[kind]
    res, res64 = op.residual() if with_res else (None, None)
    for with_bias, relu in epilogues:
        ref, absref = op.ref, op.absref
        if with_bias:
            ref, absref = ref + op.bias.double(), absref + op.bias.double().abs()
        if with_res:
            ref, absref = ref + res64, absref + res64.abs()
        if relu:
            ref = torch.relu(ref)
        outs = []
        for fam, d in descs:
            label = f"{what} {kind} bias{int(with_bias)} relu{int(relu)} [{fam}]"

            def one():
                y, G = _conv(op.x, op.w, d, out_f32, op.bias if with_bias else None, relu, res)
                yf = ops.split_to_f32(y) if y.dtype == ops.SPLIT else y
                try:
                    rep.note(kind, fam, fc.check(yf, ref, absref, odt, *_bars(kind), label))
                finally:
                    G.check(label)
                return yf
            outs.append(fail.run(label, one))
        if outs[0] is not None and outs[1] is not None:
            n = int((outs[0] != outs[1]).sum())
            rep.note_diff(kind, family, n, outs[0].numel())
            print(f"  {what} {kind} bias{int(with_bias)} relu{int(relu)}: {n} of {outs[0].numel()} elements differ in bits between [{family}] and the igemm")
            if family == "igemm" and n:
                fail.items.append(f"{what} {kind}: a call the patch kernels refuse differs from patch_conv = 0 in {n} elements")


@pytest.fixture(scope="module", autouse=True)
def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from uda_poseestimation_amd import _hip
    _hip.lib("bf16"), _hip.lib("fp16")
    yield
    torch.cuda.empty_cache()


# ---- (A) forced forms ----------------------------------------------------------------------------------------------------------------

CO16_SHAPES = [
    # name, N, H, W: tiles of 4 x 64 output pixels
    ("single_tile", 1, 4, 64),             # rows -1 and 4, columns -1 and 64 reflect inside the one patch
    ("12_tiles", 3, 8, 128),               # seams in both directions, 12 % 8 = 4: XCD remainder
    ("6_tiles", 2, 12, 64),                # fewer tiles than XCDs
]


def test_co16_forms_against_fp64():
    """patch3x3_co16_kernel<0 | 1, 4>: Ci = 64, fp32 output, Co = 1, 3, 13, 16 (lanes with co >= Co feed zeros and store nothing; the guards
    catch a store at a wrong channel stride), every epilogue."""
    rep, fail = Report(), Failures()
    for name, N, H, W in CO16_SHAPES:
        for Co in (1, 3, 13, 16):
            for kind in KINDS:
                op = Operands(kind, N, H, W, 64, Co, False, seed=H * 31 + W + Co)
                _run(op, {}, rep, fail, f"co16 {name} Co{Co}", out_f32=True, expect="co16")
                del op
    rep.print("A co16")
    fail.assert_none()


def test_ci8_forms_small_against_fp64():
    """patch3x3_ci8_kernel<0 | 1, 4> at the smallest plane (one tile) and with seams (8 tiles: one round, no second iteration), every
    epilogue, 16-bit / split output."""
    rep, fail = Report(), Failures()
    for name, N, H, W in (("single_tile", 1, 4, 64), ("8_tiles", 2, 8, 128)):
        for kind in KINDS:
            op = Operands(kind, N, H, W, 8, 64, False, seed=H * 17 + W)
            _run(op, {}, rep, fail, f"ci8 {name}", expect="ci8")
            del op
    rep.print("A ci8 small")
    fail.assert_none()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [30, 60], ids=["780_tiles", "1560_tiles"])
def test_ci8_persistent_rounds_against_fp64(N, kind):
    """The persistent loop of patch3x3_ci8_kernel: H = 52, W = 128 gives 26 tiles per image.  N = 30: 780 tiles - 12 of the 768 16-bit
    work-groups and 268 of the 512 split ones run a second iteration (which fetches nothing more); 780 % 8 = 4.  N = 60: 1560 tiles - 24
    work-groups run 3 rounds (16-bit) resp. 4 (split): a middle iteration consumes a prefetched patch and issues the next fetch.  A
    work-group that multiplies a stale patch or another image's fails per element (every image has its own seed).  bias + ReLU."""
    rep, fail = Report(), Failures()
    op = Operands(kind, N, 52, 128, 8, 64, False, seed=N)
    _run(op, {}, rep, fail, f"ci8 {N * 26}_tiles", epilogues=BIAS_RELU, expect="ci8")
    del op
    rep.print(f"A ci8 {N * 26} tiles {kind}")
    fail.assert_none()


TRUNK_CASES = [
    # name, N, Hi, Wi, Ci, Co, upsample, patch_conv policy   (instantiation in the 16-bit form; the split form always has JB = 2)
    ("4x32_single_tile", 1, 4, 32, 64, 64, False, 2),                    # whole image in one tile
    ("4x32_up_single_tile", 1, 2, 16, 64, 64, True, 2),                  # reflection at the output resolution, then >> 1
    ("4x32_seams_3_channel_tiles", 2, 8, 64, 128, 192, False, 2),
    ("4x32_co192_policy3_falls_to_jb2", 2, 8, 64, 128, 192, False, 3),   # 192 % 128 != 0
    ("4x32_jb4", 2, 4, 64, 128, 128, False, 3),
    ("4x32_jb4_up", 1, 2, 32, 64, 128, True, 3),
    ("2x64_smallest", 1, 2, 64, 64, 64, False, 2),                       # rows -1 and 2 reflect onto the tile's own two rows
    ("2x64_seams_3_channel_tiles", 2, 6, 128, 64, 192, False, 2),
    ("2x64_up", 1, 3, 32, 64, 64, True, 2),                              # Ho = 6 = 2 * odd
    ("2x64_jb4", 1, 6, 128, 256, 128, False, 3),
    ("2x64_jb4_up", 1, 3, 64, 128, 256, True, 3),
    ("ci512_8_or_16_slices", 1, 4, 32, 512, 256, False, 2),              # the longest weight double-buffer run
]


def test_trunk_forms_against_fp64():
    """patch3x3_kernel<SP, TW, JB> in its six instantiations, each without and with the folded upsample, every epilogue."""
    rep, fail = Report(), Failures()
    for name, N, Hi, Wi, Ci, Co, up, pc in TRUNK_CASES:
        for kind in KINDS:
            op = Operands(kind, N, Hi, Wi, Ci, Co, up, seed=Hi * 13 + Wi + Ci + Co)
            _run(op, {"patch_conv": pc}, rep, fail, f"trunk {name}", expect="trunk")
            del op
    rep.print("A trunk")
    fail.assert_none()


FALLBACKS = [
    # name, N, Hi, Wi, Ci, Co, upsample, out_f32, residual: one per `return 0` of patch_conv_ok / patch_trunk_ok a caller can reach
    ("trunk_Wo_48", 1, 8, 48, 64, 64, False, False, False),              # Wo % 32 != 0
    ("co16_Hi_6", 1, 6, 64, 64, 3, False, True, False),                  # Hi % 4 != 0, decoder's last layer
    ("ci8_Hi_6", 1, 6, 64, 8, 64, False, False, False),                  # Hi % 4 != 0, encoder's first layer
    ("trunk_out_f32", 1, 4, 32, 64, 64, False, True, False),
    ("trunk_residual", 1, 4, 32, 64, 64, False, False, True),
]


def test_refused_geometries_take_the_igemm_against_fp64():
    """Under the default policy: per element against fp64, and bit-identical to the same call with patch_conv = 0."""
    rep, fail = Report(), Failures()
    for name, N, Hi, Wi, Ci, Co, up, f32, res in FALLBACKS:
        for kind in KINDS:
            op = Operands(kind, N, Hi, Wi, Ci, Co, up, seed=Hi + Wi + Ci + Co)
            _run(op, {}, rep, fail, f"fallback {name}", out_f32=f32, with_res=res, expect="igemm")
            del op
    rep.print("A fallbacks")
    fail.assert_none()


# ---- (B) the style network's own layers -----------------------------------------------------------------------------------------------

def _style_net_convs(N, S):
    """Every distinct convolution of the encoder (to relu4_1) and the decoder at N x S x S, walked as _SeqRunner.run walks them:
    (name, N, Hi, Wi, Ci, Co, upsample, relu, out_f32)."""
    from uda_poseestimation_amd.lib.models import Style_net as sn
    out, H, C_ = [], S, 8                    # (the image enters with its 3 channels padded to 8)
    for i, st in enumerate(sn._compile(list(sn.vgg.children())[:31])):
        if st.kind == "pool":
            H = (H + 1) // 2                 # ceil mode
            continue
        assert st.conv.in_channels == (3 if C_ == 8 else C_) and not st.upsample
        out.append((f"enc.{i}", N, H, H, C_, st.conv.out_channels, False, st.relu, False))
        C_ = st.conv.out_channels
    steps = sn._compile(list(sn.decoder.children()))
    for i, st in enumerate(steps):
        assert st.kind == "conv" and st.conv.in_channels == C_
        out.append((f"dec.{i}", N, H, H, C_, st.conv.out_channels, st.upsample, st.relu, i == len(steps) - 1))
        H, C_ = H << int(st.upsample), st.conv.out_channels
    assert H == S and C_ == 3
    seen, uniq = set(), []
    for c in out:
        if c[1:] not in seen:
            seen.add(c[1:])
            uniq.append(c)
    return uniq


@pytest.mark.parametrize("N,S", [(1, 256), (2, 128)], ids=["n1_256", "n2_128"])
def test_style_net_layers_against_fp64(N, S):
    """Part B: the production policy of the style convolutions; bias always, ReLU and the fp32 output where the executor has them."""
    from uda_poseestimation_amd.lib.models import Style_net as sn
    rep, fail = Report(), Failures()
    convs = _style_net_convs(N, S)
    assert len(convs) >= 14
    families = set()
    for name, n, Hi, Wi, Ci, Co, up, relu, f32 in convs:
        for kind in KINDS:
            op = Operands(kind, n, Hi, Wi, Ci, Co, up, seed=sum(map(ord, name)) + S)
            families.add(_family(op.g, f32, False, sn._SeqRunner.policy_overrides))
            _run(op, dict(sn._SeqRunner.policy_overrides), rep, fail, f"style N{N} {S} {name} {Ci}->{Co}@{Hi}{' up' if up else ''}", out_f32=f32,
                 epilogues=((True, relu),))
            del op
        torch.cuda.empty_cache()
    rep.print(f"B N={N} {S}x{S}")
    assert {"ci8", "co16", "trunk"} <= families, families
    fail.assert_none()
