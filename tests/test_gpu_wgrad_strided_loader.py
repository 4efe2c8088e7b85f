"""The weight-gradient loader of strided, transposed and stem row-tap layers on power-of-two maps (udapose_policy.wgrad_fastgeo_strided,
wgrad.hip wgrad_dma_body<.., GEO = 2>): bit-field pixel coordinates and 32-bit offsets in place of the general loader's divisions.  It
changes address generation only - tiles, MFMA order, split order and stores are the general loader's - so every gradient must equal the
policy-off one to the bit: per layer through udapose_conv2d_bwd_weight (and against fp64), through the grouped and pair launches of a small
network plan (the stem's row-tap form included), and the plan must choose the loader for exactly the layers it is meant for."""
import ctypes as C

import pytest
import torch

from helpers import fp64_conv as fc

pytestmark = pytest.mark.gpu

# name, N, H, W, Ci, Co, K, stride, pad, transposed, takes the strided loader
LAYER_CASES = [
    ("c3x3s2_16_c128", 2, 16, 16, 128, 128, 3, 2, 1, False, True),
    ("c3x3s2_16_c64", 2, 16, 16, 64, 64, 3, 2, 1, False, True),
    ("c3x3s2_8_c128", 2, 8, 8, 128, 128, 3, 2, 1, False, True),       # one DMA instruction spans several image rows and both images
    ("c1x1s2_16_c128_256", 2, 16, 16, 128, 256, 1, 2, 0, False, True),
    ("up4x4s2_4_c128", 2, 4, 4, 128, 128, 4, 2, 1, True, True),
    ("up4x4s2_4_c256_128", 2, 4, 4, 256, 128, 4, 2, 1, True, True),
    ("up4x4s2_8_c128", 2, 8, 8, 128, 128, 4, 2, 1, True, True),
    ("up4x4s2_8_c256_128", 2, 8, 8, 256, 128, 4, 2, 1, True, True),
    ("c3x3s2_12_c128", 2, 12, 12, 128, 128, 3, 2, 1, False, False),   # 12 -> 6: not a power of two, keeps the general loader
]


@pytest.mark.parametrize("case", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_layer_bit_identical_and_against_fp64(case):
    """One layer, per-layer launch: wgrad_fastgeo_strided 1 against 0 under wgrad_fastgeo 1 and 2 and wgrad_ksplit 1 and 3, identical bits;
    the default policy against the fp64 reference with the 16-bit weight-gradient bound of tests/test_gpu_conv_forms.py."""
    from uda_poseestimation_amd import ops, _hip
    name, N, H, W, Ci, Co, K, s, p, tr, _ = case
    for dt in (torch.bfloat16, torch.float16):
        d = ops.conv_desc(N, H, W, Ci, Co, K, s, p, transposed=tr)
        g = fc.geom_of(d)
        gen = torch.Generator(device="cuda").manual_seed(len(name) + Ci + Co)
        x = torch.randn(g.N, g.Hi, g.Wi, g.Ci, device="cuda", generator=gen).to(dt)
        dy = torch.randn(g.N, g.Ho, g.Wo, g.Co, device="cuda", generator=gen).to(dt)
        for fg in (1, 2):
            for ks in (1, 3):
                on = ops.conv2d_bwd_weight(dy, x, ops.with_policy(d, _hip.policy(wgrad_fastgeo=fg, wgrad_ksplit=ks, wgrad_fastgeo_strided=1)))
                off = ops.conv2d_bwd_weight(dy, x, ops.with_policy(d, _hip.policy(wgrad_fastgeo=fg, wgrad_ksplit=ks, wgrad_fastgeo_strided=0)))
                torch.cuda.synchronize()
                assert torch.equal(on, off), (f"{name} {dt} wgrad_fastgeo {fg} ksplit {ks}: the strided loader differs from the general one, "
                                              f"max|d| {float((on - off).abs().max()):.3e}")
                assert float(on.abs().max()) > 0
        ref, absref = fc.wgrad(g, dy, x)
        got = ops.conv2d_bwd_weight(dy, x, d)
        tau, rho = fc.check(got, ref, absref, torch.float32, *fc.BOUNDS[("16bit", "wgrad")], f"{name} {dt} default policy")
        print(f"{name} {dt}: tau {tau:.3g} rho {rho:.3g} (bars {fc.BOUNDS[('16bit', 'wgrad')]})")


# ---- the grouped and pair launches of a small network plan ------------------------------------------------------------------------------
LAYERS, K, N, S = [2, 1, 2, 1], 16, 4, 128
BIT_ROW3, BIT_STEM, BIT_STRIDED, BIT_SWAP, BIT_S2 = 1, 2, 4, 8, 16     # form bits of a timeline stamp (stamp word 5, from bit 32)


def _net(precision, policy):
    """The small student of tests/test_gpu_wgrad_pair.py: 8-stage splits cut the stem, layer1, layer2, the head and the last deconvolution;
    layer4 and the first deconvolution run on 4x4 maps."""
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(7)
    m = pr._pose_resnet("t", K, pr.Bottleneck_default, LAYERS, False, False).cuda().train()
    m.precision = precision
    m.policy = dict({"wgrad_stages": 8}, **policy)
    return m


def _phase1(net, seeds):
    net.merge_wgrad = True
    for sd in seeds:
        x = torch.randn(N, 3, S, S, generator=torch.Generator().manual_seed(sd)).cuda()
        R = torch.randn(N, K, S // 4, S // 4, generator=torch.Generator().manual_seed(sd + 1)).cuda()
        (net(x) * R).sum().backward()
    net.merge_wgrad = False
    pend, net._pending_wg = net._pending_wg, []
    torch.cuda.synchronize()
    assert len(pend) == len(seeds) and all(p[0] is pend[0][0] for p in pend)
    return pend[0][0], [(p[1], p[2]) for p in pend]


def _flat_ptrs(buf, numels):
    ptrs, off = [], 0
    for n in numels:
        ptrs.append(buf.data_ptr() + 4 * off)
        off += n
    return (C.c_void_p * len(numels))(*ptrs)


def _weight_gradients(precision, strided, stamps=None):
    """Both launch forms on the same two gradient chains: the grouped launches of pass A alone (phase 2) and the pair launch of A and B.
    Returns the three flat gradient buffers.  stamps: a timeline buffer the single-pass launches stamp."""
    from uda_poseestimation_amd import _hip
    net = _net(precision, {"wgrad_fastgeo_strided": strided})
    hd, (A, B) = _phase1(net, (11, 21))
    pa, _, _ = net._pointers()
    nl = [p.numel() for p in net.parameters()]
    tot = sum(nl)
    single, pa_buf, pb_buf = (torch.zeros(tot, device="cuda") for _ in range(3))
    gs, ga, gb = _flat_ptrs(single, nl), _flat_ptrs(pa_buf, nl), _flat_ptrs(pb_buf, nl)
    for gp in (gs, ga, gb):
        assert hd.L.udapose_net_bind_grads(hd.h, gp) == 0
    pol = _hip.Policy()
    assert hd.L.udapose_net_get_policy(hd.h, C.byref(pol)) == 0 and pol.wgrad_fastgeo_strided == strided
    if stamps is not None:
        pol.timeline = stamps.data_ptr()
        assert hd.L.udapose_net_set_policy(hd.h, C.byref(pol)) == 0
    p = _hip.ptr
    assert hd.L.udapose_net_backward_phase(hd.h, _hip.stream(), None, pa, p(hd.wpack), p(A[0]), p(A[1]), gs, C.c_float(0.0), 0, 2) == 0
    if stamps is not None:
        torch.cuda.synchronize()
        pol.timeline = None
        assert hd.L.udapose_net_set_policy(hd.h, C.byref(pol)) == 0
    assert hd.L.udapose_net_wgrad_pair(hd.h, _hip.stream(), p(A[0]), p(A[1]), ga, C.c_float(0.0), p(B[0]), p(B[1]), gb, C.c_float(0.0), 0) == 0
    torch.cuda.synchronize()
    return [n_ for n_, _ in net.named_parameters()], nl, (single, pa_buf, pb_buf)


_RUNS = {}


def _run(precision, strided):
    """(computed once per precision and policy, shared by the tests below; the bf16 runs also carry the stamps of their single-pass launches)"""
    key = (precision, strided)
    if key not in _RUNS:
        stamps = torch.zeros(1 << 17, 8, dtype=torch.int64, device="cuda") if precision == "bf16" else None
        names, nl, bufs = _weight_gradients(precision, strided, stamps)
        rows = None
        if stamps is not None:
            rows = stamps.cpu()
            rows = rows[(rows[:, 1] != 0) & (rows[:, 4] >= 0)]
        _RUNS[key] = (names, nl, bufs, rows)
    return _RUNS[key]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_grouped_and_pair_launches_bit_identical(precision):
    """Every parameter gradient of the small student - the grouped launches of one pass and the pair launch of two - with
    wgrad_fastgeo_strided = 1 equals the one with 0 to the bit (stem row-tap form, stride-2 layers, deconvolutions on 4x4 .. 16x16 maps)."""
    names, nl, on, _ = _run(precision, 1)
    _, _, off, _ = _run(precision, 0)
    for tag, a, b in zip(("single pass", "pair launch, pass A", "pair launch, pass B"), on, off):
        o = 0
        for n_, n in zip(names, nl):
            assert torch.equal(a[o:o + n], b[o:o + n]), f"{precision} {tag}: {n_} differs, max|d| {float((a[o:o + n] - b[o:o + n]).abs().max()):.3e}"
            o += n
        assert float(a.abs().max()) > 0
    # (the pair launch's pass A is the single pass's work: the same bits again)
    assert torch.equal(on[0], on[1])


def test_plan_chooses_the_strided_loader():
    """The plan's reported form bits (the timeline stamps of its grouped launches): under the default policy the stem, the stride-2 and the
    transposed problems carry the strided-loader flag and no other problem does; under wgrad_fastgeo_strided = 0 none does."""
    from uda_poseestimation_amd import _hip
    assert _hip.policy().wgrad_fastgeo_strided == 1
    for strided in (1, 0):
        rows = _run("bf16", strided)[3]
        bits = (rows[:, 5] >> 32) & 31
        meant = (bits & (BIT_STEM | BIT_SWAP | BIT_S2)) != 0
        for b, what in ((BIT_STEM, "stem row-tap"), (BIT_SWAP, "transposed"), (BIT_S2, "stride-2")):
            assert int(((bits & b) != 0).sum()) > 0, f"the plan stamps no {what} work-group"
        assert int((~meant).sum()) > 0
        flagged = (bits & BIT_STRIDED) != 0
        if strided:
            assert bool((flagged == meant).all()), "default policy: the strided-loader flag is not on exactly the stem, stride-2 and transposed problems"
        else:
            assert not bool(flagged.any()), "wgrad_fastgeo_strided = 0: a problem still carries the strided-loader flag"
