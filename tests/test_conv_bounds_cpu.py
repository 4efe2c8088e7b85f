"""The fp64 convolution reference and its checker (tests/helpers/fp64_conv.py) on the CPU: the reference agrees with torch's own
float64 convolutions in every geometry the library runs, a correct fp32-accumulated result passes check() at the bars the GPU tests use
(helpers.fp64_conv.BOUNDS), and each planted fault of the kind a wrong kernel form makes fails it - at small shapes and at bench-like
reduction lengths (K = 2304 for a forward, M = 131072 pixels for a weight gradient); the faults of the patch-staged kernels (a wrong
padding index, a shifted pixel block, a swapped 16-byte chunk, a dropped l part, another image's tile) at the bars of
tests/test_gpu_patchconv_forms.py."""
import pytest
import torch
import torch.nn.functional as F

from helpers import fp64_conv as fc

TAU_F, RHO_F = fc.BOUNDS[("16bit", "fprop")]
TAU_W, RHO_W = fc.BOUNDS[("16bit", "wgrad")]


def _rand(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).bfloat16().float()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("case", [
    # N, Hi, Wi, Ci, Co, K, stride, pad, transposed, reflect, upsample
    (2, 7, 5, 16, 24, 3, 1, 1, False, False, False),
    (2, 9, 7, 16, 8, 3, 2, 1, False, False, False),
    (1, 6, 5, 16, 8, 1, 2, 0, False, False, False),
    (2, 5, 7, 16, 24, 4, 2, 1, True, False, False),
    (1, 6, 7, 16, 16, 3, 1, 1, False, True, False),
    (1, 5, 4, 16, 8, 3, 1, 1, False, True, True),
], ids=["3x3s1", "3x3s2_odd", "1x1s2", "deconv4x4s2", "reflect", "upsample_reflect"])
def test_reference_equals_torch_float64(case):
    """fprop, data gradient and weight gradient of the tap-loop reference against torch's float64 conv2d / conv_transpose2d and
    autograd (reflection padding and the nearest x2 upsample spelled out with F.pad / F.interpolate); absref is the op on |operands|."""
    N, Hi, Wi, Ci, Co, K, s, p, tr, refl, up = case
    g = fc.Geom(N, Hi, Wi, Ci, Co, K, K, s, p, tr, refl, up)
    x = _rand((N, Ci, Hi, Wi), 1).double().requires_grad_(True)
    w = _rand((Ci, Co, K, K) if tr else (Co, Ci, K, K), 2).double().requires_grad_(True)
    if tr:
        y = F.conv_transpose2d(x, w, stride=s, padding=p)
    else:
        xi = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
        y = F.conv2d(F.pad(xi, (p,) * 4, mode="reflect"), w, stride=s) if refl else F.conv2d(xi, w, stride=s, padding=p)
    dy = _rand(tuple(y.shape), 3).double()
    y.backward(dy)
    wp = fc.phys_weight(w, g)
    ref, absref = fc.fprop(g, _nhwc(x.detach()), wp)
    assert ref.shape == (N, g.Ho, g.Wo, Co)
    torch.testing.assert_close(ref, _nhwc(y.detach()), rtol=1e-12, atol=1e-12)
    assert bool((absref >= ref.abs() - 1e-12).all())
    dx, _ = fc.dgrad(g, _nhwc(dy), wp)
    torch.testing.assert_close(dx, _nhwc(x.grad), rtol=1e-12, atol=1e-12)
    dw, _ = fc.wgrad(g, _nhwc(dy), _nhwc(x.detach()))
    torch.testing.assert_close(dw, fc.phys_weight(w.grad, g), rtol=1e-12, atol=1e-12)


def test_stem_reference_has_the_padded_column_tap():
    """The Ci == 8 stem (3 real channels, 7x7 / s2 / p3, filter columns padded to 8): forward and the first seven column taps of the
    weight gradient equal torch's; the 8th column tap is the correlation at offset dx = 4 (what the kernel's padded tap computes)."""
    N, H, W = 2, 11, 9
    g = fc.Geom(N, H, W, 8, 16, 7, 7, 2, 3)
    x3 = _rand((N, 3, H, W), 4).double()
    x8 = torch.cat([x3, torch.zeros(N, 5, H, W, dtype=torch.float64)], 1)
    w = _rand((16, 3, 7, 7), 5).double().requires_grad_(True)
    y = F.conv2d(x3, w, stride=2, padding=3)
    dy = _rand(tuple(y.shape), 6).double()
    y.backward(dy)
    ref, _ = fc.fprop(g, _nhwc(x8), fc.phys_weight(w, g))
    torch.testing.assert_close(ref, _nhwc(y.detach()), rtol=1e-12, atol=1e-12)
    dw, _ = fc.wgrad(g, _nhwc(dy), _nhwc(x8))
    dw = dw.reshape(16, 7, 8, 8)
    torch.testing.assert_close(dw[:, :, :7, :3], w.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert float(dw[..., 3:].abs().max()) == 0.0
    w8 = torch.zeros(16, 3, 7, 8, dtype=torch.float64, requires_grad=True)
    F.conv2d(F.pad(x3, (3, 4, 3, 3)), w8, stride=2)[..., :g.Ho, :g.Wo].backward(dy)
    torch.testing.assert_close(dw[:, :, 7, :3], w8.grad[:, :, :, 7].permute(0, 2, 1), rtol=1e-12, atol=1e-12)


def test_half_ulp():
    one = torch.tensor([1.0, 1.5, -3.0, 0.0, 1e-30])
    assert fc.half_ulp(one, torch.bfloat16).tolist()[:3] == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7]
    assert fc.half_ulp(one, torch.float16).tolist()[:3] == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10]
    assert fc.half_ulp(one, torch.float16).tolist()[3] == 2.0 ** -25          # fp16 subnormal spacing 2^-24
    assert fc.half_ulp(one, torch.float32).tolist()[0] == 2.0 ** -24
    v = torch.randn(10000, generator=torch.Generator().manual_seed(0)).double()      # fp32 values: one rounding to a 16-bit type, as the kernels round
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert bool(((v.to(dt).double() - v).abs() <= fc.half_ulp(v, dt)).all())


# ---- planted faults -----------------------------------------------------------------------------------------------------------

FWD_SHAPES = [
    # N, H, W, Ci, Co, K, pad: the forward as an implicit GEMM with M = N * H * W rows (ragged), Co columns (one partial n-tile)
    pytest.param((2, 13, 11, 64, 96, 3, 1), id="small_K576_M286"),
    pytest.param((2, 13, 11, 256, 96, 3, 1), id="benchlike_K2304_M286"),
]


def _fwd_case(shape, seed=7):
    N, H, W, Ci, Co, K, p = shape
    x = _rand((N, Ci, H, W), seed)
    w = _rand((Co, Ci, K, K), seed + 1, (Ci * K * K) ** -0.5)
    g = fc.Geom(N, H, W, Ci, Co, K, K, 1, p)
    ref, absref = fc.fprop(g, _nhwc(x), fc.phys_weight(w, g))
    return x, w, g, ref, absref


def _fp32_fwd(x, w, p):
    return _nhwc(F.conv2d(x, w, padding=p))          # fp32 accumulation of exactly representable bf16 products


def _faults_fwd(x, w, p, y):
    """{name: faulted fp32 result} of the faults a wrong forward kernel form makes."""
    Co = y.shape[-1]
    out = {}
    wt = w.clone()
    wt[:, :, 1, 2] = 0                               # one tap (kh = 1, kw = 2) dropped
    out["tap_dropped"] = _fp32_fwd(x, wt, p)
    xg = x.clone()
    xg[:, 8:16] = 0                                  # one 8-channel group of the K reduction dropped
    out["channel_group_dropped"] = _fp32_fwd(xg, w, p)
    flat = y.reshape(-1, Co)
    for bm in (64, 128):                             # an m-tile replaced by its neighbour
        f = flat.clone()
        f[bm:2 * bm] = flat[2 * bm:3 * bm] if flat.shape[0] >= 3 * bm else flat[0:bm]
        out[f"m_tile{bm}_replaced"] = f.reshape(y.shape)
    f = flat.clone()
    f[:, 64:Co - 1] = flat[:, 65:Co]                 # the columns of n-tile 1 read one column off
    out["n_tile_column_offset"] = f.reshape(y.shape)
    f = flat.clone()
    f[(flat.shape[0] - 1) // 64 * 64:] = 0           # the last, partial m-tile never stored (zero)
    out["last_partial_m_tile_zeroed"] = f.reshape(y.shape)
    return out


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_forward_faults_fail_the_check(shape, out_dtype):
    x, w, g, ref, absref = _fwd_case(shape)
    y = _fp32_fwd(x, w, shape[-1])
    tau, rho = fc.check(y.to(out_dtype), ref, absref, out_dtype, TAU_F, RHO_F, "correct fp32-accumulated forward")
    print(f"{shape}: correct result, measured tau {tau:.3g}, rho {rho:.3g} (bars {TAU_F:g}, {RHO_F:g})")
    faults = _faults_fwd(x, w, shape[-1], y)
    assert len(faults) == 6
    for name, f in faults.items():
        with pytest.raises(AssertionError, match="m-tile") as e:
            fc.check(f.to(out_dtype), ref, absref, out_dtype, TAU_F, RHO_F, name)
        print(f"  {name}: {str(e.value)[:160]}")


def test_check_reports_the_faulted_tile():
    """A fault in one 64-row m-tile and one n-tile is reported at an element of that tile."""
    shape = FWD_SHAPES[0].values[0]
    x, w, g, ref, absref = _fwd_case(shape)
    y = _fp32_fwd(x, w, shape[-1]).reshape(-1, shape[4])
    y[3 * 64 + 5, 70] += 1e-2 * float(absref.reshape(-1, shape[4])[3 * 64 + 5, 70])
    with pytest.raises(AssertionError, match=r"row m = 197, column 70\): m-tile 3 of 64 rows, m-tile 1 of 128 rows, n-tile 1"):
        fc.check(y.reshape(ref.shape), ref, absref, torch.float32, TAU_F, RHO_F, "one element")


WGRAD_SHAPES = [
    # N, H, W, Ci, Co, K: the weight gradient reduces over M = N * H * W pixels in 64-pixel stages
    pytest.param((2, 13, 11, 64, 64, 3), id="small_3x3_M286"),
    pytest.param((32, 64, 64, 64, 64, 1), id="benchlike_1x1_M131072"),
]


@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_weight_gradient_stage_faults_fail_the_check(shape):
    """One 64-pixel stage of the pixel reduction dropped, or added twice: a thin fault (1/2048 of the sum at M = 131072) that only the
    whole-tensor condition must catch, though the element condition does too at these bars."""
    N, H, W, Ci, Co, K = shape
    p = K // 2
    g = fc.Geom(N, H, W, Ci, Co, K, K, 1, p)
    x = _rand((N, Ci, H, W), 11)
    dy = _rand((N, Co, H, W), 12)
    xh, dyh = _nhwc(x), _nhwc(dy)
    ref, absref = fc.wgrad(g, dyh, xh)
    # fp32 result: the per-tap products dy^T x_tap accumulated in fp32 (the stage to plant is the same sum over 64 pixels)
    M = N * H * W
    X = xh.reshape(N, H * W, Ci)
    D = dyh.reshape(M, Co)
    got = torch.zeros(Co, g.taps, Ci)
    stage = torch.zeros(Co, g.taps, Ci)
    m0 = (M // 64 // 2) * 64
    for t, idx, ok in fc._gather_plan(g, "cpu"):
        xg = (X[:, idx] * ok[None, :, None]).reshape(M, Ci)
        got[:, t, :] = D.T @ xg
        stage[:, t, :] = D[m0:m0 + 64].T @ xg[m0:m0 + 64]
    tau, rho = fc.check(got, ref, absref, torch.float32, TAU_W, RHO_W, "correct fp32 weight gradient")
    print(f"{shape}: correct result, measured tau {tau:.3g}, rho {rho:.3g} (bars {TAU_W:g}, {RHO_W:g})")
    for name, f in (("stage_dropped", got - stage), ("stage_added_twice", got + stage)):
        with pytest.raises(AssertionError, match="tile") as e:
            fc.check(f, ref, absref, torch.float32, TAU_W, RHO_W, name)
        print(f"  {name}: {str(e.value)[:160]}")
        # the whole-tensor condition alone catches it as well
        with pytest.raises(AssertionError, match="rho"):
            fc.check(f, ref, absref, torch.float32, 1.0, RHO_W, name + " (element bar disabled)")


# ---- planted faults of the patch-staged kernels (csrc/patchconv.hip; the GPU module is tests/test_gpu_patchconv_forms.py) ----------------

TAU_S, RHO_S = fc.BOUNDS[("split", "fprop")]
PATCH_GEOMS = [
    # N, Hi, Wi, Ci, Co, upsample: reflection-padded 3x3, two tile rows and two 32-wide (one 64-wide) tile columns per image
    pytest.param((2, 8, 64, 64, 64, False), id="reflect"),
    pytest.param((2, 4, 32, 64, 64, True), id="upsample_reflect"),
]


def _split_parts(v):
    """(h, l) of the f16x2 storage h + l * 2^-11 of fp32 values, as float64."""
    h = v.half().double()
    return h, ((v.double() - h) * 2048.0).half().double()


def _round_out(ref, kind):
    """The float64 reference as the kernel would store it: one rounding to the output type (split: the (h, l) pair read back as fp32)."""
    if kind == "split":
        h, l = _split_parts(ref.float())
        return (h + l / 2048.0).float()
    return ref.to(kind)


def _padded_conv(g, x, w, left):
    """The reflect (+ upsample) convolution in float64 with the LEFT padding column replaced: left(xu) -> [N, C, H] column of the upsampled
    input that output column 0 reads at tap kw = 0."""
    xu = _nchw(x).double()
    if g.upsample:
        xu = F.interpolate(xu, scale_factor=2, mode="nearest")
    xp = F.pad(xu, (1, 1, 0, 0), mode="reflect")
    xp[..., 0] = left(xu)
    return _nhwc(F.conv2d(F.pad(xp, (0, 0, 1, 1), mode="reflect"), w.double()))


def _patch_faults(y, y_border, y_h):
    """{name: corrupted stored result}.  y: the clean stored result [N, Ho, Wo, Co]; y_border: computed with the wrong left padding index;
    y_h: computed from the h parts alone (split form) or None.  A tile is 4 x 32 output pixels."""
    out = {}
    f = y.clone()
    f[:, :, 0] = y_border[:, :, 0]                                   # column 0 of every row from the wrong padding index
    out["border_column_clamped"] = f
    f = y.clone()
    f[1, 5, 32:48] = y[1, 5, 33:49]                                  # one 16-pixel block of tile (row 1, column 1) one column off
    out["pixel_block_shifted"] = f
    f = y.clone()
    f[0, 2, 37, 8:16], f[0, 2, 37, 16:24] = y[0, 2, 37, 16:24], y[0, 2, 37, 8:16]      # one 16-byte chunk swapped with its neighbour
    out["channel_chunk_swapped"] = f
    f = y.clone()
    f[1, 4:8, 0:32] = y[0, 4:8, 0:32]                # a tile of image 1 computed from image 0's patch
    out["previous_images_tile"] = f
    if y_h is not None:
        f = y.clone()
        f[0, 0:4, 32:64] = y_h[0, 0:4, 32:64]                        # acc2 * 2^-11 never added in one tile
        out["l_part_dropped"] = f
    return out


@pytest.mark.parametrize("kind", [torch.float32, torch.bfloat16, torch.float16, "split"], ids=["f32", "bf16", "fp16", "split"])
@pytest.mark.parametrize("geom", PATCH_GEOMS)
def test_patch_kernel_faults_fail_the_check(geom, kind):
    """The float64 reference of a small reflect (+ upsample) convolution, rounded to the output type, passes check() at the bars
    tests/test_gpu_patchconv_forms.py uses; corrupted the way a patch-staged kernel can go wrong, it does not.  With the folded upsample
    the clamped padding index and the reflected one name the same input column (-1 -> 1 -> 0 and -1 -> 0 -> 0), so the border fault
    there is the reflection applied at the input's resolution (-1 >> 1 = -1 -> input column 1)."""
    N, Hi, Wi, Ci, Co, up = geom
    g = fc.Geom(N, Hi, Wi, Ci, Co, 3, 3, 1, 1, False, True, up)
    split = kind == "split"
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(N, Ci, Hi, Wi, generator=gen)
    w = torch.randn(Co, Ci, 3, 3, generator=gen) * (Ci * 9) ** -0.5
    if not split:                                                    # 16-bit operands; the split form takes the fp32 operands as they are
        x, w = x.bfloat16().float(), w.bfloat16().float()
    tau, rho = (TAU_S, RHO_S) if split else (TAU_F, RHO_F)
    out_dtype = torch.float32 if split else kind
    ref, absref = fc.fprop(g, _nhwc(x), fc.phys_weight(w, g))
    y = _round_out(ref, kind)
    t, r = fc.check(y, ref, absref, out_dtype, tau, rho, "rounded reference")
    print(f"{geom} {kind}: rounded reference, measured tau {t:.3g}, rho {r:.3g} (bars {tau:g}, {rho:g})")
    border = _padded_conv(g, _nhwc(x), w, (lambda xu: xu[..., 2]) if up else (lambda xu: xu[..., 0]))
    assert float((border[:, :, 1:] - ref[:, :, 1:]).abs().max()) < 1e-12 and float((border[:, :, 0] - ref[:, :, 0]).abs().max()) > 1e-3
    y_h = None
    if split:
        y_h = fc.fprop(g, _split_parts(_nhwc(x))[0], fc.phys_weight(_split_parts(w)[0], g))[0]
    faults = _patch_faults(y, _round_out(border, kind), None if y_h is None else _round_out(y_h, kind))
    assert len(faults) == (5 if split else 4)
    for name, f in faults.items():
        assert not torch.equal(f, y), name
        with pytest.raises(AssertionError, match="m-tile") as e:
            fc.check(f, ref, absref, out_dtype, tau, rho, name)
        print(f"  {name}: {str(e.value)[:160]}")
