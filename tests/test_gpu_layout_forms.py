"""The layout and packing kernels of csrc/pointwise.hip through their exported entry points, bit for bit against torch on the CPU.  These
are exact operations - a permutation, a zero fill, one rounding to the storage type, one fp32 addition - so the bar is bit equality.
Every output is a view inside a 0xFF-filled allocation whose guard bytes must come back untouched (helpers.gpu_forms.Guards).

  entry point                                   kernel                                       test
  udapose_nchw_f32_to_nhwc_bf16 / _f32 / _split  nchw_f32_to_nhwc_k<elem_t / float / sp32>    test_nchw_to_nhwc (channel padding to and
      beyond the next multiple of 8, +0 bits in the padding, 1 .. 257 pixels, looping threads past the 8192-block grid cap, Cpad % 8
      refused before the launch with nothing written)
  udapose_nhwc_to_nchw_f32 (src_is_f32 0 / 1 / 2) nhwc_to_nchw_f32_k<elem_t / float / sp32>   test_nhwc_to_nchw (C < Cstride with NaN in
      the unread channels; with and without the per-channel clamp against torch.clamp: values on both bounds, -0.0, +-inf.  NaN inputs to
      the clamp are out of scope: include/udapose.h promises nothing for them)
  udapose_cast_f32_bf16                          cast_f32_bf16_k                              test_cast (ties, subnormals, +-0, +-inf,
      overflow to inf in fp16, looping threads, n % 8 refused; a NaN stays a NaN, its payload is not compared)
  udapose_transpose_cast                         transpose_cast_k<elem_t>                     test_transpose_cast (A, B not multiples of 32)
  udapose_pack_strided                           pack_strided_k<elem_t>                       test_pack_strided (the stem's form as
      ops.pack_weight calls it, non-contiguous sources, KWp > KW and Bp > B zero fill, more than 8192 * 256 outputs)
  udapose_f32_to_split / udapose_split_to_f32    f32_to_split_k / split_to_f32_k              test_split_conversions (in place against out of
      place, looping threads, the saturation counter; what tests/test_gpu_f16x2.py checks - round trip accuracy and range - is not repeated)
  udapose_axpy_f32                               axpy_k / axpy_tail_k                         test_axpy (the n % 4 tail, looping threads)
The 16-bit element type runs in both builds; the fp32 and split variants through the default library.  Split outputs are compared three
ways: ops.split_to_f32(result) with the CPU restatement of the format of csrc/common.h (fp64_adain.split_cpu: h = fp16(c), l = fp16((c - h)
* 2048), c = v saturated at +-65504), and the raw bytes with that restatement and with ops.f32_to_split of the fp32 reference.

Not here: the split form of nchw_f32_to_nhwc_k with a shadow pointer is internal to 'strict' plans and covered by tests/test_gpu_strict.py;
pack_multi_k, zero_k, zero_multi_k and split_sum_k have no exported entry of their own and are reached only through the network plans
(tests/test_gpu_net.py, tests/test_gpu_grad_schedules.py)."""
import time

import pytest
import torch

from helpers import fp64_adain as fa
from helpers.gpu_forms import Failures, Guards

pytestmark = pytest.mark.gpu

ELEM = {"bf16": torch.bfloat16, "fp16": torch.float16}
CAP = 8192 * 256        # threads of the largest grid (grid_for): more items than this and threads loop
COUNT = {}

MEASURED = """Every case is bit-exact on an MI355X in both builds (the module prints the number of comparisons per test)."""


def _ops():
    from uda_poseestimation_amd import ops, _hip
    return ops, _hip


@pytest.fixture(scope="module", autouse=True)
def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from uda_poseestimation_amd import _hip
    _hip.lib("bf16"), _hip.lib("fp16")
    t0 = time.time()
    yield
    print(f"\n[layout forms] module wall time {time.time() - t0:.1f} s; bit comparisons per test: {COUNT}")


@pytest.fixture(autouse=True)
def _device_still_sound():
    """Nothing is started on a device that an earlier test left in an error state."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reports an error before this test: {e}", returncode=3)
    yield


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(got, ref, what, test, nan_ok=False):
    """got (device) == ref (CPU, the same dtype and shape) bit for bit; nan_ok: a NaN matches any NaN."""
    COUNT[test] = COUNT.get(test, 0) + 1
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{what}: {tuple(got.shape)} {got.dtype} against {tuple(ref.shape)} {ref.dtype}"
    r = ref.to(got.device)
    bad = _bits(got) != _bits(r)
    if nan_ok:
        bad &= ~(torch.isnan(got) & torch.isnan(r))
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at flat index {i}: got "
                             f"{got.reshape(-1)[i].item()!r} (bits {_bits(got).reshape(-1)[i].item():#x}), expected {r.reshape(-1)[i].item()!r} "
                             f"(bits {_bits(r).reshape(-1)[i].item():#x})")


def _call(fn, *args):
    _, _hip = _ops()
    _hip.check(fn(_hip.stream(), *args), fn.__name__)
    torch.cuda.synchronize()


def _refused(fn, *args):
    _, _hip = _ops()
    code = fn(_hip.stream(), *args)
    torch.cuda.synchronize()
    assert code == -1, f"{fn.__name__}: returned {code}, expected the argument error -1"


def _split_checks(out_i32, ref32, what, test):
    """A split result [..., C] (int32 storage) against the fp32 reference on the CPU, three ways."""
    ops, _ = _ops()
    _same_bits(ops.split_to_f32(out_i32), fa.join_cpu(*fa.split_cpu(ref32)), f"{what} joined", test)
    raw = out_i32.view(torch.float16).reshape(ref32.shape[:-1] + (ref32.shape[-1] // 8, 2, 8))
    _same_bits(raw, fa.split_bytes(ref32), f"{what} bytes against the format's restatement", test)
    _same_bits(out_i32, ops.f32_to_split(ref32.cuda()).cpu(), f"{what} bytes against f32_to_split", test)


def _values(shape, g, scale=1.0):
    """N(0, scale) with a few +-0 and exact small integers planted."""
    x = torch.randn(shape, generator=g) * scale
    f = x.reshape(-1)
    if f.numel() >= 8:
        f[1], f[f.numel() // 2], f[-1] = -0.0, 0.0, 3.0
    return x


# ---- NCHW fp32 -> NHWC -----------------------------------------------------------------------------------------------------------

def _to_nhwc_ref(x, Cp):
    N, C, HW = x.shape
    ref = torch.zeros(N, HW, Cp)
    ref[:, :, :C] = x.permute(0, 2, 1)
    return ref


def _to_nhwc_all(x, Cp, fail, what):
    ops, _hip = _ops()
    N, C, HW = x.shape
    ref, xd = _to_nhwc_ref(x, Cp), x.cuda()
    for kind in ("bf16", "fp16", "f32", "split"):
        w = f"to_nhwc {kind} {what}"
        G = Guards()
        if kind in ELEM:
            out = G.new((N, HW, Cp), ELEM[kind], Cp)
            fn = _hip.lib(kind).udapose_nchw_f32_to_nhwc_bf16
        else:
            out = G.new((N, HW, Cp), torch.float32 if kind == "f32" else torch.int32, Cp)
            fn = _hip.lib().udapose_nchw_f32_to_nhwc_f32 if kind == "f32" else _hip.lib().udapose_nchw_f32_to_nhwc_split
        if fail.run(w, lambda: (_call(fn, xd.data_ptr(), out.data_ptr(), N, C, HW, Cp), G.check(w), True)) is None:
            continue
        if kind == "split":
            fail.run(w, lambda: _split_checks(out, ref, w, "nchw_to_nhwc"))
        else:
            fail.run(w, lambda: _same_bits(out, ref.to(out.dtype), w, "nchw_to_nhwc"))


def test_nchw_to_nhwc():
    fail = Failures()
    g = torch.Generator().manual_seed(1)
    for N in (1, 3):
        for C, Cp in ((1, 8), (3, 8), (8, 8), (17, 24), (17, 64), (61, 64)):
            for HW in (1, 63, 257):
                _to_nhwc_all(_values((N, C, HW), g, 50.0), Cp, fail, f"N {N} C {C} Cpad {Cp} HW {HW}")
    fail.assert_none()


def test_nchw_to_nhwc_past_the_grid_cap():
    """N * HW * Cpad / 8 = 2097176 items against 8192 * 256 = 2097152 threads: the first 24 threads take a second item."""
    fail = Failures()
    HW = 262147
    assert HW * 8 > CAP
    _to_nhwc_all(_values((1, 61, HW), torch.Generator().manual_seed(2), 50.0), 64, fail, f"N 1 C 61 Cpad 64 HW {HW}")
    fail.assert_none()


def test_nchw_to_nhwc_refuses_a_ragged_padding():
    """Cpad % 8 != 0 is refused before the launch (pw_nchw_f32_to_nhwc_*: `if (Cp % 8) return UDAPOSE_ERR_ARG`): nothing is written."""
    _, _hip = _ops()
    x = torch.randn(2, 3, 63).cuda()
    for kind in ("bf16", "fp16", "f32", "split"):
        G = Guards()
        out = G.new((2, 63, 12), ELEM.get(kind, torch.float32 if kind == "f32" else torch.int32), 12)
        fn = (_hip.lib(kind).udapose_nchw_f32_to_nhwc_bf16 if kind in ELEM else
              _hip.lib().udapose_nchw_f32_to_nhwc_f32 if kind == "f32" else _hip.lib().udapose_nchw_f32_to_nhwc_split)
        _refused(fn, x.data_ptr(), out.data_ptr(), 2, 3, 63, 12)
        assert bool((out.view(torch.uint8) == 0xFF).all()), f"{kind}: a refused call wrote to its output"
        G.check(kind)


# ---- NHWC -> NCHW fp32 -----------------------------------------------------------------------------------------------------------

def test_nhwc_to_nchw():
    _, _hip = _ops()
    fail = Failures()
    g = torch.Generator().manual_seed(3)
    nan16 = torch.tensor(float("nan"), dtype=torch.float16)
    for N in (1, 3):
        for C, Cs in ((3, 8), (8, 8), (17, 24), (64, 64)):
            for HW in (1, 63, 257):
                v = _values((N, HW, Cs), g, 2.0)
                lo = -(1.0 + torch.arange(C) / 64.0)            # exact in every storage type
                hi = 1.0 + torch.arange(C).flip(0) / 64.0
                f = v[:, :, :C].reshape(-1, C).clone()
                rows = torch.randint(0, f.shape[0], (6,), generator=g)
                f[rows[0]], f[rows[1]] = lo, hi                      # exactly on the bounds
                f[rows[2]], f[rows[3]] = float("inf"), float("-inf")
                f[rows[4], 0], f[rows[5], C - 1] = -0.0, -0.0
                v[:, :, :C] = f.reshape(N, HW, C)
                for kind in ("bf16", "fp16", "f32", "split"):
                    if kind in ELEM:
                        st = v.to(ELEM[kind])
                        val = st.float()
                        st[:, :, C:] = float("nan")
                        src, L, code = st.cuda(), _hip.lib(kind), 0
                    elif kind == "f32":
                        st = v.clone()
                        val = st.clone()
                        st[:, :, C:] = float("nan")
                        src, L, code = st.cuda(), _hip.lib(), 1
                    else:       # the split bytes from the format's restatement (+-inf saturates there: the clamp sees +-65504)
                        raw = fa.split_bytes(v)                  # [N, HW, Cs / 8, 2, 8] fp16
                        val = fa.join_cpu(*fa.split_cpu(v))
                        ch = (torch.arange(Cs) >= C).reshape(Cs // 8, 1, 8).expand(Cs // 8, 2, 8)
                        raw = torch.where(ch, nan16, raw)
                        src, L, code = raw.contiguous().view(torch.int32).reshape(N, HW, Cs).cuda(), _hip.lib(), 2
                    plain = val[:, :, :C].permute(0, 2, 1).contiguous()
                    for clamp in (False, True):
                        w = f"to_nchw {kind} N {N} C {C} Cstride {Cs} HW {HW} clamp {int(clamp)}"
                        ref = torch.clamp(plain, lo[None, :, None], hi[None, :, None]) if clamp else plain
                        G = Guards()
                        out = G.new((N, C, HW), torch.float32, HW)
                        lod, hid = (lo.cuda(), hi.cuda()) if clamp else (None, None)
                        args = (src.data_ptr(), code, out.data_ptr(), N, C, HW, Cs, _hip.ptr(lod), _hip.ptr(hid))
                        if fail.run(w, lambda: (_call(L.udapose_nhwc_to_nchw_f32, *args), G.check(w), True)) is not None:
                            fail.run(w, lambda: _same_bits(out, ref, w, "nhwc_to_nchw"))
    fail.assert_none()


# ---- casts and transposes --------------------------------------------------------------------------------------------------------

def _cast_values(n, dt, g):
    x = torch.randn(n, generator=g)
    k = min(n, 2040) // 8
    if k:
        drop = 16 if dt == torch.bfloat16 else 13               # fp32 mantissa bits the type drops
        up = torch.randint(0, 2 ** 14, (2 * k,), generator=g, dtype=torch.int32)
        base = (0x3F000000 + (up << drop)) | (1 << (drop - 1))   # exact ties, even and odd kept parts, from 0.5 up over the type's normal range
        x[:2 * k] = base.view(torch.float32) * torch.where(torch.arange(2 * k) % 2 == 0, 1.0, -1.0)
        tiny = 2.0 ** -133 if dt == torch.bfloat16 else 2.0 ** -24    # subnormals of the target type: multiples and ties of its last bit
        x[2 * k:3 * k] = tiny * torch.randint(-2048, 2048, (k,), generator=g).float() * 0.5
        sp = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 3e38, -3e38, 65520.0, -65520.0, 65504.0, 65519.996, float("nan"), 1e-45, -1e-45,
                           2.0 ** -126, 2.0 ** -14, 2.0 ** -25])
        m = min(sp.numel(), n - 3 * k)
        x[3 * k:3 * k + m] = sp[:m]
    return x


def test_cast():
    _, _hip = _ops()
    fail = Failures()
    g = torch.Generator().manual_seed(4)
    for n in (8, 2040, 8 * CAP + 8):
        for build, dt in ELEM.items():
            x = _cast_values(n, dt, g)
            w = f"cast {build} n {n}"
            G = Guards()
            out = G.new((n,), dt, 8)
            xd = x.cuda()
            if fail.run(w, lambda: (_call(_hip.lib(build).udapose_cast_f32_bf16, xd.data_ptr(), out.data_ptr(), n), G.check(w), True)) is not None:
                fail.run(w, lambda: _same_bits(out, x.to(dt), w, "cast", nan_ok=True))
    for build, dt in ELEM.items():      # n % 8 != 0: refused before the launch (pw_cast_f32_bf16)
        G = Guards()
        out = G.new((12,), dt, 8)
        _refused(_hip.lib(build).udapose_cast_f32_bf16, torch.randn(12).cuda().data_ptr(), out.data_ptr(), 12)
        assert bool((out.view(torch.uint8) == 0xFF).all())
        G.check(build)
    fail.assert_none()


def test_transpose_cast():
    _, _hip = _ops()
    fail = Failures()
    g = torch.Generator().manual_seed(5)
    for A, T, B in ((1, 1, 1), (31, 1, 33), (32, 9, 32), (33, 9, 31), (64, 16, 8), (3, 49, 64), (2048, 1, 256)):
        x = _values((A, T, B), g)
        xd = x.cuda()
        for build, dt in ELEM.items():
            w = f"transpose_cast {build} A {A} T {T} B {B}"
            G = Guards()
            out = G.new((B, T, A), dt, A)
            if fail.run(w, lambda: (_call(_hip.lib(build).udapose_transpose_cast, xd.data_ptr(), out.data_ptr(), A, T, B), G.check(w), True)) is not None:
                fail.run(w, lambda: _same_bits(out, x.permute(2, 1, 0).contiguous().to(dt), w, "transpose_cast"))
    fail.assert_none()


def test_pack_strided():
    ops, _hip = _ops()
    fail = Failures()
    g = torch.Generator().manual_seed(6)

    def run(build, src, A, KH, KWp, KW, Bp, B, sa, skh, skw, sb, ref, w):
        dt = ELEM[build]
        G = Guards()
        out = G.new((A, KH, KWp, Bp), dt, KWp * Bp)
        args = (src.data_ptr(), out.data_ptr(), A, KH, KWp, KW, Bp, B, sa, skh, skw, sb)
        if fail.run(w, lambda: (_call(_hip.lib(build).udapose_pack_strided, *args), G.check(w), True)) is not None:
            fail.run(w, lambda: _same_bits(out, ref.to(dt), w, "pack_strided"))
        return out

    for build, dt in ELEM.items():
        # the stem: [Co, 3, 7, 7] -> [Co, 7, 8, 8], the call of ops.pack_weight
        for Co in (8, 64):
            wt = _values((Co, 3, 7, 7), g)
            flat = wt.cuda().contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)        # [Co, 7, 7, 3] contiguous
            ref = torch.zeros(Co, 7, 8, 8)
            ref[:, :, :7, :3] = wt.permute(0, 2, 3, 1)
            out = run(build, flat, Co, 7, 8, 7, 8, 3, 7 * 7 * 3, 7 * 3, 3, 1, ref, f"pack_strided {build} stem Co {Co}")
            d = ops.conv_desc(1, 16, 16, 8, Co, 7, 2, 3)
            fail.run(f"pack_weight {build} Co {Co}", lambda: _same_bits(ops.pack_weight(wt.cuda(), d, dtype=dt), out.cpu(), f"ops.pack_weight {build} Co {Co}",
                                                                        "pack_strided"))
        # the torch layout [A, B, KH, KW] gathered to [A, KH, KWp, Bp]: the channel stride is the largest but the batch's
        A, B, KH, KW, KWp, Bp = 5, 13, 3, 5, 8, 16
        base = _values((A, B, KH, KW), g)
        ref = torch.zeros(A, KH, KWp, Bp)
        ref[:, :, :KW, :B] = base.permute(0, 2, 3, 1)
        run(build, base.cuda(), A, KH, KWp, KW, Bp, B, B * KH * KW, KW, 1, KH * KW, ref, f"pack_strided {build} torch layout")
        # every other channel of a [A, KH, KW, 2 B] tensor
        A, B, KH, KW, KWp, Bp = 3, 9, 2, 3, 4, 24
        base = _values((A, KH, KW, 2 * B), g)
        ref = torch.zeros(A, KH, KWp, Bp)
        ref[:, :, :KW, :B] = base[:, :, :, ::2]
        run(build, base.cuda(), A, KH, KWp, KW, Bp, B, KH * KW * 2 * B, KW * 2 * B, 2 * B, 2, ref, f"pack_strided {build} every other channel")
    # more outputs than threads in the largest grid
    A, B, KH, KW, KWp, Bp = 2049, 100, 1, 7, 8, 128
    assert A * KH * KWp * Bp > CAP
    base = _values((A, KH, KW, B), g)
    ref = torch.zeros(A, KH, KWp, Bp)
    ref[:, :, :KW, :B] = base
    run("bf16", base.cuda(), A, KH, KWp, KW, Bp, B, KH * KW * B, KW * B, B, 1, ref, "pack_strided bf16 past the grid cap")
    fail.assert_none()


# ---- f16x2 split conversions -----------------------------------------------------------------------------------------------------

def test_split_conversions():
    """In place (dst == src, which include/udapose.h promises) against out of place, 8 .. past the grid cap; split_to_f32 of the result
    against the format's restatement."""
    ops, _hip = _ops()
    fail = Failures()
    g = torch.Generator().manual_seed(7)
    L = _hip.lib()
    for n in (8, 2056, 8 * CAP + 8):
        x = _values((n,), g, 30.0)
        x[3], x[4] = 65504.0, -65504.0          # the largest values that do not saturate
        w = f"split n {n}"
        G = Guards()
        outp = G.new((n,), torch.int32, 8)
        inpl = G.new((n,), torch.float32, 8, x.cuda())
        back = G.new((n,), torch.float32, 8)
        xd = x.cuda()

        def go():
            _call(L.udapose_f32_to_split, xd.data_ptr(), outp.data_ptr(), n)
            _call(L.udapose_f32_to_split, inpl.data_ptr(), inpl.data_ptr(), n)
            _call(L.udapose_split_to_f32, outp.data_ptr(), back.data_ptr(), n)
            G.check(w)
            return True
        if fail.run(w, go) is None:
            continue
        fail.run(w, lambda: _same_bits(inpl.view(torch.int32), outp.cpu(), f"{w} in place against out of place", "split"))
        fail.run(w, lambda: _same_bits(outp.view(torch.float16).reshape(n // 8, 2, 8), fa.split_bytes(x), f"{w} bytes against the restatement", "split"))
        fail.run(w, lambda: _same_bits(back, fa.join_cpu(*fa.split_cpu(x)), f"{w} split_to_f32", "split"))
    for fn in (L.udapose_f32_to_split, L.udapose_split_to_f32):     # n % 8 != 0: refused before the launch
        G = Guards()
        out = G.new((12,), torch.float32, 8)
        _refused(fn, torch.zeros(16).cuda().data_ptr(), out.data_ptr(), 12)
        assert bool((out.view(torch.uint8) == 0xFF).all())
        G.check(fn.__name__)
    fail.assert_none()


def test_split_saturation_counter():
    """udapose_split_saturations: zero after a clean tensor, and exactly the number of planted values outside +-65504 and NaN - each planted in
    an 8-channel group of its own, the unit the stores count in.  Called outside any capture."""
    ops, _ = _ops()
    from uda_poseestimation_amd import utils as mt
    mt.split_saturations(reset=True)
    x = torch.randn(4096, generator=torch.Generator().manual_seed(8)) * 100.0
    x[0], x[9] = 65504.0, -65504.0
    ops.f32_to_split(x.cuda())
    assert mt.split_saturations(reset=False) == 0
    planted = [7.0e4, -7.0e4, float("inf"), float("-inf"), float("nan"), 65505.0, -1e30, 65504.004, float("nan"), 3e38, -65536.0]
    for i, v in enumerate(planted):
        x[8 * (37 * i + 5) + i % 8] = v
    y = ops.split_to_f32(ops.f32_to_split(x.cuda())).cpu()
    assert mt.split_saturations(reset=False) == len(planted)
    assert mt.split_saturations(reset=True) == len(planted) and mt.split_saturations(reset=True) == 0
    _same_bits(y.cuda(), fa.join_cpu(*fa.split_cpu(x)), "saturated values", "split")
    ops.f32_to_split(torch.randn(64).cuda())
    assert mt.split_saturations(reset=True) == 0


# ---- axpy ------------------------------------------------------------------------------------------------------------------------

def test_axpy():
    """y += x bit for bit against fp32 y + x; the words right after y + n stay 0xFF (the tail kernel adds n % 4 values, no more)."""
    _, _hip = _ops()
    fail = Failures()
    g = torch.Generator().manual_seed(9)
    for n in (1, 3, 4, 5, 1023, 1024, 1027, CAP * 4 + 3):
        y0, x = _values((n,), g), _values((n,), g, 1e-3)
        w = f"axpy n {n}"
        G = Guards()
        y = G.new((n,), torch.float32, 64, y0.cuda())
        xd = x.cuda()
        if fail.run(w, lambda: (_call(_hip.lib().udapose_axpy_f32, y.data_ptr(), xd.data_ptr(), n), G.check(w), True)) is not None:
            fail.run(w, lambda: _same_bits(y, y0 + x, w, "axpy"))
    fail.assert_none()
