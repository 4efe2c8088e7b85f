"""adain_k (csrc/adain.hip) in its three storage types - the 16-bit element type in both builds, fp32, f16x2 split - against the float64
reference of tests/helpers/fp64_adain.py, statistic by statistic and element by element, through ops.adain and the entry points
udapose_adain, _f32, _split and _alpha_dev with every output inside 0xFF guards (helpers.gpu_forms).

Tensors are [N, 1, HW, C], N = 2; the channels of one tensor mix the value regimes a .. i of fp64_adain.make() (c % 9), so one launch
sees all of them: a ReLU-like with exact zeros, b mean / std = 30, c mean / std = 100, d mean 100 std 0.01 (two or three values in the
16-bit types: the sums must then be exact), e constant, f zero, g = d with the first pixel 0 (the pivot is the outlier), h magnitude 1e-4,
i magnitude 1e3.  A split content is a fixed point of the format (f32_to_split of a joined split tensor): only then is "the output equals
the content bit for bit" a property of the format - a first split of an arbitrary fp32 value can leave l exactly half an ulp of h, and
its join then re-splits to the neighbouring h with the same joined value.

  case (HWc, HWs, C)      branch of adain_k
  (2, 130, 128)           126 of 128 pixel lanes empty for the content; two 64-channel slabs: block -> (n, slab)
  (7, 2, 64)              empty lanes on both operands, the smallest style; one slab
  (127, 1024, 128)        one lane empty; the style loop runs 8 times
  (128, 130, 64)          every lane exactly one pixel
  (129, 1500, 128)        one lane holds two cached pixels; ragged style
  (1023, 1024, 128)       register cache one pixel short of full
  (1024, 1024, 64)        register cache exactly full (CACHE * APL = 1024): nothing re-read
  (1025, 2, 128)          one pixel past the cache: the re-read loop runs in one lane
  (1153, 1500, 128)       the re-read loop runs once in 129 lanes, twice in one
  (2051, 130, 64)         the re-read loop runs 8 or 9 times
  forms of every case: alpha 0.6 by value with statistics (everything checked), alpha 1 without statistics, alpha 0 (the output equals the
  content bit for bit), the same three as a device scalar (bit-identical to the by-value launch; the split entry is given a by-value
  alpha of 0.25 as well, which the device scalar must override), statistics only (out == NULL, bit-identical statistics), and ops.adain
  (bit-identical to the direct call).
  HW = 1 (content or style) and C = 96 return the argument error before anything is launched (adain_launch*: `C % 64 || HWc < 2 || HWs < 2`)
  and leave the guarded outputs untouched.

Bars: fp64_adain's, derived there: for the statistics a function of HW, of the lane chain ceil(HW / 128) and of the channel's conditioning
1 + max|x - mean|^2 / var, and of nothing the kernel chooses; tests/test_adain_bounds_cpu.py shows that they hold for the kernel's
arithmetic and reject the one-pass formula the kernel used before at mean / std >= 100.  Every output must be finite wherever the
reference is.  Worst measured per storage type: see MEASURED (printed against the bars by every run)."""
import time

import pytest
import torch

from helpers import fp64_adain as fa
from helpers.gpu_forms import Failures, Guards

pytestmark = pytest.mark.gpu

EPS = 1e-5
CASES = ((2, 130, 128), (7, 2, 64), (127, 1024, 128), (128, 130, 64), (129, 1500, 128), (1023, 1024, 128), (1024, 1024, 64), (1025, 2, 128),
         (1153, 1500, 128), (2051, 130, 64))
KINDS = ("bf16", "fp16", "f32", "split")
DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32, "split": torch.int32}
OUT_T = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32, "split": "split"}
WORST = {}          # (kind, output) -> [worst measured, worst measured / bar, the case]
BY_REGIME = {}      # (kind, regime) -> worst relative error of std^2
RAW = {}            # (HW, C, seed) -> fp32 tensor on the device, shared by the storage types

# worst measured on an MI355X over this module (both builds; every run prints the same table with the case of each worst ratio)
MEASURED = """
  storage   mean error / bar   std^2 error / bar   worst relative error of std^2   out: tau over absref (bar 4.77e-7)   out error / bar
  bf16      0.714              0.590               2.87e-7                         1.93e-9                              1.000
  fp16      0.973              0.582               4.34e-6                         0                                    0.998
  fp32      1.000              0.603               9.88e-5                         2.23e-8                              0.186
  split     1.000              0.603               1.32e-4                         0                                    0.284
Three figures come within 2x of their bar, and each is a bar that is nothing but the rounding of the stored number itself, which a correct
kernel attains:
  mean: where the channel's spread is small (regime d, the constants) the bar is half an fp32 ulp of the mean plus almost nothing.  The
      kernel's mean is pivot + sum / HW in fp64, rounded once: at HW = 2 the mean of two fp32 numbers is an exact tie half of the time, and
      its rounding error is then the whole half ulp (fp32 and split at HWc 2: 1.000).
  std^2 at 0.58 .. 0.60: the constant channels (e, f), where the sums about the pivot are exactly zero, variance + eps is eps exactly, and the
      bar is the 2 * 2^-24 that rounding std to fp32 can move its square; a half-ulp rounding of std moves it by 1 .. 2 * 2^-24 of it.
  out at 1.000 / 0.998 in the 16-bit types: the bar there is half an ulp of the stored type (tau over absref is 1.9e-9 of 4.77e-7), and a
      correctly rounded 16-bit output is off by up to exactly that.  In fp32 and split storage the same check reads 0.19 / 0.28.
Relative error of std^2 per regime (content and style, worst over the cases):
  bf16    a 2.9e-7  b 1.2e-7  c 1.2e-7  d 5.9e-9  e 5.9e-9  f 5.9e-9  g 1.1e-7  h 7.3e-8  i 1.9e-7
  fp16    a 2.1e-7  b 1.2e-7  c 1.2e-7  d 1.0e-7  e 5.9e-9  f 5.9e-9  g 4.3e-6  h 7.3e-8  i 3.4e-7
  fp32    a 7.0e-7  b 2.8e-7  c 2.9e-7  d 2.7e-7  e 5.9e-9  f 5.9e-9  g 9.9e-5  h 7.4e-8  i 6.5e-7
  split   a 7.0e-7  b 3.3e-7  c 2.8e-7  d 3.5e-7  e 5.9e-9  f 5.9e-9  g 1.3e-4  h 7.4e-8  i 3.7e-7
The errors of 1e-4 are regime g, the pivot on the outlier, where kappa is about HW and the bar 3e-3; everywhere else std^2 is within 7e-7
of float64 (5.9e-9 = the fp32 rounding of std alone: the sums are exact there).
torch's own fp32 var on the same content tensors, against float64 (test_torch_var_on_the_same_tensors, on the device), worst relative error per
regime: a 2.2e-7, b 2.1e-6, c 6.4e-6, d 7.0e-4, e 0, f 0, g 1.3e-6, h 2.1e-7, i 1.9e-7 - on the CPU it stays below 1e-6 everywhere
(tests/test_adain_bounds_cpu.py: 5.3e-8).  The kernel is closer than the device's fp32 var in b, c and d (2.7e-7 against 7.0e-4 in d) and
further only in g.
With the one-pass sums about zero that the kernel used before, this module fails on an MI355X in fp16, fp32 and split storage - regimes b,
c, d, e over the bar (and a, i at HWc 2 and HWs 2), non-finite outputs in regime d in fp32, -65504 in split storage - and passes in bf16, whose
values at 100 +- 1 are multiples of 0.5 and sum exactly; regime g passes (its variance is large), as the CPU emulation says."""


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
    RAW.clear()
    print(f"\n[adain forms] module wall time {time.time() - t0:.1f} s")


@pytest.fixture(autouse=True)
def _device_still_sound():
    """Nothing is started on a device that an earlier test left in an error state."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reports an error before this test: {e}", returncode=3)
    yield


def _raw(HW, C, seed):
    key = (HW, C, seed)
    if key not in RAW:
        RAW[key] = fa.make(2, HW, C, seed).cuda()
    return RAW[key]


def _stored(x32, kind):
    """(the tensor [2, 1, HW, C] in the storage of `kind`, its values as float64 [2, HW, C])."""
    ops, _ = _ops()
    if kind == "f32":
        t = x32.clone()
        v = t.double()
    elif kind == "split":
        t = ops.f32_to_split(ops.split_to_f32(ops.f32_to_split(x32)))
        v = ops.split_to_f32(t).double()
    else:
        t = x32.to(DTYPE[kind])
        v = t.double()
    return t.reshape(2, 1, x32.shape[1], x32.shape[2]).contiguous(), v


def _launch(kind, c, s, out, st, alpha, alpha_dev=None):
    """One direct call of the entry point of `kind`; alpha_dev: a device scalar."""
    ops, _hip = _ops()
    N, _, HWc, C = c.shape
    HWs = s.shape[2]
    p, S = _hip.ptr, _hip.stream()
    if kind == "split":
        code = _hip.lib().udapose_adain_split(S, p(c), p(s), p(out), N, HWc, HWs, C, EPS, float(alpha), p(alpha_dev), p(st))
    elif alpha_dev is not None:
        L = _hip.lib() if kind == "f32" else _hip.lib(kind)
        code = L.udapose_adain_alpha_dev(S, p(c), p(s), p(out), N, HWc, HWs, C, EPS, p(alpha_dev), p(st), int(kind == "f32"))
    elif kind == "f32":
        code = _hip.lib().udapose_adain_f32(S, p(c), p(s), p(out), N, HWc, HWs, C, EPS, float(alpha), p(st))
    else:
        code = _hip.lib(kind).udapose_adain(S, p(c), p(s), p(out), N, HWc, HWs, C, EPS, float(alpha), p(st))
    _hip.check(code, "adain")


def _values(kind, out):
    ops, _ = _ops()
    v = ops.split_to_f32(out) if kind == "split" else out
    return v.reshape(out.shape[0], out.shape[2], out.shape[3])


def _note(kind, name, measured, ratio, what=""):
    w = WORST.setdefault((kind, name), [0.0, 0.0, ""])
    if ratio >= w[1]:
        w[2] = what
    w[0], w[1] = max(w[0], measured), max(w[1], ratio)


def _report(kind, t0):
    print(f"\n[adain {kind}] wall {time.time() - t0:.1f} s; worst measured and worst measured / bar of any one check:")
    for (k, name), (m, r, w) in sorted(WORST.items()):
        if k == kind:
            print(f"  {name:34s} {m:.3g}" + (f"   (measured / bar {r:.3f} at {w})" if w else ""))
    print("  relative error of std^2 per regime  " + " ".join(f"{r}:{BY_REGIME.get((kind, r), 0.0):.2g}" for r in fa.REGIMES))


def _run_case(kind, HWc, HWs, C, fail):
    ops, _ = _ops()
    what = f"{kind} HWc {HWc} HWs {HWs} C {C}"
    c, c64 = _stored(_raw(HWc, C, 11 * HWc + C), kind)
    s, s64 = _stored(_raw(HWs, C, 7 * HWs + C + 1), kind)
    sc, ss = fa.stats(c64, EPS), fa.stats(s64, EPS)
    dt = DTYPE[kind]

    def one(alpha, want_stats, want_out=True, dev=False, w=""):
        G = Guards()
        out = G.new(tuple(c.shape), dt, C) if want_out else None
        st = G.new((2, C, 4), torch.float32, C * 4) if want_stats else None
        a_dev = torch.tensor([alpha], dtype=torch.float32, device="cuda") if dev else None
        _launch(kind, c, s, out, st, 0.25 if (dev and kind == "split") else alpha, a_dev)
        torch.cuda.synchronize()
        G.check(f"{what} {w}")
        return out, st

    # alpha 0.6 by value with statistics: everything is checked
    r = fail.run(f"{what} alpha 0.6", lambda: one(0.6, True, w="alpha 0.6"))
    if r is None:
        return
    out6, st6 = r
    for tag, sref, j in (("content", sc, 0), ("style", ss, 2)):
        rel = (st6[..., j + 1].double() ** 2 - sref["vpe"]).abs() / sref["vpe"]
        for r_ in fa.REGIMES:
            BY_REGIME[(kind, r_)] = max(BY_REGIME.get((kind, r_), 0.0), float(rel[:, fa.channels_of(r_, C)].max()))
        m = fail.run(f"{what} {tag} statistics", lambda: fa.check_stats(st6[..., j], st6[..., j + 1], sref, f"{what} {tag}"))
        if m:
            _note(kind, "mean error / bar", m[0], m[0], f"{what} {tag}")
            _note(kind, "std^2 error / bar", m[1], m[1], f"{what} {tag}")
            _note(kind, "relative error of std^2", m[2], 0.0)
    for r_ in "ef":         # constant channels: the sums about the pivot are exactly zero, std^2 = eps up to the rounding of std
        cs = fa.channels_of(r_, C)
        e = ((st6[:, cs, 1].double() ** 2 - sc["vpe"][:, cs]).abs() / sc["vpe"][:, cs]).max()
        if float(e) > 2.01 * fa.U32:
            fail.items.append(f"{what}: constant regime {r_}: std^2 off by {float(e):.3g} relative, the sums are exact there")
    if kind in ("bf16", "fp16"):     # regime d quantises to a few values of the 16-bit type: exact sums there as well
        cs = fa.channels_of("d", C)
        e = ((st6[:, cs, 1].double() ** 2 - sc["vpe"][:, cs]).abs() / sc["vpe"][:, cs]).max()
        if float(e) > 2.01 * fa.U32:
            fail.items.append(f"{what}: regime d in {kind}: std^2 off by {float(e):.3g} relative, the sums are exact there")

    def check_out(out, alpha, w):
        ref, absref, extra = fa.out_ref(c64, sc, ss, alpha)
        t = fail.run(f"{what} {w} out", lambda: fa.check_out(_values(kind, out), ref, absref, extra, OUT_T[kind], f"{what} {w} out"))
        if t:
            _note(kind, "out tau over absref", t[0], t[0] / fa.TAU_OUT, f"{what} {w}")
            _note(kind, "out error / bar", t[1], t[1], f"{what} {w}")

    check_out(out6, 0.6, "alpha 0.6")
    # alpha 1 without statistics
    r = fail.run(f"{what} alpha 1", lambda: one(1.0, False, w="alpha 1"))
    out1 = r[0] if r else None
    if out1 is not None:
        check_out(out1, 1.0, "alpha 1")
    # alpha 0: the content, bit for bit
    r = fail.run(f"{what} alpha 0", lambda: one(0.0, True, w="alpha 0"))
    out0 = r[0] if r else None
    if out0 is not None:
        if not torch.equal(out0.view(torch.uint8), c.view(torch.uint8)):
            fail.items.append(f"{what} alpha 0: the output differs from the content in {int((out0 != c).sum())} elements")
        if not torch.equal(r[1], st6):
            fail.items.append(f"{what} alpha 0: the statistics differ from those of the alpha 0.6 launch")
    # the blend factor as a device scalar: the same arithmetic, the same bits
    for alpha, by_value in ((0.6, out6), (1.0, out1), (0.0, out0)):
        r = fail.run(f"{what} device alpha {alpha}", lambda: one(alpha, alpha == 0.6, dev=True, w=f"device alpha {alpha}"))
        if r is None or by_value is None:
            continue
        if not torch.equal(r[0].view(torch.uint8), by_value.view(torch.uint8)):
            fail.items.append(f"{what} device alpha {alpha}: the output differs from the by-value launch")
        if r[1] is not None and not torch.equal(r[1], st6):
            fail.items.append(f"{what} device alpha {alpha}: the statistics differ from the by-value launch")
    # statistics only
    r = fail.run(f"{what} stats only", lambda: one(0.6, True, want_out=False, w="stats only"))
    if r is not None and not torch.equal(r[1], st6):
        fail.items.append(f"{what} out == NULL: the statistics differ from those of the full launch")
    # the wrapper
    def wrapper():
        o, st = ops.adain(c, s, alpha=0.6, eps=EPS, want_stats=True)
        assert torch.equal(o.view(torch.uint8), out6.view(torch.uint8)) and torch.equal(st, st6), f"{what}: ops.adain differs from the direct call"
        st = ops.adain(c, s, eps=EPS, stats_only=True)
        assert torch.equal(st, st6), f"{what}: ops.adain(stats_only) differs from the direct call"
        if out1 is not None:
            a = torch.tensor([1.0], device="cuda")
            assert torch.equal(ops.adain(c, s, alpha=a, eps=EPS).view(torch.uint8), out1.view(torch.uint8)), f"{what}: ops.adain(device alpha) differs"
    fail.run(f"{what} ops.adain", wrapper)


@pytest.mark.parametrize("kind", KINDS)
def test_forms(kind):
    t0 = time.time()
    fail = Failures()
    for HWc, HWs, C in CASES:
        _run_case(kind, HWc, HWs, C, fail)
    _report(kind, t0)
    fail.assert_none()


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_write_nothing(kind):
    """HW < 2 and C % 64 != 0: the argument error, returned before any launch; outputs and statistics stay 0xFF."""
    fail = Failures()
    for HWc, HWs, C in ((1, 130, 64), (130, 1, 64), (130, 130, 96)):
        c, _ = _stored(_raw(HWc, C if C % 8 == 0 else 64, 3), kind)
        s, _ = _stored(_raw(HWs, C if C % 8 == 0 else 64, 4), kind)
        for dev in (False, True):
            G = Guards()
            out = G.new(tuple(c.shape), DTYPE[kind], C)
            st = G.new((2, C, 4), torch.float32, C * 4)
            a_dev = torch.tensor([0.6], device="cuda") if dev else None
            what = f"{kind} HWc {HWc} HWs {HWs} C {C} device alpha {int(dev)}"
            try:
                _launch(kind, c, s, out, st, 0.6, a_dev)
                fail.items.append(f"{what}: accepted")
            except RuntimeError as e:
                if "error -1" not in str(e):
                    fail.items.append(f"{what}: {e}")
            torch.cuda.synchronize()
            if not (bool((out.view(torch.uint8) == 0xFF).all()) and bool((st.view(torch.uint8) == 0xFF).all())):
                fail.items.append(f"{what}: a refused call wrote to its outputs")
            fail.run(what, lambda: G.check(what))
    fail.assert_none()


def test_torch_var_on_the_same_tensors():
    """What torch's own fp32 var does on this module's content tensors, against float64, per value regime: the accuracy of the implementation
    the library is modelled on.  Printed for comparison with the kernel's figures; asserted only where the regime is well conditioned (a, h,
    i: at most 1e-6) - the device's fp32 Welford update loses about mean / std * 2^-24 (measured 7e-4 in regime d), the bars here do not."""
    worst = {r: 0.0 for r in fa.REGIMES}
    for HWc, _, C in CASES:
        x = _raw(HWc, C, 11 * HWc + C)
        v64 = x.double().var(1, unbiased=True)
        rel = (x.var(1, unbiased=True).double() - v64).abs() / v64.clamp(min=1e-300)
        for r in fa.REGIMES:
            cs = fa.channels_of(r, C)
            nz = v64[:, cs] > 0
            if bool(nz.any()):
                worst[r] = max(worst[r], float(rel[:, cs][nz].max()))
    print("\n[adain] torch fp32 var against float64 on the content tensors of this module, worst relative error per regime: " +
          " ".join(f"{r}:{v:.2g}" for r, v in worst.items()))
    assert max(worst[r] for r in "ahi") <= 1e-6, worst
