"""Every BatchNorm and max-pool kernel form against the float64 references of tests/helpers/fp64_bn.py, element by element
(helpers.fp64_conv.check()), in the bf16 and fp16 builds, through the entry points that take the form selectors as arguments and
return the form that ran (udapose_bn_train_fwd_ex, udapose_bn_bwd_ex, udapose_bn_bwd_pre_ex, udapose_maxpool3x3s2_fwd_ex, ...).

Every output is a view inside a larger allocation filled with 0xFF bytes (NaN in every float type) with at least one pixel row, and at
least 256 bytes, of guard on each side: the guards must come back untouched, and an element the kernel never wrote reads as NaN.

Launchers of the BatchNorm / pooling section of csrc/pointwise.hip (and adain_train.hip's pool backward) and the case that runs each:
  pw_bn_finalize (bn_finalize_k, slab_colsum's 8- / 4- / 1-row loops, pre_bias, count == 1, clamp) ...... test_finalize_forms
  pw_bn_train_fused (bn_apply_chunk_k<elem, elem>), pw_bn_train_fused_split (<float, sp32>, and <float, sp32, true> in the fp16
    build): preludes at rows 1..128, policy values 1 / 64 / 4096, XCD remap on and off, fall-backs ......... test_apply_chunked_forms
  pw_bn_apply (bn_apply_k<elem>), pw_bn_apply_f32 (<float>), pw_bn_apply_split (<sp32, float> and the 'strict' <sp32, float, true>):
    G = 1, 3, 8, 256, looping threads, mask, XCD rows engaged / refused ...................................... test_apply_streaming_forms
  pw_bn_bwd: bn_bwd_reduce_k / bn_bwd_finalize_k / bn_bwd_apply_k and bn_bwd_reduce_chunk_k / bn_bwd_apply_chunk_k, dz 16-bit and
    fp32, relu 0 / 1 / 2, gout, beta_acc; forced streaming; 32769 pixels falls back ........................... test_backward_forms
  pw_bn_bwd_pre: bn_bwd_apply_pre_chunk_k (rows 1..128, XCD bit 30), bn_bwd_apply_pre_k (XCD bit 29 on / off / refused), the legacy
    bn_bwd_apply_k form ........................................................................................ test_backward_pre_forms
  pw_bn_relu_maxpool3x3s2, pw_bn_bwd_pooled (bn_bwd_reduce_k / bn_bwd_apply_k<elem, true>) ..................... test_stem_forms
  pw_maxpool3x3s2_fwd / _fwd_f32 / _fwd_split (plain and 'strict'), pw_maxpool3x3s2_bwd (grid-stride loop included),
    pw_maxpool2x2_ceil / _f32 / _split, maxpool2x2_ceil_bwd .................................................... test_maxpool_forms
  pw_bn_eval_coeff ............................................................................................. test_eval_coeff
  pw_bn_running_update (bn_running_update_k), pw_bn_running_update_multi (bn_running_update_multi_k, what udapose_net_apply_running
    launches: a table of layers of different widths in one grid) ................................................ test_running_update
  pw_bn_bwd_rows sizes every backward slab here (guarded).

Bars (fp64_bn.tau_of): tau = rho = (L + 6) * 2^-24 plus half an ulp of the stored type, L = the longest sequential fp32 accumulation
chain: 0 for finalize, apply and the pre-reduced backward (fp64 sums); ceil(ppb / pstep) + pstep for the streaming reduce (largest at
C = 8, pstep = 256: L = 257, tau 1.6e-5); P / 32 + 32 for the chunked reduce (largest at 32768 x 2048: L = 64, tau 4.2e-6); 4 for the
3x3 pool backward.  Finalize outputs in fp32 ulps: mean, invstd, scale, unbiased variance <= 2; shift and the running statistics <= 3
ulps of the sum of their terms' magnitudes.  The f16x2 split storage counts as a 22-bit significand (fp64_conv.MANT["split"]); it has
no NaN and no infinity (it saturates at 65504 and counts the event), so the split pools run on finite maps only.

Worst measured (tau, rho) per form on an MI355X, both builds: see MEASURED below (printed against the bars by every run)."""
import math
import time

import pytest
import torch

from helpers import fp64_bn as fb
from helpers import fp64_conv as fc
from helpers.gpu_forms import Failures, Guards

pytestmark = pytest.mark.gpu

ELEM = {"bf16": torch.bfloat16, "fp16": torch.float16}
WORST = {}          # (form, output) -> [tau, rho, largest bar, unit, worst measured / own bar]
T_MODULE = [0.0]

# worst measured on an MI355X over this module (form output: tau / rho, or ulps)
MEASURED = """
tau (rho where it rises above the output rounding's norm), bar, and the worst measured / bar of any single check
  finalize (streaming and chunk prelude)   mean, invstd, unbiased variance 0.5 ulps (bar 2); scale 1.36 (bar 2); shift 2.15 (bar 3);
                                           running mean / variance 1.58 / 1.54 (bar 3); eval scale 1.4 (bar 3), eval shift 0.5 (bar 2)
  deferred running update (one layer, table) running mean / variance 1.45 / 1.3 ulps (bar 3)
  streaming apply   16-bit 8.86e-8, fp32 5.85e-8 (rho 6.2e-10), split / strict 2.95e-8     bar 3.58e-7   worst / bar 0.25
  chunked apply     16-bit 9.48e-8, split / strict 5.63e-8                                   bar 3.58e-7   worst / bar 0.27
  backward, streaming   dy 1.69e-7, dbeta 1.76e-7, dgamma 1.79e-7             bar 5.4e-7 .. 1.57e-5 by shape   worst / bar 0.22
  backward, chunked     dy 1.37e-7, dbeta 6.43e-8, dgamma 6.77e-8             bar 2.4e-6 .. 4.17e-6 by shape   worst / bar 0.04
  backward, pre-reduced dy 1.55e-7 (streaming) / 9.6e-8 (chunked, legacy), sums 5.7e-8      bar 3.58e-7   worst / bar 0.43
  stem   fused pool 7.5e-9 (bar 3.58e-7); bn_bwd_pooled dy 6.2e-8, sums 6.4e-8 (bar 2.32e-6)                worst / bar 0.03
  pools  values (split storage included), taps and the 2x2 backward exact; 3x3 backward exact up to the output rounding (bar 5.96e-7)
No tau comes within 2x of its bar (the worst, 0.43 of it, is the streaming pre-reduced dy).  The ulp figures of scale, shift and the running statistics do, because those bars are the exact
worst-case counts, with nothing left uncounted: scale = fp32(gamma * fp32(invstd)) is off by at most 0.5 ulp of its own rounding plus the
rounding of invstd, which is worth up to 1 ulp of scale when invstd sits low in its binade and scale high in its own (1.5 in all);
shift = beta - fp32(mean) * scale adds the rounding of mean, of the product and of the difference (3 in all); a running statistic carries the
rounding of 1 - momentum, of the saved value, of two products and of the sum (3 in all)."""


def _ops():
    from uda_poseestimation_amd import ops, _hip
    return ops, _hip


def _note(form, out, tr, bar, unit="tau"):
    w = WORST.setdefault((form, out), [0.0, 0.0, bar, unit, 0.0])
    t, r = tr if isinstance(tr, tuple) else (tr, 0.0)
    w[0], w[1], w[2], w[4] = max(w[0], t), max(w[1], r), max(w[2], bar), max(w[4], max(t, r) / bar)


def _report(part, t0):
    print(f"\n[{part}] wall {time.time() - t0:.1f} s; worst measured, the largest bar of the form, and the worst measured / bar of any one check:")
    for (form, out), (t, r, bar, unit, ratio) in sorted(WORST.items()):
        if not form.startswith(part):
            continue
        if unit == "ulps":
            print(f"  {form:28s} {out:14s} {t:.3g} ulps (bar {bar:g})")
        else:
            print(f"  {form:28s} {out:14s} tau {t:.3g}  rho {r:.3g}  (bar {bar:.3g}; worst / own bar {ratio:.2f})")


@pytest.fixture(scope="module", autouse=True)
def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from uda_poseestimation_amd import _hip
    _hip.lib("bf16"), _hip.lib("fp16")
    T_MODULE[0] = time.time()
    yield
    print(f"\n[bn / pool forms] module wall time {time.time() - T_MODULE[0]:.1f} s")


@pytest.fixture(autouse=True)
def _device_still_sound():
    """Nothing is started on a device that an earlier test left in an error state."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reports an error before this test: {e}", returncode=3)
    yield


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(shape, g, scale=1.0, shift=0.0):
    return torch.randn(shape, device="cuda", generator=g) * scale + shift


# ---- forward ---------------------------------------------------------------------------------------------------------------------

def _xcd_ok(npix, C):
    """The launcher's condition for XCD-aligned rows in the streaming apply kernels (pw_bn_apply_xcd_ok)."""
    G = C // 8
    grid = min(2048, max(1, -(-npix * G // 256)))
    if 256 % G:
        grid = max(G, grid // G * G)
    return 256 % G == 0 and grid % 8 == 0 and npix >= 8 * (256 // G)


def _takes_fwd_chunk(kind, npix, C, rows, policy, pre_bias):
    return kind != "f32" and not pre_bias and policy != 0 and C >= 256 and C % 64 == 0 and 1024 <= npix <= 8192 and rows <= 128


def _slab_of(y64, rows):
    """[rows][2][C] fp32 partial sums (sum, sum of squares) of y [npix, C] over `rows` pixel ranges."""
    npix, C = y64.shape
    rid = torch.arange(npix, device=y64.device) * rows // npix
    s = torch.zeros(rows, 2, C, dtype=torch.float64, device=y64.device)
    s[:, 0].index_add_(0, rid, y64)
    s[:, 1].index_add_(0, rid, y64 * y64)
    return s.float()


def _synthetic_slab(rows, C, count, g):
    """A slab whose columns sum to count * mean and count * (var + mean^2) for drawn means and variances, spread over the rows with random
    weights; channel 0 constant with a sum of squares just below count * mean^2 (negative variance: the clamp, invstd = 1 / sqrt(eps));
    channel 1 with its mean 64 standard deviations from zero."""
    mu = _randn((C,), g, 0.5, 0.2).double()
    var = (torch.rand(C, device="cuda", generator=g) + 0.5).double()
    mu[1], var[1] = 64.0, 1.0
    w = torch.rand(rows, C, device="cuda", generator=g).double() + 0.1
    w = w / w.sum(0)
    slab = torch.stack([w * (count * mu), w * (count * (var + mu * mu))], 1).float()
    k = torch.full((rows,), math.floor(count * 64 / rows) / 64, dtype=torch.float64, device="cuda")
    k[0] += count - float(k.sum())
    slab[:, 0, 0] = (0.5 * k).float()
    slab[:, 1, 0] = (0.25 * k * (1 - 2.0 ** -20)).float()
    s = slab[:, :, 0].double().sum(0)
    assert float(s[1] / count - (s[0] / count) ** 2) < 0, "the constant channel's variance must come out negative, or the clamp is not run"
    return slab


class Fwd:
    """Operands of one forward case in every storage kind, and one run of udapose_bn_train_fwd_ex with all its checks."""

    def __init__(self, npix, C, seed):
        g = _gen(seed)
        self.npix, self.C = npix, C
        self.y32 = _randn((npix, C), g, 1.5, 0.3)
        self.res32 = _randn((npix, C), g)
        self.gamma = torch.rand(C, device="cuda", generator=g) + 0.5
        self.beta = _randn((C,), g, 0.3)
        self.pre_bias = _randn((C,), g, 0.5)
        self.rm0 = _randn((C,), g)
        self.rv0 = torch.rand(C, device="cuda", generator=g) + 0.5
        self._st = {}

    def stored(self, kind, dt):
        """(y, res, y as float64, res as float64) in the storage of `kind`."""
        key = (kind, dt if kind == "16bit" else None)
        if key not in self._st:
            ops, _ = _ops()
            if kind == "16bit":
                y, res = self.y32.to(dt), self.res32.to(dt)
                self._st[key] = (y, res, y.double(), res.double())
            elif kind == "f32":
                self._st[key] = (self.y32, self.res32, self.y32.double(), self.res32.double())
            else:
                rs = ops.f32_to_split(self.res32)
                self._st[key] = (self.y32, rs, self.y32.double(), ops.split_to_f32(rs).double())
        return self._st[key]

    def run(self, build, kind, slab, res, relu, policy, xcd_rows, want_mask, pre_bias, fail, what, form="fwd", full=True):
        """One launch.  full: every per-element check; otherwise only the guards, the form code and the raw outputs (for bit comparisons)."""
        ops, _ = _ops()
        dt = ELEM[build]
        npix, C = self.npix, self.C
        y, rs, y64, r64 = self.stored(kind, dt)
        G = Guards()
        zdt = {"16bit": dt, "f32": torch.float32}.get(kind, torch.int32)
        z = G.new((npix, C), zdt, C)
        scale, shift = G.new((C,), torch.float32, C), G.new((C,), torch.float32, C)
        save = G.new((3, C), torch.float32, C)
        rm, rv = G.new((C,), torch.float32, C, self.rm0), G.new((C,), torch.float32, C, self.rv0)
        nbt = G.new((1,), torch.int64, 1, torch.tensor([7]))
        mask = G.new((npix * C // 8,), torch.uint8, C // 8) if want_mask else None
        y16 = G.new((npix, C), torch.float16, C) if kind == "strict" else None
        z16 = G.new((npix, C), torch.float16, C) if kind == "strict" else None
        pb = self.pre_bias if pre_bias else None
        code = ops.bn_train_fwd_ex(kind, y, z, slab, self.gamma, self.beta, scale, shift, save, res=rs if res else None, pre_bias=pb, running_mean=rm,
                                   running_var=rv, nbt=nbt, momentum=0.1, eps=1e-5, relu=relu, fwd_chunked=policy, xcd_rows=xcd_rows, mask=mask, y16=y16,
                                   z16=z16, build=build)
        G.check(what)
        rows = slab.shape[0]
        chunk = _takes_fwd_chunk(kind, npix, C, rows, policy, pre_bias)
        want = (1 | (2 if xcd_rows else 0)) if chunk else (2 if (xcd_rows >= 2 and kind in ("16bit", "strict") and _xcd_ok(npix, C)) else 0)
        assert code == want, f"{what}: form code {code}, expected {want}"
        out = {"code": code, "z": z, "mask": mask, "save": save, "rm": rm, "rv": rv}
        if not full:
            return out
        fin = fb.finalize(slab, npix, self.gamma, self.beta, pb, 0.1, 1e-5, self.rm0, self.rv0)
        pre = f"{form} finalize" if not chunk else f"{form} prelude"
        names = [("mean", save[0], 2), ("invstd", save[1], 2), ("unbiased_var", save[2], 2), ("running_mean", rm, 3), ("running_var", rv, 3)]
        if not chunk:
            names += [("scale", scale, 2), ("shift", shift, 3)]
        for name, got, bar in names:
            u = fail.run(f"{what} {name}", lambda: fb.check_ulps(got, *fin[name], bar, f"{what} {name}"))
            if u is not None:
                _note(pre, name, u, bar, "ulps")
        if int(nbt) != 8:
            fail.items.append(f"{what}: num_batches_tracked went from 7 to {int(nbt)}")
        tau = fb.tau_of(0)
        if chunk:       # scale / shift stay in LDS: the apply is held to the device's saved mean and invstd
            sc = self.gamma.double() * save[1].double()
            ms = save[0].double() * sc
            ref = y64 * sc + (self.beta.double() - ms)
            absref = (y64 * sc).abs() + self.beta.double().abs() + ms.abs()
            if res:
                ref, absref = ref + r64, absref + r64.abs()
            ref = torch.relu(ref) if relu else ref
        else:
            ref, absref = fb.apply(y64, scale, shift, r64 if res else None, relu)
        zf = ops.split_to_f32(z) if zdt == torch.int32 else z
        odt = "split" if zdt == torch.int32 else zdt
        tr = fail.run(f"{what} z", lambda: fc.check(zf, ref, absref, odt, tau, tau, f"{what} z"))
        if tr:
            _note(f"{form} apply {kind}", "z", tr, tau)
        if kind == "strict":
            fail.run(f"{what} y16", lambda: fb.check_exact(y16, y.to(torch.float16), f"{what} y16 == fp16(y)"))
            fail.run(f"{what} z16", lambda: fb.check_exact(z16, fb.split_h(z), f"{what} z16 == h half of z"))
        if want_mask:
            stored = z16 if kind == "strict" else z
            fail.run(f"{what} mask", lambda: fb.check_exact(fb.mask_bits(mask, C), stored > 0, f"{what} mask == stored z > 0"))
        return out


def _kinds(build):
    return ("16bit", "f32", "split") + (("strict",) if build == "fp16" else ())


def test_strict_kind_is_refused_by_the_bf16_build():
    ops, _ = _ops()
    c = Fwd(8, 8, 1)
    t = torch.empty(8, 8, dtype=torch.float16, device="cuda")
    f = torch.empty(3, 8, device="cuda")
    with pytest.raises(RuntimeError, match="error -3"):
        ops.bn_train_fwd_ex("strict", c.y32, torch.empty(8, 8, dtype=torch.int32, device="cuda"), _slab_of(c.y32.double(), 1), c.gamma, c.beta, f[0],
                            f[1], f, y16=t, z16=t.clone(), build="bf16")
    with pytest.raises(RuntimeError, match="error -3"):
        ops.maxpool3x3s2_fwd_ex("strict", torch.zeros(1, 2, 2, 8, dtype=torch.int32, device="cuda"), torch.zeros(1, 1, 1, 8, dtype=torch.int32, device="cuda"),
                                None, y16=t, build="bf16")


def test_finalize_forms():
    """bn_finalize_k over C x slab rows (the 8-, 4- and 1-row loops of slab_colsum at 32 row lanes), synthetic slabs with a clamped constant
    channel and a channel 64 sigma from zero, pre_bias on every other case, count == 1, num_batches_tracked + 1; the apply behind it on 33
    pixels."""
    t0 = time.time()
    fail = Failures()
    for build in ELEM:
        for C in (8, 24, 64, 2048):
            case = Fwd(33, C, C)
            for i, rows in enumerate((1, 31, 33, 97, 128, 129, 225, 256, 257, 700, 1024)):
                slab = _synthetic_slab(rows, C, 33, _gen(rows + C))
                what = f"finalize {build} C {C} rows {rows}"
                fail.run(what, lambda: case.run(build, "16bit", slab, True, True, 1, 1, False, bool(i & 1), fail, what))
        for C, rows in ((8, 33), (64, 1), (2048, 129)):
            one = Fwd(1, C, C + 1)
            slab = _synthetic_slab(rows, C, 1, _gen(rows))
            for kind in _kinds(build):
                what = f"finalize {build} {kind} count 1 C {C} rows {rows}"
                fail.run(what, lambda: one.run(build, kind, slab, False, False, 1, 2, False, kind == "f32", fail, what))
    _report("fwd", t0)
    fail.assert_none()


def test_apply_streaming_forms():
    """bn_apply_k in its four instantiations: C = 8 (G = 1), 24 (G = 3: the grid is rounded), 64, 2048 (G = 256 = the block); 1 .. 66049 pixels
    (at 66049 x 64 the 2048-block grid is exceeded and threads loop; the XCD mapping is engaged there with a partial last eighth, at 1000 x
    64 with exact eighths, and is refused at 1031 x 64, 66049 x 8, every C = 24).  residual x ReLU are checked per element with the mask and
    the XCD request on; the mask-off and XCD-off launches must give the same bits."""
    t0 = time.time()
    fail = Failures()
    seen = set()
    for C in (8, 24, 64, 2048):
        for npix in (1, 33, 1000, 1031, 66049):
            case = Fwd(npix, C, npix + C)
            slabs = {}
            for build in ELEM:
                for kind in _kinds(build):
                    y64 = case.stored(kind, ELEM[build])[2]
                    key = (kind, build if kind == "16bit" else "")
                    if key not in slabs:
                        slabs[key] = _slab_of(y64, min(npix, 97))
                    slab = slabs[key]
                    masked = kind in ("16bit", "strict")
                    for res in (True, False):
                        for relu in (True, False):
                            what = f"apply {build} {kind} {npix}x{C} res {int(res)} relu {int(relu)}"
                            a = fail.run(what, lambda: case.run(build, kind, slab, res, relu, 0, 2, masked, False, fail, what, form="stream"))
                            if a is None:
                                continue
                            seen.add((a["code"], npix, C))
                            for xcd, m in ((1, masked), (2, False), (1, False)):
                                w2 = f"{what} xcd_rows {xcd} mask {int(m)}"
                                b = fail.run(w2, lambda: case.run(build, kind, slab, res, relu, 0, xcd, m, False, fail, w2, full=False))
                                if b is None:
                                    continue
                                if not torch.equal(a["z"], b["z"]) or (m and not torch.equal(a["mask"], b["mask"])):
                                    fail.items.append(f"{w2}: bits differ from the launch with the mask and the XCD request")
            del case, slabs
            torch.cuda.empty_cache()
    _report("stream", t0)
    assert (2, 66049, 64) in seen and (2, 1000, 64) in seen and (0, 1031, 64) in seen and (0, 66049, 8) in seen, sorted(seen)
    fail.assert_none()


def test_apply_chunked_forms():
    """bn_apply_chunk_k (finalize + apply in one launch) in its three instantiations: preludes at slab rows 1 .. 128 (the 64-, 32- and 8-row
    loops), each on the slab of y and on a synthetic slab with a constant channel (variance clamp, invstd = 1 / sqrt(eps)) and a channel
    with its mean at 64 sigma; shapes with ragged pixel ranges, policy values 1 / 64 / 4096 (work-group counts), XCD remap on and off; and the fall-backs to
    finalize + apply (form code 0) at 1023 and 8193 pixels, 129 rows, C = 192 and 288, policy 0, the fp32 kind, pre_bias."""
    t0 = time.time()
    fail = Failures()
    for build in ELEM:
        dt = ELEM[build]
        kinds = [k for k in _kinds(build) if k != "f32"]
        case = Fwd(1024, 256, 5)
        for rows in (1, 7, 8, 9, 25, 32, 33, 57, 64, 65, 127, 128):
            for kind in kinds:
                slab = _slab_of(case.stored(kind, dt)[2], rows)
                what = f"chunk prelude {build} {kind} rows {rows}"
                fail.run(what, lambda: case.run(build, kind, slab, True, True, 1, 1, kind != "split", False, fail, what, form="chunk"))
                # the kernel's own finalize on a slab with a clamped constant channel and a channel 64 sigma from zero (the apply is held to
                # the device's saved mean and invstd, so y need not be what the slab was summed from)
                syn = _synthetic_slab(rows, 256, 1024, _gen(rows + 256))
                what = f"chunk prelude {build} {kind} rows {rows} synthetic slab"
                fail.run(what, lambda: case.run(build, kind, syn, False, False, 1, 0, False, False, fail, what, form="chunk"))
        for npix, C in ((1024, 256), (1031, 320), (1200, 512), (8192, 256), (4100, 2048)):
            case = Fwd(npix, C, npix + C)
            for kind in kinds:
                slab = _slab_of(case.stored(kind, dt)[2], 37)
                for policy in (1, 64, 4096):
                    for res, relu in ((True, True), (False, False)):
                        what = f"chunk {build} {kind} {npix}x{C} policy {policy} res {int(res)} relu {int(relu)}"
                        a = fail.run(what, lambda: case.run(build, kind, slab, res, relu, policy, 1, kind != "split", False, fail, what, form="chunk"))
                        w2 = what + " xcd off"
                        b = fail.run(w2, lambda: case.run(build, kind, slab, res, relu, policy, 0, False, False, fail, w2, full=False))
                        if a and b and not (torch.equal(a["z"], b["z"]) and torch.equal(a["save"], b["save"]) and torch.equal(a["rm"], b["rm"])):
                            fail.items.append(f"{w2}: bits differ from the XCD-mapped launch")
        for npix, C, rows, policy, kind, pb in ((1023, 256, 37, 1, "16bit", False), (8193, 256, 37, 1, "16bit", False), (1024, 256, 129, 1, "16bit", False),
                                               (1200, 192, 37, 1, "16bit", False), (1200, 288, 37, 1, "16bit", False), (1200, 256, 37, 0, "16bit", False),
                                               (1200, 256, 37, 1, "f32", False), (1200, 256, 37, 1, "16bit", True), (1023, 256, 37, 1, "split", False),
                                               (1024, 256, 129, 64, "split", False)):
            case = Fwd(npix, C, npix + C + rows)
            slab = _slab_of(case.stored(kind, dt)[2], rows)
            what = f"chunk fall-back {build} {kind} {npix}x{C} rows {rows} policy {policy} pre_bias {int(pb)}"
            a = fail.run(what, lambda: case.run(build, kind, slab, True, True, policy, 1, kind == "16bit", pb, fail, what, form="stream"))
            if a and a["code"] & 1:
                fail.items.append(f"{what}: the chunked form took it")
    _report("chunk", t0)
    fail.assert_none()


def test_eval_coeff():
    """bn_eval_coeff_k: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale, in fp32 ulps."""
    ops, _hip = _ops()
    for C in (8, 24, 2048):
        c = Fwd(1, C, C)
        G = Guards()
        scale, shift = G.new((C,), torch.float32, C), G.new((C,), torch.float32, C)
        _hip.check(_hip.lib().udapose_bn_eval_coeff(_hip.stream(), C, _hip.ptr(c.gamma), _hip.ptr(c.beta), _hip.ptr(c.rm0), _hip.ptr(c.rv0), 1e-5,
                                                    _hip.ptr(scale), _hip.ptr(shift)), "bn_eval_coeff")
        G.check(f"eval_coeff C {C}")
        eps = float(torch.tensor(1e-5, dtype=torch.float32))
        sc = c.gamma.double() / torch.sqrt(c.rv0.double() + eps)
        _note("fwd eval_coeff", "scale", fb.check_ulps(scale, sc, sc, 3, "eval scale"), 3, "ulps")       # (add, sqrt, divide: one rounding each)
        sh = c.beta.double() - c.rm0.double() * scale.double()
        _note("fwd eval_coeff", "shift", fb.check_ulps(shift, sh, c.beta.double().abs() + (c.rm0.double() * scale.double()).abs(), 2, "eval shift"), 2, "ulps")
    _report("fwd eval_coeff", time.time())


def test_running_update():
    """The deferred running-statistics update, bn_running_update_k and bn_running_update_multi_k (one grid over a table of layers of widths
    8, 24, 2048 and 264, max_c 2048: the blocks past a layer's width must write nothing): running = (1 - momentum) * running + momentum * saved
    within 3 fp32 ulps of the sum of the terms' magnitudes (the rounding of 1 - momentum, of two products and of the sum), the counter + 1
    exactly once per layer, the saved statistics and the guards untouched."""
    import struct
    _, _hip = _ops()
    t0 = time.time()
    fail = Failures()
    m = 0.1
    m64 = float(torch.tensor(m, dtype=torch.float32))
    widths = (8, 24, 2048, 264)

    def ref(old, new):
        return (1 - m64) * old.double() + m64 * new.double(), ((1 - m64) * old.double()).abs() + (m64 * new.double()).abs()

    def check(what, C, save, rm0, rv0, rm, rv, nbt):
        for name, got, old, new in (("running_mean", rm, rm0, save[0]), ("running_var", rv, rv0, save[2])):
            u = fail.run(f"{what} {name}", lambda: fb.check_ulps(got, *ref(old, new), 3, f"{what} {name}"))
            if u is not None:
                _note("fwd running update", name, u, 3, "ulps")
        if int(nbt) != 8:
            fail.items.append(f"{what}: num_batches_tracked went from 7 to {int(nbt)}")

    for build in ELEM:
        L = _hip.lib(build)
        layers = []
        for C in widths:
            g = _gen(C)
            save = torch.stack([_randn((C,), g, 0.5, 0.2), torch.rand(C, device="cuda", generator=g) + 0.5, torch.rand(C, device="cuda", generator=g) + 0.5])
            layers.append((C, save, _randn((C,), g), torch.rand(C, device="cuda", generator=g) + 0.5))
        for C, save, rm0, rv0 in layers:
            G = Guards()
            rm, rv, nbt = G.new((C,), torch.float32, C, rm0), G.new((C,), torch.float32, C, rv0), G.new((1,), torch.int64, 1, torch.tensor([7]))
            what = f"running update {build} C {C}"
            fail.run(what, lambda: _hip.check(L.udapose_bn_running_update(_hip.stream(), _hip.ptr(save), C, _hip.ptr(rm), _hip.ptr(rv), _hip.ptr(nbt), m), what))
            fail.run(what, lambda: G.check(what))
            check(what, C, save, rm0, rv0, rm, rv, nbt)
        # every layer in one launch: the saved statistics sit in one arena at 256-byte offsets, as the executor's do
        G = Guards()
        offs, total = [], 0
        for C, *_ in layers:
            offs.append(total)
            total += -(-3 * C * 4 // 256) * 256
        act = G.new((total,), torch.uint8, 256)
        outs, table = [], b""
        for (C, save, rm0, rv0), off in zip(layers, offs):
            act[off:off + 3 * C * 4].view(torch.float32).view(3, C).copy_(save)
            rm, rv, nbt = G.new((C,), torch.float32, C, rm0), G.new((C,), torch.float32, C, rv0), G.new((1,), torch.int64, 1, torch.tensor([7]))
            outs.append((rm, rv, nbt))
            table += struct.pack("<QQQQii", off, rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), C, 0)     # (size_t, three pointers, int C, int pad)
        jobs = torch.frombuffer(bytearray(table), dtype=torch.uint8).cuda()
        what = f"running update multi {build}"
        fail.run(what, lambda: _hip.check(L.udapose_bn_running_update_multi(_hip.stream(), _hip.ptr(jobs), len(layers), max(widths), _hip.ptr(act), m), what))
        torch.cuda.synchronize()
        for (C, save, rm0, rv0), off, (rm, rv, nbt) in zip(layers, offs, outs):
            if not torch.equal(act[off:off + 3 * C * 4].view(torch.float32).view(3, C), save):
                fail.items.append(f"{what}: the saved statistics of the layer of width {C} changed")
            check(f"{what} C {C}", C, save, rm0, rv0, rm, rv, nbt)
        fail.run(what, lambda: G.check(what))
    _report("fwd running update", t0)
    fail.assert_none()


# ---- backward --------------------------------------------------------------------------------------------------------------------

class Bwd:
    def __init__(self, npix, C, dt, seed):
        g = _gen(seed)
        self.npix, self.C, self.dt = npix, C, dt
        self.y = _randn((npix, C), g, 1.5, 0.3).to(dt)
        self.mean = _randn((C,), g, 0.2, 0.3)
        self.invstd = torch.rand(C, device="cuda", generator=g) * 0.5 + 0.4
        self.gamma = torch.rand(C, device="cuda", generator=g) + 0.5
        self.beta = _randn((C,), g, 0.3)
        self.zero = torch.zeros(npix, C, dtype=torch.bool, device="cuda")
        pix = torch.tensor(sorted({0, npix // 3, npix // 2, npix - 1}), device="cuda")
        self.plant_zero(0, pix)
        self.plant_zero(C - 1, pix)
        sc = self.gamma * self.invstd
        self.z = torch.relu(self.y.float() * sc + (self.beta - self.mean * sc) + _randn((npix, C), g)).to(dt)       # (any stored z serves as a mask source)
        dz = _randn((npix, C), g, 1.0, 0.5)                   # (a mean of 0.5: the sums do not cancel, so a wrong S / M shows in dy)
        self.dz = {"f32": torch.where(dz == 0, torch.ones_like(dz), dz)}
        d16 = dz.to(dt)
        self.dz["16bit"] = torch.where(d16 == 0, torch.ones_like(d16), d16)
        self.old = (_randn((C,), g), _randn((C,), g))

    def plant_zero(self, ch, pix=None):
        """Channel ch gets mean 0.5, invstd 2, gamma 1, beta 0, and y = 0.5 at the pixels pix (everywhere when None).  There sc = 2, sh = -1 and
        y * sc + sh is exactly 0 in fp32, fused or not: the relu == 2 test is strictly > 0, so these elements are masked out."""
        self.mean[ch], self.invstd[ch], self.gamma[ch], self.beta[ch] = 0.5, 2.0, 1.0, 0.0
        sel = slice(None) if pix is None else pix
        self.y[sel, ch] = 0.5
        self.zero[sel, ch] = True


def _run_bwd(case, dzk, relu, gout_on, beta_acc, chunked, fail, what):
    ops, _hip = _ops()
    npix, C, dt = case.npix, case.C, case.dt
    G = Guards()
    dy = G.new((npix, C), dt, C)
    gout = G.new((npix, C), dt, C) if gout_on else None
    rows = _hip.lib().udapose_bn_bwd_rows(npix)
    slab, coef = G.new((rows, 2, C), torch.float32, 2 * C), G.new((3, C), torch.float32, C)
    dgamma, dbeta = G.new((C,), torch.float32, C, case.old[0]), G.new((C,), torch.float32, C, case.old[1])
    code = ops.bn_bwd_ex(case.dz[dzk], case.z if relu == 1 else None, case.y, dy, case.gamma, case.mean, case.invstd, slab, coef, dgamma, dbeta, relu=relu,
                         gout=gout, beta=case.beta if relu == 2 else None, beta_acc=beta_acc, chunked=chunked)
    G.check(what)
    want = int(bool(chunked) and C >= 256 and 1024 <= npix <= 32768)
    assert code == want, f"{what}: form code {code}, expected {want}"
    return dy, gout, dgamma, dbeta


def _backward_case(build, npix, C, chunked, fail, form):
    case = Bwd(npix, C, ELEM[build], npix + C)
    dt = case.dt
    taken = bool(chunked) and C >= 256 and 1024 <= npix <= 32768
    L = fb.chunk_chain(npix, C) if taken else fb.stream_chain(npix, C)
    tau = fb.tau_of(L)
    for dzk in ("16bit", "f32"):
        for relu in (0, 1, 2):
            what = f"{form} {build} {npix}x{C} chunked {chunked} dz {dzk} relu {relu}"
            r = fail.run(what, lambda: _run_bwd(case, dzk, relu, True, 0.0, chunked, fail, what))
            if r is None:
                continue
            dy, gout, dgamma, dbeta = r
            dz = case.dz[dzk]
            if relu == 2:
                keep, und = fb.relu_mask_from_y(case.y, case.mean, case.invstd, case.gamma, case.beta, gout)
                if und > 1e-3 * keep.numel():
                    fail.items.append(f"{what}: {und} undecided mask elements of {keep.numel()}")
                # the planted exact zeros: decided (masked) by the reference, and the device must have masked them (dz has no zeros)
                nz = int(case.zero.sum())
                if nz < 2 or bool(keep[case.zero].any()) or bool((gout[case.zero] != 0).any()):
                    fail.items.append(f"{what}: of {nz} planted exact zeros (y * sc + sh == 0) the reference keeps {int(keep[case.zero].sum())} and "
                                      f"the device passes {int((gout[case.zero] != 0).sum())} (the test is strictly > 0)")
            else:
                keep = (case.z > 0) if relu == 1 else None
            ref = fb.backward(dz, case.y, case.mean, case.invstd, case.gamma, keep)
            fail.run(what + " gout", lambda: fb.check_exact(gout, ref["g"].to(dt), what + " gout == mask * dz in the stored type"))
            tr = fail.run(f"{what} dy", lambda: fc.check(dy, *ref["dy"], dt, tau, tau, f"{what} dy"))
            if tr:
                _note(form, "dy", tr, tau)
            for name, got in (("dbeta", dbeta), ("dgamma", dgamma)):
                tr = fail.run(f"{what} {name}", lambda: fb.check_sums(got, *ref[name], tau, f"{what} {name}"))
                if tr:
                    _note(form, name, tr, tau)
            if dzk == "16bit":      # the sums of the device's own gout: a reduce and an apply that mask differently part here
                g64 = gout.double()
                for name, got, s, a in (("dbeta", dbeta, g64.sum(0), g64.abs().sum(0)),
                                        ("dgamma", dgamma, (g64 * ref["xhat"]).sum(0), (g64 * ref["xhat"]).abs().sum(0))):
                    fail.run(f"{what} {name} vs gout", lambda: fb.check_sums(got, s, a, tau, f"{what} {name} against the sums of gout"))
            for gout_on, acc in ((False, 0.0), (True, 0.5), (False, 0.5)):
                w2 = f"{what} gout {int(gout_on)} beta_acc {acc}"
                r2 = fail.run(w2, lambda: _run_bwd(case, dzk, relu, gout_on, acc, chunked, fail, w2))
                if r2 is None:
                    continue
                if not torch.equal(r2[0], dy) or (gout_on and not torch.equal(r2[1], gout)):
                    fail.items.append(f"{w2}: dy / gout bits differ from the launch with gout and beta_acc 0")
                if acc == 0.0:
                    if not (torch.equal(r2[2], dgamma) and torch.equal(r2[3], dbeta)):
                        fail.items.append(f"{w2}: dgamma / dbeta bits differ from the launch with gout")
                    continue
                for name, got, old in (("dgamma", r2[2], case.old[0]), ("dbeta", r2[3], case.old[1])):
                    s, a = ref[name]
                    tr = fail.run(f"{w2} {name}", lambda: fb.check_sums(got, 0.5 * old.double() + s, 0.5 * old.double().abs() + a, tau, f"{w2} {name}"))
                    if tr:
                        _note(form, name + " (acc)", tr, tau)
            del ref
    del case
    torch.cuda.empty_cache()


def test_backward_forms():
    """pw_bn_bwd.  Streaming (reduce / finalize / apply): C = 8, 64, 128, 2048 at 1, 31, 1031 pixels; C = 256 just under the chunked form's
    1024 pixels and at 40000 (slab rows capped at 1024); forced (chunked = 0) at 1200 x 256; 32769 pixels, just over its upper limit.
    Chunked: C = 256, 2048 at 1024, 1031, 1200, 32768 pixels."""
    t0 = time.time()
    fail = Failures()
    for build in ELEM:
        for C in (8, 64, 128, 2048):
            for npix in (1, 31, 1031):
                _backward_case(build, npix, C, 1, fail, "bwd stream")
        for npix, C, chunked in ((1023, 256, 1), (40000, 256, 1), (1200, 256, 0), (32769, 256, 1), (32769, 2048, 1)):
            _backward_case(build, npix, C, chunked, fail, "bwd stream")
        for C in (256, 2048):
            for npix in (1024, 1031, 1200, 32768):
                _backward_case(build, npix, C, 1, fail, "bwd chunk")
    _report("bwd", t0)
    fail.assert_none()


def _slab_of_g(g64, xhat, rows):
    npix, C = g64.shape
    rid = torch.arange(npix, device=g64.device) * rows // npix
    s = torch.zeros(rows, 2, C, dtype=torch.float64, device=g64.device)
    s[:, 0].index_add_(0, rid, g64)
    s[:, 1].index_add_(0, rid, g64 * xhat)
    return s.float()


def test_backward_pre_forms():
    """pw_bn_bwd_pre on an already masked gradient and its slab of partial sums: the chunked form at slab rows 1 .. 128 with the XCD remap
    (bit 30) on and off, 129 rows falling back; the streaming form with the XCD rows (bit 29) on - engaged at 1000 x 64 and 66049 x 64,
    refused at 1031 x 64 - and off; the legacy form; g 16-bit and fp32; beta_acc 0 and 0.5."""
    ops, _hip = _ops()
    t0 = time.time()
    fail = Failures()
    tau = fb.tau_of(0)
    seen = set()
    B29, B30 = 1 << 29, 1 << 30
    plan = [(1200, 256, rows, sel, 0) for rows in (1, 9, 57, 65, 128, 129) for sel in (1, 1 | B30, 64 | B30)]
    plan += [(npix, 64, 37, sel, 0) for npix in (1000, 1031, 66049) for sel in (1, 1 | B29)]
    plan += [(1200, 256, 37, 0, 0), (1200, 256, 37, B29, 0), (1031, 8, 5, 1 | B29, 0), (33, 2048, 3, 1 | B29, 0),
             (1200, 256, 129, 1, 1), (1031, 64, 37, 1 | B29, 1), (1200, 256, 37, 0, 1)]
    for build in ELEM:
        dt = ELEM[build]
        cases = {}
        for npix, C, rows, sel, legacy in plan:
            if (npix, C) not in cases:
                c = Bwd(npix, C, dt, npix + C + 1)
                c.xhat = (c.y.double() - c.mean.double()) * c.invstd.double()
                cases[(npix, C)] = c
            case = cases[(npix, C)]
            for gk in ("16bit", "f32"):
                g = torch.where(case.z > 0, case.dz[gk], torch.zeros_like(case.dz[gk]))
                slab = _slab_of_g(g.double(), case.xhat, rows)
                ref = fb.backward_pre(g, case.y, case.mean, case.invstd, case.gamma, slab)
                first = None
                for acc in (0.0, 0.5):
                    what = f"bwd pre {build} {npix}x{C} rows {rows} chunked {sel & ~(3 << 29)} bits {sel >> 29} legacy {legacy} g {gk} beta_acc {acc}"
                    G = Guards()
                    dy, coef = G.new((npix, C), dt, C), G.new((3, C), torch.float32, C)
                    dgamma, dbeta = G.new((C,), torch.float32, C, case.old[0]), G.new((C,), torch.float32, C, case.old[1])
                    code = fail.run(what, lambda: ops.bn_bwd_pre_ex(g, case.y, dy, case.gamma, case.mean, case.invstd, slab, coef, dgamma, dbeta,
                                                                    beta_acc=acc, chunked=sel, legacy=legacy))
                    if code is None:
                        continue
                    fail.run(what, lambda: G.check(what))
                    taken = bool(sel & ~(3 << 29)) and C >= 256 and 1024 <= npix <= 32768 and rows <= 128
                    want = (1 | (2 if sel & B30 else 0)) if taken else (2 if (sel & B29 and not legacy and _xcd_ok(npix, C)) else 0)
                    if code != want:
                        fail.items.append(f"{what}: form code {code}, expected {want}")
                    seen.add((code, npix, C, rows <= 128, legacy))
                    form = "bwd pre " + ("chunk" if taken else ("legacy" if legacy else "stream"))
                    if acc == 0.0:
                        first = dy
                        tr = fail.run(what + " dy", lambda: fc.check(dy, *ref["dy"], dt, tau, tau, what + " dy"))
                        if tr:
                            _note(form, "dy", tr, tau)
                    elif first is not None and not torch.equal(first, dy):
                        fail.items.append(f"{what}: dy bits differ from beta_acc 0")
                    for name, got, old in (("dgamma", dgamma, case.old[0]), ("dbeta", dbeta, case.old[1])):
                        s, a = ref[name]
                        tr = fail.run(f"{what} {name}", lambda: fb.check_sums(got, acc * old.double() + s, acc * old.double().abs() + a, tau, f"{what} {name}"))
                        if tr:
                            _note(form, name, tr, tau)
        del cases
        torch.cuda.empty_cache()
    _report("bwd pre", t0)
    for want in ((1, 1200, 256, True, 0), (3, 1200, 256, True, 0), (0, 1200, 256, False, 0), (2, 1000, 64, True, 0), (2, 66049, 64, True, 0),
                 (0, 1031, 64, True, 0), (0, 1200, 256, False, 1), (0, 1031, 64, True, 1)):
        assert want in seen, (want, sorted(seen))
    fail.assert_none()


# ---- stem ------------------------------------------------------------------------------------------------------------------------

def test_stem_forms():
    """bn_relu_maxpool3x3s2_k per element against fp64 and bit-equal to bn_apply_k followed by maxpool3x3s2_fwd_k; pw_bn_bwd_pooled per element
    against fp64 (on the gradient maxpool3x3s2_bwd_k leaves, itself checked in test_maxpool_forms) and bit-equal to maxpool3x3s2_bwd_k
    followed by the streaming bn_bwd with the mask recomputed from y.  One channel is all planted exact zeros (y * sc + sh == 0): its windows
    tie, the first in-range tap carries the gradient, and the strict > 0 mask must stop all of it."""
    ops, _hip = _ops()
    t0 = time.time()
    fail = Failures()
    C, N = 64, 3
    for build in ELEM:
        dt = ELEM[build]
        for H, W in ((8, 8), (7, 9), (9, 7), (16, 12)):
            what = f"stem {build} {N}x{H}x{W}x{C}"
            npix = N * H * W
            case = Bwd(npix, C, dt, H * W)
            case.plant_zero(1)      # a whole channel of exact zeros: z = 0 everywhere, so every window's first in-range tap wins and carries gradient
            Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            scale = case.gamma * case.invstd
            shift = case.beta - case.mean * scale
            y4 = case.y.reshape(N, H, W, C)
            G = Guards()
            p, idx = G.new((N, Ho, Wo, C), dt, Wo * C), G.new((N, Ho, Wo, C), torch.uint8, Wo * C)
            ops.bn_relu_maxpool3x3s2(y4, p, idx, scale, shift)
            z, p2, idx2 = G.new((npix, C), dt, C), G.new((N, Ho, Wo, C), dt, Wo * C), G.new((N, Ho, Wo, C), torch.uint8, Wo * C)
            save = torch.stack([case.mean, case.invstd])
            check = _hip.check
            check(_hip.lib(build).udapose_bn_apply(_hip.stream(), _hip.ptr(case.y), None, _hip.ptr(z), npix * C, C, _hip.ptr(scale), _hip.ptr(shift), 1), "bn_apply")
            ops.maxpool3x3s2_fwd_ex("16bit", z.reshape(N, H, W, C), p2, idx2)
            fail.run(what, lambda: G.check(what))
            fail.run(what + " pool", lambda: fb.check_exact(p, p2, what + ": fused pooled values against apply + max-pool"))
            fail.run(what + " idx", lambda: fb.check_exact(idx, idx2, what + ": fused taps against apply + max-pool"))
            zr, za = fb.apply(case.y, scale, shift, None, True)
            pr, _ = fb.maxpool3x3s2(zr.reshape(N, H, W, C))
            pa = fb.maxpool3x3s2(za.reshape(N, H, W, C))[0]          # (the largest |terms| in the window: covers whichever tap won)
            tau = fb.tau_of(0)
            tr = fail.run(what + " fp64", lambda: fc.check(p, pr, pa, dt, tau, tau, what + " pooled value"))
            if tr:
                _note("stem bn_relu_maxpool", "y", tr, tau)
            # backward: gradient of the pooled map -> dy of the stem's BatchNorm
            pdy = _randn((N, Ho, Wo, C), _gen(H), 1.0, 0.5).to(dt)
            pdy = torch.where(pdy == 0, torch.ones_like(pdy), pdy)
            rows = _hip.lib().udapose_bn_bwd_rows(npix)
            outs = []
            for fused in (True, False):
                dy, slab, coef = G.new((npix, C), dt, C), G.new((rows, 2, C), torch.float32, 2 * C), G.new((3, C), torch.float32, C)
                dgamma, dbeta = G.new((C,), torch.float32, C, case.old[0]), G.new((C,), torch.float32, C, case.old[1])
                if fused:
                    ops.bn_bwd_pooled(pdy, idx, y4, dy, case.gamma, case.mean, case.invstd, case.beta, slab, coef, dgamma, dbeta, beta_acc=0.5)
                else:
                    dzs, gout = G.new((N, H, W, C), dt, W * C), G.new((npix, C), dt, C)
                    check(_hip.lib(build).udapose_maxpool3x3s2_bwd(_hip.stream(), _hip.ptr(pdy), _hip.ptr(idx), _hip.ptr(dzs), N, H, W, C), "maxpool_bwd")
                    code = ops.bn_bwd_ex(dzs.reshape(npix, C), None, case.y, dy, case.gamma, case.mean, case.invstd, slab, coef, dgamma, dbeta, relu=2,
                                         gout=gout, beta=case.beta, beta_acc=0.5, chunked=1)
                    assert code == 0
                fail.run(what, lambda: G.check(what + " backward"))
                outs.append((dy, dgamma, dbeta))
            for name, a, b in zip(("dy", "dgamma", "dbeta"), *outs):
                if not torch.equal(a, b):
                    fail.items.append(f"{what}: bn_bwd_pooled {name} differs in bits from max-pool backward + bn_bwd(relu = 2)")
            keep, und = fb.relu_mask_from_y(case.y, case.mean, case.invstd, case.gamma, case.beta, gout)
            # the planted exact zeros receive pooled gradient and are masked out by the reference and by the unfused device path; the fused
            # kernel has no gout: its dy and sums are held to this reference per element below
            hit = int((dzs.reshape(npix, C)[case.zero] != 0).sum())
            if hit < Ho * Wo or bool(keep[case.zero].any()) or bool((gout[case.zero] != 0).any()):
                fail.items.append(f"{what}: planted exact zeros: {hit} carry pooled gradient, the reference keeps {int(keep[case.zero].sum())}, the "
                                  f"device passes {int((gout[case.zero] != 0).sum())} (the test is strictly > 0)")
            ref = fb.backward(dzs.reshape(npix, C), case.y, case.mean, case.invstd, case.gamma, keep)
            tau = fb.tau_of(fb.stream_chain(npix, C))
            dy, dgamma, dbeta = outs[0]
            tr = fail.run(what + " dy", lambda: fc.check(dy, *ref["dy"], dt, tau, tau, what + " bn_bwd_pooled dy"))
            if tr:
                _note("stem bn_bwd_pooled", "dy", tr, tau)
            for name, got, old in (("dgamma", dgamma, case.old[0]), ("dbeta", dbeta, case.old[1])):
                s, a = ref[name]
                tr = fail.run(f"{what} {name}", lambda: fb.check_sums(got, 0.5 * old.double() + s, 0.5 * old.double().abs() + a, tau, f"{what} bn_bwd_pooled {name}"))
                if tr:
                    _note("stem bn_bwd_pooled", name, tr, tau)
    _report("stem", t0)
    fail.assert_none()


# ---- max-pool --------------------------------------------------------------------------------------------------------------------

def _maps(shape, seed):
    g = _gen(seed)
    x = torch.randn(shape, device="cuda", generator=g).bfloat16().float() * 0.5        # (few distinct values: ties inside windows)
    out = {"random": x, "all_negative": -x.abs() - 0.5, "post_relu": torch.relu(x), "all_equal": torch.full(shape, 1.25, device="cuda")}
    xi = x.clone()
    xi[torch.rand(shape, device="cuda", generator=g) < 0.3] = float("-inf")
    out["neg_inf"] = xi
    xn = x.clone()
    xn[torch.rand(shape, device="cuda", generator=g) < 0.15] = float("nan")
    out["nan"] = xn
    return out


def _pool_case(build, name, x32, fail, what):
    """Every pool form of one build on one map (values representable in both 16-bit types)."""
    ops, _hip = _ops()
    dt = ELEM[build]
    N, H, W, C = x32.shape
    finite = name not in ("neg_inf", "nan")
    Ho, Wo, H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1, (H + 1) // 2, (W + 1) // 2
    x16 = x32.to(dt)
    refs = {}
    for kind in _kinds(build):
        if kind in ("split", "strict") and not finite:
            continue                # (the split storage has neither NaN nor infinity)
        x = x16 if kind == "16bit" else (x32 if kind == "f32" else ops.f32_to_split(x32))
        rk = "split" if kind == "strict" else kind
        if rk not in refs:          # (the references pool what the kernel reads: the input as stored in this kind)
            xs = ops.split_to_f32(x) if rk == "split" else x
            refs[rk] = fb.maxpool3x3s2(xs) + (fb.maxpool2x2_ceil(xs)[0],)
        val3, tap3, val2 = refs[rk]
        odt = {"16bit": dt, "f32": torch.float32}.get(kind, torch.int32)
        G = Guards()
        y, idx = G.new((N, Ho, Wo, C), odt, Wo * C), G.new((N, Ho, Wo, C), torch.uint8, Wo * C)
        y16 = G.new((N, Ho, Wo, C), torch.float16, Wo * C) if kind == "strict" else None
        w = f"{what} 3x3 {kind}"
        ops.maxpool3x3s2_fwd_ex(kind, x, y, idx, y16=y16, build=build)
        fail.run(w, lambda: G.check(w))
        if odt == torch.int32:
            yf = ops.split_to_f32(y)
            fail.run(w, lambda: fb.check_exact(yf, val3, w + " value (a pool only selects: the winner's (h, l) pair, bit for bit)"))
            if kind == "strict":
                fail.run(w, lambda: fb.check_exact(y16, fb.split_h(y.reshape(-1, C)).reshape(y16.shape), w + " y16 == h half of y"))
        else:
            fail.run(w, lambda: fb.check_exact(y, val3, w + " value"))
        fail.run(w, lambda: fb.check_exact(idx, tap3, w + " tap"))
        if kind == "strict":
            continue
        y2 = G.new((N, H2, W2, C), odt, W2 * C)
        w = f"{what} 2x2 {kind}"
        fn = {"16bit": _hip.lib(build).udapose_maxpool2x2_ceil, "f32": _hip.lib(build).udapose_maxpool2x2_ceil_f32,
              "split": _hip.lib(build).udapose_maxpool2x2_ceil_split}[kind]
        _hip.check(fn(_hip.stream(), _hip.ptr(x), _hip.ptr(y2), N, H, W, C), "maxpool2x2")
        fail.run(w, lambda: G.check(w))
        if odt == torch.int32:
            y2f = ops.split_to_f32(y2)
            fail.run(w, lambda: fb.check_exact(y2f, val2, w + " value"))
        else:
            fail.run(w, lambda: fb.check_exact(y2, val2, w + " value"))
    # backwards (16-bit)
    val3, tap3, val2 = refs["16bit"]
    G = Guards()
    g = _gen(H * W + C)
    dy3 = _randn((N, Ho, Wo, C), g).to(dt)
    dx3 = G.new((N, H, W, C), dt, W * C)
    _hip.check(_hip.lib(build).udapose_maxpool3x3s2_bwd(_hip.stream(), _hip.ptr(dy3), _hip.ptr(tap3.to(torch.uint8)), _hip.ptr(dx3), N, H, W, C), "maxpool_bwd")
    ref, absref = fb.maxpool3x3s2_bwd(dy3, tap3, H, W)
    tau = fb.tau_of(4)
    fail.run(what, lambda: G.check(what + " 3x3 backward"))
    tr = fail.run(what, lambda: fc.check(dx3, ref, absref, dt, tau, tau, what + " 3x3 backward"))
    if tr:
        _note("pool 3x3 backward", "dx", tr, tau)
    dy2 = _randn((N, H2, W2, C), g).to(dt)
    for rm in (False, True):
        dx2 = G.new((N, H, W, C), dt, W * C)
        ops.maxpool2x2_ceil_bwd(x16, dy2, relu_mask=rm, dx=dx2)
        r2, _ = fb.maxpool2x2_ceil_bwd(x16, dy2, relu_mask=rm)
        fail.run(what, lambda: fb.check_exact(dx2, r2, f"{what} 2x2 backward relu_mask {int(rm)}"))
    fail.run(what, lambda: G.check(what + " backward"))


def test_maxpool_forms():
    """3x3 / s2 / p1 and 2x2 ceil pools, forward in every storage and backward: H or W of 1 and 2, odd sizes, C = 8, 24, 64; all-negative
    maps (a padding of 0 instead of -inf shows), post-ReLU zeros and all-equal maps (ties: the first in-range tap wins), -inf, NaN (wins,
    as in torch); values exact, taps exact; one 3x3 backward large enough (N * H * W * C / 8 > 2,097,152) for the grid-stride loop."""
    ops, _hip = _ops()
    t0 = time.time()
    fail = Failures()
    for build in ELEM:
        for H, W in ((1, 1), (1, 7), (2, 2), (7, 9), (8, 8), (18, 20)):
            for C in (8, 24, 64):
                for name, x in _maps((2, H, W, C), H * W + C).items():
                    what = f"pool {build} {name} 2x{H}x{W}x{C}"
                    fail.run(what, lambda: _pool_case(build, name, x, fail, what))
        dt = ELEM[build]
        N, H, W, C = 4, 257, 258, 64
        assert N * H * W * C // 8 > 2097152
        x = torch.relu(torch.randn(N, H, W, C, device="cuda", generator=_gen(3))).to(dt)
        G = Guards()
        Ho, Wo = 129, 129
        y, idx = G.new((N, Ho, Wo, C), dt, Wo * C), G.new((N, Ho, Wo, C), torch.uint8, Wo * C)
        ops.maxpool3x3s2_fwd_ex("16bit", x, y, idx)
        val, tap = fb.maxpool3x3s2(x)
        fail.run("pool large", lambda: fb.check_exact(y, val, f"pool {build} large value"))
        fail.run("pool large", lambda: fb.check_exact(idx, tap, f"pool {build} large tap"))
        dy = _randn((N, Ho, Wo, C), _gen(4)).to(dt)
        dx = G.new((N, H, W, C), dt, W * C)
        _hip.check(_hip.lib(build).udapose_maxpool3x3s2_bwd(_hip.stream(), _hip.ptr(dy), _hip.ptr(idx), _hip.ptr(dx), N, H, W, C), "maxpool_bwd")
        fail.run("pool large", lambda: G.check(f"pool {build} large"))
        ref, absref = fb.maxpool3x3s2_bwd(dy, tap, H, W)
        tau = fb.tau_of(4)
        tr = fail.run("pool large", lambda: fc.check(dx, ref, absref, dt, tau, tau, f"pool {build} large 3x3 backward (grid-stride loop)"))
        if tr:
            _note("pool 3x3 backward", "dx", tr, tau)
        del x, y, idx, val, tap, dy, dx, ref, absref
        torch.cuda.empty_cache()
    _report("pool", t0)
    fail.assert_none()
