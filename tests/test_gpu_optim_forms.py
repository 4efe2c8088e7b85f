"""The optimizer, EMA and loss-scaler kernels of csrc/optim.hip against the references of tests/helpers/fp64_optim.py, element by element,
through the public optimizers (FusedAdam, FusedSGD, OldWeightEMA) and - where a form is reachable no other way - the entry points they
call (udapose_adam_multi, udapose_sgd_multi, udapose_ema_multi, udapose_grad_scaler_check2, udapose_grad_scaler_update) with a
_MultiTensorTable.

Every tensor a kernel writes (parameters, moments, teacher) and every gradient the found-inf check reads is a view inside one 0xFF-filled
allocation per operand (NaN in fp32) with at least 256 bytes of guard on each side of each tensor: the guards must come back untouched,
and a clean gradient between NaN guards must leave the found-inf flag at 0 (a 16-byte load that runs past a tensor's end raises it).

Shapes.  CHUNK is 4096 elements, 256 threads, 4-wide vectors: one multi-tensor list of 1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8191
and 12291 elements (33,551 in all), laid out with every tensor 16-byte aligned ('a0'), 4, 8 or 12 bytes off ('o4', 'o8', 'o12': ema_k's
scalar path, grad_check_k's per-chunk alignment test), or mixed ('mix': offsets 0, 4, 8, 12 in turn).  The parameters are leaf Parameters
over those views.

Value regimes (fp64_optim.regime): a p, g ~ 0.05 N(0,1) | b |g| ~ 1e-8: sqrt(v) ~ eps | c log-uniform |g| in [1e-15, 1e3], a tenth 0 | d g = 0
on m = v = 0: the step is exactly 0 | e p = 0: the step without the parameter's rounding | f grad_scale = 1 / 65536 on gradients times 65536,
with +-FLT_MAX and +-3e38 among them (for Adam their square exceeds fp32's range: v = +inf and a step of exactly 0, as in torch's fp32 Adam).
Three consecutive steps per case; m, v / the momentum buffer and the step p_new - p_old are checked after every step against the one-step
reference on the kernel's own stored inputs.

Cases and the kernel branch each one runs:
  adam_k, device state (FusedAdam.step: adam_tick_k, then lr / grad_scale / bias corrections read from the state)
    a a0 wd 0 ......... the wd == 0 branch            a mix wd 1e-4 ..... the wd != 0 branch, mixed alignment
    b o4 wd 0 ......... eps against sqrt(v)           c o8 wd 1e-4 ...... 18 decades of |g|, exact zeros
    d a0 wd 0 ......... 0 / (0 + eps): no NaN         e o12 wd 0 ........ the bare step
    f mix wd 0 ........ grad_scale from state[4], v overflow
    c a0 t0 1000 ...... the counter, and with it the bias corrections, restored by load_state_dict (storage kept)
  adam_k, host state (udapose_adam_multi with dev_state NULL: step, lr, grad_scale by value; both library builds)
    b a0 wd 1e-4 | f o4 wd 0
  sgd_k, device state (FusedSGD.step: sgd_tick_k, first_step = counter == 1; the buffer is pre-filled with 3.0: the first step overwrites it)
    script 0.9 / 1e-4 / Nesterov: a mix, c o4, f a0, d o12 | plain 0.9 / 0 / off: b o8, e a0 | momentum 0: a a0 (wd 0), c o12 (wd 1e-4)
  sgd_k, host state (udapose_sgd_multi with dev_state NULL, first_step by value; both builds): a a0 script
  ema_k ............. test_ema_bits: vector path (a0), scalar path (o4, o8, o12, mix, and an aligned teacher with an unaligned student),
                      the n % 4 tails, alpha 0.999 / 0.9 / 0.5 / 0, values with +-0, subnormals and +-3e38: bit equality
  grad_check_k ...... test_found_inf: 16-byte and scalar loads, the scalar remainder, chunk edges, g + g2 at byte distances that are and
                      are not multiples of 16, inf / -inf / NaN raise, +-FLT_MAX do not, the flagged sweep leaves everything alone
  scaler_update_k, the ticks .. test_scaler_trajectories
  _MultiTensorTable keys ...... test_stale_table_* (a middle gradient, a middle exp_avg, a middle EMA source moved)
  opt_tail_k<Adam / SGD> ...... test_tail_anchor: the one-sweep tail on the [2, 1, 1, 1] network against the same references and bars

Bars: fp64_optim.K - m: k_gr + 3, v: 2 k_gr + 4, Adam's step: k_m + 7 + (k_v + 1) / 2 * absref_v / v, SGD's buffer k_gr (+ 1 after the
first step), SGD's step + 1 (+ 3 with Nesterov), all times 2^-24 of the sum of the terms' magnitudes plus half an ulp of the stored value
(of p_new for the step); k_gr = 1 + [wd: 2] + [g2: 1].  Derived in the helper, shown to hold and to bite in tests/test_optim_bounds_cpu.py.

MEASURED below: the worst measured k against its bar per kernel and output, printed by every run."""
import time

import numpy as np
import pytest
import torch

from helpers import fp64_optim as fo
from helpers.gpu_forms import Failures

pytestmark = pytest.mark.gpu

MEASURED = """
worst measured k (units of 2^-24 of absref, beyond the granted half ulp) on an MI355X, its bar, and the worst measured / own bar of any
single check; adam_k / sgd_k figures over both library builds
  adam_k, device state     m 1.64 (bar 4 .. 6)   v 3.92 (bar 6 .. 10)   step 3.83 (bar 14.5 .. 18.5 and up)   worst / own bar 0.27 / 0.39 / 0.26
  adam_k, host state       m 1.80                v 4.06                 step 3.99                              worst / own bar 0.30 / 0.41 / 0.22
  sgd_k, device state      buffer 1.26 (bar 1 .. 4)   step 2.67 (bar 2 .. 7)                                   worst / own bar 0.44 / 0.43
  sgd_k, host state        buffer 0.94                step 1.86                                                worst / own bar 0.24 / 0.27
  opt_tail_k, Adam         m 1.93 (bar 6)   v 4.70 (bar 10)   step 4.12 (bar 18.5 and up)    both builds alike   worst / own bar 0.32 / 0.47 / 0.22
  opt_tail_k, SGD          buffer 0.99 (bar 3)   step 2.13 (bar 6)                           both builds alike   worst / own bar 0.33 / 0.36
  ema_k                    0 of 939,428 elements differ from the two-rounding reference (bar: 0); the teacher of the tail likewise
  grad_check_k             268 launches: every plant raised the flag, no +-FLT_MAX and no clean gradient between NaN guards did
  bits against the float32 emulation (not asserted): adam_k 0 of 3,623,508 values differ, sgd_k 0 of 2,214,366
No measured k comes within 2x of its bar.  The whole module takes 7 s."""

SIZES = (1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8191, 12291)
NTOT = sum(SIZES)
LAYOUTS = {"a0": (0,) * 12, "o4": (4,) * 12, "o8": (8,) * 12, "o12": (12,) * 12, "mix": (0, 4, 8, 12) * 3}
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
WORST = {}          # (kernel, output) -> [worst measured k, its bar, worst measured / bar]
BITS = {}           # kernel -> [elements whose bits differ from the fp32 emulation, elements compared]


def _hip():
    from uda_poseestimation_amd import _hip
    return _hip


def _note(kernel, out, k):
    for name, (meas, ratio) in out.items():
        w = WORST.setdefault((kernel, name), [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], meas), max(w[1], k[name]), max(w[2], ratio)


def _bits(kernel, pairs):
    b = BITS.setdefault(kernel, [0, 0])
    for got, emu in pairs:
        b[0] += fo.bits_differ(got, emu)
        b[1] += int(np.asarray(emu).size)


def _report(part, t0):
    print(f"\n[{part}] wall {time.time() - t0:.1f} s; worst measured k (units of 2^-24 of absref), the bar, worst measured / own bar:")
    for (kernel, name), (meas, bar, ratio) in sorted(WORST.items()):
        if kernel.startswith(part):
            print(f"  {kernel:24s} {name:3s} k {meas:7.3f}  (bar {bar:g}{'+' if name == 'd' and 'adam' in kernel else ''}; worst / own bar {ratio:.2f})")
    for kernel, (diff, n) in sorted(BITS.items()):
        if kernel.startswith(part):
            print(f"  {kernel:24s} {diff} of {n} values differ in their bits from the float32 emulation (for information)")


@pytest.fixture(scope="module", autouse=True)
def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _hip().lib("bf16"), _hip().lib("fp16")
    t0 = time.time()
    yield
    print(f"\n[optim forms] module wall time {time.time() - t0:.1f} s")


@pytest.fixture(autouse=True)
def _device_still_sound():
    """Nothing is started on a device that an earlier test left in an error state."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reports an error before this test: {e}", returncode=3)
    yield


class Arena:
    """The tensors of one multi-tensor operand as fp32 views inside ONE 0xFF-filled allocation: tensor i starts offs[i] (+ shift) bytes
    past a 16-byte boundary and has at least 256 guard bytes on each side."""

    def __init__(self, sizes=SIZES, offs=LAYOUTS["a0"], shift=0, fill=None):
        pos, self.spans = 256, []
        for n, o in zip(sizes, offs):
            pos = -(-pos // 16) * 16 + o
            self.spans.append((pos + shift, n))          # (a shifted arena keeps the layout: every tensor `shift` bytes further on)
            pos += 4 * n + 256
        self.buf = torch.full((pos + 32,), 0xFF, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[p:p + 4 * n].view(torch.float32) for p, n in self.spans]
        guard = torch.ones(self.buf.numel(), dtype=torch.bool)
        for p, n in self.spans:
            guard[p:p + 4 * n] = False
        self.guard = guard.cuda()
        if fill is not None:
            self.fill(fill)

    def fill(self, flat):
        flat = torch.as_tensor(flat, dtype=torch.float32).cuda() if not (torch.is_tensor(flat) and flat.is_cuda) else flat
        if flat.numel() == 1:
            flat = flat.expand(sum(n for _, n in self.spans))
        o = 0
        for v in self.views:
            v.copy_(flat[o:o + v.numel()])
            o += v.numel()

    def flat(self):
        return torch.cat(self.views)

    def check(self, what):
        assert bool((self.buf[self.guard] == 0xFF).all()), f"{what}: guard bytes were overwritten"


def _table(*arenas):
    from uda_poseestimation_amd.utils import _MultiTensorTable
    return _MultiTensorTable([a.views for a in arenas])


def _state(step=0.0, lr=LR, gscale=1.0, scale=65536.0):
    return torch.tensor([step, 0.0, 0.0, lr, gscale, 0.0, scale, 0.0], dtype=torch.float32, device="cuda")


# ---- Adam --------------------------------------------------------------------------------------------------------------------------

def _adam_case(fail, regime, layout, wd=0.0, t0=0, host=None):
    """Three steps of adam_k in one value regime and layout.  host: None = FusedAdam (device state), else the library build whose
    udapose_adam_multi is called with dev_state NULL."""
    from uda_poseestimation_amd.optim import FusedAdam
    hip = _hip()
    what = f"adam {'host ' + host if host else 'device'} state, regime {regime} {layout} wd {wd:g} t0 {t0}"
    kernel = "adam_k host" if host else "adam_k"
    offs = LAYOUTS[layout]
    p0, _, gs = fo.regime(regime, NTOT, 21)
    P, G, M, V = Arena(offs=offs, fill=p0), Arena(offs=offs), Arena(offs=offs, fill=0.0), Arena(offs=offs, fill=0.0)
    k = fo.K("adam", wd)
    if host is None:
        params = [torch.nn.Parameter(v) for v in P.views]
        assert all(p.data_ptr() == v.data_ptr() and p.is_leaf for p, v in zip(params, P.views))
        opt = FusedAdam(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd, grad_scale=gs)
        for p, g, m, v in zip(params, G.views, M.views, V.views):
            p.grad = g
            opt.state[p] = {"exp_avg": m, "exp_avg_sq": v}
        if t0:
            gen = torch.Generator().manual_seed(4)
            M.fill(torch.randn(NTOT, generator=gen) * 0.01)
            V.fill(torch.rand(NTOT, generator=gen) * 1e-3)
            sd = opt.state_dict()
            sd["param_groups"][0]["step"] = t0
            opt.load_state_dict(sd)
            assert all(opt.state[p]["exp_avg"].data_ptr() == m.data_ptr() for p, m in zip(params, M.views)), "load_state_dict moved the moments"
    else:
        tab = _table(P, G, M, V)
    for step in range(3):
        t = t0 + step + 1
        _, g, _ = fo.regime(regime, NTOT, 21, step)
        G.fill(g)
        p_old, m_old, v_old = P.flat(), M.flat(), V.flat()

        def launch():
            if host is None:
                opt.step()
            else:
                ptr = hip.ptr
                hip.check(hip.lib(host).udapose_adam_multi(hip.stream(), ptr(tab.ptrs[0]), ptr(tab.ptrs[1]), ptr(tab.ptrs[2]), ptr(tab.ptrs[3]),
                                                           ptr(tab.sizes), ptr(tab.blk_t), ptr(tab.blk_o), tab.nblocks, LR, B1, B2, EPS, wd, t, gs, None),
                          "adam_multi")
            torch.cuda.synchronize()
            return True
        if fail.run(what, launch) is None:
            return
        for a in (P, G, M, V):
            fail.run(what, lambda: a.check(f"{what} step {step}"))
        if not torch.equal(G.flat().cpu(), g):
            fail.items.append(f"{what} step {step}: the sweep changed the gradients")
        p_new, m_new, v_new = P.flat(), M.flat(), V.flat()
        ref = fo.adam(p_old, g.cuda(), m_old, v_old, LR, B1, B2, EPS, t, wd, gs)
        out = fail.run(what, lambda: fo.check_adam(p_old, p_new, m_new, v_new, ref, k, f"{what} step {step}"))
        if out:
            _note(kernel, out, k)
        if regime == "d" and wd == 0 and t0 == 0 and not (torch.equal(p_new, p_old) and not bool(m_new.any()) and not bool(v_new.any())):
            fail.items.append(f"{what} step {step}: g = 0 on m = v = 0 must leave p, m and v exactly as they were")
        e = fo.emu_adam(p_old, g, m_old, v_old, LR, B1, B2, EPS, t, wd, gs)
        _bits(kernel, zip((p_new, m_new, v_new), e))
    if host is None:
        assert opt.state_dict()["param_groups"][0]["step"] == t0 + 3, what


ADAM_DEVICE = [("a", "a0", 0.0, 0), ("a", "mix", 1e-4, 0), ("b", "o4", 0.0, 0), ("c", "o8", 1e-4, 0), ("d", "a0", 0.0, 0), ("e", "o12", 0.0, 0),
               ("f", "mix", 0.0, 0), ("c", "a0", 0.0, 1000)]
ADAM_HOST = [("b", "a0", 1e-4), ("f", "o4", 0.0)]


def test_adam_forms():
    t0 = time.time()
    fail = Failures()
    for regime, layout, wd, start in ADAM_DEVICE:
        _adam_case(fail, regime, layout, wd, start)
    for build in ("bf16", "fp16"):
        for regime, layout, wd in ADAM_HOST:
            _adam_case(fail, regime, layout, wd, 0, host=build)
    _report("adam_k", t0)
    fail.assert_none()


# ---- SGD ---------------------------------------------------------------------------------------------------------------------------

SGD_SETTINGS = {"script": (0.9, 1e-4, True), "plain": (0.9, 0.0, False), "mu0": (0.0, 0.0, False), "mu0 wd": (0.0, 1e-4, False)}
SGD_LR = 1e-2


def _sgd_case(fail, regime, layout, setting, host=None):
    from uda_poseestimation_amd.optim import FusedSGD
    hip = _hip()
    mu, wd, nesterov = SGD_SETTINGS[setting]
    what = f"sgd {'host ' + host if host else 'device'} state, regime {regime} {layout} {setting}"
    kernel = "sgd_k host" if host else "sgd_k"
    offs = LAYOUTS[layout]
    p0, _, gs = fo.regime(regime, NTOT, 22)
    P, G, Bf = Arena(offs=offs, fill=p0), Arena(offs=offs), Arena(offs=offs, fill=3.0)     # (the first step must overwrite the buffer)
    if host is None:
        params = [torch.nn.Parameter(v) for v in P.views]
        opt = FusedSGD(params, lr=SGD_LR, momentum=mu, weight_decay=wd, nesterov=nesterov, grad_scale=gs)
        for p, g, b in zip(params, G.views, Bf.views):
            p.grad = g
            opt.state[p] = {"momentum_buffer": b}
    else:
        tab = _table(P, G, Bf)
    for step in range(3):
        first = step == 0
        _, g, _ = fo.regime(regime, NTOT, 22, step)
        G.fill(g)
        p_old, b_old = P.flat(), Bf.flat()

        def launch():
            if host is None:
                opt.step()
            else:
                ptr = hip.ptr
                hip.check(hip.lib(host).udapose_sgd_multi(hip.stream(), ptr(tab.ptrs[0]), ptr(tab.ptrs[1]), ptr(tab.ptrs[2]), ptr(tab.sizes), ptr(tab.blk_t),
                                                          ptr(tab.blk_o), tab.nblocks, SGD_LR, mu, wd, int(nesterov), int(first), gs, None), "sgd_multi")
            torch.cuda.synchronize()
            return True
        if fail.run(what, launch) is None:
            return
        for a in (P, G, Bf):
            fail.run(what, lambda: a.check(f"{what} step {step}"))
        p_new, b_new = P.flat(), Bf.flat()
        k = fo.K("sgd", wd, False, nesterov, first)
        ref = fo.sgd(p_old, g.cuda(), b_old, SGD_LR, mu, wd, nesterov, first, gs)
        out = fail.run(what, lambda: fo.check_sgd(p_old, p_new, b_new, ref, k, f"{what} step {step}"))
        if out:
            _note(kernel, out, k)
        if regime == "d" and wd == 0 and not (torch.equal(p_new, p_old) and not bool(b_new.any())):
            fail.items.append(f"{what} step {step}: g = 0 must leave p as it was and the buffer at 0")
        e = fo.emu_sgd(p_old, g, b_old, SGD_LR, mu, wd, nesterov, first, gs)
        _bits(kernel, zip((p_new, b_new), e))
    if host is None:
        assert opt.state_dict()["param_groups"][0]["step"] == 3, what


SGD_DEVICE = [("a", "mix", "script"), ("c", "o4", "script"), ("f", "a0", "script"), ("d", "o12", "script"), ("b", "o8", "plain"), ("e", "a0", "plain"),
              ("d", "a0", "plain"), ("a", "a0", "mu0"), ("c", "o12", "mu0 wd")]


def test_sgd_forms():
    t0 = time.time()
    fail = Failures()
    for regime, layout, setting in SGD_DEVICE:
        _sgd_case(fail, regime, layout, setting)
    for build in ("bf16", "fp16"):
        _sgd_case(fail, "a", "a0", "script", host=build)
    _report("sgd_k", t0)
    fail.assert_none()


# ---- EMA ---------------------------------------------------------------------------------------------------------------------------

class _Net:
    def __init__(self, params):
        self._p = list(params)

    def parameters(self):
        return iter(self._p)


def _ema_values(seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(NTOT, generator=gen)
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 3e-39, -1.1e-38, 3e38, -3e38, 1.17549435e-38], dtype=torch.float32)
    idx = torch.arange(NTOT)
    sel = (idx % 7 == seed % 7)
    x[sel] = special[(idx[sel] // 7 + seed) % special.numel()]
    return x


def test_ema_bits():
    """OldWeightEMA.step -> ema_k: bit equality with fl(fl(t * a) + fl(s * b)) on the size list, aligned (16-byte path with its n % 4 tail)
    and unaligned (scalar path), for alpha 0.999, 0.9, 0.5 and 0; +-0, subnormals and +-3e38 among the values of both operands."""
    from uda_poseestimation_amd.utils import OldWeightEMA
    t0 = time.time()
    fail = Failures()
    compared = differ = 0
    for lt, ls in (("a0", "a0"), ("o4", "o4"), ("o8", "o8"), ("o12", "o12"), ("mix", "mix"), ("a0", "o8"), ("o4", "a0")):
        T, S = Arena(offs=LAYOUTS[lt]), Arena(offs=LAYOUTS[ls])
        S.fill(_ema_values(1))
        tp, sp = [torch.nn.Parameter(v) for v in T.views], [torch.nn.Parameter(v) for v in S.views]
        ema = OldWeightEMA(_Net(tp), _Net(sp))
        for i, alpha in enumerate((0.999, 0.9, 0.5, 0.0)):
            what = f"ema teacher {lt} student {ls} alpha {alpha}"
            t_old = _ema_values(2 + i)
            T.fill(t_old)
            ema.alpha = alpha

            def launch():
                ema.step()
                torch.cuda.synchronize()
                return True
            if fail.run(what, launch) is None:
                break
            fail.run(what, lambda: T.check(what))
            fail.run(what, lambda: S.check(what))
            want = fo.ema(t_old, S.flat(), alpha)
            n = fo.bits_differ(T.flat(), want)
            compared, differ = compared + want.size, differ + n
            if n:
                got = T.flat().cpu().numpy()
                w = int(np.nonzero(got.view(np.int32) != want.view(np.int32))[0][0])
                fail.items.append(f"{what}: {n} of {want.size} elements differ in their bits; first at {w}: got {got[w]!r}, want {want[w]!r} "
                                  f"(teacher {float(t_old[w])!r}, student {float(S.flat()[w])!r})")
            if not torch.equal(S.flat().cpu().view(torch.int32), _ema_values(1).view(torch.int32)):
                fail.items.append(f"{what}: the student changed")
    print(f"\n[ema_k] wall {time.time() - t0:.1f} s; {differ} of {compared} elements differ in their bits from the two-rounding reference (bar: 0)")
    fail.assert_none()


# ---- found-inf check ---------------------------------------------------------------------------------------------------------------

INF, NAN, FLT_MAX = float("inf"), float("nan"), fo.FLT_MAX
# (tensor of the size list, element): first and last element of a tensor; the last element of a 4096 chunk and the first of the next; the first
# element of the scalar remainder off + 4 * n4 of a last chunk (257: 256; 4095: 4092; 4097: 4096; 12291: chunk 3 holds 12288 .. 12290)
POSITIONS = [(0, 0), (11, 0), (11, 12290), (10, 4095), (10, 4096), (6, 256), (7, 4092), (9, 4096), (11, 12288)]


def test_found_inf():
    """udapose_grad_scaler_check2 -> grad_check_k, one launch per planted value (one flag covers the whole table), then the Adam sweep under
    the raised flag: parameters, moments and the device counter stay as they were."""
    hip = _hip()
    ptr = hip.ptr
    L = hip.lib()
    t0 = time.time()
    fail = Failures()
    gen = torch.Generator().manual_seed(9)
    clean = torch.randn(NTOT, generator=gen) * 0.05
    clean2 = torch.randn(NTOT, generator=gen) * 0.05
    launches = 0
    # (layout of g, byte shift of g2's arena: None = no second buffer, 0 = a distance that is a multiple of 16, 4 / 8 = one that is not)
    for layout, shift2 in (("a0", None), ("o4", None), ("mix", None), ("a0", 0), ("a0", 4), ("o8", 8), ("mix", 0)):
        offs = LAYOUTS[layout]
        P, G, M, V = Arena(offs=offs, fill=clean), Arena(offs=offs, fill=clean), Arena(offs=offs, fill=0.0), Arena(offs=offs, fill=0.0)
        G2 = Arena(offs=offs, shift=shift2, fill=clean2) if shift2 is not None else None
        delta = G2.views[0].data_ptr() - G.views[0].data_ptr() if G2 is not None else 0
        if G2 is not None:
            assert all(b.data_ptr() - a.data_ptr() == delta for a, b in zip(G.views, G2.views)) and (delta % 16 == 0) == (shift2 == 0)
        tab = _table(P, G, M, V)
        state = _state()

        def flag_after(plants, what):
            """Plant, run the check, return the flag; the arenas are restored afterwards."""
            nonlocal launches
            for arena, ti, ei, val in plants:
                arena.views[ti][ei] = val
            state[5] = 0.0

            def launch():
                hip.check(L.udapose_grad_scaler_check2(hip.stream(), ptr(tab.ptrs[1]), ptr(tab.sizes), ptr(tab.blk_t), ptr(tab.blk_o), tab.nblocks,
                                                       ptr(state), delta), "grad_scaler_check2")
                torch.cuda.synchronize()
                return float(state[5])
            launches += 1
            return fail.run(what, launch)

        def restore(plants):
            for arena, ti, ei, _ in plants:
                src = clean if arena is G else clean2
                arena.views[ti][ei] = float(src[sum(SIZES[:ti]) + ei])

        cfg = f"found-inf g {layout}" + ("" if G2 is None else f", g2 at a distance of {delta % 16} mod 16")
        f = flag_after([], cfg + " clean")
        if f is None:
            break
        if f != 0.0:
            fail.items.append(f"{cfg}: a clean gradient between NaN guards raised the flag (a load ran past a tensor's end)")
        cases = []
        full = layout == "a0" and shift2 is None
        for pi, (ti, ei) in enumerate(POSITIONS):
            vals = (INF, -INF, NAN) if full else ((INF, -INF, NAN)[pi % 3],)
            for val in vals:
                cases.append(([(G, ti, ei, val)], True, f"{val} at tensor {ti} element {ei}"))
            for val in ((FLT_MAX, -FLT_MAX) if full else ((FLT_MAX, -FLT_MAX)[pi % 2],)):
                cases.append(([(G, ti, ei, val)], False, f"{val:.9g} at tensor {ti} element {ei}"))
            if G2 is not None:
                cases.append(([(G2, ti, ei, (INF, -INF, NAN)[(pi + 1) % 3])], True, f"a non-finite value in g2 only, tensor {ti} element {ei}"))
                cases.append(([(G, ti, ei, 3e38), (G2, ti, ei, 3e38)], True, f"g = g2 = 3e38 (only the sum overflows) at tensor {ti} element {ei}"))
                cases.append(([(G, ti, ei, FLT_MAX), (G2, ti, ei, -FLT_MAX)], False, f"g = FLT_MAX, g2 = -FLT_MAX at tensor {ti} element {ei}"))
        for plants, raises, desc in cases:
            what = f"{cfg}: {desc}"
            f = flag_after(plants, what)
            if f is None:
                break
            if (f != 0.0) != raises or f not in (0.0, 1.0):
                fail.items.append(f"{what}: flag {f}, expected {'1' if raises else '0'}")
            if raises and f == 1.0:        # the sweep under the raised flag
                before = [a.buf.clone() for a in (P, M, V)]

                def sweep():
                    hip.check(L.udapose_adam_multi(hip.stream(), ptr(tab.ptrs[0]), ptr(tab.ptrs[1]), ptr(tab.ptrs[2]), ptr(tab.ptrs[3]), ptr(tab.sizes),
                                                   ptr(tab.blk_t), ptr(tab.blk_o), tab.nblocks, LR, B1, B2, EPS, 0.0, 1, 1.0, ptr(state)), "adam_multi")
                    torch.cuda.synchronize()
                    return True
                if fail.run(what, sweep) is None:
                    break
                if not all(torch.equal(a.buf, b) for a, b in zip((P, M, V), before)) or float(state[0]) != 0.0 or float(state[5]) != 1.0:
                    fail.items.append(f"{what}: the sweep under a raised flag changed parameters, moments or the counter (counter {float(state[0])})")
            restore(plants)
        for a in (P, G, M, V) + ((G2,) if G2 is not None else ()):
            fail.run(cfg, lambda: a.check(cfg))
    print(f"\n[grad_check_k] wall {time.time() - t0:.1f} s; {launches} check launches")
    fail.assert_none()


# ---- loss scaler -------------------------------------------------------------------------------------------------------------------

SCALER_FLAGS = ("000000000000", "100100100100", "001000110001", "111111111111")


@pytest.mark.parametrize("flags", SCALER_FLAGS)
def test_scaler_trajectories(flags):
    """FusedAdam(dynamic_loss_scale=True, growth_interval=3): found-inf check, tick, sweep, scaler_update_k per step.  After every step the
    device state equals fp64_optim.scaler_trajectory exactly: the optimizer's counter (clean steps only), grad_scale = 1 / scale, the flag
    re-armed, scale and tracker; a flagged step leaves the parameters alone."""
    from uda_poseestimation_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(5)
    sizes = (5, 257, 4097)
    P, G = Arena(sizes, (0, 4, 0), fill=torch.randn(sum(sizes), generator=gen)), Arena(sizes, (0, 4, 0))
    params = [torch.nn.Parameter(v) for v in P.views]
    for p, g in zip(params, G.views):
        p.grad = g
    opt = FusedAdam(params, lr=LR, dynamic_loss_scale=True, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    assert float(opt.loss_scale()) == 65536.0
    want = fo.scaler_trajectory(flags, 65536.0, 2.0, 0.5, 3)
    for i, (f, (scale, tracker, gscale, count)) in enumerate(zip(flags, want)):
        g = torch.randn(sum(sizes), generator=gen) * 65536.0
        if f == "1":
            g[(5 + 256, 5 + 257 + 4096, 0)[i % 3]] = (INF, -INF, NAN)[i % 3]
        G.fill(g)
        before = P.flat()
        opt.step()
        torch.cuda.synchronize()
        st = opt._dev[0][0].tolist()
        assert (st[0], st[4], st[5], st[6], st[7]) == (float(count), gscale, 0.0, scale, float(tracker)), (flags, i, st, want[i])
        assert torch.equal(P.flat(), before) == (f == "1"), (flags, i)
        assert bool(torch.isfinite(P.flat()).all())
    P.check("scaler"), G.check("scaler")
    sd = opt.state_dict()["param_groups"][0]
    assert (sd["step"], sd["loss_scale"], sd["growth_tracker"]) == (want[-1][3], want[-1][0], want[-1][1])


# ---- stale tables ------------------------------------------------------------------------------------------------------------------

def _five(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.05).cuda()) for n in (7, 300, 5, 4097, 33)]


def _check_adam_step(what, params, p_old, grads, m_old, v_old, opt, t):
    for i, p in enumerate(params):
        ref = fo.adam(p_old[i], grads[i], m_old[i], v_old[i], LR, B1, B2, EPS, t)
        st = opt.state[p]
        fo.check_adam(p_old[i], p.detach(), st["exp_avg"], st["exp_avg_sq"], ref, fo.K("adam"), f"{what}, parameter {i}")


def _stepped_adam():
    """FusedAdam over five small parameters, stepped once (its table is built)."""
    from uda_poseestimation_amd.optim import FusedAdam
    params = _five(1)
    opt = FusedAdam(params, lr=LR)
    gen = torch.Generator().manual_seed(2)
    for p in params:
        p.grad = (torch.randn(p.numel(), generator=gen) * 0.05).cuda()
    opt.step()
    torch.cuda.synchronize()
    return params, opt, gen


def _step_and_check(what, params, opt, t):
    p_old, grads = [p.detach().clone() for p in params], [p.grad.clone() for p in params]
    m_old, v_old = [opt.state[p]["exp_avg"].clone() for p in params], [opt.state[p]["exp_avg_sq"].clone() for p in params]
    opt.step()
    torch.cuda.synchronize()
    _check_adam_step(what, params, p_old, grads, m_old, v_old, opt, t)


def test_stale_table_middle_gradient_reallocated():
    """A table is rebuilt when ANY tensor of any list moved: the middle parameter of five gets a freshly allocated gradient with other
    values (the old tensor is kept alive, so that a stale pointer reads defined memory); the next step must use the new one."""
    params, opt, gen = _stepped_adam()
    keep_alive = params[2].grad
    params[2].grad = (torch.randn(5, generator=gen) * 0.05 + 1.0).cuda()
    assert params[2].grad.data_ptr() != keep_alive.data_ptr()
    _step_and_check("a reallocated middle gradient", params, opt, 2)
    del keep_alive


def test_stale_table_middle_exp_avg_restored_into_fresh_storage():
    """The middle parameter's state is dropped and restored: load_state_dict keeps the storage of the state that exists and allocates the
    rest, so exp_avg of that one parameter arrives in fresh storage with other values; the next step must read it."""
    params, opt, _ = _stepped_adam()
    old_m = opt.state[params[2]]["exp_avg"]               # (kept alive)
    sd = opt.state_dict()
    sd["state"][2] = dict(sd["state"][2], exp_avg=old_m.clone() * 2.0 + 0.5)
    del opt.state[params[2]]
    opt.load_state_dict(sd)
    assert opt.state[params[2]]["exp_avg"].data_ptr() != old_m.data_ptr()
    assert opt.state[params[1]]["exp_avg"].data_ptr() != opt.state[params[2]]["exp_avg"].data_ptr()
    assert torch.equal(opt.state[params[2]]["exp_avg"], old_m * 2.0 + 0.5)
    _step_and_check("exp_avg restored into fresh storage", params, opt, 2)
    del old_m


def test_stale_table_middle_ema_source_replaced():
    """OldWeightEMA after a middle source parameter's .data was replaced: the teacher follows the new tensor."""
    from uda_poseestimation_amd.utils import OldWeightEMA
    src, tgt = _five(3), _five(4)
    ema = OldWeightEMA(_Net(tgt), _Net(src), alpha=0.9)
    for p in tgt:
        p.data.mul_(1.5)
    ema.step()
    torch.cuda.synchronize()
    keep_src = src[2].data
    src[2].data = torch.full((5,), 7.0, device="cuda")
    assert src[2].data_ptr() != keep_src.data_ptr()
    t_old = [p.detach().clone() for p in tgt]
    ema.step()
    torch.cuda.synchronize()
    for i, (t, s, o) in enumerate(zip(tgt, src, t_old)):
        assert fo.bits_differ(t.detach(), fo.ema(o, s.detach(), 0.9)) == 0, f"EMA after a middle source parameter moved: teacher parameter {i}"
    del keep_src


# ---- one anchor for the one-sweep tail ---------------------------------------------------------------------------------------------

K_PTS = 16


def _net(seed, prec):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(seed)
    m = pr._pose_resnet("t", K_PTS, pr.Bottleneck_default, [2, 1, 1, 1], False, False, False).cuda()
    m.precision = prec
    return m


@pytest.mark.parametrize("which,prec", [("adam", "bf16"), ("adam", "fp16"), ("sgd", "bf16"), ("sgd", "fp16")])
def test_tail_anchor(which, prec):
    """opt_tail_k through fused_tail_step on the [2, 1, 1, 1] network at 2 x 3 x 128 x 128, once: gradients of regime (c) written into
    _flat_grad, weight decay 1e-4, grad_scale 0.5.  Parameters (as steps), moments / momentum buffers against fp64_optim at adam_k's / sgd_k's
    bars; the teacher bit for bit from the sweep's own new parameters; a parameter without a gradient gets the EMA only."""
    from uda_poseestimation_amd import optim as fo_
    from uda_poseestimation_amd.utils import OldWeightEMA
    t0 = time.time()
    s_, t_ = _net(3, prec), _net(4, prec)
    wd, gs = 1e-4, 0.5
    if which == "adam":
        opt = fo_.FusedAdam(s_.parameters(), lr=LR, weight_decay=wd, grad_scale=gs)
    else:
        opt = fo_.FusedSGD(s_.parameters(), lr=SGD_LR, momentum=0.9, weight_decay=wd, nesterov=True, grad_scale=gs)
    ema = OldWeightEMA(t_, s_, alpha=0.9)
    with torch.no_grad():
        for p in t_.parameters():
            p.mul_(1.01)
    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(1)).cuda()
    R = torch.randn(2, K_PTS, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()
    s_.zero_grad(set_to_none=True)
    (s_(x) * R).sum().backward()
    with torch.no_grad():
        t_(x)
    n = s_._flat_grad.numel()
    s_._flat_grad.copy_(fo.regime("c", n, 31)[1])
    sp, tp = list(s_.parameters()), list(t_.parameters())
    p_old = [p.detach().clone() for p in sp]
    t_old = [p.detach().clone() for p in tp]
    grads = [None if p.grad is None else p.grad.clone() for p in sp]
    assert opt.fused_tail_step(s_, t_, ema) is True
    torch.cuda.synchronize()
    assert s_._last_hd.precision == prec
    fail = Failures()
    kernel = f"opt_tail_k {which}"
    k = fo.K("adam", wd) if which == "adam" else fo.K("sgd", wd, False, True, True)
    with_grad = 0
    for i, (p, po, g) in enumerate(zip(sp, p_old, grads)):
        what = f"tail {which} {prec} parameter {i} {tuple(p.shape)}"
        if g is None:
            if not torch.equal(p.detach(), po):
                fail.items.append(f"{what}: a parameter without a gradient moved")
        else:
            with_grad += 1
            z = torch.zeros_like(po)
            st = opt.state[p]
            if which == "adam":
                ref = fo.adam(po, g, z, z, LR, B1, B2, EPS, 1, wd, gs)
                out = fail.run(what, lambda: fo.check_adam(po, p.detach(), st["exp_avg"], st["exp_avg_sq"], ref, k, what))
            else:
                ref = fo.sgd(po, g, z, SGD_LR, 0.9, wd, True, True, gs)
                out = fail.run(what, lambda: fo.check_sgd(po, p.detach(), st["momentum_buffer"], ref, k, what))
            if out:
                _note(kernel, out, k)
        nd = fo.bits_differ(tp[i].detach(), fo.ema(t_old[i], p.detach(), 0.9))
        if nd:
            fail.items.append(f"{what}: {nd} teacher elements differ in their bits from the EMA of the sweep's own new parameter")
    assert with_grad >= len(sp) - 2 and opt.state_dict()["param_groups"][0]["step"] == 1
    _report(kernel, t0)
    fail.assert_none()
