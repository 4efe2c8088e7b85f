"""Clipping by global norm on the device (udapose_grad_sumsq / udapose_grad_clip / udapose_grad_clip_restore; FusedAdam / FusedSGD
max_grad_norm; MeanTeacherTrainer.max_grad_norm; GraphedTrainStep).  The norm is held to the derived bar of helpers/fp64_gradnorm against
an exact reference; everything else is bits: the coefficient against its host restatement from the stored norm, a clipped step against
the same step with grad_scale pre-multiplied on the host, measure-only against no clipping, captured against eager.

MEASURED on an MI355X (printed by every run): see the docstring of test_kernel_norm_and_coef."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import fp64_gradnorm as gn
from helpers import fp64_optim as fo

pytestmark = pytest.mark.gpu

K = 16
SMALL = (1, 3, 5, 4095, 4096, 4097, 777)      # (the last one is the view at element 1: 4-byte but not 16-byte aligned)
BIG = 300 * 4096 + 7                          # 301 blocks: the finisher's loop over partials wraps
SIZES = SMALL + (BIG,)
NTOT = sum(SIZES)


@pytest.fixture(autouse=True)
def _bf16_unless_stated(monkeypatch):
    from uda_poseestimation_amd.lib.models.pose_resnet import PoseResNet
    monkeypatch.setattr(PoseResNet, "default_precision", "bf16")


@pytest.fixture(autouse=True)
def _device_still_sound():
    """Nothing is started on a device that an earlier test left in an error state."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reports an error before this test: {e}", returncode=3)
    yield


def _hip():
    from uda_poseestimation_amd import _hip
    return _hip


# ---- 1. / 2. the kernels ----------------------------------------------------------------------------------------------------------

class Arena:
    """g and g2 views inside ONE NaN-filled allocation: every tensor starts on a 16-byte boundary except the 777-element one (one element
    past it), g2's tensor lies `delta` bytes (a multiple of 16) behind g's.  A load past a tensor's end reads a NaN and shows in the norm."""

    def __init__(self, g, g2=None):
        pos, spans = 64, []
        for n in SIZES:
            pos = -(-pos // 4) * 4 + (1 if n == 777 else 0)
            spans.append((pos, n))
            pos += n + 64
        half = -(-pos // 4) * 4
        self.buf = torch.full((2 * half,), float("nan"), dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.g = [self.buf[p:p + n] for p, n in spans]
        self.g2 = [self.buf[half + p:half + p + n] for p, n in spans] if g2 is not None else None
        self.delta = 4 * half if g2 is not None else 0
        assert self.g[6].data_ptr() % 16 == 4 and all(v.data_ptr() % 16 == 0 for i, v in enumerate(self.g) if i != 6)
        for views, src in ((self.g, g), (self.g2, g2)):
            if src is not None:
                o = 0
                for v in views:
                    v.copy_(src[o:o + v.numel()])
                    o += v.numel()


def _state(gscale, scale=0.0):
    return torch.tensor([0.0, 0.0, 0.0, 1e-3, gscale, 0.0, scale, 0.0], dtype=torch.float32, device="cuda")


def _tables(views, cuts):
    from uda_poseestimation_amd.utils import _MultiTensorTable
    return [_MultiTensorTable([views[a:b]]) for a, b in cuts]


def _launch(tabs, states, clip, part, delta, dev_state=None):
    """One sum-of-squares launch per table into consecutive ranges of `part`, then the finisher."""
    hip = _hip()
    L, ptr = hip.lib(), hip.ptr
    begin, end, b = [], [], 0
    for t in tabs:
        hip.check(L.udapose_grad_sumsq(hip.stream(), ptr(t.ptrs[0]), ptr(t.sizes), ptr(t.blk_t), ptr(t.blk_o), t.nblocks, delta,
                                       ptr(dev_state), part.data_ptr() + 8 * b), "grad_sumsq")
        begin.append(b)
        b += t.nblocks
        end.append(b)
    n = len(tabs)
    arr = (C.c_void_p * n)(*[s.data_ptr() for s in states])
    hip.check(L.udapose_grad_clip(hip.stream(), ptr(part), (C.c_int * n)(*begin), (C.c_int * n)(*end), n, arr, ptr(clip)), "grad_clip")
    torch.cuda.synchronize()
    return arr


_DATA = {}


def _data(regime, with_g2):
    """The regime's gradient vector (CPU generator, fixed seed), its second buffer, and the exact reference of the two-group norm."""
    key = (regime, with_g2)
    if key not in _DATA:
        _, g, gs = fo.regime(regime, NTOT, 17)
        g2 = fo.regime(regime, NTOT, 17, step=1)[1] if with_g2 else None
        cut = lambda v: [v[sum(SIZES[:i]):sum(SIZES[:i + 1])].numpy() for i in range(len(SIZES))]
        ts, t2 = cut(g), (cut(g2) if with_g2 else None)
        k = len(SMALL)
        groups = [(ts[:k], t2[:k] if t2 else None, gs), (ts[k:], t2[k:] if t2 else None, gs * 4.0)]
        _DATA[key] = (g, g2, gs, groups, gn.ref_norm(groups))
    return _DATA[key]


@pytest.mark.parametrize("regime", ["a", "c", "f"])
@pytest.mark.parametrize("with_g2", [False, True], ids=["g", "g+g2"])
def test_kernel_norm_and_coef(regime, with_g2):
    """1. Tensors of 1, 3, 5, 4095, 4096, 4097 elements, a 777-element view one element past a 16-byte boundary and one of 300 * 4096 + 7
    (301 blocks) in two groups (the second at four times the first's grad_scale), with and without g2, regimes a, c, f: the stored norm
    within half an fp32 ulp + n * 2^-53 * ref of the exact reference, the coefficient the host restatement of the stored norm to the bit,
    state[4] = fl32(old * coef) with the old value saved, the restore launch, two calls with equal bits, max_norm = +inf -> 1.0f exactly.
    MEASURED (MI355X): worst |norm - ref| beyond the half ulp, in units of 2^-53 ref: <= 0 in every case (the fp32 rounding alone)."""
    hip = _hip()
    g, g2, gs, groups, ref = _data(regime, with_g2)
    ar = Arena(g, g2)
    k = len(SMALL)
    tabs = _tables(ar.g, [(0, k), (k, len(SIZES))])
    assert tabs[1].nblocks == 301 and sum(t.nblocks for t in tabs) == 309
    part = torch.full((309,), float("nan"), dtype=torch.float64, device="cuda")
    gss = [float(np.float32(gs)), float(np.float32(gs * 4.0))]
    M = 0.5 * float(ref)
    results = []
    for rep in range(2):
        states = [_state(x) for x in gss]
        clip = torch.zeros(12, dtype=torch.float32, device="cuda")
        clip[0] = M
        arr = _launch(tabs, states, clip, part, ar.delta)
        c = clip.cpu().numpy()
        norm, coef = c[1], c[2]
        meas = gn.check_norm(norm, ref, NTOT, f"regime {regime} g2 {with_g2}")
        print(f"\n[grad clip kernel] regime {regime} g2 {with_g2}: norm {norm!r}, ref {float(ref)!r}, beyond the half ulp {meas:.3g} x 2^-53 ref")
        assert gn.same_bits(coef, gn.coef_host(norm, M)), (coef, gn.coef_host(norm, M))
        assert 0.49 < float(coef) < 0.51
        for gi, s in enumerate(states):
            assert gn.same_bits(float(s[4]), np.float32(gss[gi]) * np.float32(coef)) and gn.same_bits(c[4 + gi], gss[gi])
            assert s.cpu().tolist()[:4] == [0.0, 0.0, 0.0, float(np.float32(1e-3))] and float(s[5]) == 0.0
        hip.check(hip.lib().udapose_grad_clip_restore(hip.stream(), 2, arr, hip.ptr(clip)), "grad_clip_restore")
        torch.cuda.synchronize()
        assert all(gn.same_bits(float(s[4]), gss[gi]) for gi, s in enumerate(states))
        results.append((np.float32(norm).view(np.int32), np.float32(coef).view(np.int32), part.clone()))
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1] and torch.equal(results[0][2], results[1][2])
    # measure only
    states = [_state(x) for x in gss]
    clip = torch.zeros(12, dtype=torch.float32, device="cuda")
    clip[0] = math.inf
    _launch(tabs, states, clip, part, ar.delta)
    assert float(clip[2]) == 1.0 and np.float32(float(clip[1])).view(np.int32) == results[0][0]
    assert all(gn.same_bits(float(s[4]), gss[gi]) for gi, s in enumerate(states))


def test_kernel_argument_checks():
    hip = _hip()
    L, ptr = hip.lib(), hip.ptr
    g = torch.ones(8, device="cuda")
    tab = _tables([g], [(0, 1)])[0]
    part = torch.zeros(1, dtype=torch.float64, device="cuda")
    clip = torch.zeros(12, device="cuda")
    st = _state(1.0)
    one, zero, arr = (C.c_int * 1)(1), (C.c_int * 1)(0), (C.c_void_p * 1)(st.data_ptr())
    s = hip.stream()
    assert L.udapose_grad_sumsq(s, ptr(tab.ptrs[0]), ptr(tab.sizes), ptr(tab.blk_t), ptr(tab.blk_o), 1, 0, None, None) == -1
    assert L.udapose_grad_sumsq(s, ptr(tab.ptrs[0]), ptr(tab.sizes), ptr(tab.blk_t), ptr(tab.blk_o), 1, 6, None, ptr(part)) == -1
    assert L.udapose_grad_sumsq(s, None, ptr(tab.sizes), ptr(tab.blk_t), ptr(tab.blk_o), 1, 0, None, ptr(part)) == -1
    assert L.udapose_grad_clip(s, ptr(part), zero, one, 0, arr, ptr(clip)) == -1
    assert L.udapose_grad_clip(s, ptr(part), zero, one, 9, arr, ptr(clip)) == -1
    assert L.udapose_grad_clip(s, ptr(part), one, zero, 1, arr, ptr(clip)) == -1
    assert L.udapose_grad_clip(s, ptr(part), zero, one, 1, arr, None) == -1
    assert L.udapose_grad_clip(s, ptr(part), zero, one, 1, (C.c_void_p * 1)(None), ptr(clip)) == -1
    assert L.udapose_grad_clip_restore(s, 1, arr, None) == -1 and L.udapose_grad_clip_restore(s, 0, arr, ptr(clip)) == -1
    torch.cuda.synchronize()
    assert st.cpu().tolist()[4] == 1.0 and not clip.any() and not part.any()


def test_found_inf_leaves_every_grad_scale_alone():
    """2. One non-finite value planted (in g, in g2 only, a sum that overflows): the fused check + norm raises state[5] wherever
    udapose_grad_scaler_check2 does on the same inputs - and not for +-FLT_MAX or a clean gradient - and under the raised flag the clip
    kernel leaves state[4] alone."""
    hip = _hip()
    L, ptr = hip.lib(), hip.ptr
    g, g2, _, _, _ = _data("a", True)
    ar = Arena(g, g2)
    tab = _tables(ar.g, [(0, len(SIZES))])[0]
    part = torch.zeros(tab.nblocks, dtype=torch.float64, device="cuda")
    INF, NAN = math.inf, math.nan
    plants = [None, (ar.g, 0, 0, INF), (ar.g, 7, BIG - 1, -INF), (ar.g, 6, 776, NAN), (ar.g, 5, 4096, INF), (ar.g2, 3, 4092, NAN),
              (ar.g2, 7, 4096 * 256, INF), ("sum", 4, 4095, 3e38), (ar.g, 2, 4, fo.FLT_MAX), ("cancel", 7, 5, fo.FLT_MAX)]
    for plant in plants:
        saved = []
        if plant is not None:
            where, ti, ei, val = plant
            both = {"sum": ((ar.g, val), (ar.g2, val)), "cancel": ((ar.g, val), (ar.g2, -val))}
            for views, v in (both[where] if isinstance(where, str) else ((where, val),)):
                saved.append((views[ti], ei, float(views[ti][ei])))
                views[ti][ei] = v
        ref_state = _state(1.0 / 65536.0, 65536.0)
        hip.check(L.udapose_grad_scaler_check2(hip.stream(), ptr(tab.ptrs[0]), ptr(tab.sizes), ptr(tab.blk_t), ptr(tab.blk_o), tab.nblocks,
                                               ptr(ref_state), ar.delta), "grad_scaler_check2")
        state = _state(1.0 / 65536.0, 65536.0)
        clip = torch.zeros(12, dtype=torch.float32, device="cuda")
        clip[0] = 1e-4
        _launch([tab], [state], clip, part, ar.delta, dev_state=state)
        want = 0.0 if plant is None or plant[3] == fo.FLT_MAX else 1.0
        assert float(ref_state[5]) == want, plant[1:] if plant else plant
        assert float(state[5]) == float(ref_state[5]), (plant[1:] if plant else plant, float(state[5]))
        if want:
            assert gn.same_bits(float(state[4]), 1.0 / 65536.0), "the clip kernel scaled grad_scale under a raised found_inf"
        else:
            assert float(clip[2]) < 1.0 and gn.same_bits(float(state[4]), np.float32(1.0 / 65536.0) * np.float32(float(clip[2])))
        for v, ei, old in saved:
            v[ei] = old


# ---- 3. a clipped step is the step with grad_scale * coef ---------------------------------------------------------------------------

def _net(seed, prec="bf16", finetune=False):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(seed)
    m = pr._pose_resnet("t", K, pr.Bottleneck_default, [2, 1, 1, 1], False, False, finetune).cuda()
    m.precision = prec
    return m


def _twin(make_opt, finetune):
    from uda_poseestimation_amd.utils import OldWeightEMA
    s_, t_ = _net(3, "bf16", finetune), _net(4, "bf16", finetune)
    opt = make_opt(s_)
    ema = OldWeightEMA(t_, s_, alpha=0.9)
    with torch.no_grad():
        for p in t_.parameters():
            p.mul_(1.01)
    return s_, t_, opt, ema


@pytest.mark.parametrize("grouped", [False, True], ids=["one_group", "three_groups"])
@pytest.mark.parametrize("tail", [False, True], ids=["step", "fused_tail_step"])
@pytest.mark.parametrize("which", ["adam", "sgd"])
def test_clipped_step_is_the_rescaled_step(which, tail, grouped):
    """3. Twin A steps with max_grad_norm = half the norm of a dry read of its gradients; twin B has no clipping and gets grad_scale =
    fl32(grad_scale * coef_A) on the host.  Parameters, optimizer state and (fused tail) the teacher are equal bit for bit over two steps,
    and every group's state[4] is back at grad_scale afterwards."""
    from uda_poseestimation_amd import optim as fo_
    GS = 0.5
    kw = dict(lr=1e-2, weight_decay=1e-2, grad_scale=GS) if which == "adam" else dict(lr=1e-2, momentum=0.9, weight_decay=1e-4, nesterov=True, grad_scale=GS)
    cls = fo_.FusedAdam if which == "adam" else fo_.FusedSGD
    names = ("exp_avg", "exp_avg_sq") if which == "adam" else ("momentum_buffer",)

    def make(s_):
        return cls(s_.get_parameters(1e-2) if grouped else s_.parameters(), **kw)
    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(1)).cuda()
    R = torch.randn(2, K, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()
    (sa, ta, oa, ea), (sb, tb, ob, eb) = _twin(make, grouped), _twin(make, grouped)
    assert len(oa.param_groups) == (3 if grouped else 1) and ob.max_grad_norm is None
    for step in range(2):
        sa.zero_grad(set_to_none=True); sb.zero_grad(set_to_none=True)
        (sa(x) * R).sum().backward()
        (sb(x) * R).sum().backward()
        with torch.no_grad():
            ta(x); tb(x)
        sb._flat_grad.copy_(sa._flat_grad)
        dry = GS * math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in sa.parameters() if p.grad is not None))
        oa.max_grad_norm = 0.5 * dry
        if tail:
            assert oa.fused_tail_step(sa, ta, ea) is True
        else:
            oa.step()
        norm, coef = float(oa.grad_norm()), float(oa.clip_coef())
        assert abs(norm - dry) <= 1e-5 * dry and gn.same_bits(coef, gn.coef_host(norm, 0.5 * dry)) and 0.49 < coef < 0.51
        for gi, grp in enumerate(oa.param_groups):
            assert gn.same_bits(float(oa._dev[gi][0][4]), GS), f"group {gi}: state[4] was not restored"
            assert float(oa._dev[gi][0][0]) == step + 1
        for grp in ob.param_groups:
            grp["grad_scale"] = float(np.float32(GS) * np.float32(coef))
        if tail:
            assert ob.fused_tail_step(sb, tb, eb) is True
        else:
            ob.step()
        for (n, pa), (_, pb) in zip(sa.named_parameters(), sb.named_parameters()):
            assert torch.equal(pa.detach(), pb.detach()), (step, n)
            if pa.grad is not None:
                for nm in names:
                    assert torch.equal(oa.state[pa][nm], ob.state[pb][nm]), (step, n, nm)
        if tail:
            for (n, pa), (_, pb) in zip(ta.named_parameters(), tb.named_parameters()):
                assert torch.equal(pa.detach(), pb.detach()), (step, "teacher", n)
            assert torch.equal(sa._last_hd.wpack, sb._last_hd.wpack)
    assert any(float(oa.state[p][names[0]].abs().max()) > 0 for p in sa.parameters() if p.grad is not None)


# ---- 4. - 6. the trainer ------------------------------------------------------------------------------------------------------------

def _args(seed=6, n=4):
    from uda_poseestimation_amd import synthetic
    b = synthetic.mean_teacher_batch(n, num_keypoints=K, image_size=128, heatmap_size=32, seed=seed)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    return (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])


def _trainer(precision="bf16", max_grad_norm=None, **kw):
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    stu, tea = _net(4, precision), _net(4, precision)
    tr = MeanTeacherTrainer(stu, tea, lr=1e-3, image_size=128, heatmap_size=32, precision=precision, **kw)
    tr.max_grad_norm = max_grad_norm
    assert tr.stu_optimizer.max_grad_norm == max_grad_norm
    return stu, tea, tr


def _snap(stu, tea, tr):
    out = [p.detach().clone() for p in list(stu.parameters()) + list(tea.parameters())]
    for p in stu.parameters():
        st = tr.stu_optimizer.state.get(p)
        if st:
            out += [v.clone() for _, v in sorted(st.items()) if torch.is_tensor(v)]
    return out


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: tensor {i} differs"


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_measure_only_is_bit_identical_to_no_clipping(precision):
    """4. max_grad_norm = inf over three trainer steps against None: parameters, teacher, optimizer state and (fp16, growth every two clean
    steps) the loss scaler's trajectory equal; the norm is there to read and the coefficient is exactly 1."""
    args = _args()
    kw = dict(loss_scale_interval=2) if precision == "fp16" else {}
    res, traj = {}, {}
    for m in (math.inf, None):
        stu, tea, tr = _trainer(precision, m, **kw)
        assert tr._tail_sums_splits() is False
        traj[m] = []
        for _ in range(3):
            tr.train_step(*args)
            assert tr.fused_last
            sd = tr.stu_optimizer.state_dict()["param_groups"][0]
            traj[m].append((sd["step"], sd.get("loss_scale"), sd.get("growth_tracker"), float(tr.stu_optimizer._dev[0][0][4])))
        res[m] = _snap(stu, tea, tr)
        if m is not None:
            n, c = float(tr.stu_optimizer.grad_norm()), float(tr.stu_optimizer.clip_coef())
            assert math.isfinite(n) and n > 0 and c == 1.0
        else:
            assert tr.stu_optimizer.grad_norm() is None and tr.stu_optimizer._clip is None
    _same(res[math.inf], res[None], f"{precision}: measure only vs no clipping")
    assert traj[math.inf] == traj[None], (traj[math.inf], traj[None])
    if precision == "fp16":
        print(f"\n[grad clip] fp16 scaler trajectory (step, scale, tracker, 1 / scale): {traj[None]}")
        assert len({t[1] for t in traj[None]}) > 1              # (the scale moved: growth after two clean steps, or a back-off)


def test_captured_step_equals_eager_and_follows_a_host_change():
    """5. GraphedTrainStep on a clipping trainer against its eager twin over three replays, max_grad_norm quartered on the host between them;
    the step's "grad_norm" metric is stu_optimizer.grad_norm(); a twin at a hundredth of the bound ends elsewhere; enabling clipping after
    capture is refused."""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    args = _args()
    _, _, tr_d = _trainer(max_grad_norm=math.inf)               # the dry read
    tr_d.train_step(*args)
    M = 0.5 * float(tr_d.stu_optimizer.grad_norm())
    assert math.isfinite(M) and M > 0
    stu_g, tea_g, tr_g = _trainer(max_grad_norm=M)
    stu_e, tea_e, tr_e = _trainer(max_grad_norm=M)
    stu_k, tea_k, tr_k = _trainer(max_grad_norm=M / 100.0)
    gs = GraphedTrainStep(tr_g, *args, warmup=1)
    assert tr_g.fused_last and gs.one_graph and gs._fused_tail and gs._mextra == ["grad_norm"]
    tr_e.train_step(*args)
    tr_k.train_step(*args)
    assert gn.same_bits(float(tr_e.stu_optimizer.clip_coef()), gn.coef_host(float(tr_e.stu_optimizer.grad_norm()), M))
    assert float(tr_e.stu_optimizer.clip_coef()) < 1.0
    for it in range(3):
        if it == 1:
            for tr in (tr_g, tr_e, tr_k):
                tr.max_grad_norm = tr.max_grad_norm / 4.0
        gs.step(*args)
        tr_e.train_step(*args)
        tr_k.train_step(*args)
        torch.cuda.synchronize()
        _same(_snap(stu_g, tea_g, tr_g), _snap(stu_e, tea_e, tr_e), f"replay {it}")
        og, oe = tr_g.stu_optimizer, tr_e.stu_optimizer
        assert torch.equal(og.grad_norm(), oe.grad_norm()) and torch.equal(og.clip_coef(), oe.clip_coef())
        assert gn.same_bits(float(og.clip_coef()), gn.coef_host(float(og.grad_norm()), tr_g.max_grad_norm))
        assert gs._metrics_dict(gs._mvec)["grad_norm"] == float(og.grad_norm())
        assert gn.same_bits(float(og._dev[0][0][4]), 1.0)
    assert not torch.equal(stu_k.head.weight.detach(), stu_g.head.weight.detach())
    tr_g.max_grad_norm = None
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        gs.step(*args)
    gs.release()
    # enabling after capture
    _, _, tr_n = _trainer()
    gs_n = GraphedTrainStep(tr_n, *args, warmup=1)
    assert gs_n._mextra == []
    gs_n.step(*args)
    tr_n.max_grad_norm = 1.0
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        gs_n.step(*args)
    gs_n.release()


def test_fp16_skipped_step_with_clipping_on():
    """6. precision='fp16', use_sgd=True, clipping on: a step whose gradients are not finite leaves parameters and momentum buffers alone,
    does not tick, halves the loss scale and leaves grad_scale = 1 / S of the new S; the next step clips normally; fused tail and separate
    launches agree throughout."""
    from uda_poseestimation_amd import warp
    args = _args(seed=7)
    M = 1e-6
    snaps = {}
    for fuse in (True, False):
        stu, tea, tr = _trainer("fp16", M, use_sgd=True)
        tr.fuse_tail = fuse
        opt = tr.stu_optimizer
        opt.zero_grad()
        st = tr._forward_part(args[0], args[1], args[2], args[3], [args[4]], warp.recon_thetas(args[5], 4, 4.0, "cuda"),
                              [warp.recon_thetas(args[6], 4, 4.0, "cuda")])
        tr._loss_backward_part(st, None)
        assert stu._last_hd.precision == "fp16"
        ws = [p.detach().clone() for p in stu.parameters()]
        stu.backbone.bn1.weight.grad[5] = float("inf")
        tr._update()
        assert tr.fused_last is fuse
        sd = opt.state_dict()["param_groups"][0]
        assert sd["step"] == 0 and sd["loss_scale"] == 32768.0 and sd["growth_tracker"] == 0
        assert float(opt._dev[0][0][4]) == 1.0 / 32768.0 and float(opt._dev[0][0][5]) == 0.0
        for p, w in zip(stu.parameters(), ws):
            assert torch.equal(p.detach(), w)
            if p in opt.state:
                assert not opt.state[p]["momentum_buffer"].any()
        log = [_snap(stu, tea, tr)]
        tr.train_step(*args)
        assert tr.fused_last is fuse
        sd = opt.state_dict()["param_groups"][0]
        norm, coef = float(opt.grad_norm()), float(opt.clip_coef())
        assert sd["step"] == 1 and sd["loss_scale"] == 32768.0 and math.isfinite(norm) and norm > M
        assert gn.same_bits(coef, gn.coef_host(norm, M)) and 0.0 < coef < 1.0
        assert float(opt._dev[0][0][4]) == 1.0 / 32768.0
        assert all(torch.isfinite(p).all() for p in stu.parameters())
        log.append(_snap(stu, tea, tr) + [opt.grad_norm().clone(), opt.clip_coef().clone()])
        snaps[fuse] = log
    for i, (a, b) in enumerate(zip(snaps[True], snaps[False])):
        _same(a, b, f"fp16 SGD with clipping, stage {i}")
