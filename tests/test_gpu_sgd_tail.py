"""The one-sweep optimizer tail (opt_tail_k: optimizer + EMA + both networks' weight packs) for SGD with momentum and for parameter
groups (PoseResNet.get_parameters: the backbone at a tenth of the rate), through udapose_net_bind_update_groups /
udapose_net_fused_update_groups.  The sweep replaces launches whose arithmetic it repeats expression for expression, so every comparison
here is torch.equal on raw bits; no tolerance appears anywhere in this file."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 16


@pytest.fixture(autouse=True)
def _bf16_unless_stated(monkeypatch):
    """Networks start in 'bf16' (BASELINE.json's benched precision) unless a test sets another precision."""
    from uda_poseestimation_amd.lib.models.pose_resnet import PoseResNet
    monkeypatch.setattr(PoseResNet, "default_precision", "bf16")


def _net(seed, prec="bf16", finetune=False):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(seed)
    m = pr._pose_resnet("t", K, pr.Bottleneck_default, [2, 1, 1, 1], False, False, finetune).cuda()
    m.precision = prec
    return m


def _twin(make_opt, prec="bf16", finetune=False):
    from uda_poseestimation_amd.utils import OldWeightEMA
    s_, t_ = _net(3, prec, finetune), _net(4, prec, finetune)
    opt = make_opt(s_)
    ema = OldWeightEMA(t_, s_, alpha=0.9)
    with torch.no_grad():                       # teacher != student, so that the EMA is visible
        for p in t_.parameters():
            p.mul_(1.01)
    return s_, t_, opt, ema


def _tail_against_separate_launches(make_opt, names, prec="bf16", finetune=False, steps=3, before_step=None):
    """Twin A: optimizer.step() (one launch per group), ema.step(), prepare() (the packs); twin B: fused_tail_step on a bit copy of A's
    gradients.  Everything the sweep writes is compared after every step."""
    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(1)).cuda()
    R = torch.randn(2, K, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()
    (sa, ta, oa, ea), (sb, tb, ob, eb) = _twin(make_opt, prec, finetune), _twin(make_opt, prec, finetune)
    for step in range(steps):
        if before_step is not None:
            before_step(step, oa)
            before_step(step, ob)
        sa.zero_grad(set_to_none=True); sb.zero_grad(set_to_none=True)
        (sa(x) * R).sum().backward()
        (sb(x) * R).sum().backward()
        with torch.no_grad():
            ta(x); tb(x)
        sb._flat_grad.copy_(sa._flat_grad)
        oa.step(); ea.step()
        assert ob.fused_tail_step(sb, tb, eb) is True
        hd_a, hd_b, ht_b = sa._last_hd, sb._last_hd, tb._last_hd
        assert hd_b.precision == prec
        sa.prepare(x)                               # A re-packs from its masters the ordinary way
        with torch.no_grad():
            ta.prepare(x)
        for (n, pa), (_, pb) in zip(sa.named_parameters(), sb.named_parameters()):
            assert torch.equal(pa.detach(), pb.detach()), (step, n)
            if pa.grad is not None:
                for nm in names:
                    assert torch.equal(oa.state[pa][nm], ob.state[pb][nm]), (step, n, nm)
        for (n, pa), (_, pb) in zip(ta.named_parameters(), tb.named_parameters()):
            assert torch.equal(pa.detach(), pb.detach()), (step, "teacher", n)
        assert torch.equal(hd_a.wpack, hd_b.wpack), "student packs differ"
        # the teacher plan holds forward packs only: compare through a forward (eval-free: same batch statistics)
        with torch.no_grad():
            assert torch.equal(ta(x), tb(x))
        assert hd_b.wpack_version == (sb.version_key(), True) and ht_b.wpack_version == (tb.version_key(), False)
    ga, gb = oa.state_dict()["param_groups"], ob.state_dict()["param_groups"]
    assert len(ga) == len(gb)
    assert all(a["step"] == b["step"] == steps for a, b in zip(ga, gb)), ([a["step"] for a in ga], [b["step"] for b in gb])
    fc = sb.backbone.fc.weight
    assert fc.grad is None and fc not in ob.state
    return sa, sb, oa, ob


SGD_CASES = [
    ("script", dict(momentum=0.9, weight_decay=1e-4, nesterov=True), "bf16"),          # train_human.py:136-137
    ("plain", dict(momentum=0.9, weight_decay=0.0, nesterov=False), "bf16"),
    ("grad_scale", dict(momentum=0.9, weight_decay=1e-4, nesterov=True, grad_scale=0.5), "bf16"),
    ("script_fp16_build", dict(momentum=0.9, weight_decay=1e-4, nesterov=True), "fp16"),
]


@pytest.mark.parametrize("case", SGD_CASES, ids=[c[0] for c in SGD_CASES])
def test_sgd_tail_is_bit_identical_to_sgd_then_ema_then_pack(case):
    """1. FusedSGD.fused_tail_step against FusedSGD.step(), ema.step(), prepare() on identical gradients and state over three steps (the
    first initialises the momentum buffer, the later ones use it): parameters, momentum buffers, teacher, the student's whole pack buffer and
    the teacher's forward output; backbone.fc (no gradient) gets the EMA only."""
    from uda_poseestimation_amd import optim as fo
    _, kw, prec = case
    _, sb, _, ob = _tail_against_separate_launches(lambda s_: fo.FusedSGD(s_.parameters(), lr=1e-2, **kw), ("momentum_buffer",), prec)
    assert any(float(ob.state[p]["momentum_buffer"].abs().max()) > 0 for p in sb.parameters() if p.grad is not None)


def _args(seed=6, n=4):
    from uda_poseestimation_amd import synthetic
    b = synthetic.mean_teacher_batch(n, num_keypoints=K, image_size=128, heatmap_size=32, seed=seed)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    return (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])


def _trainer(precision="bf16", finetune=False, grouped=False, **kw):
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    stu, tea = _net(4, precision, finetune), _net(4, precision, finetune)
    if grouped:
        kw["params"] = stu.get_parameters(1e-3)
    tr = MeanTeacherTrainer(stu, tea, lr=1e-3, image_size=128, heatmap_size=32, precision=precision, **kw)
    return stu, tea, tr


def _state(stu, tea, tr):
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


@pytest.mark.parametrize("sum_in_tail", [True, False], ids=["sum_in_tail", "sum_before"])
def test_sgd_trainer_eager_fused_tail_equals_the_separate_launches(sum_in_tail):
    """2. MeanTeacherTrainer(use_sgd=True) with and without the fused tail over three steps: every student and teacher parameter (and
    momentum buffer) equal; with the two passes' gradient buffers added inside the sweep, and with the axpy in front of it."""
    args = _args()
    res = {}
    for fuse in (True, False):
        stu, tea, tr = _trainer(use_sgd=True)
        tr.fuse_tail = fuse
        tr.sum_grads_in_tail = sum_in_tail
        assert tr._tail_sums_splits() is False
        for _ in range(3):
            tr.train_step(*args)
            assert tr.fused_last is fuse
            assert stu.pending_grad_sum() == 0
        res[fuse] = _state(stu, tea, tr)
    _same(res[True], res[False], "SGD fused tail vs separate launches")


def test_sgd_trainer_captured_follows_an_lr_change_and_equals_its_eager_twin():
    """3. GraphedTrainStep on a use_sgd=True trainer: one warm-up step, three replays with lr scaled by 0.1 on the host between them (as
    MultiStepLR would) against an eager twin given the same change; the device counter counts warm-up plus replays."""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    args = _args()
    stu_g, tea_g, tr_g = _trainer(use_sgd=True)
    stu_e, tea_e, tr_e = _trainer(use_sgd=True)
    gs = GraphedTrainStep(tr_g, *args, warmup=1)
    assert tr_g.fused_last and gs.one_graph and gs._fused_tail
    tr_e.train_step(*args)
    for it in range(3):
        if it == 1:
            for tr in (tr_g, tr_e):
                for grp in tr.stu_optimizer.param_groups:
                    grp["lr"] *= 0.1
        gs.step(*args)
        tr_e.train_step(*args)
        assert tr_e.fused_last
        torch.cuda.synchronize()
        _same(_state(stu_g, tea_g, tr_g), _state(stu_e, tea_e, tr_e), f"replay {it}")
    assert tr_g.stu_optimizer.state_dict()["param_groups"][0]["step"] == 4
    # (the lr change did reach the replays: a twin that keeps the old rate ends elsewhere)
    stu_k, tea_k, tr_k = _trainer(use_sgd=True)
    for _ in range(4):
        tr_k.train_step(*args)
    assert not torch.equal(stu_k.head.weight.detach(), stu_g.head.weight.detach())
    gs.release()


def test_sgd_fp16_skipped_step_leaves_student_and_counter_and_next_step_is_the_first():
    """4. precision='fp16', use_sgd=True: a step whose gradients are not finite leaves parameters and momentum buffers alone, moves the
    teacher, does not tick and halves the loss scale; the next step is then the FIRST one - it initialises the buffer (whatever it held: the
    buffers are filled with NaN in between) - and everything equals the unfused twin throughout."""
    from uda_poseestimation_amd import warp
    args = _args(seed=7)
    snaps = {}
    for fuse in (True, False):
        stu, tea, tr = _trainer(precision="fp16", use_sgd=True)
        tr.fuse_tail = fuse
        opt = tr.stu_optimizer
        log = []
        # a clean forward / backward, then one gradient poisoned before the update (tests/test_gpu_fp16.py)
        opt.zero_grad()
        st = tr._forward_part(args[0], args[1], args[2], args[3], [args[4]], warp.recon_thetas(args[5], 4, 4.0, "cuda"),
                              [warp.recon_thetas(args[6], 4, 4.0, "cuda")])
        tr._loss_backward_part(st, None)
        assert stu._last_hd.precision == "fp16"
        ws = [p.detach().clone() for p in stu.parameters()]
        ts = [p.detach().clone() for p in tea.parameters()]
        stu.backbone.bn1.weight.grad[5] = float("inf")
        tr._update()
        assert tr.fused_last is fuse
        sd = opt.state_dict()["param_groups"][0]
        assert sd["step"] == 0 and sd["loss_scale"] == 32768.0 and sd["growth_tracker"] == 0            # skipped, backed off
        for p, w in zip(stu.parameters(), ws):
            assert torch.equal(p.detach(), w)                                                           # the student did not move
            if p in opt.state:
                assert not opt.state[p]["momentum_buffer"].any()                                        # ... nor did its (zero) buffers
        for p_t, p_s, t0 in zip(tea.parameters(), stu.parameters(), ts):
            assert torch.equal(p_t.detach(), t0.mul(0.999).add(p_s.detach() * (1.0 - 0.999)))           # the EMA still ran
        log.append(_state(stu, tea, tr))
        for p in stu.parameters():
            if p in opt.state:
                opt.state[p]["momentum_buffer"].fill_(float("nan"))
        for it in range(2):
            tr.train_step(*args)
            assert tr.fused_last is fuse
            sd = opt.state_dict()["param_groups"][0]
            assert sd["step"] == it + 1 and sd["loss_scale"] == 32768.0
            if it == 0:         # the first counted step overwrote the buffers with its gradient
                assert all(torch.isfinite(opt.state[p]["momentum_buffer"]).all() for p in stu.parameters() if p in opt.state)
            log.append(_state(stu, tea, tr))
        assert all(torch.isfinite(p).all() for p in stu.parameters())
        snaps[fuse] = log
    for i, (a, b) in enumerate(zip(snaps[True], snaps[False])):
        _same(a, b, f"fp16 SGD, stage {i}")


def _grouped(cls, **kw):
    def make(s_):
        opt = cls(s_.get_parameters(1e-2), **kw)
        opt.param_groups[2]["weight_decay"] = 0.0          # (weight decay differs per group as well)
        return opt
    return make


def _lr_change(step, opt):
    if step == 2:
        opt.param_groups[1]["lr"] *= 0.1


@pytest.mark.parametrize("which,prec", [("adam", "bf16"), ("sgd", "bf16"), ("sgd", "fp16")])
def test_grouped_tail_is_bit_identical_to_per_group_steps(which, prec):
    """5a. get_parameters(lr) of a finetune=True net (three groups, the backbone at a tenth of the rate, weight decay differing too): the
    fused tail against the per-group step() launches + ema.step() + prepare() over three steps, one group's lr changed before the third."""
    from uda_poseestimation_amd import optim as fo
    if which == "adam":
        make, names = _grouped(fo.FusedAdam, lr=1e-2, weight_decay=1e-2), ("exp_avg", "exp_avg_sq")
    else:
        make, names = _grouped(fo.FusedSGD, lr=1e-2, momentum=0.9, weight_decay=1e-4, nesterov=True), ("momentum_buffer",)
    _, sb, _, ob = _tail_against_separate_launches(make, names, prec, finetune=True, before_step=_lr_change)
    lrs = [g["lr"] for g in ob.param_groups]
    assert len(lrs) == 3 and lrs[0] == pytest.approx(1e-3) and lrs[1] == pytest.approx(1e-3) and lrs[2] == pytest.approx(1e-2)
    assert fo.group_partition(ob.param_groups, sb.parameters()) is not None


@pytest.mark.parametrize("use_sgd", [False, True], ids=["adam", "sgd"])
def test_grouped_trainer_captured_equals_its_eager_twin(use_sgd):
    """5b. MeanTeacherTrainer(params=student.get_parameters(1e-3)) captured (one graph, the one-launch tail) against its eager twin, a group's
    lr changed between replays; and against a twin that runs the separate launches."""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    args = _args()
    stu_g, tea_g, tr_g = _trainer(finetune=True, grouped=True, use_sgd=use_sgd)
    stu_e, tea_e, tr_e = _trainer(finetune=True, grouped=True, use_sgd=use_sgd)
    stu_u, tea_u, tr_u = _trainer(finetune=True, grouped=True, use_sgd=use_sgd)
    tr_u.fuse_tail = False
    assert [g["lr"] for g in tr_g.stu_optimizer.param_groups] == pytest.approx([1e-4, 1e-3, 1e-3])
    gs = GraphedTrainStep(tr_g, *args, warmup=1)
    assert tr_g.fused_last and gs.one_graph and gs._fused_tail
    tr_e.train_step(*args)
    tr_u.train_step(*args)
    assert tr_e.fused_last and not tr_u.fused_last
    for it in range(3):
        if it == 1:
            for tr in (tr_g, tr_e, tr_u):
                tr.stu_optimizer.param_groups[0]["lr"] *= 0.1
        gs.step(*args)
        tr_e.train_step(*args)
        tr_u.train_step(*args)
    torch.cuda.synchronize()
    _same(_state(stu_g, tea_g, tr_g), _state(stu_e, tea_e, tr_e), "captured vs eager")
    _same(_state(stu_g, tea_g, tr_g), _state(stu_u, tea_u, tr_u), "captured vs separate launches")
    assert [g["step"] for g in tr_g.stu_optimizer.state_dict()["param_groups"]] == [4, 4, 4]
    gs.release()


def test_groups_that_disagree_on_betas_fall_back_and_still_match():
    """5c. Groups with different betas cannot share the sweep's by-value hyper-parameters: fused_tail_step returns False and the step equals
    the unfused one."""
    args = _args()
    res = {}
    for fuse in (True, False):
        stu, tea, tr = _trainer(finetune=True, grouped=True)
        tr.stu_optimizer.param_groups[0]["betas"] = (0.8, 0.999)
        tr.fuse_tail = fuse
        for _ in range(2):
            tr.train_step(*args)
            assert tr.fused_last is False
        res[fuse] = _state(stu, tea, tr)
        if fuse:
            assert tr.stu_optimizer.fused_tail_step(stu, tea, tr.tea_optimizer) is False
    _same(res[True], res[False], "disagreeing betas")


def test_single_group_adam_through_the_group_entry_points_gives_the_bits_of_fused_update():
    """6. One FusedAdam group: fused_tail_step (udapose_net_bind_update_groups / udapose_net_fused_update_groups) on twin A, the original
    udapose_net_bind_update / udapose_net_fused_update called by hand on twin B, identical gradients: parameters, both moments, teacher,
    every byte of the student's pack buffer and the teacher's forward on its packs equal over two steps."""
    from uda_poseestimation_amd import _hip, optim as fo
    ptr = _hip.ptr
    make = lambda s_: fo.FusedAdam(s_.parameters(), lr=1e-3, weight_decay=1e-2)
    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(1)).cuda()
    R = torch.randn(2, K, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()
    (sa, ta, oa, ea), (sb, tb, ob, eb) = _twin(make), _twin(make)
    for step in range(2):
        sa.zero_grad(set_to_none=True); sb.zero_grad(set_to_none=True)
        (sa(x) * R).sum().backward()
        (sb(x) * R).sum().backward()
        with torch.no_grad():
            ta(x); tb(x)
        sb._flat_grad.copy_(sa._flat_grad)
        assert oa.fused_tail_step(sa, ta, ea) is True
        # twin B through the original entry points
        hs, ht = sb._last_hd, tb._last_hd
        group = ob.param_groups[0]
        ps, tps = list(sb.parameters()), list(tb.parameters())
        assert ob._gather(0, group) is not None
        ent = ob._dev_state(0, group, ps[0].device)
        arr = lambda vals: (C.c_void_p * len(ps))(*vals)
        st = [ob.state[p] if p.grad is not None else None for p in ps]
        pa_s, pa_t = arr([p.data_ptr() for p in ps]), arr([p.data_ptr() for p in tps])
        ga = arr([p.grad.data_ptr() if p.grad is not None else None for p in ps])
        ma = arr([s_["exp_avg"].data_ptr() if s_ else None for s_ in st])
        va = arr([s_["exp_avg_sq"].data_ptr() if s_ else None for s_ in st])
        _hip.check(hs.L.udapose_net_bind_update(hs.h, ht.h, pa_s, ga, ma, va, pa_t, ptr(hs.wpack), ptr(ht.wpack)), "net_bind_update")
        group["step"] += 1
        _hip.check(hs.L.udapose_net_fused_update(hs.h, ht.h, _hip.stream(), pa_s, ga, ma, pa_t, ptr(hs.wpack), ptr(ht.wpack), float(group["lr"]),
                                                 0.9, 0.999, float(group["eps"]), float(group["weight_decay"]), int(group["step"]), 1.0,
                                                 ptr(ent[0]), float(eb.alpha), float(1.0 - eb.alpha), 1, 0), "net_fused_update")
        torch.cuda.synchronize()
        for (n, pa), (_, pb) in zip(sa.named_parameters(), sb.named_parameters()):
            assert torch.equal(pa.detach(), pb.detach()), (step, n)
            if pa.grad is not None:
                assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"]) and torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])
        for (n, pa), (_, pb) in zip(ta.named_parameters(), tb.named_parameters()):
            assert torch.equal(pa.detach(), pb.detach()), (step, "teacher", n)
        assert torch.equal(sa._last_hd.wpack, hs.wpack), "student packs differ"
        # (twin B's packs were written behind the module's back: tell it, as fused_tail_step does)
        from uda_poseestimation_amd.utils import _bump_versions
        _bump_versions(ps); _bump_versions(tps)
        sb.packs_refreshed(hs, True); tb.packs_refreshed(ht, False)
        # the teacher plan holds forward packs only (the rest of its buffer is never written): compare through a forward on the sweep's packs
        with torch.no_grad():
            assert torch.equal(ta(x), tb(x))
        assert ht.wpack_version == (tb.version_key(), False)
    assert oa.state_dict()["param_groups"][0]["step"] == ob.state_dict()["param_groups"][0]["step"] == 2
    # a table bound for one kind is stale for the other: the update only reports it
    hs, ht = sa._last_hd, ta._last_hd
    cache = oa._tail
    one = (C.c_void_p * 1)(oa._dev[0][0].data_ptr())
    wd = (C.c_float * 1)(0.0)
    rc = hs.L.udapose_net_fused_update_groups(hs.h, ht.h, _hip.stream(), 1, cache[1], cache[2], cache[3], cache[5], ptr(hs.wpack), ptr(ht.wpack),
                                              0.9, 0.0, 0.0, 1, 1, one, wd, 0.9, 0.1, 1, 0)
    assert rc == -4, rc
