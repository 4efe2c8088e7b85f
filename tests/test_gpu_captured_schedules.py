"""Values a captured step follows (trainer.scheduled), on the MI355X, at the smallest step the suite trusts
(tests/helpers/captured_twin.py): the loss weights, teacher_alpha and mask_ratio are read from device memory, so a replay follows a ramp of
them; with nothing scheduled a change is refused as before; the device-scalar forms compute the bits of the by-value forms."""
import pytest
import torch

from helpers import captured_twin as T

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _bf16(monkeypatch):
    from uda_poseestimation_amd.lib.models.pose_resnet import PoseResNet
    monkeypatch.setattr(PoseResNet, "default_precision", "bf16")


def _captured(**attrs):
    from uda_poseestimation_amd.engine import GraphedTrainStep
    tr = T.trainer(**attrs)
    return tr, GraphedTrainStep(tr, *T.batch(50), warmup=1)


def test_default_still_refuses_a_changed_weight():
    """5. scheduled = (): lambda_c is baked into the graph and a change raises at the next step."""
    tr, gs = _captured()
    assert tr.scheduled == ()
    gs.step(*T.batch(51))
    tr.lambda_c = 0.5
    with pytest.raises(RuntimeError, match="changed after capture"):
        gs.step(*T.batch(52))


def test_a_scheduled_lambda_c_reaches_the_replay():
    """6. captured at 1.0; at 0.0 loss_all IS loss_s; at 2.0 it is loss_s + 2 loss_c to one fp32 ulp."""
    tr, gs = _captured(scheduled=("lambda_c",))
    tr.lambda_c = 0.0
    out = gs.step(*T.batch(51))
    assert float(out["loss_c"]) > 0 and torch.equal(out["loss_all"], out["loss_s"])
    tr.lambda_c = 2.0
    out = gs.step(*T.batch(52))
    la, ls, lc = (out[n].float().reshape(()) for n in ("loss_all", "loss_s", "loss_c"))
    want = ls + 2.0 * lc
    ulp = torch.nextafter(want.abs(), want.abs() + 1) - want.abs()
    print(f"loss_all {float(la):.9e}, loss_s + 2 loss_c {float(want):.9e}, ulp {float(ulp):.3e}")
    assert float(lc) > 0 and float((la - want).abs()) <= float(ulp)
    tr.scheduled = ()                   # the list itself is frozen
    with pytest.raises(RuntimeError, match="scheduled"):
        gs.step(*T.batch(53))


@pytest.mark.parametrize("fuse_tail", [True, False])
def test_a_scheduled_teacher_alpha_reaches_both_ema_forms(fuse_tail):
    """7. alpha = 1: the teacher stands still while the student moves; alpha = 0: the teacher becomes the student, bit for bit - in the
    one-sweep tail and in udapose_ema_multi."""
    tr, gs = _captured(scheduled=("teacher_alpha",), fuse_tail=fuse_tail)
    assert bool(tr.fused_last) == fuse_tail
    tea0, stu0 = T.params(tr.teacher), T.params(tr.student)
    tr.tea_optimizer.alpha = 1.0
    gs.step(*T.batch(51))
    torch.cuda.synchronize()
    assert all(torch.equal(a.detach(), b) for a, b in zip(tr.teacher.parameters(), tea0))
    assert any(not torch.equal(a.detach(), b) for a, b in zip(tr.student.parameters(), stu0))
    tr.tea_optimizer.alpha = 0.0
    gs.step(*T.batch(52))
    torch.cuda.synchronize()
    assert any(not torch.equal(a.detach(), b) for a, b in zip(tr.teacher.parameters(), tea0))
    bad = [n for (n, a), s in zip(tr.teacher.named_parameters(), tr.student.parameters()) if not torch.equal(a.detach(), s.detach())]
    assert not bad, bad[:4]


@pytest.mark.parametrize("mode,ratios", [("global", (0.25, 0.75)), ("per_joint", (0.5, 0.75))])
def test_a_scheduled_mask_ratio_moves_the_kth_index(mode, ratios):
    """8. the replay's tea_mask against torch.kthvalue on the replay's own teacher map: the same `>`, so exact whatever ties there are."""
    tr, gs = _captured(scheduled=("mask_ratio",), mask_mode=mode)
    for i, ratio in enumerate(ratios):
        tr.mask_ratio = ratio
        out = gs.step(*T.batch(51 + i))
        act = out["y_t_tea_recon"].float().amax(dim=(2, 3))
        if mode == "global":
            k = int(ratio * act.numel())
            want = act > torch.kthvalue(act.flatten(), k).values
        else:
            k = int(ratio * T.N)
            want = act > torch.kthvalue(act, k, dim=0).values[None]
        print(f"{mode}, ratio {ratio}: k = {k}, {int(out['tea_mask'].sum())} of {act.numel()} joints kept")
        assert (T.N * T.K, k) in ((64, 16), (64, 48)) if mode == "global" else k in (2, 3)
        assert torch.equal(out["tea_mask"], want)
    if mode == "per_joint":
        tr.mask_ratio = 0.1             # k = int(0.1 * 4) = 0: the mode's own range check, on the host, before the replay
        with pytest.raises(ValueError, match="outside"):
            gs.step(*T.batch(53))


def test_the_device_scalar_forms_compute_the_same_bits():
    """9. two eager trainers from identical state, one with all five names scheduled, the same values, two steps: every parameter equal."""
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    from uda_poseestimation_amd.lib.models.loss import EntLoss, GramCoralLoss
    trs = []
    for scheduled in ((), MeanTeacherTrainer.SCHEDULABLE):
        tr = T.trainer(scheduled=scheduled, lambda_c=0.7, lambda_ent=0.3, lambda_coral=0.45, mask_ratio=0.3,
                       ent_criterion=EntLoss(), coral_criterion=GramCoralLoss(2))
        tr.tea_optimizer.alpha = 0.97
        trs.append(tr)
    for seed in (60, 61):
        outs = [tr.train_step(*T.batch(seed)) for tr in trs]
        assert "loss_ent" in outs[0] and "loss_coral" in outs[0]
        print(f"loss_all by value {float(outs[0]['loss_all']):.9e}, from device scalars {float(outs[1]['loss_all']):.9e}")
        assert torch.equal(outs[0]["tea_mask"], outs[1]["tea_mask"])
    torch.cuda.synchronize()
    assert trs[1].tea_optimizer.alpha_dev is not None and trs[0].tea_optimizer.alpha_dev is None
    for which in ("student", "teacher"):
        pairs = list(zip(getattr(trs[0], which).named_parameters(), getattr(trs[1], which).parameters()))
        bad = [(n, float((a.detach() - c.detach()).abs().max())) for (n, a), c in pairs if not torch.equal(a.detach(), c.detach())]
        print(f"{which}: {len(bad)} of {len(pairs)} tensors differ {bad[:4]}")
        assert not bad, which


def test_a_ramp_reaches_the_captured_step_as_it_reaches_the_eager_twin():
    """10. four steps of lambda_c = sigmoid_rampup(i, 4), alpha = ema_alpha_warmup(i, 0.999), mask_ratio 0.25 ... 0.75 on a captured step
    (scheduled) and on its eager twin (plain host values), inside the bars of the captured-against-eager comparison."""
    from uda_poseestimation_amd import utils
    from uda_poseestimation_amd.engine import GraphedTrainStep
    tr_g, tr_e = T.trainer(scheduled=("lambda_c", "teacher_alpha", "mask_ratio")), T.trainer()
    start = T.params(tr_g.student)
    gs = GraphedTrainStep(tr_g, *T.batch(50), warmup=1)
    T.copy_state(tr_g, tr_e)
    for i in range(4):
        for tr in (tr_g, tr_e):
            tr.lambda_c = utils.sigmoid_rampup(i, 4)
            tr.tea_optimizer.alpha = utils.ema_alpha_warmup(i, 0.999)
            tr.mask_ratio = 0.25 + 0.5 * i / 3
        b = T.batch(51 + i)
        T.check_bars(gs.step(*b), T.eager_step(tr_e, b))
    T.check_drift(tr_g, tr_e, start)


def test_the_single_group_tail_with_a_device_pair_gives_the_bits_of_the_by_value_call():
    """11. udapose_net_fused_update_dev (the EMA pair in device memory) against udapose_net_fused_update (the pair by value), both called by
    hand on twins with identical gradients, over two steps with two rates: parameters, both moments, the teacher, every byte of the student's pack
    buffer and the teacher's forward on its packs are equal."""
    import ctypes as C
    from uda_poseestimation_amd import _hip, optim as fo, utils
    ptr = _hip.ptr
    x = torch.randn(2, 3, T.S, T.S, generator=torch.Generator().manual_seed(1)).cuda()
    R = torch.randn(2, T.K, T.S // 4, T.S // 4, generator=torch.Generator().manual_seed(2)).cuda()
    twins = []
    for _ in range(2):
        s_, t_ = T.tiny(3).cuda(), T.tiny(4).cuda()
        opt = fo.FusedAdam(s_.parameters(), lr=1e-3, weight_decay=1e-2)
        ema = utils.OldWeightEMA(t_, s_, alpha=0.9)
        with torch.no_grad():                       # teacher != student, so that the EMA is visible
            for p in t_.parameters():
                p.mul_(1.01)
        twins.append((s_, t_, opt, ema))
    pair_dev = torch.zeros(2, dtype=torch.float32, device="cuda")
    for step, alpha in enumerate((0.9, 0.37)):
        pair_dev.copy_(torch.tensor(utils.ema_pair(alpha), dtype=torch.float32))
        for s_, t_, _, _ in twins:
            s_.zero_grad(set_to_none=True)
            (s_(x) * R).sum().backward()
            with torch.no_grad():
                t_(x)
        twins[1][0]._flat_grad.copy_(twins[0][0]._flat_grad)
        for which, (s_, t_, opt, ema) in enumerate(twins):
            hs, ht = s_._last_hd, t_._last_hd
            group = opt.param_groups[0]
            ps, tps = list(s_.parameters()), list(t_.parameters())
            assert opt._gather(0, group) is not None
            ent = opt._dev_state(0, group, ps[0].device)
            arr = lambda vals: (C.c_void_p * len(ps))(*vals)     # noqa: E731
            st = [opt.state[p] if p.grad is not None else None for p in ps]
            pa_s, pa_t = arr([p.data_ptr() for p in ps]), arr([p.data_ptr() for p in tps])
            ga = arr([p.grad.data_ptr() if p.grad is not None else None for p in ps])
            ma = arr([s1["exp_avg"].data_ptr() if s1 else None for s1 in st])
            va = arr([s1["exp_avg_sq"].data_ptr() if s1 else None for s1 in st])
            _hip.check(hs.L.udapose_net_bind_update(hs.h, ht.h, pa_s, ga, ma, va, pa_t, ptr(hs.wpack), ptr(ht.wpack)), "net_bind_update")
            group["step"] += 1
            head = (hs.h, ht.h, _hip.stream(), pa_s, ga, ma, pa_t, ptr(hs.wpack), ptr(ht.wpack), float(group["lr"]), 0.9, 0.999,
                    float(group["eps"]), float(group["weight_decay"]), int(group["step"]), 1.0, ptr(ent[0]))
            if which == 0:
                a, oma = utils.ema_pair(alpha)
                _hip.check(hs.L.udapose_net_fused_update(*head, a, oma, 1, 0), "net_fused_update")
            else:
                _hip.check(hs.L.udapose_net_fused_update_dev(*head, ptr(pair_dev), 1, 0), "net_fused_update_dev")
                assert hs.L.udapose_net_fused_update_dev(*head, None, 1, 0) == -1          # (UDAPOSE_ERR_ARG: no pair, nothing launched)
        torch.cuda.synchronize()
        (sa, ta, oa, _), (sb, tb, ob, _) = twins
        moved = False
        for (n, pa), pb in zip(sa.named_parameters(), sb.parameters()):
            assert torch.equal(pa.detach(), pb.detach()), (step, n)
            if pa.grad is not None:
                assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"]) and torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])
        for (n, pa), pb, ps_ in zip(ta.named_parameters(), tb.parameters(), sa.parameters()):
            assert torch.equal(pa.detach(), pb.detach()), (step, "teacher", n)
            moved = moved or not torch.equal(pa.detach(), ps_.detach())
        assert moved
        assert torch.equal(sa._last_hd.wpack, sb._last_hd.wpack), "student packs differ"
        for s_, t_, _, _ in twins:      # (the packs were written behind the modules' backs: tell them, as fused_tail_step does)
            utils._bump_versions(s_.parameters()); utils._bump_versions(t_.parameters())
            s_.packs_refreshed(s_._last_hd, True); t_.packs_refreshed(t_._last_hd, False)
        # the teacher plan holds forward packs only (the rest of its buffer is never written): compare through a forward on the sweep's packs
        with torch.no_grad():
            assert torch.equal(ta(x), tb(x))
