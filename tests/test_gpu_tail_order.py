"""The step's exposed tail: work order of the grouped weight-gradient launches (udapose_policy.wgrad_order) and the split sums taken over
by the optimizer sweep (udapose_net_wgrad_pair_defer -> udapose_net_fused_update).  Neither changes what is computed, so every comparison
here is torch.equal on raw bits; no tolerance appears anywhere in this file."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 16
PLANS = {
    # the benched plan: PoseResNet-101, N = 32, 256 x 256, production split length
    "r101_n32_256": dict(layers=[3, 4, 23, 3], N=32, S=256, policy={}),
    # a small plan whose layer1 / layer2 / last deconvolution / head / stem are split (8-stage splits)
    "r50_n4_128": dict(layers=[3, 4, 6, 3], N=4, S=128, policy={"wgrad_stages": 8}),
}


def _net(layers, policy):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(7)
    m = pr._pose_resnet("t", K, pr.Bottleneck_default, list(layers), False, False).cuda().train()
    m.precision = "bf16"
    m.policy = dict(policy)
    return m


def _phase1(net, N, S, seeds):
    """Forward + gradient chain of one pass per seed from fixed synthetic inputs; returns the plan and each pass's (act, ws) arenas."""
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


def _order_default():
    from uda_poseestimation_amd import _hip
    return _hip.policy().wgrad_order


def _set_order(hd, order):
    from uda_poseestimation_amd import _hip
    pol = _hip.Policy()
    assert hd.L.udapose_net_get_policy(hd.h, C.byref(pol)) == 0
    pol.wgrad_order = order
    assert hd.L.udapose_net_set_policy(hd.h, C.byref(pol)) == 0


@pytest.mark.parametrize("plan", list(PLANS))
def test_work_order_does_not_change_a_single_gradient_bit(plan):
    """Order 0 (deal order by unit load, the parent's) against order 1 (longest work-groups first, levelled lists) on the same phase-1 state:
    the pair launch of two passes into two buffers, a single pass (phase 2 of the backward) and a pair with overlapping gradient tensors
    (one buffer, betas 0 then 1: two launches in order) - every gradient tensor of every pass identical.  A table of the other order is not
    found by a launch (UDAPOSE_ERR_NOT_PREPARED) until udapose_net_bind_grads has built it."""
    assert _order_default() == 1
    from uda_poseestimation_amd import _hip
    cfg = PLANS[plan]
    net = _net(cfg["layers"], cfg["policy"])
    hd, (A, B) = _phase1(net, cfg["N"], cfg["S"], (11, 21))
    pa, _, _ = net._pointers()
    nl = [p.numel() for p in net.parameters()]
    tot = sum(nl)
    p = _hip.ptr
    gen = torch.Generator(device="cuda").manual_seed(3)
    init_a, init_b = torch.randn(tot, device="cuda", generator=gen), torch.randn(tot, device="cuda", generator=gen)
    res = {}
    for order in (0, 1):
        _set_order(hd, order)
        out = {}
        # (a) the pair launch, two buffers, overwrite
        ba, bb = init_a.clone(), init_b.clone()
        ga, gb = _flat_ptrs(ba, nl), _flat_ptrs(bb, nl)
        if order == 0:      # (the plan's tables were bound under the default order, 1: tables of another order do not qualify for this one)
            rc = hd.L.udapose_net_wgrad_pair(hd.h, _hip.stream(), p(A[0]), p(A[1]), ga, C.c_float(0.0), p(B[0]), p(B[1]), gb, C.c_float(0.0), 0)
            assert rc == -4, rc
        assert hd.L.udapose_net_bind_grads(hd.h, ga) == 0 and hd.L.udapose_net_bind_grads(hd.h, gb) == 0
        assert hd.L.udapose_net_wgrad_pair(hd.h, _hip.stream(), p(A[0]), p(A[1]), ga, C.c_float(0.0), p(B[0]), p(B[1]), gb, C.c_float(0.0), 0) == 0
        torch.cuda.synchronize()
        out["pair"] = (ba, bb)
        # (b) a single pass, accumulating onto random contents
        bs = init_a.clone()
        gs = _flat_ptrs(bs, nl)
        assert hd.L.udapose_net_bind_grads(hd.h, gs) == 0
        assert hd.L.udapose_net_backward_phase(hd.h, _hip.stream(), None, pa, p(hd.wpack), p(A[0]), p(A[1]), gs, C.c_float(1.0), 0, 2) == 0
        torch.cuda.synchronize()
        out["single"] = (bs,)
        # (c) overlapping gradient tensors: B accumulates onto A's result in ONE buffer (two launches in order)
        bo = init_b.clone()
        go = _flat_ptrs(bo, nl)
        assert hd.L.udapose_net_bind_grads(hd.h, go) == 0
        assert hd.L.udapose_net_wgrad_pair(hd.h, _hip.stream(), p(A[0]), p(A[1]), go, C.c_float(0.0), p(B[0]), p(B[1]), go, C.c_float(1.0), 0) == 0
        torch.cuda.synchronize()
        out["one_buffer"] = (bo,)
        res[order] = out
    for what in ("pair", "single", "one_buffer"):
        for a, b in zip(res[0][what], res[1][what]):
            assert torch.equal(a, b), f"{plan} {what}: order 1 changed a gradient, max|d| {float((a - b).abs().max()):.3e}"
    assert not torch.equal(res[1]["pair"][0], init_a)          # (the launches wrote something)


def _tiny_trainer(seed, wd, gscale, defer):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    nets = []
    for _ in range(2):
        torch.manual_seed(seed)
        m = pr._pose_resnet("t", K, pr.Bottleneck_default, [2, 1, 2, 1], False, False)
        m.policy = {"wgrad_stages": 8}          # (8-stage splits: layer1, layer2, the last deconvolution, the head and the stem are split at 128 x 128)
        nets.append(m.cuda())
    tr = MeanTeacherTrainer(nets[0], nets[1], lr=1e-3, image_size=128, heatmap_size=32, precision="bf16")
    tr.sum_splits_in_tail = defer
    grp = tr.stu_optimizer.param_groups[0]
    grp["weight_decay"] = wd
    if gscale != 1.0:
        grp["grad_scale"] = gscale
    return nets[0], nets[1], tr


def _state(stu, tea, tr):
    out = [p.detach().clone() for p in list(stu.parameters()) + list(tea.parameters())]
    for p in stu.parameters():
        st = tr.stu_optimizer.state.get(p)
        if st:
            out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    out += [stu._last_hd.wpack.clone(), tea._last_hd.wpack.clone()]     # (student forward + data-gradient packs, teacher forward packs)
    return out


def _batches(n):
    from uda_poseestimation_amd import synthetic
    out = []
    for sd in range(n):
        b = synthetic.mean_teacher_batch(4, num_keypoints=K, image_size=128, heatmap_size=32, seed=70 + sd)
        g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
        out.append((g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"]))
    return out


@pytest.mark.parametrize("wd,gscale", [(0.0, 1.0), (1e-2, 0.5)], ids=["plain", "wd_gscale"])
def test_split_sums_inside_the_sweep_equal_the_separate_launch_over_20_captured_steps(wd, gscale):
    """20 captured bf16 steps with the split layers' partial tiles added inside the optimizer sweep against 20 with split_sum_k as its own
    launch, from the same state and batches: parameters, Adam moments, teacher and the weight packs of both plans identical after EVERY step;
    once plain, once with weight decay and a gradient scale, so that every branch of the sweep's update sees a split layer."""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    batches = _batches(3)
    runs = {}
    for defer in (False, True):
        stu, tea, tr = _tiny_trainer(5, wd, gscale, defer)
        gs = GraphedTrainStep(tr, *batches[0], warmup=2)
        assert tr.fused_last
        # (the first eager step binds the update table after its weight gradients: from the second step on, and in the capture, the sums are deferred)
        assert (stu.split_sums_deferred > 0) == defer, stu.split_sums_deferred
        snaps = []
        for it in range(20):
            gs.step(*batches[it % 3])
            torch.cuda.synchronize()
            snaps.append(_state(stu, tea, tr))
        runs[defer] = snaps
        gs.release()
    for it, (a, b) in enumerate(zip(runs[False], runs[True])):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), f"step {it}: tensor {i} differs between the deferred and the separate split sums"
    assert not torch.equal(runs[True][0][0], runs[True][-1][0])       # (training moved the weights)


def test_captured_step_with_order_and_deferred_sums_replays_to_the_bit_of_its_eager_twin():
    """The captured step with the new work order and the deferred split sums, replayed 50 times, against an eager twin that runs the same
    50 steps launch by launch: parameters, moments, teacher and packs identical at the end, losses identical at every step."""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    batches = _batches(3)
    stu_g, tea_g, tr_g = _tiny_trainer(9, 0.0, 1.0, True)
    stu_e, tea_e, tr_e = _tiny_trainer(9, 0.0, 1.0, True)
    gs = GraphedTrainStep(tr_g, *batches[0], warmup=2)
    for _ in range(2):                       # (the twin takes the capture's two warm-up steps eagerly)
        tr_e.train_step(*batches[0])
    assert stu_g.split_sums_deferred > 0 and stu_e.split_sums_deferred > 0
    for it in range(50):
        lg = gs.step(*batches[it % 3])["loss_all"].clone()
        le = tr_e.train_step(*batches[it % 3])["loss_all"].clone()
        assert torch.equal(lg, le), f"step {it}: loss {float(lg)} (captured) != {float(le)} (eager)"
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(_state(stu_g, tea_g, tr_g), _state(stu_e, tea_e, tr_e))):
        assert torch.equal(x, y), f"tensor {i} differs between the replayed graph and the eager twin"
    gs.release()


def test_pending_split_sum_is_flushed_on_demand_and_guards_the_next_weight_gradients():
    """A deferred split sum that no update consumed: finish_grads() completes p.grad (the sums as their own launch), equal to a run that never
    deferred; and at the C ABI a weight-gradient call on a plan with a pending sum fails with UDAPOSE_ERR_NOT_PREPARED instead of computing
    on stale tensors."""
    from uda_poseestimation_amd import warp
    batches = _batches(1)
    args = batches[0]
    grads = {}
    for defer in (False, True):
        stu, tea, tr = _tiny_trainer(3, 0.0, 1.0, defer)
        for _ in range(2):
            tr.train_step(*args)
        theta = lambda ap: warp.recon_thetas(ap, 4, 4.0, "cuda")
        tr._forward_backward(args[0], args[1], args[2], args[3], [args[4]], theta(args[5]), [theta(args[6])])
        torch.cuda.synchronize()
        if defer:
            hd = stu._split_sum_hd
            assert hd is not None
            # any other weight-gradient call on this plan is refused while the sum is pending
            pa, _, _ = stu._pointers()
            rc = hd.L.udapose_net_backward_phase(hd.h, None, None, pa, None, None, None, stu._grad_ptrs[1], C.c_float(0.0), 0, 2)
            assert rc == -4, rc
        stu.finish_grads()
        torch.cuda.synchronize()
        assert getattr(stu, "_split_sum_hd", None) is None
        grads[defer] = [p.grad.detach().clone() for p in stu.parameters() if p.grad is not None]
    assert len(grads[False]) == len(grads[True])
    for a, b in zip(grads[False], grads[True]):
        assert torch.equal(a, b)
