"""The mean-teacher step with warp_mode="bilinear" on the MI355X: what the mode changes and what it must not change in an eager step, the
captured step against its eager twin to the bit, the frozen-value report, and two independent runs agreeing to the bit (the backward of
the bilinear re-warp is a gather in a fixed order; float atomics there would break this).  The tiny network of the step tests, K = 4, N = 4,
64x64 images (16x16 heat-maps), bf16 executor (where a captured step equals its eager twin to the bit, tests/test_gpu_tail_order.py)."""
import pytest
import torch

from helpers.affine_bilinear_fp64 import chain_ref

pytestmark = pytest.mark.gpu

K, N, S = 4, 4, 64
LAYERS = [1, 1, 1, 1]
EPS = float(torch.finfo(torch.float32).eps)


def _net(sd=None):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(17)
    m = pr._pose_resnet("t", K, pr.Bottleneck_default, LAYERS, False, False)
    if sd is not None:
        m.load_state_dict(sd)
    return m.cuda()


@pytest.fixture(scope="module")
def setup():
    from uda_poseestimation_amd import synthetic
    sd = {k: v.clone() for k, v in _net().cpu().state_dict().items()}
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=41)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    args = (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])
    return sd, args


def _trainer(sd, mode):
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    return MeanTeacherTrainer(_net(sd), _net(sd), lr=1e-3, image_size=S, heatmap_size=S // 4, precision="bf16", warp_mode=mode)


def _state(tr):
    out = [p.detach().clone() for p in list(tr.student.parameters()) + list(tr.teacher.parameters())]
    for p in tr.student.parameters():
        st = tr.stu_optimizer.state.get(p)
        if st:
            out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    return out


def test_eager_step_bilinear_against_nearest_and_the_fp64_helper(setup):
    from uda_poseestimation_amd import utils as mt, warp
    from uda_poseestimation_amd.lib.models.loss import ConsLoss
    sd, args = setup
    assert any(float(torch.as_tensor(v).abs().max()) > 0 for v in (args[5][0], args[5][1][0], args[5][2][0]))      # (a non-trivial aug_param)
    tr_n, tr_b = _trainer(sd, "nearest"), _trainer(sd, "bilinear")
    twin = _net(sd)                     # the student before the step, for its heat-maps on x_t_stu
    twin.precision = tr_b.student.precision
    twin.train()
    y_t_stu = twin.forward_deferred_bn(args[3]).detach().float()          # (the call the step makes)
    o_n, o_b = tr_n.train_step(*args), tr_b.train_step(*args)
    torch.cuda.synchronize()
    # the source branch never sees the warp
    assert torch.equal(o_n["loss_s"], o_b["loss_s"]) and torch.equal(o_n["y_s"], o_b["y_s"])
    # the student's re-warped heat-maps: the fp64 helper on the twin's heat-maps, to the forward bar of tests/test_gpu_warp_bilinear.py
    th = warp.recon_thetas(args[5], N, tr_b.ratio, "cuda").cpu()
    y64 = chain_ref(y_t_stu.cpu(), th, torch.float64, "bilinear")
    y32 = chain_ref(y_t_stu.cpu(), th, torch.float32, "bilinear")
    yard = float((y32.double() - y64).abs().max())
    err = float((o_b["y_t_stu_recon"].float().cpu().double() - y64).abs().max())
    bar = max(4.0 * yard, 4.0 * EPS * float(y_t_stu.abs().max()))
    print(f"y_t_stu_recon (bilinear): max|device - fp64| {err:.3e}, fp32 helper {yard:.3e}, bar {bar:.3e}, max|y| {float(y_t_stu.abs().max()):.3e}")
    assert err <= bar
    # loss_c is the consistency loss of what the step returned
    for o in (o_n, o_b):
        want = ConsLoss()(o["y_t_stu_recon"], mt.rectify(o["y_t_tea_recon"], sigma=tr_b.sigma), tea_mask=o["tea_mask"])
        assert abs(float(o["loss_c"]) - float(want)) <= 1e-6 * abs(float(want)), (float(o["loss_c"]), float(want))
    # ... and the mode reached both re-warps (a silent fall-through to nearest would make these equal)
    print(f"loss_c nearest {float(o_n['loss_c']):.6e}, bilinear {float(o_b['loss_c']):.6e}")
    assert float(o_n["loss_c"]) != float(o_b["loss_c"])
    assert not torch.equal(o_n["y_t_tea_recon"], o_b["y_t_tea_recon"]) and not torch.equal(o_n["y_t_stu_recon"], o_b["y_t_stu_recon"])


@pytest.mark.parametrize("order", ["captured_first", "eager_first"])
def test_captured_bilinear_step_equals_its_eager_twin_to_the_bit(setup, order):
    from uda_poseestimation_amd.engine import GraphedTrainStep
    sd, args = setup

    def captured():
        tr = _trainer(sd, "bilinear")
        gs = GraphedTrainStep(tr, *args, warmup=1)          # (the warm-up step is a real step: the twin takes it eagerly)
        for _ in range(3):
            gs.step(*args)
        torch.cuda.synchronize()
        return tr, gs

    def eager():
        tr = _trainer(sd, "bilinear")
        for _ in range(4):
            tr.train_step(*args)
        torch.cuda.synchronize()
        return tr

    if order == "captured_first":
        (tr_g, gs), tr_e = captured(), eager()
    else:
        tr_e = eager()
        tr_g, gs = captured()
    sg, se = _state(tr_g), _state(tr_e)
    assert len(sg) == len(se)
    for i, (a, b) in enumerate(zip(sg, se)):
        assert torch.equal(a, b), f"{order}: tensor {i} differs between the captured and the eager bilinear step"
    name0 = next(n for n, _ in tr_g.student.named_parameters())
    assert not torch.equal(sg[0], sd[name0].cuda())          # (the weights moved)
    # the mode is captured with the step: changing it afterwards is reported like the other frozen values
    tr_g.warp_mode = "nearest"
    with pytest.raises(RuntimeError, match="warp_mode"):
        gs.step(*args)
    tr_g.warp_mode = "bilinear"
    gs.step(*args)
    gs.release()


def test_two_independent_bilinear_trainers_agree_to_the_bit(setup):
    sd, args = setup
    states = []
    for _ in range(2):
        tr = _trainer(sd, "bilinear")
        for _ in range(3):
            tr.train_step(*args)
        torch.cuda.synchronize()
        states.append(_state(tr))
    for i, (a, b) in enumerate(zip(*states)):
        assert torch.equal(a, b), f"tensor {i} differs between two runs of three bilinear steps"


def test_captured_step_refuses_heat_maps_beyond_the_lds_budget(setup):
    """A bilinear re-warp of planes over the LDS budget allocates scratch memory: a captured step must not, and says so before it captures."""
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    sd, args = setup
    tr = MeanTeacherTrainer(_net(sd), _net(sd), image_size=640, heatmap_size=160, precision="bf16", warp_mode="bilinear")
    big = torch.zeros(1, 3, 640, 640, device="cuda")
    with pytest.raises(RuntimeError, match="LDS budget"):
        GraphedTrainStep(tr, big, args[1], args[2], big, big, args[5], args[6])
