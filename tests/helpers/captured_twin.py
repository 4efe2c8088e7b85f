"""What tests/test_gpu_captured_views.py and tests/test_gpu_captured_schedules.py share: the smallest step the suite trusts
(tests/test_gpu_steps.py: a [1,1,1,1] bottleneck PoseResNet, N = 4, K = 16, 128 x 128 images, 32 x 32 heat-maps), batches with k teacher
views, a trainer pair in identical state and the eager twin's step, driven through trainer._forward_backward with matrices that
warp.thetas_from_packed makes from the packed values the captured step stages."""
import copy

import numpy as np
import torch

N, K, S = 4, 16, 128


def tiny(seed=8):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(seed)
    return pr._pose_resnet("t", K, pr.Bottleneck_default, [1, 1, 1, 1], False, False)


def batch(seed, k=1, as_list=None):
    """(x_s, label_s, weight_s, x_t_stu, x_t_tea, aug_param_stu, aug_param_tea) on the device; x_t_tea / aug_param_tea are lists of k views
    (views 1 .. k-1 from synthetic.images / synthetic.aug_params) when k > 1 or as_list, else the tensor and the collated tuple."""
    from uda_poseestimation_amd import synthetic
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=seed)
    g = {n: (v.cuda() if torch.is_tensor(v) else v) for n, v in b.items()}
    views, augs = [g["x_t_tea"]], [g["aug_param_tea"]]
    rs = np.random.RandomState(1000 + seed)
    for i in range(1, k):
        views.append(synthetic.images(N, S, 100 * seed + i).cuda())
        augs.append(synthetic.aug_params(N, rs))
    if k == 1 and not as_list:
        views, augs = views[0], augs[0]
    return (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], views, g["aug_param_stu"], augs)


def trainer(seed=8, lr=1e-4, **attrs):
    """A trainer on two tiny networks (the teacher starts as the student: OldWeightEMA's constructor); attrs are set as attributes."""
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    tr = MeanTeacherTrainer(tiny(seed).cuda(), tiny(seed).cuda(), lr=lr, image_size=S, heatmap_size=S // 4)
    for n, v in attrs.items():
        setattr(tr, n, v)
    return tr


def copy_state(src, dst):
    """dst's networks (parameters and BatchNorm buffers) and optimizer state become src's, bit for bit."""
    dst.student.load_state_dict(src.student.state_dict())
    dst.teacher.load_state_dict(src.teacher.state_dict())
    # (a deep copy: torch's load keeps a state tensor that already has the parameter's dtype and device, and the twin's moments would BE
    # the captured step's - each step would then advance them twice)
    dst.stu_optimizer.load_state_dict(copy.deepcopy(src.stu_optimizer.state_dict()))
    torch.cuda.synchronize()
    assert not any(a.data_ptr() == b.data_ptr() for p, q in zip(src.student.parameters(), dst.student.parameters())
                   for a, b in zip(src.stu_optimizer.state[p].values(), dst.stu_optimizer.state[q].values()) if torch.is_tensor(a) and torch.is_tensor(b))


def eager_step(tr, b):
    """One eager step of the twin: trainer.train_step's parts, with the matrices made on the device from the packed aug_param values."""
    from uda_poseestimation_amd import warp
    x_s, label_s, weight_s, x_t_stu, views, aug_stu, augs = b
    if not isinstance(views, (list, tuple)):
        views, augs = [views], [augs]

    def thetas(ap):
        return warp.thetas_from_packed(warp.pack_aug_param(ap, N).cuda(), tr.ratio)[0]
    tr._occl = None
    out = tr._forward_backward(x_s, label_s, weight_s, x_t_stu, list(views), thetas(aug_stu), [thetas(ap) for ap in augs])
    tr._sync_grads()
    tr._update()
    return out


def params(net):
    return [p.detach().clone() for p in net.parameters()]


def drift(net_a, net_b, start):
    """||a - b|| / ||b - start|| over every parameter."""
    num = sum(float(((a.detach() - b.detach()) ** 2).sum()) for a, b in zip(net_a.parameters(), net_b.parameters()))
    den = sum(float(((b.detach() - q) ** 2).sum()) for b, q in zip(net_b.parameters(), start))
    return (num / max(den, 1e-30)) ** 0.5


def check_bars(og, oe):
    """The bars of tests/test_gpu_steps.py::test_captured_steps_equal_eager_steps_from_identical_state_with_varying_batches on one step."""
    la, le = float(og["loss_all"]), float(oe["loss_all"])
    ca, ce = float(og["loss_c"]), float(oe["loss_c"])
    print(f"  loss_all captured {la:.6e} eager {le:.6e}; loss_c captured {ca:.6e} eager {ce:.6e}")
    assert abs(la - le) <= 2e-3 * abs(le)
    assert abs(ca - ce) <= 5e-3 * abs(ce) + 1e-7


def check_drift(tr_g, tr_e, start):
    rs, rt = drift(tr_g.student, tr_e.student, start), drift(tr_g.teacher, tr_e.teacher, start)
    print(f"  student drift ratio {rs:.3e}, teacher drift ratio {rt:.3e}")
    assert rs < 0.2
    assert rt < 0.1
