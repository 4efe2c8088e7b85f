"""Mirrored views through MeanTeacherTrainer.train_step and GraphedTrainStep on the MI355X, at the smallest step the suite
trusts (tests/helpers/captured_twin.py: a [1,1,1,1] bottleneck PoseResNet, N = 4, K = 16, 128 x 128 images).  A step without flags is the
step it always was; with flags every re-warp of the step is the composition of tests/helpers/mirror_views_ref.py on the step's own heat-maps;
the captured step follows the flags of the batch it is given and agrees with an eager twin driven through trainer._forward_backward with
the same mirror tensors."""
import numpy as np
import pytest
import torch

from helpers import captured_twin as T
from helpers import mirror_views_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _bf16(monkeypatch):
    from uda_poseestimation_amd.lib.models.pose_resnet import PoseResNet
    monkeypatch.setattr(PoseResNet, "default_precision", "bf16")


def _flagged(b, flags):
    """The batch with its aug_params extended by flip flags: flags = one list of N values per view (student first), None = all zero."""
    b = list(b)
    views = isinstance(b[4], (list, tuple))
    augs = [b[5]] + (list(b[6]) if views else [b[6]])
    flags = flags if flags is not None else [[0] * T.N] * len(augs)
    augs = [list(ap) + [torch.tensor(f, dtype=torch.int64)] for ap, f in zip(augs, flags)]
    b[5], b[6] = augs[0], (augs[1:] if views else augs[1])
    return tuple(b)


def _recorded(monkeypatch):
    """Record every warp.warp_chain call of a step: (x, theta, mode, mirror, perm, out)."""
    from uda_poseestimation_amd import warp
    plain, calls = warp.warp_chain, []

    def spy(x, theta, mode="nearest", mirror=None, perm=None):
        out = plain(x, theta, mode, mirror, perm)
        calls.append((x.detach().clone(), theta, mode, mirror, perm, out.detach().clone()))
        return out
    monkeypatch.setattr(warp, "warp_chain", spy)
    return plain, calls


def _is_composition(plain, call):
    x, theta, mode, mirror, perm, out = call
    return torch.equal(out, R.compose_forward(lambda a, t: plain(a, t, mode), x.float(), theta, mirror.tolist(), perm))


@pytest.mark.parametrize("flip_pairs", [None, "body16"])
def test_eager_step_without_flags_is_unchanged(flip_pairs):
    """12. 5-entry aug_params of all-zero flags against the 4-entry ones, from identical state."""
    tr_a, tr_b = T.trainer(flip_pairs=flip_pairs), T.trainer(flip_pairs=flip_pairs)
    b = T.batch(41)
    out_a, out_b = tr_a.train_step(*b), tr_b.train_step(*_flagged(b, None))
    torch.cuda.synchronize()
    for name in ("y_t_tea_recon", "tea_mask", "loss_all"):
        assert torch.equal(out_a[name], out_b[name]), name
    for p, q in zip(tr_a.student.parameters(), tr_b.student.parameters()):
        assert torch.equal(p.detach(), q.detach())


def test_eager_step_with_flags_rewarps_by_the_composition(monkeypatch):
    """13. k = 2 views with mixed flags: every re-warp of the step, on the step's own heat-maps."""
    from uda_poseestimation_amd import warp
    tr = T.trainer(flip_pairs="body16")
    b = T.batch(41, 2)
    flags = [[1, 0, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]]           # (the second teacher view has no flagged sample: its warp stays the plain one)
    with pytest.raises(ValueError, match="flip_pairs"):
        T.trainer().train_step(*_flagged(b, flags))
    plain, calls = _recorded(monkeypatch)
    out = tr.train_step(*_flagged(b, flags))
    torch.cuda.synchronize()
    assert len(calls) == 3
    tea0, tea1, stu = calls
    assert tea0[3].tolist() == flags[1] and tea1[3] is None and stu[3].tolist() == flags[0]
    assert tea0[4] is not None and tea0[4].tolist() == warp.mirror_perm("body16", T.K, "cpu").tolist()
    assert _is_composition(plain, tea0) and _is_composition(plain, stu)
    assert torch.equal(tea1[5], plain(tea1[0], tea1[1]))
    assert torch.equal(out["y_t_tea_recon"], warp.mean_views([tea0[5], tea1[5]]))
    assert torch.equal(out["y_t_stu_recon"], stu[5])
    # the flags did change the result
    assert not torch.equal(tea0[5], plain(tea0[0], tea0[1]))
    assert torch.isfinite(out["loss_all"])


def test_adversarial_probe_takes_the_mirrored_rewarp(monkeypatch):
    """15. adv_eps set, one probe, a flagged student view: the probe's re-warp (the first warp of the student's heat-maps in the step) is
    the composition too."""
    tr = T.trainer(flip_pairs="body16", adv_eps=0.05, adv_norm="linf")
    b = T.batch(41)
    flags = [[1, 1, 0, 1], [0, 0, 0, 0]]
    plain, calls = _recorded(monkeypatch)
    out = tr.train_step(*_flagged(b, flags))
    torch.cuda.synchronize()
    assert len(calls) == 3                                      # the teacher's re-warp, the probe's, the student's
    tea, probe, stu = calls
    assert tea[3] is None
    for call in (probe, stu):
        assert call[3].tolist() == flags[0] and call[4] is not None
        assert _is_composition(plain, call)
    assert not torch.equal(probe[0], stu[0])                    # (the probe saw the clean view, the step the perturbed one)
    assert "x_t_stu_adv" in out and bool((out["adv_gnorm"] > 0).all())


# ---------------------------------------------------------------------------------------------------------------- captured
def _twin_step(tr, b, flags):
    """One eager step of the twin through trainer._forward_backward: matrices from the packed values as the captured step makes them, the
    occlusion's uniforms from the twin's own generator (in step with the captured trainer's), mirror tensors from `flags` (None: none)."""
    from uda_poseestimation_amd import warp
    x_s, label_s, weight_s, x_t_stu, views, aug_stu, augs = b
    packed = warp.pack_aug_param(aug_stu, T.N).cuda()
    thetas = lambda ap: warp.thetas_from_packed(warp.pack_aug_param(ap, T.N).cuda(), tr.ratio)[0]
    tr._occl = None
    if tr.occlude_rate > -1:
        tr._occl = ("device", warp.thetas_from_packed(packed, tr.ratio, want_fwd=False, want_back=True)[1], tr.draw_occlusion_uniforms(T.N, "cuda"))
    mir = [None] * (1 + len(views)) if flags is None else [torch.tensor(f, dtype=torch.uint8, device="cuda") for f in flags]
    out = tr._forward_backward(x_s, label_s, weight_s, x_t_stu, list(views), thetas(aug_stu), [thetas(ap) for ap in augs], mir[0], mir[1:])
    tr._sync_grads()
    tr._update()
    return out


FLAGS = {41: [[1, 0, 1, 0], [0, 1, 1, 0], [1, 1, 0, 0]], 42: [[0, 1, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0]],
         43: [[1, 1, 1, 1], [0, 0, 1, 0], [0, 1, 0, 1]], 44: [[0, 0, 0, 1], [1, 0, 0, 0], [1, 0, 1, 1]]}


@pytest.mark.parametrize("occlusion", [False, True])
def test_captured_step_follows_the_flags_like_its_eager_twin(occlusion):
    """14. k = 2, mixed flags that differ from step to step; then a step without flags."""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    attrs = dict(flip_pairs="body16")
    if occlusion:
        attrs.update(occlude_rate=0.5, occlude_thresh=-1e9, occlude_size=10, device_occlusion=True)
    tr_g, tr_e = T.trainer(rng=np.random.RandomState(123), **attrs), T.trainer(rng=np.random.RandomState(123), **attrs)
    start = T.params(tr_g.student)
    gs = GraphedTrainStep(tr_g, *T.batch(40, 2), warmup=1)
    assert gs.mirrored and gs.static["mirror"].shape == (3, T.N) and gs.static["mirror"].dtype == torch.uint8
    assert int(gs.static["mirror"].sum()) == 0                  # (4-entry structures stage zeros)
    T.copy_state(tr_g, tr_e)
    if occlusion:
        tr_e.draw_occlusion_uniforms(T.N)                       # (the warm-up step's draw)
    b = T.batch(41, 2)
    og, oe = gs.step(*_flagged(b, FLAGS[41])), _twin_step(tr_e, b, FLAGS[41])
    assert gs.static["mirror"].tolist() == FLAGS[41]
    same = torch.equal(og["y_t_tea_recon"], oe["y_t_tea_recon"])
    print(f"occlusion {occlusion}: y_t_tea_recon equal {same}, tea_mask differs in {int((og['tea_mask'] != oe['tea_mask']).sum())} elements")
    assert same and torch.equal(og["tea_mask"], oe["tea_mask"])
    T.check_bars(og, oe)
    # the flags matter: the un-mirrored re-warp of the same heat-maps is another tensor
    for seed in (42, 43, 44):
        b = T.batch(seed, 2)
        T.check_bars(gs.step(*_flagged(b, FLAGS[seed])), _twin_step(tr_e, b, FLAGS[seed]))
        assert gs.static["mirror"].tolist() == FLAGS[seed]
    T.check_drift(tr_g, tr_e, start)
    if occlusion:
        assert np.array_equal(tr_g.rng.get_state()[1], tr_e.rng.get_state()[1])
    # a step without flags after steps with them: the twin's UN-mirrored step, from the captured trainer's state
    T.copy_state(tr_g, tr_e)
    b = T.batch(45, 2)
    og, oe = gs.step(*b), _twin_step(tr_e, b, None)
    assert int(gs.static["mirror"].sum()) == 0
    assert torch.equal(og["y_t_tea_recon"], oe["y_t_tea_recon"]) and torch.equal(og["tea_mask"], oe["tea_mask"])
    T.check_bars(og, oe)


def test_captured_step_built_without_flip_pairs_refuses_flags():
    from uda_poseestimation_amd.engine import GraphedTrainStep
    tr = T.trainer()
    gs = GraphedTrainStep(tr, *T.batch(40, 2), warmup=1)
    assert not gs.mirrored and "mirror" not in gs.static
    with pytest.raises(ValueError, match="flip_pairs"):
        gs.step(*_flagged(T.batch(41, 2), FLAGS[41]))
    out = gs.step(*_flagged(T.batch(41, 2), None))              # all-zero flags: accepted
    assert torch.isfinite(out["loss_all"])
    tr.flip_pairs = "body16"                                    # frozen: the captured launches are the plain ones
    with pytest.raises(RuntimeError, match="flip_pairs"):
        gs.step(*T.batch(42, 2))
