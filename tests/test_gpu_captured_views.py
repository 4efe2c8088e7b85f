"""GraphedTrainStep with k teacher views and the agreement merge, on the MI355X, at the smallest step the suite trusts
(tests/helpers/captured_twin.py).  The captured step and an eager twin start every comparison from IDENTICAL state: the twin takes the
captured trainer's networks, BatchNorm buffers and optimizer state after the warm-up step, bit for bit, and is then driven through
trainer._forward_backward with matrices warp.thetas_from_packed makes from the same packed values.  The teacher's forward, the re-warp,
mean_views / merge_views and the mask's select have no atomics: the first replay's teacher side is compared bit for bit."""
import pytest
import torch

from helpers import captured_twin as T

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _bf16(monkeypatch):
    from uda_poseestimation_amd.lib.models.pose_resnet import PoseResNet
    monkeypatch.setattr(PoseResNet, "default_precision", "bf16")


def _pair(k, **attrs):
    """A captured step on k views (its warm-up step is step 1, on batch 0) and an eager twin in the state that step left."""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    tr_g, tr_e = T.trainer(**attrs), T.trainer(**attrs)
    start = T.params(tr_g.student)
    gs = GraphedTrainStep(tr_g, *T.batch(40, k), warmup=1)
    T.copy_state(tr_g, tr_e)
    return gs, tr_g, tr_e, start


@pytest.mark.parametrize("k", [2, 3])
def test_k_views_captured_equal_the_eager_twin(k):
    """1. view_merge = None: the first replay's y_t_tea_recon and tea_mask bit for bit, then three more steps inside the bars."""
    gs, tr_g, tr_e, start = _pair(k)
    assert gs.k == k and gs.static["aug"].shape == (1 + k, T.N, 6)
    b = T.batch(41, k)
    og, oe = gs.step(*b), T.eager_step(tr_e, b)
    same_recon = torch.equal(og["y_t_tea_recon"], oe["y_t_tea_recon"])
    diff = float((og["y_t_tea_recon"].float() - oe["y_t_tea_recon"].float()).abs().max())
    print(f"k = {k}: y_t_tea_recon equal {same_recon} (max |diff| {diff:.3e}), tea_mask differs in "
          f"{int((og['tea_mask'] != oe['tea_mask']).sum())} of {og['tea_mask'].numel()}")
    assert same_recon
    assert torch.equal(og["tea_mask"], oe["tea_mask"])
    T.check_bars(og, oe)
    for seed in (42, 43, 44):
        b = T.batch(seed, k)
        T.check_bars(gs.step(*b), T.eager_step(tr_e, b))
    T.check_drift(tr_g, tr_e, start)


def test_trimmed_merge_is_captured_and_follows_the_radius():
    """2. k = 3, view_merge = "trimmed", view_min = 2: the merge's outputs bit for bit with the twin; view_radius = 0 reaches the replay."""
    gs, tr_g, tr_e, start = _pair(3, view_merge="trimmed", view_min=2)
    b = T.batch(41, 3)
    og, oe = gs.step(*b), T.eager_step(tr_e, b)
    for name in ("view_agree", "view_n_inliers", "view_spread2", "tea_mask", "y_t_tea_recon"):
        same = torch.equal(og[name], oe[name])
        print(f"{name}: equal {same}")
        assert same, name
    n_before = og["view_n_inliers"].clone()
    # the same inputs again at radius 0: only views whose peak IS the medoid's stay inliers
    tr_g.view_radius = 0.0
    n_zero = gs.step(*b)["view_n_inliers"].clone()
    print(f"inliers at radius 2: {n_before.flatten().tolist()}\ninliers at radius 0: {n_zero.flatten().tolist()}")
    assert int(n_zero.min()) >= 1                      # the medoid is its own inlier (every view of these batches has a positive maximum)
    assert bool((n_zero != n_before).any())


def test_refusals():
    """3. view_merge with a single view, another count than the step was built with, more than eight views."""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    tr = T.trainer(view_merge="trimmed")
    with pytest.raises(ValueError, match="view_merge"):
        GraphedTrainStep(tr, *T.batch(40, 1), warmup=1)
    b9 = T.batch(40, 9)
    with pytest.raises(NotImplementedError, match="at most 8"):
        GraphedTrainStep(T.trainer(), *b9, warmup=1)
    gs = GraphedTrainStep(T.trainer(), *T.batch(40, 2), warmup=1)
    with pytest.raises(ValueError, match=r"k = 2 .* 3"):
        gs.step(*T.batch(41, 3))
    with pytest.raises(NotImplementedError, match="at most 8"):
        gs.step(*b9)


def test_one_view_through_the_list_form_gives_the_bits_of_the_tensor_form():
    """4. [x_t_tea], [aug_param_tea] against the tensor form: two captured steps built independently from identical state, every student
    and teacher parameter equal after three replays.  (The stem's weight gradient accumulates with fp32 atomics whose order the two
    runs need not share: should this ever differ, the difference is printed per tensor before the assertion.)"""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    trs = [T.trainer(), T.trainer()]
    steps = [GraphedTrainStep(trs[0], *T.batch(40, 1), warmup=1), GraphedTrainStep(trs[1], *T.batch(40, 1, as_list=True), warmup=1)]
    assert steps[1].k == 1 and set(steps[0].static) == set(steps[1].static)
    for seed in (41, 42, 43):
        steps[0].step(*T.batch(seed, 1))
        steps[1].step(*T.batch(seed, 1, as_list=True))
    torch.cuda.synchronize()
    for which in ("student", "teacher"):
        pairs = list(zip(getattr(trs[0], which).named_parameters(), getattr(trs[1], which).parameters()))
        bad = [(n, float((a.detach() - c.detach()).abs().max())) for (n, a), c in pairs if not torch.equal(a.detach(), c.detach())]
        print(f"{which}: {len(bad)} of {len(pairs)} tensors differ {bad[:4]}")
        assert not bad, which
