"""The style pass of a captured step with k = 2 teacher views, on the MI355X at the smallest step the suite trusts: an
FDANet in both directions with seeded host draws, against an eager twin with the same draws from identical state - "enc_rest" summarises
the second view only when t2s was drawn, t2s transfers both views, a view not transferred is copied - and prefetch() with a list of views."""
import numpy as np
import pytest
import torch

from helpers import captured_twin as T

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
LO, HI = (-2.1179, -2.0357, -1.8044), (2.2489, 2.4285, 2.64)
SEED = 123


@pytest.fixture(autouse=True)
def _bf16(monkeypatch):
    from uda_poseestimation_amd.lib.models.pose_resnet import PoseResNet
    monkeypatch.setattr(PoseResNet, "default_precision", "bf16")


def _styled_trainer():
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    from uda_poseestimation_amd.lib.models import fda
    lo, hi = torch.tensor(LO).cuda(), torch.tensor(HI).cuda()
    return MeanTeacherTrainer(T.tiny().cuda(), T.tiny().cuda(), lr=1e-4, image_size=T.S, heatmap_size=T.S // 4, style_net=fda.FDANet(0.05, MEAN, STD),
                              recover=(lo, hi), rng=np.random.RandomState(SEED), s2t_freq=0.5, t2s_freq=0.5)


def test_two_views_with_a_style_net_captured_equal_the_eager_twin_and_prefetch_takes_a_list():
    from uda_poseestimation_amd.engine import GraphedTrainStep
    from uda_poseestimation_amd.lib.models import fda
    batches = [T.batch(s, 2) for s in (70, 71, 72, 73, 74)]
    probe, seen = np.random.RandomState(SEED), []
    for _ in batches:           # the step's draws, in the reference's order: rand, [uniform], rand, [uniform]
        a = probe.rand() < 0.5
        if a:
            probe.uniform(0, 1)
        b_ = probe.rand() < 0.5
        if b_:
            probe.uniform(0, 1)
        seen.append((a, b_))
    print("style decisions (s2t, t2s) per step:", seen)
    assert any(t2s for _, t2s in seen[1:]) and any(not t2s for _, t2s in seen[1:]), seen       # both rules of "enc_rest" are exercised by replays
    tr_g, tr_e = _styled_trainer(), _styled_trainer()
    gs = GraphedTrainStep(tr_g, *batches[0], warmup=1)             # the warm-up step IS step 1 (on batch 0, with step 1's draws)
    assert set(gs.g_style) == {"enc", "enc_rest", "s2t", "t2s"} and {"sp_t", "sp_t1", "x_t_tea_in", "x_t_tea_in1"} <= set(gs.static)
    tr_e.train_step(*batches[0])
    for i, bt in enumerate(batches[1:]):
        if i == len(batches) - 2:       # the last step takes its batch through prefetch(): a list of views into the staging buffers
            gs.prefetch(*bt[:5])
            og = gs.step(None, None, None, None, None, bt[5], bt[6])
            assert all(torch.equal(gs.static[key], v) for key, v in zip(("x_t_tea", "x_t_tea1"), bt[4]))
        else:
            og = gs.step(*bt)
        oe = tr_e.train_step(*bt)
        for name in ("loss_all", "loss_s", "loss_c"):
            assert torch.isfinite(og[name]) and float(og[name]) == float(oe[name]), (i, name, float(og[name]), float(oe[name]))
        assert torch.equal(og["y_t_tea_recon"], oe["y_t_tea_recon"]), i
    for (n, pg), pe in zip(tr_g.student.named_parameters(), tr_e.student.parameters()):
        assert torch.equal(pg.detach(), pe.detach()), n
    sa, sb = tr_g.rng.get_state(), tr_e.rng.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]           # both consumed exactly the same host draws
    # the t2s graph transfers EVERY view from its own summary: a replay against the eager call, view by view
    st = gs.static
    st["alpha_t2s"].fill_(0.625)
    for which in ("enc", "enc_rest", "t2s"):
        gs.g_style[which].replay()
    for s in ("", "1"):
        want = fda.fda_transfer(st["x_t_tea" + s], st["x_s"], 0.05, 0.625, clamp=tr_g.recover, mean=MEAN, std=STD)
        assert torch.equal(st["x_t_tea_in" + s], want) and not torch.equal(want, st["x_t_tea" + s]), s
