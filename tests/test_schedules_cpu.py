"""Scheduled values without a GPU: the ramp functions of utils.py against values recorded from the reference's own functions
(tests/golden/ramps.npz, made by tests/golden/make_golden_ramps.py), ema_alpha_warmup against its formula, the trainer's `scheduled`
switch and its refusals, and the five device-scalar exports in every place the ABI lives."""
import ctypes as C
import inspect
import os
import re
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ramps.npz")
NEW_EXPORTS = ("udapose_kth_mask_dev", "udapose_joint_kth_mask_dev", "udapose_ema_multi_dev", "udapose_net_fused_update_dev",
               "udapose_net_fused_update_groups_dev")


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def test_the_four_ramps_equal_the_recorded_reference_values_exactly():
    from uda_poseestimation_amd import utils
    g = np.load(GOLDEN)
    assert g["lengths"].tolist() == [0, 1, 7, 40]
    assert np.array_equal(g["progress"], np.arange(-10, 31) * 0.05) and g["progress"][0] == -0.5 and g["progress"][-1] == 1.5
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # (cosine_rampdown at length 0 is 0 / 0, in the reference as here)
        for L in g["lengths"].tolist():
            cur = g[f"current/{L}"]
            assert cur[0] == -2.0 and cur[-1] == L + 2.0 and np.all(np.diff(cur) == 0.5)
            got_up = [utils.sigmoid_rampup(float(c), L) for c in cur]
            got_down = [utils.cosine_rampdown(float(c), L) for c in cur]
            assert all(type(v) is float for v in got_up + got_down)
            assert _same(got_up, g[f"sigmoid_rampup/{L}"]), L
            assert _same(got_down, g[f"cosine_rampdown/{L}"]), L
    assert np.isnan(g["cosine_rampdown/0"]).all() and (g["sigmoid_rampup/0"] == 1.0).all()
    assert _same([utils.rev_sigmoid(float(p)) for p in g["progress"]], g["rev_sigmoid"])
    assert _same([utils.sigmoid(float(p)) for p in g["progress"]], g["sigmoid"])
    # the shapes the recipes rely on: the rise ends at 1, the fall starts at 1 and ends at 0, the two logistic curves mirror each other
    assert utils.sigmoid_rampup(40, 40) == 1.0 and utils.sigmoid_rampup(0, 40) == float(np.exp(-5.0))
    assert utils.cosine_rampdown(0, 7) == 1.0 and abs(utils.cosine_rampdown(7, 7)) < 1e-16
    assert abs(utils.sigmoid(0.5) - 0.5) < 1e-16 and abs(utils.sigmoid(0.3) + utils.rev_sigmoid(0.3) - 1.0) < 1e-15


def test_ema_alpha_warmup_is_its_formula():
    from uda_poseestimation_amd import utils
    for alpha in (0.0, 0.5, 0.99, 0.999):
        for step in (0, 1, 2, 9, 99, 998, 999, 1000, 10 ** 6):
            assert utils.ema_alpha_warmup(step, alpha) == min(1 - 1 / (step + 1), alpha)
    assert utils.ema_alpha_warmup(0, 0.999) == 0.0 and utils.ema_alpha_warmup(10 ** 6, 0.999) == 0.999
    assert utils.ema_pair(0.999) == (0.999, 1.0 - 0.999)


def test_the_dropin_utils_offers_the_ramps():
    """`from utils import sigmoid_rampup` as the reference's scripts spell it, with the package's directory first on sys.path."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from utils import sigmoid_rampup, cosine_rampdown, rev_sigmoid, sigmoid, ema_alpha_warmup; "
            "import utils, uda_poseestimation_amd.utils as u; assert utils is u and sigmoid_rampup is u.sigmoid_rampup; print(sigmoid_rampup(2, 4))"
            % os.path.join(ROOT, "uda_poseestimation_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert float(r.stdout.strip()) == float(np.exp(-5.0 * 0.25))


def test_scheduled_is_an_attribute_frozen_after_capture_and_refuses_unknown_names():
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    assert MeanTeacherTrainer.SCHEDULABLE == ("lambda_c", "lambda_ent", "lambda_coral", "teacher_alpha", "mask_ratio")
    assert "self.scheduled = ()" in inspect.getsource(MeanTeacherTrainer.__init__)
    assert "scheduled" not in inspect.signature(MeanTeacherTrainer.__init__).parameters
    src = inspect.getsource(GraphedTrainStep._frozen_hyper)
    assert "scheduled" in src and '("k", self.k)' in src and "view_min" in src
    assert "sync_schedule" in inspect.getsource(GraphedTrainStep.step) and "sync_view_radius" in inspect.getsource(GraphedTrainStep.step)
    tr = MeanTeacherTrainer.__new__(MeanTeacherTrainer)
    tr.scheduled = ("lambda_c", "momentum")
    with pytest.raises(ValueError, match="momentum"):
        tr.sync_schedule()
    tr.scheduled = "lambda_x"
    with pytest.raises(ValueError, match="lambda_x"):
        tr.sync_schedule()
    tr.scheduled = ("mask_ratio", "teacher_alpha")
    assert tr._scheduled_names() == ("mask_ratio", "teacher_alpha")


def test_the_words_of_a_schedule_are_what_the_by_value_calls_round_to():
    """The host side of sync_schedule, which needs no device: fp32 roundings of the weights, OldWeightEMA.step's pair, confidence_mask's k."""
    from uda_poseestimation_amd import utils
    from uda_poseestimation_amd.engine import MeanTeacherTrainer

    class _Ema:
        alpha = 0.999
    tr = MeanTeacherTrainer.__new__(MeanTeacherTrainer)
    tr.lambda_c, tr.lambda_ent, tr.lambda_coral, tr.mask_ratio, tr.mask_mode = 0.3, 0.1, 0.7, 0.3, "global"
    tr.tea_optimizer, tr._sched_pool = _Ema(), 64
    w = tr._schedule_words(MeanTeacherTrainer.SCHEDULABLE)
    assert w.dtype == np.float32 and w.shape == (8,)
    assert w[:5].tolist() == [np.float32(0.3), np.float32(0.1), np.float32(0.7), np.float32(0.999), np.float32(1.0 - 0.999)]
    assert int(w.view(np.int32)[5]) == int(0.3 * 64) == 19 and not w[6:].any()
    assert not tr._schedule_words(("lambda_ent",))[[0, 2, 3, 4, 5]].any()          # slots of names not scheduled stay zero
    tr.mask_mode, tr._sched_pool = "per_joint", 4
    assert int(tr._schedule_words(("mask_ratio",)).view(np.int32)[5]) == 1
    tr.mask_ratio = 0.2
    with pytest.raises(ValueError, match="outside"):
        tr._schedule_words(("mask_ratio",))
    tr.mask_mode = "threshold"                                                      # ignores mask_ratio, as before
    assert int(tr._schedule_words(("mask_ratio",)).view(np.int32)[5]) == 0
    assert utils.mask_kth_index(0.5, 64) == 32
    with pytest.raises(ValueError, match="outside"):
        utils.mask_kth_index(0.0, 64)


def test_the_new_exports_are_declared_bound_built_and_documented():
    from uda_poseestimation_amd import _hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "udapose.h")).read(), flags=re.S)
    capi = open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "capi.hip")).read()
    readme, design, integ = (open(os.path.join(ROOT, n)).read() for n in ("README.md", "DESIGN.md", "INTEGRATION.md"))
    assert "4.22" in design
    section = design.split("4.22", 1)[1]
    for name in NEW_EXPORTS:
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M), name
        assert f"int {name}(" in capi and name in _hip._SIGS and name in _hip.EXPORTS, name
        assert f"`{name}`" in integ and name in section, name
    vp, ci = C.c_void_p, C.c_int
    assert re.search(r"^int udapose_kth_mask_dev\(void\* stream, const float\* act, const float\* tea_mask, int n, const int\* k_dev,", hdr, flags=re.M)
    assert re.search(r"^int udapose_ema_multi_dev\(.*?const float\* ema_dev\);", hdr, flags=re.M | re.S)
    assert _hip._SIGS["udapose_kth_mask_dev"] == (ci, [vp, vp, vp, ci, vp, vp, vp, vp, ci])
    assert _hip._SIGS["udapose_joint_kth_mask_dev"] == (ci, [vp, vp, ci, ci, vp, vp, vp, ci, vp, vp])
    assert _hip._SIGS["udapose_ema_multi_dev"] == (ci, [vp, vp, vp, vp, vp, vp, ci, vp])
    # one fewer argument than the by-value forms: the pair (alpha, 1 - alpha) became one pointer
    for name in ("udapose_net_fused_update", "udapose_net_fused_update_groups"):
        assert len(_hip._SIGS[name + "_dev"][1]) == len(_hip._SIGS[name][1]) - 1
    for kind in ("bf16", "fp16"):
        if os.path.exists(_hip.LIB_PATHS[kind]):
            so = C.CDLL(_hip.LIB_PATHS[kind])
            for name in NEW_EXPORTS:
                assert hasattr(so, name), (kind, name)
    assert "scheduled" in readme and "sync_schedule" in readme and "view_merge" in readme
    assert "GraphedTrainStep` stages one view and refuses it" not in readme
    assert "sync_schedule" in section and "GraphedTrainStep" in section


def _collated(n, v=0.0):
    import torch
    z = torch.full((n,), float(v), dtype=torch.float64)
    return (z, (z.clone(), z.clone()), (z.clone(), z.clone()), z.clone() + 1.0)


@pytest.mark.parametrize("k", [1, 3])
def test_every_staging_call_takes_the_next_ring_slot_and_keeps_its_event_there(k, monkeypatch):
    """_stage_aug on host tensors with a counting stand-in for the device event: m calls occupy m distinct ring slots (the guard of a slot is
    the event of the copy that last read it), a fifth call waits for the first call's event and no other, every view lands in its own row."""
    import torch
    from uda_poseestimation_amd.engine import GraphedTrainStep

    class Event:
        made = []

        def __init__(self):
            self.recorded, self.waited = False, 0
            Event.made.append(self)

        def record(self):
            self.recorded = True

        def synchronize(self):
            self.waited += 1
    monkeypatch.setattr(torch.cuda, "Event", Event)
    n = 2
    gs = GraphedTrainStep.__new__(GraphedTrainStep)
    gs.n, gs.k = n, k
    gs.static = {"aug": torch.zeros(1 + k, n, 6, dtype=torch.float64)}
    gs._aug_pin = [torch.zeros(1 + k, n, 6, dtype=torch.float64) for _ in range(4)]
    gs._aug_ev, gs._aug_i, gs._aug_last = [None] * 4, 0, None
    for m in range(1, 5):
        gs._stage_aug(_collated(n, m), [_collated(n, 10 * m + v) for v in range(k)])
        assert sum(e is not None for e in gs._aug_ev) == m and gs._aug_ev[gs._aug_i] is Event.made[-1] and Event.made[-1].recorded
        assert gs._aug_last is gs._aug_pin[gs._aug_i]
        assert gs.static["aug"][:, 0, 0].tolist() == [float(m)] + [float(10 * m + v) for v in range(k)]
    assert len({id(e) for e in gs._aug_ev}) == 4 and not any(e.waited for e in Event.made)
    gs._stage_aug(_collated(n, 5), None)            # the teacher's side not given: it keeps the previous values
    assert [e.waited for e in Event.made] == [1, 0, 0, 0, 0] and gs._aug_ev[gs._aug_i] is Event.made[4]
    assert gs.static["aug"][:, 0, 0].tolist() == [5.0] + [float(40 + v) for v in range(k)]


def test_the_call_forms_of_the_teacher_side_are_normalised_in_both_branches():
    from uda_poseestimation_amd.engine import GraphedTrainStep
    gs = GraphedTrainStep.__new__(GraphedTrainStep)
    x, ap = object(), _collated(2)
    assert gs._views(x, ap, fix_k=True) == ([x], [ap]) and gs.k == 1
    assert gs._views(x, [ap]) == ([x], [ap])                    # a tensor with a one-element list: not wrapped twice
    assert gs._views([x], ap) == ([x], [ap]) and gs._views([x], [ap]) == ([x], [ap]) and gs._views(None, ap) == (None, [ap])
    assert gs._views(None, None) == (None, None)
    with pytest.raises(ValueError, match=r"k = 1 .* 2 in x_t_tea"):
        gs._views([x, x], [ap, ap])
    with pytest.raises(ValueError, match=r"k = 1 .* 2 in aug_param_tea"):
        gs._views(x, [ap, ap])
    g3 = GraphedTrainStep.__new__(GraphedTrainStep)
    assert g3._views([x, x, x], [ap, ap, ap], fix_k=True) == ([x, x, x], [ap, ap, ap]) and g3.k == 3
    g4 = GraphedTrainStep.__new__(GraphedTrainStep)            # four views: a list of four is not mistaken for one collated 4-tuple
    assert g4._views([x] * 4, [ap] * 4, fix_k=True)[1] == [ap] * 4 and g4.k == 4
    with pytest.raises(NotImplementedError, match="at most 8"):
        g4._views([x] * 9, None)
