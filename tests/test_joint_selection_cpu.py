"""Joint selection without a GPU: the fp64 restatement (tests/helpers/joint_selection_fp64.py) against torch.topk / torch.kthvalue and an
explicit stable sort, the refusals that come before any launch, and the public surface (lib.models.loss, utils.confidence_mask, the
trainer's attributes, the C ABI's documents)."""
import inspect
import os
import re

import pytest
import torch

from helpers import joint_selection_fp64 as R64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(N, K, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    scale = 0.3 + 2.0 * torch.rand(N, K, 1, 1, generator=g, dtype=torch.float64)
    p = torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * scale
    t = p + 0.5 * torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * scale
    w = torch.where(torch.rand(N, K, generator=g) < 0.25, torch.zeros(N, K), 0.5 + torch.rand(N, K, generator=g)).double()
    m = torch.rand(N, K, generator=g) < 0.6
    return p, t, w, m


@pytest.mark.parametrize("topk", [1, 5, 12])
def test_the_restatement_equals_torch_topk_on_distinct_rows(topk):
    p, t, w, m = _inputs(6, 12, 9, 7, seed=1)
    rows = R64.rows_joints(p, t, w)
    assert rows[w != 0].unique().numel() == int((w != 0).sum())            # distinct where they are not zero
    loss, sample, sel = R64.joints_ohkm(p, t, w, topk)
    # a zero-weight row is 0 and adds nothing, so torch.topk over the rows gives the value whichever zeros it takes
    want = torch.topk(rows, topk, dim=1).values.sum(1) / topk
    assert torch.allclose(sample, want, rtol=1e-14, atol=0) and abs(float(loss) - float(want.mean())) <= 1e-14 * float(want.mean())
    assert not sel[w == 0].any() and (sel.sum(1) <= topk).all()
    # smallest first, among the admitted joints only
    rc = R64.rows_cons(p, t, m)
    loss, sample, sel = R64.cons_topk(p, t, m, topk, largest=False)
    for n in range(p.shape[0]):
        adm = rc[n][m[n]]
        k = min(topk, adm.numel())
        want_n = torch.topk(adm, k, largest=False).values.sum() / topk if k else torch.zeros((), dtype=torch.float64)
        assert abs(float(sample[n]) - float(want_n)) <= 1e-14 * max(float(want_n), 1e-300)
        assert int(sel[n].sum()) == k and not sel[n][~m[n]].any()


@pytest.mark.parametrize("largest", [True, False])
def test_the_restatement_equals_a_stable_sort_on_tied_rows(largest):
    g = torch.Generator().manual_seed(2)
    rows = torch.randint(0, 4, (8, 10), generator=g).double()              # many exact ties
    zero = torch.rand(8, 10, generator=g) < 0.2
    rows = torch.where(zero, torch.zeros_like(rows), rows + 1.0)
    for topk in (1, 3, 7, 10):
        sel, cand = R64.select(rows, zero, topk, largest)
        for n in range(rows.shape[0]):
            order = sorted((j for j in range(10) if cand[n, j]), key=lambda j: ((-rows[n, j] if largest else rows[n, j]), j))      # stable: ties by index
            want = [j for j in order[:topk] if not zero[n, j]]
            assert sorted(want) == [j for j in range(10) if sel[n, j]], (topk, n)


def test_per_joint_thresholds_equal_torch_kthvalue_per_column():
    g = torch.Generator().manual_seed(3)
    pool = torch.rand(37, 17, generator=g, dtype=torch.float64)
    pool[5:9, 3] = pool[4, 3]              # duplicates
    pool[11, 6] = float("nan")
    for k in (1, 18, 36, 37):
        thr = R64.joint_thresholds(pool, k)
        want = torch.kthvalue(pool, k, dim=0).values
        assert torch.equal(torch.isnan(thr), torch.isnan(want)) and torch.equal(thr[~torch.isnan(thr)], want[~torch.isnan(want)])
    assert torch.isnan(R64.joint_thresholds(pool, 37)[6]) and not torch.isnan(R64.joint_thresholds(pool, 36)).any()
    mask, thr = R64.joint_mask(pool, 37, pool)
    assert not mask.any()                   # nothing exceeds a column's maximum; a NaN threshold gives an all-false column


def test_topk_equal_to_K_reduces_to_the_joints_mse_mean():
    p, t, w, _ = _inputs(5, 9, 8, 8, seed=4)
    loss, _, sel = R64.joints_ohkm(p, t, w, 9)
    mse = (0.5 * ((p - t) ** 2) * w[:, :, None, None]).mean()
    assert abs(float(loss) - float(mse)) <= 1e-14 * float(mse) and torch.equal(sel, w != 0)
    loss, _, _ = R64.cons_topk(p, t, None, 9, largest=False)
    assert abs(float(loss) - float(((p - t) ** 2).mean())) <= 1e-14 * float(loss)


def test_refusals_come_before_any_kernel_is_loaded(monkeypatch):
    from uda_poseestimation_amd import _hip, utils
    from uda_poseestimation_amd.lib.models import loss as L

    def no_lib(*a, **k):
        raise AssertionError("a refusal loaded the library")
    monkeypatch.setattr(_hip, "lib", no_lib)
    monkeypatch.setattr(L, "lib", no_lib)
    monkeypatch.setattr(utils, "lib", no_lib)
    for cls in (L.JointsOHKMMSELoss, L.ConsTopKLoss):
        for bad in (0, -1, 2.5):
            with pytest.raises(ValueError, match="topk"):
                cls(bad)
    x = torch.zeros(2, 4, 8, 8)
    for crit, args in ((L.JointsOHKMMSELoss(8), (x, x, None)), (L.ConsTopKLoss(5), (x, x))):
        with pytest.raises(ValueError, match="exceeds"):
            crit(*args)
    big = torch.zeros(1, 65, 2, 2)
    with pytest.raises(ValueError, match="K <= 64"):
        L.JointsOHKMMSELoss(8)(big, big)
    with pytest.raises(ValueError, match="K <= 64"):
        L.ConsTopKLoss(8)(big, big)
    crit = L.JointsOHKMMSELoss(2)
    crit.topk = 0
    with pytest.raises(ValueError, match="topk"):
        crit(x, x)
    with pytest.raises(NotImplementedError, match="valid_mask"):
        L.ConsTopKLoss(2)(x, x, valid_mask=torch.ones(2, 8, 8, dtype=torch.bool))
    # CPU tensors: there is no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.JointsOHKMMSELoss(2)(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.ConsTopKLoss(2)(x, x, tea_mask=torch.ones(2, 4, dtype=torch.bool))
    act = torch.rand(4, 16)
    with pytest.raises(ValueError, match="mode"):
        utils.confidence_mask(x, 0.5, activates=act, mode="joint")
    with pytest.raises(ValueError, match="k = int"):
        utils.confidence_mask(x, 0.2, activates=act, mode="per_joint")             # int(0.2 * 4) = 0
    with pytest.raises(ValueError, match="k = int"):
        utils.confidence_mask(x, 0.01, activates=act, gathered_activates=torch.rand(8 * 16), mode="per_joint")
    with pytest.raises(ValueError, match="multiple"):
        utils.confidence_mask(x, 0.5, activates=act, gathered_activates=torch.rand(30), mode="per_joint")
    with pytest.raises(ValueError, match="threshold"):
        utils.confidence_mask(x, 0.5, activates=act, mode="threshold")
    with pytest.raises(ValueError, match="0-d"):
        utils.confidence_mask(x, 0.5, activates=act, mode="threshold", threshold=torch.zeros(2))
    for kw in (dict(mode="per_joint"), dict(mode="threshold", threshold=0.5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            utils.confidence_mask(x, 0.5, activates=act, **kw)


def test_a_new_trainer_masks_globally_and_the_signature_is_additive():
    from uda_poseestimation_amd import utils
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    net = lambda: pr._pose_resnet("t", 4, pr.Bottleneck_default, [1, 1, 1, 1], False, False)
    tr = MeanTeacherTrainer(net(), net())
    assert tr.mask_mode == "global" and tr.mask_threshold == 0.5
    ps = inspect.signature(utils.confidence_mask).parameters
    assert list(ps) == ["recon", "mask_ratio", "tea_mask", "gathered_activates", "activates", "mode", "threshold"]
    assert ps["mode"].default == "global" and ps["mode"].kind is inspect.Parameter.KEYWORD_ONLY and ps["threshold"].default is None
    assert utils.MASK_MODES == ("global", "per_joint", "threshold")


def test_the_loss_module_exports_the_two_classes():
    from uda_poseestimation_amd.lib.models import loss as L
    for name, params in (("JointsOHKMMSELoss", ["topk", "reduction"]), ("ConsTopKLoss", ["topk", "largest"])):
        cls = getattr(L, name)
        assert issubclass(cls, torch.nn.Module)
        sig = inspect.signature(cls.__init__).parameters
        assert list(sig)[1:] == params and sig["topk"].default == 8
    assert inspect.signature(L.ConsTopKLoss.__init__).parameters["largest"].default is True
    assert list(inspect.signature(L.JointsOHKMMSELoss.forward).parameters) == ["self", "output", "target", "target_weight"]
    assert list(inspect.signature(L.ConsTopKLoss.forward).parameters) == ["self", "stu_out", "tea_out", "valid_mask", "tea_mask"]
    assert L.JointsOHKMMSELoss().last_selection is None
    assert "squares it" in " ".join(L.JointsOHKMMSELoss.__doc__.split())          # the MSRA code's squared weight is stated


def test_the_source_is_built_and_the_exports_are_documented():
    """(Prototypes against ctypes rows: test_host_cpu.py::test_ctypes_signatures_and_policy_fields_match_the_header.)"""
    from uda_poseestimation_amd import _hip
    mk = open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "Makefile")).read()
    assert "select.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "kth_select.h" in re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1).split()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in ("topk_select", "topk_sqdiff_bwd", "joint_kth_mask", "thr_mask"):
        assert f"udapose_{n}" in _hip.EXPORTS and f"`udapose_{n}`" in doc, n
    # the radix select exists once: both kernels call the one device function
    heat = open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "heatmap.hip")).read()
    sel = open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "select.hip")).read()
    assert "hm_kth_smallest(" in heat and "hm_kth_smallest(" in sel and "atomicAdd(&hist" not in heat + sel
