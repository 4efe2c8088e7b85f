"""The skeleton prior without a GPU: the fp64 restatement (tests/helpers/prior_map_fp64.py) against the reference's own outputs
(tests/golden/prior_map.npz), the diagonal weight, the refusals of CPU tensors, the trainer's attributes, the pair statistics by hand, and the
C ABI's declarations."""
import os

import numpy as np
import pytest
import torch

from helpers import prior_map_fp64 as P64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "prior_map.npz"))


def test_the_golden_file_holds_the_cases_it_is_made_of(golden):
    names = [str(n) for n in golden["names"]]
    assert names == [c[0] for c in P64.golden_cases()]
    for name, shape, seed, gamma, sigma, inf_std, neg in P64.golden_cases():
        preds, mean, std = P64.case_inputs(shape, seed, inf_std, neg)
        for k, v in (("preds", preds), ("mean", mean), ("std", std)):
            assert np.array_equal(golden[f"{name}/{k}"], v), (name, k)
        assert float(golden[f"{name}/gamma"]) == gamma and float(golden[f"{name}/sigma"]) == sigma
        assert bool(np.isinf(std).any()) == inf_std
        assert bool((preds.reshape(shape[0], shape[1], -1).max(-1) < 0).any()) == neg
    assert {c[1] for c in P64.golden_cases()} >= set(P64.GOLDEN_SHAPES)


@pytest.mark.parametrize("case", P64.golden_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("mode", ["default", "v3"])
def test_helper_against_the_reference_outputs(golden, case, mode):
    """The reference sums K fp32 terms per element: max|helper - golden| / max|helper| <= 4 * 2^-24 * K (measured 1e-7 to 3e-7)."""
    name, shape = case[0], case[1]
    T = lambda k: torch.from_numpy(golden[f"{name}/{k}"])
    truth = P64.prior_map(T("mean"), T("std"), T("preds"), gamma=case[3], sigma=case[4], v3=mode == "v3")
    assert truth.dtype == torch.float64 and bool(torch.isfinite(truth).all())
    err = P64.rel_err(T(mode), truth)
    print(f"prior map {name} {mode}: golden against fp64 helper {err:.2e}")
    assert err <= 4 * 2.0 ** -24 * shape[1]


def test_a_non_positive_maximum_casts_its_rings_from_the_origin(golden):
    name = "2x3x5x7_negrow"
    preds = torch.from_numpy(golden[f"{name}/preds"])
    coords, conf = P64.decode(preds)
    assert float(conf[0, 2]) < 0 and coords[0, 2].tolist() == [0.0, 0.0]
    assert int(preds[0, 2].reshape(-1).argmax()) != 0          # (the arg-max is elsewhere: the zeroing is what puts the rings at (0, 0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_diagonal_weight_is_exactly_zero_above_one_joint_and_one_at_one_joint(dtype):
    for K in (2, 3, 16, 64):
        std = torch.from_numpy(P64.case_inputs((1, K, 2, 2), K)[2]).to(dtype)
        w = P64.weights(std, gamma=2)
        assert torch.equal(w.diagonal(), torch.zeros(K, dtype=dtype))
        assert float((w.sum(0) - 1).abs().max()) <= 4 * float(torch.finfo(dtype).eps)
    assert P64.weights(torch.tensor([[0.7]], dtype=dtype)).tolist() == [[1.0]]
    # std = +inf off the diagonal weighs 0 (a column with nothing else left gives its weight to the diagonal, as in the reference);
    # v3 includes the diagonal
    std = torch.tensor([[1.0, float("inf")], [2.0, 1.0]], dtype=dtype)
    assert P64.weights(std).tolist() == [[0.0, 0.0], [1.0, 1.0]]
    assert P64.weights(std, v3=True).tolist() == [[0.5, 0.0], [float(torch.tensor(1, dtype=dtype) / 3), 0.5]]


def test_generate_prior_map_and_skeleton_prior_refuse_cpu_tensors():
    from uda_poseestimation_amd import utils
    prior = {"mean": torch.zeros(3, 3), "std": torch.ones(3, 3)}
    with pytest.raises(RuntimeError, match="MI355X"):
        utils.generate_prior_map(prior, torch.rand(2, 3, 5, 7))
    with pytest.raises(RuntimeError, match="MI355X"):
        utils.generate_prior_map(prior, torch.rand(2, 3, 5, 7), v3=True, multiply=True)
    with pytest.raises(RuntimeError, match="MI355X"):
        utils.SkeletonPrior(3, "cpu")
    sp = utils.SkeletonPrior(3, "cuda")          # (nothing is allocated before the first update)
    with pytest.raises(RuntimeError, match="MI355X"):
        sp.update(torch.rand(2, 3, 5, 7), torch.ones(2, 3, 1))
    with pytest.raises(RuntimeError, match="MI355X"):
        sp.update_coords(torch.rand(2, 3, 2), torch.ones(2, 3))
    for k in (0, 65):
        with pytest.raises(ValueError):
            utils.SkeletonPrior(k, "cuda")
    import inspect
    sig = inspect.signature(utils.generate_prior_map)
    assert list(sig.parameters) == ["prior", "preds", "gamma", "sigma", "epsilon", "v3", "multiply"]
    assert [sig.parameters[k].default for k in ("gamma", "sigma", "epsilon", "v3", "multiply")] == [2, 2, -10e10, False, False]
    assert sig.parameters["multiply"].kind is inspect.Parameter.KEYWORD_ONLY


def test_the_trainer_has_the_prior_switched_off_by_default():
    """The constructor's parameter list is pinned by earlier tests, so the prior and its settings are attributes of the trainer."""
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    net = lambda: pr._pose_resnet("t", 4, pr.Bottleneck_default, [1, 1, 1, 1], False, False)
    tr = MeanTeacherTrainer(net(), net())
    assert tr.skeleton_prior is None and tr.prior_gamma == 2 and tr.prior_sigma == 2 and tr.prior_v3 is False


def test_pair_statistics_of_three_samples_by_hand():
    """K = 3.  Joints 0 and 1 are 3, 4 and 5 apart in the three samples, all visible: mean 4, variance (9 + 16 + 25) / 3 - 16 = 2/3.
    Joint 2 is visible in sample 0 only, 5 from joint 0 ((0,0) -> (3,4)) and 4 from joint 1 ((3,0) -> (3,4)): one sample, std 0.  Then joint 2 is hidden
    everywhere: its pairs are never seen."""
    coords = np.zeros((3, 3, 2), dtype=np.float32)
    coords[0, 1], coords[1, 1], coords[2, 1] = (3, 0), (0, 4), (3, 4)
    coords[0, 2] = (3, 4)
    coords[1, 2], coords[2, 2] = (100, 100), (-7, 2)             # hidden: must not count
    vis = np.array([[1, 1, 1], [1, 1, 0], [1, 1, 0]])
    n, mu, sd, m2 = P64.pair_stats(coords, vis)
    assert n.tolist() == [[3, 3, 1], [3, 3, 1], [1, 1, 1]]
    assert mu[0, 1] == mu[1, 0] == 4.0 and abs(sd[0, 1] - np.sqrt(2 / 3)) < 1e-15 and abs(m2[0, 1] - 50 / 3) < 1e-14
    assert mu[0, 2] == 5.0 and sd[0, 2] == 0.0 and mu[1, 2] == 4.0 and sd[1, 2] == 0.0
    assert mu.diagonal().tolist() == [0, 0, 0] and sd.diagonal().tolist() == [0, 0, 0]
    vis[:, 2] = 0
    n, mu, sd, _ = P64.pair_stats(coords, vis)
    assert n[2].tolist() == [0, 0, 0] and n[:, 2].tolist() == [0, 0, 0]
    assert mu[2].tolist() == [0, 0, 0] and np.isinf(sd[2]).all() and np.isinf(sd[:, 2]).all() and sd[0, 1] > 0
    # a never-seen pair weighs 0 in both modes, and the map stays finite
    std_t = torch.from_numpy(sd)
    assert P64.weights(std_t)[2, :2].tolist() == [0, 0] and P64.weights(std_t, v3=True)[2].tolist() == [0, 0, 0]
    preds = torch.from_numpy(P64.case_inputs((2, 3, 5, 7), 1)[0])
    for v3 in (False, True):
        assert bool(torch.isfinite(P64.prior_map(torch.from_numpy(mu), std_t, preds, v3=v3)).all())


def test_the_header_cites_the_reference():
    """(The four exports' prototypes and ctypes rows: test_host_cpu.py::test_ctypes_signatures_and_policy_fields_match_the_header.)"""
    text = open(os.path.join(ROOT, "include", "udapose.h")).read()
    assert "utils.py:111-145" in text
