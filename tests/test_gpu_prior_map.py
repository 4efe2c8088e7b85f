"""The skeleton prior on the MI355X (csrc/prior_map.hip): utils.generate_prior_map, utils.SkeletonPrior and the trainer's hook.

The truth is tests/helpers/prior_map_fp64.py in fp64.  Error measure: max|delta| / max|truth|.  The bar is not a constant: e32 is the error of the
reference's own fp32 output where tests/golden/prior_map.npz holds the case (the seeded inputs are the same), otherwise that of the helper
evaluated in torch fp32 on the CPU, and the device must be within 4 x max(e32, 2^-24) - the floor is the half-ulp rounding of the result itself
(at (1,1,1,1) e32 is exactly 0), the margin of 4 is the project's convention for a different summation order."""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import prior_map_fp64 as P64

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prior_map.npz")
SHAPES = [(1, 1, 1, 1), (1, 2, 3, 5), (2, 3, 5, 7), (2, 5, 7, 4), (1, 21, 17, 17), (3, 18, 16, 16), (1, 64, 4, 4), (2, 16, 64, 64)]
U24 = 2.0 ** -24


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ids(s):
    return "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(GOLDEN)


def _gpm(mean, std, preds, **kw):
    from uda_poseestimation_amd.utils import generate_prior_map
    return generate_prior_map({"mean": mean, "std": std}, preds, **kw)


def _bar(e32):
    return 4.0 * max(e32, U24)


@functools.lru_cache(maxsize=None)
def _case(shape, v3, setting):
    """(preds, mean, std) as CPU fp32 tensors, the fp64 truth and e32.  Computed once per case and left unchanged."""
    gamma, sigma = setting
    preds, mean, std = (torch.from_numpy(a) for a in P64.case_inputs(shape, P64.seed_of(shape)))
    truth = P64.prior_map(mean, std, preds, gamma=gamma, sigma=sigma, v3=v3)
    name = _ids(shape) + ("" if setting == P64.SETTINGS[0] else f"_g{gamma}_s{sigma}")
    g = _golden()
    if name in [str(n) for n in g["names"]]:
        assert np.array_equal(g[f"{name}/preds"], preds.numpy()) and np.array_equal(g[f"{name}/mean"], mean.numpy())
        e32, src = P64.rel_err(torch.from_numpy(g[f"{name}/" + ("v3" if v3 else "default")]), truth), "golden"
    else:
        e32, src = P64.rel_err(P64.prior_map(mean, std, preds, gamma=gamma, sigma=sigma, v3=v3, dtype=torch.float32), truth), "fp32 helper"
    return preds, mean, std, truth, e32, src


# ---------------------------------------------------------------------------------------------- map parity
@pytest.mark.parametrize("setting", P64.SETTINGS, ids=lambda s: f"g{s[0]}s{s[1]}")
@pytest.mark.parametrize("v3", [False, True], ids=["default", "v3"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_map_against_fp64(shape, v3, setting):
    preds, mean, std, truth, e32, src = _case(shape, v3, setting)
    got = _gpm(mean, std, preds.cuda(), gamma=setting[0], sigma=setting[1], v3=v3)
    assert got.shape == preds.shape and got.dtype == torch.float32 and got.is_cuda and not got.requires_grad
    err = P64.rel_err(got.cpu(), truth)
    print(f"prior map {_ids(shape)} {'v3' if v3 else 'default'} gamma {setting[0]} sigma {setting[1]}: device {err:.2e}  e32 {e32:.2e} ({src})")
    assert err <= _bar(e32)


@pytest.mark.parametrize("v3", [False, True], ids=["default", "v3"])
@pytest.mark.parametrize("case", P64.golden_cases(), ids=lambda c: c[0])
def test_the_inputs_of_the_golden_file_on_the_device(case, v3):
    """Every recorded case, infinite std entries and the negative plane among them, from the arrays the file holds."""
    g, name = _golden(), case[0]
    T = lambda k: torch.from_numpy(g[f"{name}/{k}"])
    gamma, sigma = float(g[f"{name}/gamma"]), float(g[f"{name}/sigma"])
    truth = P64.prior_map(T("mean"), T("std"), T("preds"), gamma=gamma, sigma=sigma, v3=v3)
    e32 = P64.rel_err(T("v3" if v3 else "default"), truth)
    got = _gpm(T("mean"), T("std"), T("preds").cuda(), gamma=gamma, sigma=sigma, v3=v3)
    err = P64.rel_err(got.cpu(), truth)
    print(f"prior map golden {name} {'v3' if v3 else 'default'}: device {err:.2e}  e32 {e32:.2e}")
    assert bool(torch.isfinite(got).all()) and err <= _bar(e32)


# ---------------------------------------------------------------------------------------------- fixed cases
def _e32_helper(mean, std, preds, truth, **kw):
    return P64.rel_err(P64.prior_map(mean, std, preds, dtype=torch.float32, **kw), truth)


@pytest.mark.parametrize("v3", [False, True], ids=["default", "v3"])
def test_a_plane_with_maximum_zero_or_below_casts_from_the_origin(v3):
    from uda_poseestimation_amd.utils import get_max_preds_torch
    shape = (2, 3, 5, 7)
    preds, mean, std = (torch.from_numpy(a) for a in P64.case_inputs(shape, 901, negative_row=True))
    preds[1, 0] = 0.0                                           # maximum exactly 0
    coords, conf = get_max_preds_torch(preds.cuda())
    assert coords[0, 2].tolist() == [0.0, 0.0] and coords[1, 0].tolist() == [0.0, 0.0] and float(conf[0, 2]) < 0 and float(conf[1, 0]) == 0
    truth = P64.prior_map(mean, std, preds, v3=v3)
    got = _gpm(mean, std, preds.cuda(), v3=v3).cpu()
    assert bool(torch.isfinite(got).all())
    assert P64.rel_err(got, truth) <= _bar(_e32_helper(mean, std, preds, truth, v3=v3))


def test_two_equal_maxima_the_first_index_wins():
    from uda_poseestimation_amd.utils import get_max_preds_torch
    shape = (1, 2, 5, 7)
    preds, mean, std = (torch.from_numpy(a) for a in P64.case_inputs(shape, 902))
    preds[0, 0] = preds[0, 0].clamp(max=0.875) * 0.5           # everything else below the two maxima
    preds[0, 0, 1, 4] = preds[0, 0, 3, 2] = 1.0                 # flat 11 and flat 23
    coords, conf = get_max_preds_torch(preds.cuda())
    assert coords[0, 0].tolist() == [4.0, 1.0] and float(conf[0, 0]) == 1.0
    truth = P64.prior_map(mean, std, preds, coords=coords.cpu(), conf=conf.cpu().reshape(1, 2))
    assert torch.equal(P64.decode(preds)[0], coords.cpu())      # (torch's CPU arg-max takes the first index too)
    got = _gpm(mean, std, preds.cuda()).cpu()
    assert P64.rel_err(got, truth) <= _bar(_e32_helper(mean, std, preds, truth))
    other = P64.prior_map(mean, std, preds, coords=torch.tensor([[[2.0, 3.0], coords[0, 1].tolist()]]), conf=conf.cpu().reshape(1, 2))
    assert P64.rel_err(got, other) > 1e-3                       # (the second maximum would have given another map)


def test_a_nan_plane():
    from uda_poseestimation_amd.utils import get_max_preds_torch
    shape = (2, 3, 5, 7)
    preds, mean, std = (torch.from_numpy(a) for a in P64.case_inputs(shape, 903))
    preds[0, 1, 2, 3] = float("nan")
    coords, conf = get_max_preds_torch(preds.cuda())
    assert bool(torch.isnan(conf[0, 1])) and coords[0, 1].tolist() == [0.0, 0.0]      # (NaN > 0 is false: the coordinates are zeroed)
    coords, conf = coords.cpu(), conf.cpu().reshape(2, 3)
    got = _gpm(mean, std, preds.cuda()).cpu()
    truth = P64.prior_map(mean, std, preds, coords=coords, conf=conf)
    e32 = P64.rel_err(P64.prior_map(mean, std, preds, coords=coords, conf=conf, dtype=torch.float32), truth)
    assert bool(torch.isfinite(got).all()) and P64.rel_err(got, truth) <= _bar(e32)
    v3 = _gpm(mean, std, preds.cuda(), v3=True).cpu()
    assert bool(torch.isnan(v3[0]).all()) and bool(torch.isfinite(v3[1]).all())
    clean = preds.clone()
    clean[0, 1, 2, 3] = 0.5
    truth1 = P64.prior_map(mean, std, clean, v3=True)[1]
    assert P64.rel_err(v3[1], truth1) <= _bar(P64.rel_err(P64.prior_map(mean, std, clean, v3=True, dtype=torch.float32)[1], truth1))


def test_refusals_of_the_function_and_of_the_abi():
    from uda_poseestimation_amd._hip import lib, ptr, stream
    from uda_poseestimation_amd.utils import generate_prior_map, SkeletonPrior
    L = lib()
    prior65 = {"mean": torch.zeros(65, 65), "std": torch.ones(65, 65)}
    with pytest.raises(ValueError):
        generate_prior_map(prior65, torch.rand(1, 65, 2, 2, device="cuda"))
    prior3 = {"mean": torch.zeros(3, 3), "std": torch.ones(3, 3)}
    x = torch.rand(2, 3, 5, 7, device="cuda")
    for sigma in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            generate_prior_map(prior3, x, sigma=sigma)
    with pytest.raises(ValueError):
        generate_prior_map({"mean": torch.zeros(3, 4), "std": torch.ones(3, 3)}, x)
    with pytest.raises(ValueError):
        generate_prior_map({"mean": torch.zeros(4, 4), "std": torch.ones(4, 4)}, x)
    with pytest.raises(ValueError):
        generate_prior_map(prior3, x, gamma=0)
    with pytest.raises(RuntimeError, match="MI355X"):
        generate_prior_map(prior3, x.cpu())
    with pytest.raises(ValueError):
        SkeletonPrior(3, "cuda").update_coords(torch.zeros(2, 4, 2, device="cuda"), torch.ones(2, 4, device="cuda"))
    # the ABI, with buffers large enough for what is asked: an error code, and the NaN-filled output untouched
    B, H, W = 1, 2, 2
    for K, code in ((65, -3), (0, -1), (-4, -1)):
        n = max(K, 1)
        coords, conf = torch.zeros(B, n, 2, device="cuda"), torch.ones(B, n, device="cuda")
        mean, w, acc = torch.zeros(n, n, device="cuda"), torch.ones(n, n, device="cuda"), torch.zeros(3, n, n, dtype=torch.float64, device="cuda")
        out = torch.full((B, n, H, W), float("nan"), device="cuda")
        vis = torch.ones(B, n, dtype=torch.uint8, device="cuda")
        assert L.udapose_prior_map(stream(), ptr(coords), ptr(conf), ptr(mean), ptr(w), None, B, K, H, W, 2.0, 0, ptr(out)) == code
        assert L.udapose_prior_weights(stream(), ptr(mean), K, 2.0, -1e11, 0, ptr(w)) == code
        assert L.udapose_pair_dist_accumulate(stream(), ptr(coords), ptr(vis), B, K, ptr(acc)) == code
        assert L.udapose_pair_dist_finish(stream(), ptr(acc), K, ptr(mean), ptr(w)) == code
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and float(w.min()) == 1.0 and float(acc.abs().max()) == 0.0
    K = 3
    coords, conf = torch.zeros(B, K, 2, device="cuda"), torch.ones(B, K, device="cuda")
    mean, w = torch.zeros(K, K, device="cuda"), torch.ones(K, K, device="cuda")
    out = torch.full((B, K, H, W), float("nan"), device="cuda")
    good = [ptr(coords), ptr(conf), ptr(mean), ptr(w), None, B, K, H, W, 2.0, 0, ptr(out)]

    def changed(i, v):
        a = list(good)
        a[i] = v
        return a

    for i, v in ((0, None), (2, None), (3, None), (11, None), (5, 0), (7, 0), (8, 0), (9, 0.0), (9, -2.0), (9, float("inf")), (9, float("nan"))):
        assert L.udapose_prior_map(stream(), *changed(i, v)) == -1, (i, v)
    a = changed(1, None)
    a[10] = 1
    assert L.udapose_prior_map(stream(), *a) == -1              # v3 without confidences
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert L.udapose_prior_map(stream(), *changed(1, None)) == 0        # (the default mode does not read them)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    assert L.udapose_prior_weights(stream(), None, K, 2.0, -1e11, 0, ptr(w)) == -1 and L.udapose_prior_weights(stream(), ptr(mean), K, 0.0, -1e11, 0, ptr(w)) == -1
    acc = torch.zeros(3, K, K, dtype=torch.float64, device="cuda")
    vis = torch.ones(B, K, dtype=torch.uint8, device="cuda")
    assert L.udapose_pair_dist_accumulate(stream(), ptr(coords), ptr(vis), 0, K, ptr(acc)) == -1
    assert L.udapose_pair_dist_accumulate(stream(), None, ptr(vis), B, K, ptr(acc)) == -1
    assert L.udapose_pair_dist_finish(stream(), None, K, ptr(mean), ptr(w)) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize("v3", [False, True], ids=["default", "v3"])
def test_multiply_is_one_fp32_product_and_two_calls_agree_to_the_bit(v3):
    for shape in ((2, 3, 5, 7), (3, 18, 16, 16), (2, 16, 64, 64)):
        preds, mean, std, _, _, _ = _case(shape, v3, P64.SETTINGS[0])
        x = preds.cuda()
        a, b = _gpm(mean, std, x, v3=v3), _gpm(mean, std, x, v3=v3)
        assert torch.equal(_bits(a), _bits(b)), shape
        m = _gpm(mean, std, x, v3=v3, multiply=True)
        assert torch.equal(_bits(m), _bits(x.float() * a)), shape
        assert not torch.equal(m, a)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_sixteen_bit_inputs_are_the_fp32_call_rounded_once(dtype):
    preds, mean, std, _, _, _ = _case((3, 18, 16, 16), False, P64.SETTINGS[0])
    x = preds.cuda().to(dtype)
    for kw in ({}, {"v3": True}, {"multiply": True}, {"v3": True, "multiply": True}):
        got = _gpm(mean, std, x, **kw)
        want = _gpm(mean, std, x.float(), **kw)
        assert got.dtype == dtype and want.dtype == torch.float32
        assert torch.equal(got, want.to(dtype)), kw


def test_the_tables_are_cached_on_what_they_were_made_from():
    from uda_poseestimation_amd import utils
    preds, mean, std, truth, e32, _ = _case((2, 3, 5, 7), False, P64.SETTINGS[0])
    mean, std, x = mean.clone(), std.clone(), preds.cuda()
    a = _gpm(mean, std, x)
    n = len(utils._PRIOR_CACHE)
    b = _gpm(mean, std, x)
    assert len(utils._PRIOR_CACHE) == n and torch.equal(a, b)
    dm, ds = mean.cuda(), std.cuda()                            # device tables give the same bits
    assert torch.equal(_gpm(dm, ds, x), a)
    mean.mul_(0.5)                                              # an in-place change is seen (the version counter is part of the key)
    c = _gpm(mean, std, x).cpu()
    truth2 = P64.prior_map(mean, std, preds)
    assert P64.rel_err(c, truth2) <= _bar(_e32_helper(mean, std, preds, truth2)) and P64.rel_err(c, truth) > 1e-3
    assert P64.rel_err(_gpm(mean, std, x, gamma=0.5).cpu(), P64.prior_map(mean, std, preds, gamma=0.5)) <= _bar(
        _e32_helper(mean, std, preds, P64.prior_map(mean, std, preds, gamma=0.5), gamma=0.5))


@pytest.mark.parametrize("v3", [False, True], ids=["default", "v3"])
def test_a_call_replayed_from_a_graph_on_fresh_inputs_equals_eager_to_the_bit(v3):
    shape = (3, 18, 16, 16)
    preds, mean, std = (torch.from_numpy(a) for a in P64.case_inputs(shape, 950))
    prior = {"mean": mean, "std": std}                          # CPU tables: uploaded by the warm-up call, found in the cache by the capture
    from uda_poseestimation_amd.utils import generate_prior_map
    x = preds.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        generate_prior_map(prior, x, v3=v3, multiply=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = generate_prior_map(prior, x, v3=v3, multiply=True)
    for i in range(3):
        fresh = torch.from_numpy(P64.case_inputs(shape, 951 + i)[0]).cuda()
        x.copy_(fresh)
        graph.replay()
        eager = generate_prior_map(prior, fresh, v3=v3, multiply=True)
        torch.cuda.synchronize()
        assert torch.equal(_bits(captured), _bits(eager)), i
        assert float(eager.abs().max()) > 0


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 7), (1, 21, 17, 17), (2, 9, 17, 31)], ids=_ids)
def test_every_element_of_a_nan_filled_output_is_written(shape):
    from uda_poseestimation_amd._hip import lib, ptr, stream
    B, K, H, W = shape
    preds, mean, std = (torch.from_numpy(a) for a in P64.case_inputs(shape, 960))
    coords, conf = P64.decode(preds)
    for v3 in (0, 1):
        w = P64.weights(std, v3=bool(v3)).float().contiguous().cuda()
        out = torch.full((B * K * H * W + 64,), float("nan"), device="cuda")          # 64 guard elements behind the output
        c, f, m, hm = coords.contiguous().cuda(), conf.contiguous().cuda(), mean.contiguous().cuda(), preds.cuda()
        assert lib().udapose_prior_map(stream(), ptr(c), ptr(f), ptr(m), ptr(w), ptr(hm), B, K, H, W, 2.0, v3, ptr(out)) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out[:B * K * H * W]).all()) and bool(torch.isnan(out[B * K * H * W:]).all())
        truth = P64.prior_map(mean, std, preds, v3=bool(v3)) * preds.double()
        e32 = P64.rel_err(P64.prior_map(mean, std, preds, v3=bool(v3), dtype=torch.float32) * preds, truth)
        assert P64.rel_err(out[:B * K * H * W].reshape(shape).cpu(), truth) <= _bar(e32)


def test_the_weight_table_kernel_against_the_helper():
    from uda_poseestimation_amd._hip import lib, ptr, stream
    for K in (1, 2, 5, 21, 64):
        std = torch.from_numpy(P64.case_inputs((1, K, 2, 2), 970 + K, inf_std=K > 2)[2])
        for v3, gamma in ((0, 2.0), (0, 0.75), (1, 2.0)):
            w = torch.full((K, K), float("nan"), device="cuda")
            assert lib().udapose_prior_weights(stream(), ptr(std.cuda()), K, gamma, P64.EPSILON, v3, ptr(w)) == 0
            want = P64.weights(std.double(), gamma, v3=bool(v3))
            w = w.cpu()
            # a soft-max of K fp32 terms: each weight within a few ulps of the fp64 value, relative to the largest (1 at most)
            assert float((w.double() - want).abs().max()) <= 8 * U24, (K, v3, gamma)
            assert torch.equal(w == 0, want == 0)
            if not v3:
                assert torch.equal(w.diagonal(), torch.ones(1) if K == 1 else torch.zeros(K))


# ---------------------------------------------------------------------------------------------- statistics
SK = 6


@functools.lru_cache(maxsize=None)
def _samples(M):
    """coords on a quarter-pixel grid, random visibility; joint 1 = joint 0 + (3, 4) (a rigid pair, both always visible); joints 4 and 5 are
    never visible together."""
    rs = np.random.RandomState(1000 + M)
    coords = (np.floor(rs.uniform(0, 64, size=(M, SK, 2)) * 4) / 4).astype(np.float32)
    coords[:, 1] = coords[:, 0] + np.array([3, 4], dtype=np.float32)
    vis = rs.rand(M, SK) > 0.3
    vis[:, 0] = vis[:, 1] = True
    vis[:, 5] &= ~vis[:, 4]
    return coords, vis, P64.pair_stats(coords, vis)


def _run_prior(coords, vis, parts):
    from uda_poseestimation_amd.utils import SkeletonPrior
    sp = SkeletonPrior(SK, "cuda")
    c, v = torch.from_numpy(coords).cuda(), torch.from_numpy(vis).cuda()
    for cc, vv in zip(torch.tensor_split(c, parts), torch.tensor_split(v, parts)):
        sp.update_coords(cc, vv)
    p = sp.finalize()
    return p["mean"], p["std"], sp.count


def _check_stats(mean, std, count, want, tag):
    n, mu, sd, m2 = want
    mean, std = mean.cpu().double().numpy(), std.cpu().double().numpy()
    assert np.array_equal(count.cpu().numpy(), n.astype(np.int64)), tag
    seen = n > 0
    assert not seen[4, 5] and not seen[5, 4]
    assert np.array_equal(mean[~seen], np.zeros((~seen).sum())) and np.isinf(std[~seen]).all() and np.isfinite(std[seen]).all()
    # mean: one fp32 rounding of the fp64 value (whose own sum of n terms carries n 2^-53)
    bar_mean = (U24 + 2 * n * 2.0 ** -53) * mu
    assert (np.abs(mean - mu)[seen] <= bar_mean[seen]).all(), (tag, np.abs(mean - mu).max())
    # variance: the worst case of the two fp64 sums, 2 n 2^-53 mean(d^2), plus the fp32 rounding of std (2^-24 relative on std, twice that on
    # its square)
    var = sd ** 2
    bar_var = 2 * n * 2.0 ** -53 * m2 + 2.001 * U24 * np.where(seen, var, 0) + 2.0 ** -149
    with np.errstate(invalid="ignore"):
        dv = np.abs(std ** 2 - var)
    print(f"skeleton prior {tag}: max mean err / bar {np.max((np.abs(mean - mu) / np.maximum(bar_mean, 1e-300))[seen]):.2f}, "
          f"max variance err / bar {np.max((dv / bar_var)[seen]):.2f}")
    assert (dv[seen] <= bar_var[seen]).all(), tag
    assert abs(mean[0, 1] - 5.0) <= 5 * U24 and std[0, 1] ** 2 <= bar_var[0, 1]          # the rigid pair


@pytest.mark.parametrize("M", [1, 7, 300, 4096])
def test_pair_statistics_in_one_call_and_split_over_three(M):
    coords, vis, want = _samples(M)
    one = _run_prior(coords, vis, 1)
    _check_stats(*one, want, f"M={M} one call")
    split = _run_prior(coords, vis, 3)
    _check_stats(*split, want, f"M={M} three calls")
    again = _run_prior(coords, vis, 3)
    for a, b in zip(split, again):
        assert torch.equal(a, b)
    for a, b in zip(one, _run_prior(coords, vis, 1)):
        assert torch.equal(a, b)


def test_update_from_labels_equals_update_from_their_decode():
    from uda_poseestimation_amd.utils import SkeletonPrior, get_max_preds_torch
    N, K, H, W = 9, SK, 12, 20
    rs = np.random.RandomState(77)
    label = torch.from_numpy(rs.rand(N, K, H, W).astype(np.float32))
    label[0, 2] = 0.0                   # an empty label plane: maximum 0, not visible
    label[3, 1] = -label[3, 1] - 0.1
    weight = torch.from_numpy((rs.rand(N, K, 1) > 0.25).astype(np.float32))
    weight[1, 0, 0], weight[2, 3, 0] = 0.0, 2.5
    a = SkeletonPrior(K, "cuda").update(label.cuda(), weight.cuda())
    coords, maxv = get_max_preds_torch(label.cuda())
    vis = (maxv.reshape(N, K) > 0) & (weight.cuda().reshape(N, K) > 0)
    assert not bool(vis[0, 2]) and not bool(vis[3, 1]) and not bool(vis[1, 0]) and bool(vis.any())
    b = SkeletonPrior(K, "cuda").update_coords(coords, vis)
    assert torch.equal(a._acc, b._acc) and torch.equal(a.count, b.count)
    pa, pb = a.finalize(), b.finalize()
    assert torch.equal(pa["mean"], pb["mean"]) and torch.equal(pa["std"], pb["std"])
    n, mu, sd, _ = P64.pair_stats(coords.cpu().numpy(), vis.cpu().numpy())
    assert np.array_equal(a.count.cpu().numpy(), n.astype(np.int64))
    # without weights every joint with a positive maximum counts; [N,K] weights are taken as well
    c = SkeletonPrior(K, "cuda").update(label.cuda())
    assert int(c.count[2, 2]) == N - 1 and int(c.count[1, 1]) == N - 1 and int(c.count[0, 0]) == N
    d = SkeletonPrior(K, "cuda").update(label.cuda(), weight.cuda().reshape(N, K))
    assert torch.equal(d._acc, a._acc)
    # what finalize() returns is what generate_prior_map takes
    from uda_poseestimation_amd.utils import generate_prior_map
    out = generate_prior_map(pa, label.cuda())
    truth = P64.prior_map(pa["mean"].cpu(), pa["std"].cpu(), label)
    assert P64.rel_err(out.cpu(), truth) <= _bar(_e32_helper(pa["mean"].cpu(), pa["std"].cpu(), label, truth))
    assert int(SkeletonPrior(K, "cuda").count.sum()) == 0
    empty = SkeletonPrior(K, "cuda").finalize()
    assert bool(torch.isinf(empty["std"]).all()) and float(empty["mean"].abs().max()) == 0


# ---------------------------------------------------------------------------------------------- in the step
TK_, TN, TS = 4, 2, 64


def _net(sd=None):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(23)
    m = pr._pose_resnet("t", TK_, pr.Bottleneck_default, [1, 1, 1, 1], False, False)
    if sd is not None:
        m.load_state_dict(sd)
    return m.cuda()


@pytest.fixture(scope="module")
def setup():
    from uda_poseestimation_amd import synthetic
    from uda_poseestimation_amd.utils import SkeletonPrior
    sd = {k: v.clone() for k, v in _net().cpu().state_dict().items()}
    b = synthetic.mean_teacher_batch(TN, num_keypoints=TK_, image_size=TS, heatmap_size=TS // 4, seed=51)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    src = synthetic.mean_teacher_batch(16, num_keypoints=TK_, image_size=TS, heatmap_size=TS // 4, seed=52)
    prior = SkeletonPrior(TK_, "cuda").update(src["label_s"].cuda(), src["weight_s"].cuda()).finalize()
    assert bool(torch.isfinite(prior["mean"]).all())
    return sd, (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"]), prior


def _trainer(sd, prior, v3=False):
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    tr = MeanTeacherTrainer(_net(sd), _net(sd), lr=1e-3, image_size=TS, heatmap_size=TS // 4, precision="bf16")
    if prior is not None:
        tr.skeleton_prior, tr.prior_v3 = prior, v3
    return tr


@pytest.mark.parametrize("v3", [False, True], ids=["default", "v3"])
def test_eager_step_sees_the_product_everywhere(setup, v3):
    from uda_poseestimation_amd import utils, warp
    sd, args, prior = setup
    tr = _trainer(sd, prior, v3)
    th_s = warp.recon_thetas(args[5], TN, tr.ratio, "cuda")
    th_t = [warp.recon_thetas(args[6], TN, tr.ratio, "cuda")]
    st = tr._forward_part(args[0], args[1], args[2], args[3], [args[4]], th_s, th_t)
    torch.cuda.synchronize()
    raw = st["y_t_tea_raw"]
    assert raw.shape == (TN, TK_, TS // 4, TS // 4)
    want = utils.generate_prior_map(prior, raw, 2, 2, v3=v3, multiply=True)
    assert torch.equal(_bits(st["y_t_tea_recon"].float()), _bits(want.float())) and not torch.equal(want, raw)
    assert torch.equal(st["activates"], utils.heatmap_activations(want))
    assert torch.equal(st["y_t_tea_rect"], utils.rectify(want, tr.sigma))
    out = tr._loss_backward_part(st, None)
    tr._sync_grads()
    torch.cuda.synchronize()
    assert out["prior_map"] is st["y_t_tea_recon"] and out["y_t_tea_recon"] is out["prior_map"] and out["y_t_tea_raw"] is raw
    mask, _, _ = utils.confidence_mask(want, tr.mask_ratio)
    assert torch.equal(out["tea_mask"], mask)
    assert all(bool(torch.isfinite(out[k])) for k in ("loss_all", "loss_s", "loss_c"))
    # the whole step through the public entry point carries the two keys
    out2 = _trainer(sd, prior, v3).train_step(*args)
    torch.cuda.synchronize()
    assert set(out2) == {"loss_all", "loss_s", "loss_c", "y_s", "tea_mask", "y_t_tea_recon", "y_t_stu_recon", "prior_map", "y_t_tea_raw"}
    assert torch.equal(out2["prior_map"], utils.generate_prior_map(prior, out2["y_t_tea_raw"], 2, 2, v3=v3, multiply=True))
    # the settings reach the kernel
    tr3 = _trainer(sd, prior, v3)
    tr3.prior_gamma, tr3.prior_sigma = 0.75, 1.25
    out3 = tr3.train_step(*args)
    assert torch.equal(out3["prior_map"], utils.generate_prior_map(prior, out3["y_t_tea_raw"], 0.75, 1.25, v3=v3, multiply=True))
    assert torch.equal(out3["y_t_tea_raw"], out2["y_t_tea_raw"]) and not torch.equal(out3["prior_map"], out2["prior_map"])


def _state(tr):
    out = [p.detach().clone() for p in list(tr.student.parameters()) + list(tr.teacher.parameters())]
    for p in tr.student.parameters():
        st = tr.stu_optimizer.state.get(p)
        if st:
            out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    return out


def test_three_captured_steps_with_the_prior_equal_three_eager_steps_to_the_bit(setup):
    from uda_poseestimation_amd.engine import GraphedTrainStep
    sd, args, prior = setup
    tr_g, tr_e = _trainer(sd, prior), _trainer(sd, prior)
    gs = GraphedTrainStep(tr_g, *args, warmup=1)          # (the warm-up step is a real step: the twin takes it eagerly)
    tr_e.train_step(*args)
    for _ in range(3):
        og = gs.step(*args)
        oe = tr_e.train_step(*args)
        torch.cuda.synchronize()
        for k in ("loss_all", "loss_s", "loss_c"):
            assert torch.equal(_bits(og[k].float().reshape(1)), _bits(oe[k].float().reshape(1))), k
        for k in ("prior_map", "y_t_tea_raw", "tea_mask"):
            assert torch.equal(og[k], oe[k]), k
    sg, se = _state(tr_g), _state(tr_e)
    assert len(sg) == len(se)
    for i, (a, b) in enumerate(zip(sg, se)):
        assert torch.equal(a, b), f"tensor {i} differs between the captured and the eager step"
    name0 = next(n for n, _ in tr_g.student.named_parameters())
    assert not torch.equal(sg[0], sd[name0].cuda())
    gs.release()


def test_without_a_prior_the_step_is_what_it_was(setup):
    """A trainer whose prior is None - whatever its other prior settings say - returns the keys the step always returned, and every value is
    that of a trainer on which none of the attributes was touched."""
    sd, args, prior = setup
    plain, odd = _trainer(sd, None), _trainer(sd, None)
    odd.prior_gamma, odd.prior_sigma, odd.prior_v3 = 0.3, 7.0, True
    for _ in range(2):
        a, b = plain.train_step(*args), odd.train_step(*args)
        torch.cuda.synchronize()
        assert set(a) == set(b) == {"loss_all", "loss_s", "loss_c", "y_s", "tea_mask", "y_t_tea_recon", "y_t_stu_recon"}
        for k in a:
            assert torch.equal(a[k], b[k]), k
    for x, y in zip(_state(plain), _state(odd)):
        assert torch.equal(x, y)
    with_prior = _trainer(sd, prior).train_step(*args)
    assert "prior_map" in with_prior
