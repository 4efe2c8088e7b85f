"""The mirrored re-warp on the MI355X (udapose_affine_nearest_mirror / udapose_affine_bilinear_mirror through warp.warp_chain(mirror=, perm=)),
DESIGN.md 4.23: forward and backward of both modes must be, bit for bit, the composition of torch.flip(., [-1]), a channel index_select by the
flip permutation and the plain warp_chain (tests/helpers/mirror_views_ref.py states the composition); a sample whose byte is 0, and a call
without `mirror`, are the plain launch."""
import numpy as np
import pytest
import torch

from helpers import mirror_views_ref as R

pytestmark = pytest.mark.gpu

TABLES = {"body16": (16, "body16"), "k5_one_pair": (5, ((1, 3),))}
PLANES = {"32x32": (32, 32), "24x40": (24, 40)}


def _thetas(N, stages, seed):
    """The loop's chain for synthetic.aug_params, the last sample's view scaled by 0.6 (its un-warp magnifies: several outputs share an
    input pixel); stages = 1 keeps the rotate-and-scale stage."""
    from uda_poseestimation_amd import synthetic, warp
    ap = list(synthetic.aug_params(N, np.random.RandomState(seed)))
    scale = ap[3].clone()
    scale[N - 1] = 1.0 / 0.6
    ap[3] = scale
    th = warp.recon_thetas(ap, N, 4.0, "cuda")
    return th if stages == 3 else th[:, 1:2].contiguous()


def _perm(table, C):
    from uda_poseestimation_amd import warp
    return warp.mirror_perm(table, C, "cuda")


def _check_case(x, th, bits, perm, mode):
    from uda_poseestimation_amd import warp
    plain = lambda a, t: warp.warp_chain(a, t, mode)
    mirror = torch.tensor(bits, dtype=torch.uint8, device="cuda")
    xg = x.clone().requires_grad_(True)
    out = warp.warp_chain(xg, th, mode, mirror=mirror, perm=perm)
    assert torch.equal(out.detach(), R.compose_forward(plain, x, th, bits, perm))
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).cuda()
    out.backward(g)
    assert torch.equal(xg.grad, R.compose_backward(R.autograd_backward(warp.warp_chain, mode), g, th, bits, perm))
    # samples whose byte is 0: the plain call, forward and backward
    xp = x.clone().requires_grad_(True)
    ref = warp.warp_chain(xp, th, mode)
    ref.backward(g)
    for n, m in enumerate(bits):
        if m == 0:
            assert torch.equal(out[n].detach(), ref[n].detach()) and torch.equal(xg.grad[n], xp.grad[n])
    assert float(out.detach().abs().sum()) > 0 and float(xg.grad.abs().sum()) > 0


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("stages", [3, 1])
@pytest.mark.parametrize("plane", sorted(PLANES))
@pytest.mark.parametrize("table", sorted(TABLES))
def test_mirrored_warp_chain_is_the_composition(table, plane, stages, mode):
    C, pairs = TABLES[table]
    H, W = PLANES[plane]
    x = torch.randn(3, C, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    _check_case(x, _thetas(3, stages, 5), (1, 0, 1), _perm(pairs, C), mode)


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_mirror_in_and_both_bits_without_perm(mode):
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()
    _check_case(x, _thetas(3, 3, 6), (2, 3, 0), None, mode)
    _check_case(x, _thetas(3, 1, 6), (3, 2, 1), None, mode)


def test_both_bits_with_perm_take_no_swap():
    """perm is applied when exactly one bit is set: M o chain o M keeps the channels where they are."""
    from uda_poseestimation_amd import warp
    x = torch.randn(2, 16, 32, 32, generator=torch.Generator().manual_seed(3)).cuda()
    th = _thetas(2, 3, 8)
    perm = _perm("body16", 16)
    _check_case(x, th, (3, 2), perm, "nearest")
    both = warp.warp_chain(x, th, "nearest", mirror=torch.tensor([3, 3], dtype=torch.uint8, device="cuda"), perm=perm)
    assert torch.equal(both, torch.flip(warp.warp_chain(torch.flip(x, [-1]), th), [-1]))


def test_mirror_none_is_todays_call():
    from uda_poseestimation_amd import warp
    x = torch.randn(3, 16, 32, 32, generator=torch.Generator().manual_seed(4)).cuda()
    th = _thetas(3, 3, 9)
    zeros = torch.zeros(3, dtype=torch.uint8, device="cuda")
    for mode in warp.MODES:
        ref = warp.warp_chain(x, th, mode)
        assert torch.equal(warp.warp_chain(x, th, mode, mirror=None, perm=None), ref)
        assert torch.equal(warp.warp_chain(x, th, mode, mirror=zeros, perm=_perm("body16", 16)), ref)


def test_image_sized_nearest_forward():
    from uda_poseestimation_amd import warp
    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(5)).cuda()
    th = _thetas(2, 3, 10)
    plain = lambda a, t: warp.warp_chain(a, t)
    for bits in ((1, 2), (2, 1), (3, 0)):
        got = warp.warp_chain(x, th, mirror=torch.tensor(bits, dtype=torch.uint8, device="cuda"))
        assert torch.equal(got, R.compose_forward(plain, x, th, bits))


def test_image_sized_nearest_backward_without_shared_pixels():
    """128 x 128 planes exceed the deterministic backward's LDS budget and take the atomic form; with integer shifts every input pixel has at
    most one output, so that form too has one answer - the composition's."""
    from uda_poseestimation_amd import warp
    th = torch.tensor([[[1, 0, 3, 0, 1, -2]], [[1, 0, -5, 0, 1, 4]]], dtype=torch.float32).cuda()
    g = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(6)).cuda()
    for bits in ((1, 2), (3, 0)):
        x = torch.zeros_like(g, requires_grad=True)
        warp.warp_chain(x, th, mirror=torch.tensor(bits, dtype=torch.uint8, device="cuda")).backward(g)
        assert torch.equal(x.grad, R.compose_backward(R.autograd_backward(warp.warp_chain, "nearest"), g, th, bits))


def test_refusals():
    from uda_poseestimation_amd import warp
    x = torch.randn(2, 16, 32, 32).cuda()
    th = _thetas(2, 3, 11)
    mirror = torch.tensor([1, 0], dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError):       # two 160 x 160 planes exceed the 150 KB LDS budget
        warp.warp_chain(torch.zeros(2, 1, 160, 160, device="cuda"), th, "bilinear", mirror=mirror)
    with pytest.raises(ValueError):
        warp.warp_chain(x, th, mirror=mirror, perm=_perm("body16", 16)[:15].contiguous())
    with pytest.raises(ValueError):
        warp.warp_chain(x, th, mirror=mirror, perm=_perm("animal18", 18))
    with pytest.raises(ValueError):
        warp.warp_chain(x, th, mirror=mirror.cpu())
    with pytest.raises(ValueError):
        warp.warp_chain(x, th, mirror=torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        warp.warp_chain(x, th, mirror=mirror.int())
    cycle = torch.tensor([1, 2, 0] + list(range(3, 16)), dtype=torch.int32, device="cuda")      # a permutation, but no involution
    with pytest.raises(ValueError):
        warp.warp_chain(x, th, mirror=mirror, perm=cycle)
    with pytest.raises(ValueError):
        warp.warp_chain(x, th, mirror=mirror, perm=torch.tensor([16] + list(range(1, 16)), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        warp.warp_chain(x, th, perm=_perm("body16", 16))
    from uda_poseestimation_amd import synthetic
    flagged = synthetic.aug_params(2, np.random.RandomState(0)) + [torch.tensor([0, 1])]
    with pytest.raises(ValueError):       # flagged samples and no table
        warp.recon_heatmaps(x, flagged, 4.0)
    assert torch.equal(warp.recon_heatmaps(x, flagged, 4.0, flip_pairs="body16"),
                       warp.warp_chain(x, warp.recon_thetas(flagged, 2, 4.0, "cuda"), mirror=mirror.flip(0), perm=_perm("body16", 16)))


def test_mirrored_deterministic_backward_repeats():
    from uda_poseestimation_amd import warp
    th = _thetas(3, 3, 12)
    mirror = torch.tensor([1, 2, 1], dtype=torch.uint8, device="cuda")
    perm = _perm("body16", 16)
    g = torch.randn(3, 16, 32, 32, generator=torch.Generator().manual_seed(8)).cuda()
    grads = []
    for _ in range(2):
        x = torch.zeros_like(g, requires_grad=True)
        warp.warp_chain(x, th, "nearest", mirror=mirror, perm=perm).backward(g)
        grads.append(x.grad)
    assert torch.equal(grads[0], grads[1])
    # the magnifying sample does share input pixels: fewer non-zero gradients than outputs that hit the plane
    hit = warp.warp_chain(torch.ones(3, 1, 32, 32, device="cuda"), th)[2]
    assert int((grads[0][2, 0] != 0).sum()) < int(hit.sum())
