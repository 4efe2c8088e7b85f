"""The grouped weight-gradient launches of a network plan at the C ABI (include/udapose.h): udapose_net_wgrad_pair against the two
udapose_net_backward_phase(..., phase 2) calls it stands for, on the same phase-1 state, for every placement of the two passes'
gradient tensors; and what the backward does when udapose_net_set_policy changes the split form after udapose_net_bind_grads."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

LAYERS, K, N, S = [2, 1, 2, 1], 16, 4, 128


def _net(policy=None):
    """A small student whose plans split the pixel reductions of layer1, layer2, the last deconvolution, the head and the stem (8-stage
    splits: at 128x128 the production split length of 128 stages splits no layer), so that the split sums take part."""
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(7)
    m = pr._pose_resnet("t", K, pr.Bottleneck_default, LAYERS, False, False).cuda().train()
    m.precision = "bf16"
    m.policy = dict({"wgrad_stages": 8}, **(policy or {}))
    return m


def _phase1(net, seeds):
    """Forward + gradient chain (phase 1) of one pass per seed; returns the plan and each pass's (act, ws) arenas, whose dy buffers
    and saved inputs are what phase 2 reads."""
    net.merge_wgrad = True
    for sd in seeds:
        x = torch.randn(N, 3, S, S, generator=torch.Generator().manual_seed(sd)).cuda()
        R = torch.randn(N, K, S // 4, S // 4, generator=torch.Generator().manual_seed(sd + 1)).cuda()
        (net(x) * R).sum().backward()
    net.merge_wgrad = False
    pend, net._pending_wg = net._pending_wg, []
    torch.cuda.synchronize()
    assert len(pend) == len(seeds) and all(p[0] is pend[0][0] for p in pend)
    return pend[0][0], [(p[1], p[2]) for p in pend]


def _numels(net):
    return [p.numel() for p in net.parameters()]


def _flat_ptrs(buf, numels, order=None):
    """Pointer array of one gradient tensor per parameter inside `buf`, laid out in `order` (default: parameter order, the placement of
    the module's own flat gradient buffer).  Parameter 0 always sits at the start, so that every offset a table of another placement
    holds relative to it stays inside `buf`."""
    order = order or list(range(len(numels)))
    assert order[0] == 0
    ptrs, off = [None] * len(numels), 0
    for i in order:
        ptrs[i] = buf.data_ptr() + 4 * off
        off += numels[i]
    assert off <= buf.numel()
    return (C.c_void_p * len(numels))(*ptrs)


def _phase2(hd, pa, act, ws, gp, beta, part=0):
    from uda_poseestimation_amd import _hip
    return hd.L.udapose_net_backward_phase(hd.h, _hip.stream(), None, pa, _hip.ptr(hd.wpack), _hip.ptr(act), _hip.ptr(ws), gp, C.c_float(beta), part, 2)


def _pair(hd, A, gA, bA, B, gB, bB, part=0):
    from uda_poseestimation_amd import _hip
    p = _hip.ptr
    return hd.L.udapose_net_wgrad_pair(hd.h, _hip.stream(), p(A[0]), p(A[1]), gA, C.c_float(bA), p(B[0]), p(B[1]), gB, C.c_float(bB), part)


def _bind(hd, gp):
    assert hd.L.udapose_net_bind_grads(hd.h, gp) == 0


@pytest.mark.parametrize("case", ["same_placement", "other_placement", "one_buffer"])
def test_wgrad_pair_equals_two_phase2_calls(case):
    """udapose_net_wgrad_pair(A, B) = phase 2 of A, then phase 2 of B, to the bit (wgrad_det = 1), from random initial gradient contents:
    (a) same_placement: two flat buffers of the same relative layout (one table per beta; the split sums share it at equal betas),
        betas (0,0), (1,1), (0,1);
    (b) other_placement: B's tensors in another order inside their own buffer (another table, GA != GB), equal betas - before the fix
        B's split sums ran on A's job table and wrote to A's offsets from B's first tensor;
    (c) one_buffer: h_grads_a == h_grads_b with betas (0,1), B accumulating onto A: the result is A + B (before the fix one grid ran
        both, and B's adds could land before A's stores)."""
    from uda_poseestimation_amd import _hip
    net = _net()
    hd, (A, B) = _phase1(net, (11, 21))
    pa, _, _ = net._pointers()
    nl = _numels(net)
    tot = sum(nl)
    rev = [0] + list(range(len(nl) - 1, 0, -1))
    betas = {"same_placement": [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0)], "other_placement": [(0.0, 0.0), (1.0, 1.0)],
             "one_buffer": [(0.0, 1.0)]}[case]
    gen = torch.Generator(device="cuda").manual_seed(3)
    for bA, bB in betas:
        init_a = torch.randn(2 * tot, device="cuda", generator=gen)
        init_b = torch.randn(2 * tot, device="cuda", generator=gen)
        bufs = {}
        for tag in ("ref", "pair"):
            ba = init_a.clone()
            bb = ba if case == "one_buffer" else init_b.clone()
            ga = _flat_ptrs(ba, nl)
            gb = ga if case == "one_buffer" else _flat_ptrs(bb, nl, rev if case == "other_placement" else None)
            _bind(hd, ga)
            _bind(hd, gb)
            if tag == "ref":
                assert _phase2(hd, pa, A[0], A[1], ga, bA) == 0
                assert _phase2(hd, pa, B[0], B[1], gb, bB) == 0
            else:
                assert _pair(hd, A, ga, bA, B, gb, bB) == 0
            torch.cuda.synchronize()
            bufs[tag] = (ba, bb)
        for which in (0, 1):
            r, p = bufs["ref"][which], bufs["pair"][which]
            d = float((r - p).abs().max())
            assert torch.equal(r, p), f"{case} betas ({bA:g},{bB:g}): pass {'AB'[which]}'s buffer differs from two phase-2 calls, max|d| {d:.3e}"
        # (the launches wrote something: the conv weight gradients moved away from the initial contents)
        assert not torch.equal(bufs["pair"][0], init_a)


@pytest.mark.parametrize("start", [1, 0], ids=["det_to_atomic", "atomic_to_det"])
def test_policy_change_after_bind_grads_needs_a_new_bind(start):
    """udapose_net_set_policy after udapose_net_bind_grads, wgrad_det toggled in each direction, the workspace sized by what
    udapose_net_ws_bytes reports after the change (udapose.h): the backward returns UDAPOSE_ERR_NOT_PREPARED (-4) instead of running the
    tables of the old policy (before the fix: the det -> atomic change left the stem scratch uncleared or the partial tiles unsized);
    after a new udapose_net_bind_grads it equals a plan created with the new policy - to the bit when that policy is the deterministic one."""
    from uda_poseestimation_amd import _hip
    target = 1 - start
    net = _net({"wgrad_det": start})
    hd, (A,) = _phase1(net, (31,))
    fresh = _net({"wgrad_det": target})
    hdf, (F,) = _phase1(fresh, (31,))
    pa, _, _ = net._pointers()
    pf, _, _ = fresh._pointers()
    nl = _numels(net)
    tot = sum(nl)
    buf_f = torch.zeros(tot, device="cuda")
    gf = _flat_ptrs(buf_f, nl)
    _bind(hdf, gf)
    assert _phase2(hdf, pf, F[0], F[1], gf, 0.0) == 0
    # the bound plan, policy changed
    pol = _hip.Policy()
    assert hd.L.udapose_net_get_policy(hd.h, C.byref(pol)) == 0 and pol.wgrad_det == start
    pol.wgrad_det = target
    assert hd.L.udapose_net_set_policy(hd.h, C.byref(pol)) == 0
    nb = hd.L.udapose_net_ws_bytes(hd.h)
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    keep = min(nb, A[1].numel())
    ws[:keep].copy_(A[1][:keep])                 # (the phase-1 state: the dy buffers sit in front of the partial tiles)
    buf = torch.zeros(tot, device="cuda")
    gp = _flat_ptrs(buf, nl)                      # (the placement the phase-1 pass bound)
    torch.cuda.synchronize()
    rc = _phase2(hd, pa, A[0], ws, gp, 0.0)
    assert rc == -4, f"backward after a policy change returned {rc}, not UDAPOSE_ERR_NOT_PREPARED"
    _bind(hd, gp)
    assert _phase2(hd, pa, A[0], ws, gp, 0.0) == 0
    torch.cuda.synchronize()
    names = [n_ for n_, _ in net.named_parameters()]
    off = 0
    for n_, n in zip(names, nl):
        a, b = buf[off:off + n], buf_f[off:off + n]
        if target:
            assert torch.equal(a, b), n_
        else:
            assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()) + 1e-7, n_      # (fp32 atomics: summation order)
        off += n
    assert float(buf.abs().max()) > 0
