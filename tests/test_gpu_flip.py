"""Flip-test evaluation on the MI355X (csrc/flip.hip through ops.hflip_batch, lib.keypoint_detection.flip_back / flip_merge,
engine.flip_forward and engine.validate_flip), against the plain-torch restatement of tests/helpers/flip_ref.py (checked on the
CPU by tests/test_flip_cpu.py).

Every comparison is exact.  The merge is one fp32 add and a halving, so the device must give the restatement's bits; the decode that
comes out of the merge launch must be what udapose_heatmap_argmax gives for the merged map, NaN rows and ties included (compared as bit
patterns where a NaN can appear); the image flip is a copy.  Shapes are the smallest at which the kernels can go wrong: one pixel, an odd
width with an unpaired middle joint, widths that are no multiple of 4, a plane that is no multiple of the 256-thread block, a non-square
map, the product shape and the 18-joint layout.
"""
import functools

import pytest
import torch

from helpers import flip_ref as R

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1, 1), (1, 3, 2, 5), (2, 4, 3, 6), (2, 5, 7, 4), (1, 2, 17, 17), (2, 16, 48, 64), (2, 16, 64, 64), (1, 18, 16, 16)]
NAMED = {16: "body16", 18: "animal18"}


def _kd():
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    return kd


def _bits(t):
    return t.contiguous().view(torch.int32)


def pair_sets(K):
    """none / some / the named table that matches K (where there is one)."""
    sets = [[]]
    if K >= 2:
        sets.append([(0, K - 1)])
    if K in NAMED:
        sets.append(NAMED[K])
    return sets


def as_perm(pairs, K):
    return _kd().flip_perm(pairs, K).tolist()


@functools.lru_cache(maxsize=None)
def random_maps(N, K, H, W, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * N + 100 * K + 10 * H + W)
    return torch.randn(N, K, H, W, generator=g), torch.randn(N, K, H, W, generator=g)


def argmax_of(hm):
    """(maxvals, flat_idx, preds) of udapose_heatmap_argmax for hm."""
    from uda_poseestimation_amd import _hip
    B, K, H, W = hm.shape
    maxv = torch.empty(B, K, 1, dtype=torch.float32, device=hm.device)
    idx = torch.empty(B * K, dtype=torch.int32, device=hm.device)
    preds = torch.empty(B, K, 2, dtype=torch.float32, device=hm.device)
    _hip.check(_hip.lib().udapose_heatmap_argmax(_hip.stream(), _hip.ptr(hm), B * K, H, W, _hip.ptr(maxv), _hip.ptr(idx), _hip.ptr(preds),
                                                 None, None, 0), "heatmap_argmax")
    return maxv, idx, preds


def merge_raw(a, f, perm_dev, shift, mode, out=None):
    """udapose_flip_merge with every output: (code, out, maxvals, flat_idx, preds)."""
    from uda_poseestimation_amd import _hip
    B, K, H, W = f.shape
    out = torch.empty_like(f) if out is None else out
    maxv = torch.empty(B, K, 1, dtype=torch.float32, device=f.device)
    idx = torch.empty(B * K, dtype=torch.int32, device=f.device)
    preds = torch.empty(B, K, 2, dtype=torch.float32, device=f.device)
    code = _hip.lib().udapose_flip_merge(_hip.stream(), _hip.ptr(a) if mode else None, _hip.ptr(f), _hip.ptr(perm_dev), B, K, H, W, int(shift),
                                         int(mode), _hip.ptr(out), _hip.ptr(maxv), _hip.ptr(idx), _hip.ptr(preds))
    return code, out, maxv, idx, preds


# ---------------------------------------------------------------------------------------------- flip back / merge
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flip_back_and_merge_equal_the_restatement(shape):
    kd = _kd()
    N, K, H, W = shape
    a, f = random_maps(*shape)
    ad, fd = a.cuda(), f.cuda()
    for pairs in pair_sets(K):
        perm = as_perm(pairs, K)
        for shift in (False, True):
            back = kd.flip_back(fd, pairs, shift=shift)
            assert back.shape == fd.shape and back.dtype == torch.float32
            assert torch.equal(back.cpu(), R.flip_back(f, perm, shift)), (pairs, shift, "mode 0")
            merged = kd.flip_merge(ad, fd, pairs, shift=shift)
            assert torch.equal(merged.cpu(), R.flip_merge(a, f, perm, shift)), (pairs, shift, "mode 1")
            m2, preds, maxv = kd.flip_merge(ad, fd, pairs, shift=shift, decode=True)
            assert torch.equal(m2, merged) and preds.shape == (N, K, 2) and maxv.shape == (N, K, 1)
    assert torch.equal(ad.cpu(), a) and torch.equal(fd.cpu(), f)          # the inputs are left alone
    # numpy in -> numpy out
    pairs = pair_sets(K)[-1]
    out_np = kd.flip_merge(a.numpy(), f.numpy(), pairs, shift=True, decode=True)
    assert all(type(o).__module__ == "numpy" for o in out_np)
    assert torch.equal(torch.from_numpy(out_np[0]), R.flip_merge(a, f, as_perm(pairs, K), True))
    assert torch.equal(torch.from_numpy(kd.flip_back(f.numpy(), pairs)), R.flip_back(f, as_perm(pairs, K)))


def test_merge_in_place_over_the_plain_heatmaps():
    """out may be a: the same thread reads and writes the same element."""
    a, f = random_maps(2, 16, 48, 64)
    ad, fd = a.cuda(), f.cuda()
    perm = as_perm("body16", 16)
    code, out, _, _, _ = merge_raw(ad, fd, torch.tensor(perm, dtype=torch.int32, device="cuda"), 1, 1, out=ad)
    assert code == 0 and out.data_ptr() == ad.data_ptr()
    assert torch.equal(ad.cpu(), R.flip_merge(a, f, perm, True))


# ---------------------------------------------------------------------------------------------- decode out of the merge launch
def decode_inputs(N, K, H, W):
    """name -> (a, f): random; mirror-symmetric maps whose flipped partner is their exact mirror image (every off-centre value ties with
    its mirror: the first flat index has to win); all-negative rows; a row with one NaN; a row with +inf."""
    a, f = random_maps(N, K, H, W, seed=7)
    out = {"random": (a, f)}
    sym = torch.maximum(a, torch.flip(a, [3]))
    out["mirror"] = (sym, None)                        # f = flip(sym) with swapped channels, filled in per table
    out["negative"] = (-a.abs() - 0.125, -f.abs() - 0.125)
    for name, val in (("nan", float("nan")), ("inf", float("inf"))):
        a2, f2 = a.clone(), f.clone()
        a2[0, 0, H // 2, W // 2] = val                 # reaches the merged map through a (mode 1 only)
        f2[N - 1, K - 1, H - 1, W // 2] = val          # ... and through f (both modes; not column 0, whose mirror the shift drops)
        out[name] = (a2, f2)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_decode_equals_heatmap_argmax_of_the_merged_map(shape):
    N, K, H, W = shape
    for name, (a, f) in decode_inputs(*shape).items():
        for pairs in pair_sets(K):
            perm = as_perm(pairs, K)
            perm_dev = torch.tensor(perm, dtype=torch.int32, device="cuda")
            if f is None:
                ff = torch.flip(a, [3])[:, perm].contiguous()
            else:
                ff = f
            ad, fd = a.cuda(), ff.cuda()
            for shift in (0, 1):
                for mode in (0, 1):
                    code, out, maxv, idx, preds = merge_raw(ad, fd, perm_dev, shift, mode)
                    assert code == 0
                    ref = R.flip_merge(a, ff, perm, bool(shift)) if mode else R.flip_back(ff, perm, bool(shift))
                    torch.testing.assert_close(out.cpu(), ref, rtol=0, atol=0, equal_nan=True)
                    m2, i2, p2 = argmax_of(out)
                    tag = (name, pairs, shift, mode)
                    assert torch.equal(_bits(maxv), _bits(m2)), tag
                    assert torch.equal(idx, i2), tag
                    assert torch.equal(_bits(preds), _bits(p2)), tag
                    if name == "mirror" and not shift and mode:
                        # merged = sym: the winner is in the left half (or the middle column) of its row
                        assert torch.equal(out.cpu(), a), tag
                        assert bool((idx.cpu() % W <= (W - 1) // 2).all()), tag
                    if name == "negative":
                        assert not preds.any() and bool((maxv < 0).all()), tag
                    if name == "nan":
                        assert bool(torch.isnan(maxv.flatten()).any()), tag
                    if name == "inf":
                        assert bool(torch.isinf(maxv.flatten()).any()), tag


@pytest.mark.parametrize("H,W", [(5, 7), (8, 8), (72, 72)], ids=["5x7_scalar_loads", "8x8_vector_loads", "72x72_rows_past_4096"])
def test_every_user_of_the_block_argmax_gives_the_same_index_and_maximum_bits(H, W):
    """udapose_heatmap_argmax, the decode of flip_merge, udapose_soft_argmax_fwd's saved index and udapose_refine_decode (quarter mode) reduce
    with one block arg-max (csrc/common.h): the same first flat index and the same bits of the maximum on a row with one NaN, a row of
    -inf, a constant row (first index wins), an all-negative row and two ordinary ones.  72x72 rows are longer than the 4096 floats the
    soft-argmax keeps in registers; that size runs the first and the third only."""
    from uda_poseestimation_amd import _hip
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(1, 6, H, W, generator=g)
    x[0, 0, H // 2, W // 3] = float("nan")
    x[0, 1] = float("-inf")
    x[0, 2] = 0.375
    x[0, 3] = -x[0, 3].abs() - 0.125
    xd = x.cuda()
    R = 6
    want_idx = [H // 2 * W + W // 3, 0, 0] + [int(x[0, r].argmax()) for r in (3, 4, 5)]
    maxv, idx, _ = argmax_of(xd)
    assert idx.tolist() == want_idx
    assert torch.equal(_bits(maxv).flatten()[1:].cpu(), _bits(x.reshape(R, -1).amax(1))[1:]) and bool(torch.isnan(maxv.flatten()[0]))

    def new():
        return torch.full((R,), -1, dtype=torch.int32, device="cuda"), torch.full((R,), 7.0, device="cuda")

    got = {}
    i2, m2 = new()
    coords, stats = torch.empty(R, 2, device="cuda"), torch.empty(4 * R, device="cuda")
    _hip.check(_hip.lib().udapose_soft_argmax_fwd(_hip.stream(), _hip.ptr(xd), R, H, W, 10.0, 2, _hip.ptr(coords), _hip.ptr(m2), _hip.ptr(i2),
                                                  _hip.ptr(stats)), "soft_argmax_fwd")
    got["soft_argmax_fwd"] = (i2, m2)
    if H * W <= 4096:
        # (x + flip_back(flip(x))) * 0.5 is x, bit for bit: the merge decodes the map itself
        code, out, mf, i_f, _ = merge_raw(xd, torch.flip(xd, [3]).contiguous(), torch.arange(6, dtype=torch.int32, device="cuda"), 0, 1)
        assert code == 0 and torch.equal(_bits(out), _bits(xd))
        got["flip_merge"] = (i_f, mf.flatten())
        i3, m3 = new()
        _hip.check(_hip.lib().udapose_refine_decode(_hip.stream(), _hip.ptr(xd), R, H, W, 0, 0, 0.0, _hip.ptr(coords), _hip.ptr(m3), _hip.ptr(i3)),
                   "refine_decode")
        got["refine_decode"] = (i3, m3)
    for name, (i, m) in got.items():
        assert torch.equal(i, idx), (name, i.tolist(), idx.tolist())
        assert torch.equal(_bits(m), _bits(maxv.flatten())), name


# ---------------------------------------------------------------------------------------------- table guard and argument checks
def test_table_entries_out_of_range_are_the_identity():
    """An argument check, not a fault: the kernel clamps, so nothing outside f is read whatever the table holds."""
    for shape in [(2, 4, 3, 6), (2, 16, 64, 64)]:
        N, K, H, W = shape
        a, f = random_maps(*shape, seed=3)
        perm = list(range(K))
        perm[0], perm[1], perm[2], perm[3] = -1, K, 3, 2
        if K > 4:
            perm[4], perm[5] = 2 ** 31 - 1, -2 ** 31
        perm_dev = torch.tensor(perm, dtype=torch.int32, device="cuda")
        for shift in (0, 1):
            code, out, maxv, idx, preds = merge_raw(a.cuda(), f.cuda(), perm_dev, shift, 1)
            assert code == 0
            assert torch.equal(out.cpu(), R.flip_merge(a, f, perm, bool(shift)))
            assert torch.equal(out.cpu(), R.flip_merge(a, f, [0, 1, 3, 2] + list(range(4, K)), bool(shift)))
            m2, i2, p2 = argmax_of(out)
            assert torch.equal(maxv, m2) and torch.equal(idx, i2) and torch.equal(preds, p2)


def test_argument_checks():
    from uda_poseestimation_amd import _hip
    L, s, ptr = _hip.lib(), _hip.stream(), _hip.ptr
    a, f = (t.cuda() for t in random_maps(2, 4, 3, 6))
    perm = torch.arange(4, dtype=torch.int32, device="cuda")
    keep = f.clone()
    assert merge_raw(a, f, perm, 0, 1, out=f)[0] == -1                     # out == f
    assert merge_raw(a, f, perm, 0, 0, out=f)[0] == -1
    buf = torch.zeros(1024, device="cuda")
    n = f.numel()
    ov_f, ov_out = buf[:n].view_as(f), buf[n // 2:n // 2 + n].view_as(f)     # out overlaps f partially
    assert merge_raw(a, ov_f, perm, 0, 1, out=ov_out)[0] == -1
    assert L.udapose_flip_merge(s, None, ptr(f), ptr(perm), 2, 4, 3, 6, 0, 1, ptr(a), None, None, None) == -1       # mode 1 without a
    assert L.udapose_flip_merge(s, ptr(a), ptr(f), ptr(perm), 2, 4, 3, 6, 2, 1, ptr(buf), None, None, None) == -1    # shift / mode are 0 or 1
    assert L.udapose_flip_merge(s, ptr(a), ptr(f), ptr(perm), 2, 4, 3, 6, 0, 2, ptr(buf), None, None, None) == -1
    assert L.udapose_flip_merge(s, ptr(a), ptr(f), ptr(perm), 2, 0, 3, 6, 0, 1, ptr(buf), None, None, None) == -1
    # the image side: dst overlapping src, with and without the kept copy
    x = buf[:2 * 3 * 5 * 8]
    rows, W = 3 * 5, 8
    assert L.udapose_hflip_batch(s, ptr(x), ptr(x), 2, rows, W, 0) == -1
    assert L.udapose_hflip_batch(s, ptr(x), x.data_ptr() + 4 * (x.numel() - 4), 2, rows, W, 0) == -1
    assert L.udapose_hflip_batch(s, x.data_ptr() + 4 * x.numel(), ptr(x), 2, rows, W, 0) == 0           # adjacent: no overlap
    assert L.udapose_hflip_batch(s, x.data_ptr() + 4 * x.numel(), ptr(x), 2, rows, W, 1) == -1          # the 2N result reaches into src
    assert L.udapose_hflip_batch(s, ptr(x), x.data_ptr() + 4 * x.numel(), 2, rows, W, 2) == -1
    torch.cuda.synchronize()
    assert torch.equal(f, keep)                       # refused calls wrote nothing


# ---------------------------------------------------------------------------------------------- the image side
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 3, 64, 64), (2, 3, 6, 10)], ids=lambda s: "x".join(map(str, s)))
def test_hflip_batch_equals_torch_flip(shape):
    from uda_poseestimation_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g)
    xd = x.cuda()
    flipped = torch.flip(x, [3])
    assert torch.equal(ops.hflip_batch(xd).cpu(), flipped)
    both = ops.hflip_batch(xd, keep_original=True)
    assert both.shape == (2 * shape[0],) + shape[1:]
    assert torch.equal(both.cpu(), torch.cat([x, flipped]))
    assert torch.equal(xd.cpu(), x)


def test_hflip_batch_unaligned_rows_take_the_scalar_path():
    """W % 4 == 0 but the batch starts 4 bytes off a 16-byte boundary: element by element, same result."""
    from uda_poseestimation_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 6, 8, generator=g)
    store = torch.zeros(x.numel() + 1, device="cuda")
    xd = store[1:].view(2, 3, 6, 8)
    xd.copy_(x)
    assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    assert torch.equal(ops.hflip_batch(xd, keep_original=True).cpu(), torch.cat([x, torch.flip(x, [3])]))


# ---------------------------------------------------------------------------------------------- the network: flip_forward, validate
@functools.lru_cache(maxsize=None)
def seeded_net_and_batches():
    """pose_resnet50, K = 16, eval mode, with running statistics of one train-mode forward (so that eval-mode BatchNorm is not the
    identity) and a head wide enough for distinct peaks; two batches of two 64x64 images with labels."""
    from uda_poseestimation_amd import synthetic
    import uda_poseestimation_amd.lib.models as models
    torch.manual_seed(0)
    net = models.pose_resnet50(16, pretrained_backbone=False)
    torch.nn.init.normal_(net.head.weight, std=0.05)
    net = net.cuda()
    batches = []
    for i in range(2):
        b = synthetic.mean_teacher_batch(2, num_keypoints=16, image_size=64, heatmap_size=16, seed=40 + i)
        batches.append((b["x_s"], b["label_s"], b["weight_s"]))
    net.train()
    net.bn_momentum = 1.0
    with torch.no_grad():
        net(torch.cat([b[0] for b in batches]).cuda())
    net.bn_momentum = 0.1
    net.eval()
    return net, batches


def restated_merged(net, x, perm, shift):
    """The restatement applied to two separate forwards of the product network."""
    with torch.no_grad():
        y, yf = net(x.cuda()), net(torch.flip(x, [3]).cuda())
    return R.flip_merge(y.cpu(), yf.cpu(), perm, shift)


@pytest.mark.parametrize("shift", [False, True])
def test_flip_forward_equals_the_restatement_on_two_forwards(shift):
    from uda_poseestimation_amd import engine
    net, batches = seeded_net_and_batches()
    x = batches[0][0]
    perm = as_perm("body16", 16)
    merged = engine.flip_forward(net, x.cuda(), "body16", shift_heatmap=shift)
    ref = restated_merged(net, x, perm, shift)
    assert merged.shape == (2, 16, 16, 16) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    assert torch.equal(merged.cpu(), ref)
    with torch.no_grad():
        assert not torch.equal(merged, net(x.cuda()))              # the flip test is not the plain forward
    net.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            engine.flip_forward(net, x.cuda(), "body16")
    finally:
        net.eval()


@pytest.mark.parametrize("decode", ["argmax", "soft"])
def test_validate_flip(decode):
    from uda_poseestimation_amd import engine
    from uda_poseestimation_amd.lib.models.loss import JointsMSELoss
    kd = _kd()
    net, batches = seeded_net_and_batches()
    perm = as_perm("body16", 16)
    crit = JointsMSELoss()
    # what the existing accuracy_device and criterion give on the restated merged maps, accumulated as validate() accumulates
    acc_sum = torch.zeros(16, dtype=torch.float64)
    acc_cnt = torch.zeros(16, dtype=torch.float64)
    loss_sum, seen = torch.zeros((), dtype=torch.float64), 0
    for x, label, weight in batches:
        m = restated_merged(net, x, perm, False).cuda()
        acc = kd.accuracy_device(m, label.cuda(), decode=decode)[0].cpu()
        loss = crit(m, label.cuda(), weight.cuda()).cpu()
        n = x.shape[0]
        present = (acc != -1).to(torch.float32)
        acc_sum += (acc * present).double() * n
        acc_cnt += present.double() * n
        loss_sum += loss.double() * n
        seen += n
    exp_acc = torch.where(acc_cnt > 0, acc_sum / acc_cnt.clamp(min=1), torch.zeros_like(acc_sum)).tolist()
    exp_loss = (loss_sum / seen).item()
    got_acc, got_loss = engine.validate_flip(batches, net, "body16", decode=decode)
    assert got_acc == exp_acc and got_loss == exp_loss, (got_acc, exp_acc, got_loss, exp_loss)
    assert not net.training
    # validate() itself: the plain evaluation of the plain forward's maps, and not the same numbers (the flip test cannot be a no-op)
    p_sum, p_cnt, p_loss = torch.zeros(16, dtype=torch.float64), torch.zeros(16, dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    for x, label, weight in batches:
        with torch.no_grad():
            y = net(x.cuda())
        acc = kd.accuracy_device(y, label.cuda(), decode=decode)[0].cpu()
        present = (acc != -1).to(torch.float32)
        p_sum += (acc * present).double() * x.shape[0]
        p_cnt += present.double() * x.shape[0]
        p_loss += crit(y, label.cuda(), weight.cuda()).cpu().double() * x.shape[0]
    plain = engine.validate(batches, net, decode=decode)
    assert plain == (torch.where(p_cnt > 0, p_sum / p_cnt.clamp(min=1), torch.zeros_like(p_sum)).tolist(), (p_loss / seen).item())
    assert plain != (got_acc, got_loss)
    shifted = engine.validate_flip(batches, net, "body16", decode=decode, shift_heatmap=True)
    assert shifted[1] != got_loss
    net.train()
    try:
        assert engine.validate_flip(batches, net, "body16", decode=decode) == (got_acc, got_loss) and net.training     # the mode is restored
    finally:
        net.eval()
    with pytest.raises(ValueError):
        engine.validate_flip(batches, net, [(0, 16)])


# ---------------------------------------------------------------------------------------------- capture
def test_flip_merge_with_decode_captures_and_replays():
    kd = _kd()
    shape = (2, 16, 64, 64)
    a, f = (t.cuda() for t in random_maps(*shape, seed=21))
    sa, sf = a.clone(), f.clone()

    def run():
        return kd.flip_merge(sa, sf, "body16", shift=True, decode=True) + (kd.flip_back(sf, "body16"),)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for i in range(2):
        na, nf = (t.cuda() for t in random_maps(*shape, seed=22 + i))
        sa.copy_(na)
        sf.copy_(nf)
        graph.replay()
        eager = kd.flip_merge(na, nf, "body16", shift=True, decode=True) + (kd.flip_back(nf, "body16"),)
        torch.cuda.synchronize()
        assert len(captured) == len(eager) == 4
        for j, (c, e) in enumerate(zip(captured, eager)):
            assert torch.equal(_bits(c), _bits(e)), (i, j)
        assert torch.equal(eager[0].cpu(), R.flip_merge(na.cpu(), nf.cpu(), as_perm("body16", 16), True))
