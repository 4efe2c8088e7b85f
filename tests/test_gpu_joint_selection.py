"""Joint selection on the MI355X (csrc/select.hip through lib.models.loss, utils.confidence_mask and the mean-teacher step): top-k mining
losses against the fp64 restatement (tests/helpers/joint_selection_fp64.py), the per-joint and fixed-threshold confidence masks against
torch.kthvalue and `>` exactly, capture and replay, and the step with the new criteria and mask modes.

THE BARS are derived, not measured (u = 2^-24, the unit roundoff of fp32; the fp64 reference is evaluated on the same fp32 inputs):
  row      <= 8u relative: fl(a - b), its square, the cast of the double sum, two roundings in the factor - 7u; a zero row is exactly 0
  sample   <= 10u: the rows' 8u, the exact double sum of them, one cast
  mean     <= 12u: the samples' 10u, one cast
  gradient <= 6u relative PER ELEMENT: three roundings in the coefficient, one in a - b, one product
A selection can only be compared where fp32 rounding cannot change it: every test that compares selections first asserts, on the host in
fp64 and over EVERY sample, that the two rows on either side of the selection boundary differ by at least 64u relative (or are both zero,
a tie by index).  Every test prints its measured worst figure beside the bar.
"""
import pytest
import torch

from helpers import joint_selection_fp64 as R64

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
ROW_BAR, SAMPLE_BAR, MEAN_BAR, GRAD_BAR, GAP_BAR = 8 * U, 10 * U, 12 * U, 6 * U, 64 * U
SHAPES = [(4, 16, 64, 64), (3, 17, 15, 17), (2, 1, 8, 8), (5, 64, 16, 16), (32, 16, 64, 64)]


def _L():
    from uda_poseestimation_amd.lib.models import loss as L
    return L


def _lib():
    from uda_poseestimation_amd import _hip
    return _hip.lib(), _hip.stream()


def make_inputs(N, K, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    scale = 0.3 + 5.7 * torch.rand(N, K, 1, 1, generator=g)
    stu = torch.randn(N, K, H, W, generator=g) * scale
    tea = stu + 0.5 * torch.randn(N, K, H, W, generator=g) * scale
    label = torch.exp(-12 * torch.rand(N, K, H, W, generator=g))
    label[label < 0.02] = 0.0
    weight = torch.where(torch.rand(N, K, 1, generator=g) < 0.25, torch.zeros(N, K, 1), 0.5 + torch.rand(N, K, 1, generator=g))      # 0 on about a quarter, non-unit elsewhere
    weight[0, 0] = 1.25
    tea_mask = torch.rand(N, K, generator=g) < 0.6
    tea_mask[0, 0] = True
    return {"stu": stu, "tea": tea, "label": label, "weight": weight, "tea_mask": tea_mask}


def _topks(K):
    return sorted({1, min(8, K), K})


# kind -> (second operand, factor, largest, device criterion, restatement)
def _kinds(topk):
    L = _L()
    return {
        "ohkm": ("label", "weight", True, lambda x, d: L.JointsOHKMMSELoss(topk), lambda x, d: R64.joints_ohkm(x, d["label"], d["weight"], topk)),
        "cons_hard": ("tea", "tea_mask", True, lambda x, d: L.ConsTopKLoss(topk), lambda x, d: R64.cons_topk(x, d["tea"], d["tea_mask"], topk, True)),
        "cons_small": ("tea", "tea_mask", False, lambda x, d: L.ConsTopKLoss(topk, largest=False),
                       lambda x, d: R64.cons_topk(x, d["tea"], d["tea_mask"], topk, False)),
    }


def _call(crit, kind, x, d):
    return crit(x, d["label"], d["weight"]) if kind == "ohkm" else crit(x, d["tea"], tea_mask=d["tea_mask"])


def _cast(d, dtype=None, device=None):
    out = {}
    for k, v in d.items():
        if v.dtype.is_floating_point and dtype is not None:
            v = v.to(dtype)
        out[k] = v.to(device) if device is not None else v
    return out


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int16) if t.element_size() == 2 else t.view(torch.uint8))


def _rel(dev, ref):
    """Worst |dev - ref| / |ref| over the elements with ref != 0; elements with ref == 0 must be exactly 0 on the device."""
    dev, ref = dev.detach().double().reshape(-1), ref.detach().double().reshape(-1)
    z = ref == 0
    assert bool((dev[z] == 0).all()), "an element that is zero in fp64 is not exactly zero on the device"
    return float(((dev[~z] - ref[~z]).abs() / ref[~z].abs()).max()) if bool((~z).any()) else 0.0


def dev_select(kind, d, topk, largest, want_mean=True):
    """The two forward launches at the C ABI: (rows [N,K], sel bool [N,K], sample [N], mean) of device inputs d."""
    lib, st = _lib()
    x = d["stu"].float().contiguous()
    N, K = x.shape[:2]
    R, HW = N * K, x[0, 0].numel()
    rows = torch.empty(R, device="cuda")
    sel = torch.empty(R, dtype=torch.uint8, device="cuda")
    sample = torch.empty(N, device="cuda")
    mean = torch.empty((), device="cuda")
    w = m = None
    if kind == "ohkm":
        y, w = d["label"].float().contiguous(), d["weight"].float().reshape(-1).contiguous()
        assert lib.udapose_joints_mse_fwd(st, x.data_ptr(), y.data_ptr(), w.data_ptr(), R, HW, rows.data_ptr(), None) == 0
    else:
        y, m = d["tea"].float().contiguous(), d["tea_mask"].to(torch.uint8).reshape(-1).contiguous()
        assert lib.udapose_cons_loss_fwd(st, x.data_ptr(), y.data_ptr(), m.data_ptr(), R, HW, rows.data_ptr(), None) == 0
    rc = lib.udapose_topk_select(st, rows.data_ptr(), None if w is None else w.data_ptr(), None if m is None else m.data_ptr(), N, K, topk,
                                 int(largest), sel.data_ptr(), sample.data_ptr(), mean.data_ptr() if want_mean else None)
    assert rc == 0, rc
    return rows.reshape(N, K), sel.bool().reshape(N, K), sample, mean


def _rows64(kind, d64):
    if kind == "ohkm":
        return R64.rows_joints(d64["stu"], d64["label"], d64["weight"]), d64["weight"].reshape(d64["stu"].shape[:2]) == 0
    return R64.rows_cons(d64["stu"], d64["tea"], d64["tea_mask"]), ~d64["tea_mask"]


# ---------------------------------------------------------------------------------------------- values, selections, gradients
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_selection_values_and_gradients_match_the_fp64_restatement(shape):
    N, K, H, W = shape
    d = make_inputs(*shape, seed=11 + K)
    d64, dd = _cast(d, torch.float64), _cast(d, None, "cuda")
    worst = {"row": 0.0, "sample": 0.0, "mean": 0.0, "grad": 0.0, "vs_plain": 0.0}
    gap = float("inf")
    for topk in _topks(K):
        for kind, (other, factor, largest, make, ref_fn) in _kinds(topk).items():
            rows64, zero = _rows64(kind, d64)
            # the selection condition, over every sample: fp32 rounding (<= 8u per row) cannot move a row across the boundary
            g_ = R64.boundary_gap(rows64, zero, topk, largest)
            gap = min(gap, g_)
            assert g_ >= GAP_BAR, (kind, topk, g_ / U)
            x64 = d64["stu"].clone().requires_grad_(True)
            l64, s64, sel64 = ref_fn(x64, d64)
            l64.backward()
            rows, sel, sample, mean = dev_select(kind, dd, topk, largest)
            crit = make(None, None)
            x = dd["stu"].clone().requires_grad_(True)
            loss = _call(crit, kind, x, dd)
            loss.backward()
            torch.cuda.synchronize()
            assert loss.dtype == torch.float32 and x.grad.dtype == torch.float32 and x.grad.shape == x.shape
            assert torch.equal(_bits(loss), _bits(mean))                            # the class issues exactly those launches
            assert crit.last_selection.dtype == torch.bool and not crit.last_selection.requires_grad
            assert torch.equal(crit.last_selection.cpu(), sel64) and torch.equal(sel.cpu(), sel64), (kind, topk)
            assert not sel.cpu()[zero].any()
            worst["row"] = max(worst["row"], _rel(rows.cpu(), rows64))
            worst["sample"] = max(worst["sample"], _rel(sample.cpu(), s64.detach()))
            worst["mean"] = max(worst["mean"], _rel(loss.cpu(), l64.detach()))
            worst["grad"] = max(worst["grad"], _rel(x.grad.cpu(), x64.grad))
            # rows that are unselected or have a zero factor: gradient exactly 0 (x64.grad is exactly 0 there, _rel asserted it)
            assert bool((x.grad.cpu()[~sel64] == 0).all())
            if topk == K:
                plain = _L().JointsMSELoss()(dd["stu"], dd["label"], dd["weight"]) if kind == "ohkm" else _L().ConsLoss()(dd["stu"], dd["tea"], tea_mask=dd["tea_mask"])
                worst["vs_plain"] = max(worst["vs_plain"], _rel(loss.cpu(), plain.cpu()))
    print(f"\n{shape}: smallest boundary gap {gap / U:.0f}u (bar >= 64u); row {worst['row'] / U:.2f}u (bar 8u), sample {worst['sample'] / U:.2f}u (10u), "
          f"mean {worst['mean'] / U:.2f}u (12u), gradient element {worst['grad'] / U:.2f}u (6u), topk == K against the plain loss {worst['vs_plain'] / U:.2f}u (12u)")
    assert worst["row"] <= ROW_BAR and worst["sample"] <= SAMPLE_BAR and worst["mean"] <= MEAN_BAR and worst["grad"] <= GRAD_BAR
    assert worst["vs_plain"] <= MEAN_BAR


@pytest.mark.parametrize("kind", ["ohkm", "cons_hard", "cons_small"])
def test_exact_ties_go_to_the_lower_joint_index(kind):
    d = make_inputs(3, 16, 16, 16, seed=5)
    n = 1
    for k in ("stu", "tea", "label", "weight", "tea_mask"):
        d[k][n, 5] = d[k][n, 2]                                      # row 5 is a bit-copy of row 2
    d["weight"][n, 2] = d["weight"][n, 5] = 0.75
    d["tea_mask"][n, 2] = d["tea_mask"][n, 5] = True
    d64, dd = _cast(d, torch.float64), _cast(d, None, "cuda")
    rows64, zero = _rows64(kind, d64)
    largest = kind != "cons_small"
    cand = torch.ones_like(zero) if largest else ~zero
    topk = int(R64.ranks(rows64, cand, largest)[n, 2]) + 1           # row 2 is the last one that fits; row 5 is the first that does not
    assert rows64[n, 2] == rows64[n, 5] and 1 <= topk < 16
    _, _, _, make, ref_fn = _kinds(topk)[kind]
    _, _, sel64 = ref_fn(d64["stu"], d64)
    crit = make(None, None)
    x = dd["stu"].clone().requires_grad_(True)
    _call(crit, kind, x, dd).backward()
    sel = crit.last_selection.cpu()
    print(f"\n{kind}: topk {topk}, selection of the tied sample {sel[n].int().tolist()}")
    assert bool(sel[n, 2]) and not bool(sel[n, 5]) and torch.equal(sel, sel64)
    assert bool((x.grad[n, 5] == 0).all()) and bool((x.grad[n, 2] != 0).any())


@pytest.mark.parametrize("kind", ["ohkm", "cons_hard", "cons_small"])
def test_fewer_candidates_than_topk_keep_the_divisor(kind):
    d = make_inputs(2, 16, 16, 16, seed=6)
    keep = [1, 7, 12]
    d["weight"][0] = 0.0
    d["tea_mask"][0] = False
    for j in keep:
        d["weight"][0, j] = 0.5 + 0.1 * j
        d["tea_mask"][0, j] = True
    d64, dd = _cast(d, torch.float64), _cast(d, None, "cuda")
    rows64, _ = _rows64(kind, d64)
    _, _, largest, make, _ = _kinds(8)[kind]
    rows, sel, sample, _ = dev_select(kind, dd, 8, largest)
    want = float(rows64[0, keep].sum() / 8)
    got = float(sample[0])
    print(f"\n{kind}: 3 admitted joints, topk 8: sample {got:.9e}, fp64 3-row sum / 8 {want:.9e} ({abs(got - want) / want / U:.2f}u, bar 10u)")
    assert sel[0].nonzero().flatten().tolist() == keep and abs(got - want) <= SAMPLE_BAR * want
    crit = make(None, None)
    x = dd["stu"].clone().requires_grad_(True)
    _call(crit, kind, x, dd).backward()
    assert int(crit.last_selection[0].sum()) == 3
    gone = [j for j in range(16) if j not in keep]
    assert bool((x.grad[0, gone] == 0).all()) and bool((x.grad[0, keep] != 0).any())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_16bit_inputs_return_gradients_in_the_input_dtype(dtype):
    d = make_inputs(3, 5, 16, 16, seed=3)
    d16 = _cast({k: (v.to(dtype) if k in ("stu", "tea", "label") else v) for k, v in d.items()}, None, "cuda")
    d32 = {k: (v.float() if v.dtype == dtype else v) for k, v in d16.items()}
    for kind, (_, _, _, make, _) in _kinds(3).items():
        out = []
        for dd in (d16, d32):
            crit = make(None, None)
            x = dd["stu"].clone().requires_grad_(True)
            loss = _call(crit, kind, x, dd)
            loss.backward()
            out.append((loss.detach(), x.grad, crit.last_selection))
        (l16, g16, s16), (l32, g32, s32) = out
        assert g16.dtype == dtype and l16.dtype == torch.float32, kind
        # the operands are taken as fp32 rows: the same numbers as the fp32 call on the widened inputs, the gradient rounded once
        assert torch.equal(g16, g32.to(dtype)) and torch.equal(l16, l32) and torch.equal(s16, s32), kind


def test_two_runs_agree_to_the_bit_and_a_sample_does_not_depend_on_its_batch():
    d = _cast(make_inputs(6, 16, 32, 32, seed=8), None, "cuda")
    for kind, (_, _, largest, make, _) in _kinds(5).items():
        runs = []
        for _ in range(2):
            crit = make(None, None)
            x = d["stu"].clone().requires_grad_(True)
            loss = _call(crit, kind, x, d)
            loss.backward()
            runs.append((loss.detach(), x.grad, crit.last_selection.clone()))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs)), kind
        _, sel, sample, _ = dev_select(kind, d, 5, largest)
        for i in range(6):
            one = {k: v[i:i + 1].contiguous() for k, v in d.items()}
            _, sel1, sample1, mean1 = dev_select(kind, one, 5, largest)
            assert torch.equal(sel1[0], sel[i]) and torch.equal(_bits(sample1[0]), _bits(sample[i])), (kind, i)
            assert torch.equal(_bits(mean1), _bits(sample1[0]))          # N = 1: the mean is the sample


@pytest.mark.parametrize("N,K", [(1100, 3), (33, 16), (16, 64), (1, 5)])
def test_the_select_launch_alone_on_given_rows_at_every_round_structure(N, K):
    """udapose_topk_select on rows handed to it: more samples than the ordered sum keeps in LDS (1024), one more sample than a round of
    the work-group's waves takes (2 x 16), exactly a wave per sample, one sample.  Rows are distinct fp32 numbers (a permutation of a grid),
    so the selection is decided by the inputs and the oracle's sums are exact sums of the same fp32 values."""
    lib, st = _lib()
    g = torch.Generator().manual_seed(N + K)
    rows = ((torch.randperm(N * K, generator=g).float() + 1.0) / 64.0).reshape(N, K)
    w = torch.where(torch.rand(N, K, generator=g) < 0.25, torch.zeros(N, K), 0.5 + torch.rand(N, K, generator=g))
    m = torch.rand(N, K, generator=g) < 0.6
    worst = 0.0
    for topk in _topks(K):
        for largest, fac in ((True, "w"), (False, "m"), (True, None)):
            zero = (w == 0) if fac == "w" else (~m if fac == "m" else None)
            r = rows if zero is None else torch.where(zero, torch.zeros_like(rows), rows)        # (a sweep leaves 0 where the factor is 0)
            l64, s64, sel64 = R64.topk_loss(r.double(), zero, topk, largest)
            rd, wd, md = r.reshape(-1).cuda(), w.reshape(-1).cuda(), m.to(torch.uint8).reshape(-1).cuda()
            sel = torch.empty(N * K, dtype=torch.uint8, device="cuda")
            sample, mean = torch.empty(N, device="cuda"), torch.empty((), device="cuda")
            rc = lib.udapose_topk_select(st, rd.data_ptr(), wd.data_ptr() if fac == "w" else None, md.data_ptr() if fac == "m" else None, N, K, topk,
                                         int(largest), sel.data_ptr(), sample.data_ptr(), mean.data_ptr())
            assert rc == 0
            assert torch.equal(sel.bool().reshape(N, K).cpu(), sel64), (topk, largest, fac)
            e_s, e_m = _rel(sample.cpu(), s64), _rel(mean.cpu(), l64)
            worst = max(worst, e_s, e_m)
            # here the rows ARE the fp32 inputs: a sample is one rounding of an exact sum, the mean one more
            assert e_s <= 1 * U and e_m <= 3 * U, (topk, largest, fac, e_s / U, e_m / U)
    print(f"\nselect alone, N {N} K {K}: worst sample / mean error {worst / U:.2f}u (bars 1u / 3u: one rounding per cast)")


def test_loss_forward_and_backward_replayed_from_a_graph_equal_eager_bit_for_bit():
    """Loss + backward alone, captured into a hipGraph and replayed on fresh inputs: the same kernels in the same order and no atomics, so
    the results - selections included - are the eager run's bits."""
    N, K, H, W = 4, 16, 32, 32
    static = _cast(make_inputs(N, K, H, W, seed=20), None, "cuda")
    x = static["stu"].clone().requires_grad_(True)
    scale = torch.tensor(3.0, device="cuda")
    crits = {kind: v[3](None, None) for kind, v in _kinds(6).items()}

    def run(xx, dd):
        outs = []
        for kind, crit in crits.items():
            loss = _call(crit, kind, xx, dd)
            (g,) = torch.autograd.grad(loss * scale, xx)
            outs += [loss, g, crit.last_selection]
        return outs

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(x, static)
        run(x, static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(x, static)
    seen = set()
    for i in range(3):
        fresh = _cast(make_inputs(N, K, H, W, seed=21 + i), None, "cuda")
        for k, v in fresh.items():
            static[k].copy_(v)
        with torch.no_grad():
            x.copy_(fresh["stu"])
        graph.replay()
        xe = fresh["stu"].clone().requires_grad_(True)
        eager = [t.clone() for t in run(xe, fresh)]
        torch.cuda.synchronize()
        assert len(captured) == len(eager) == 9
        for j, (c, e) in enumerate(zip(captured, eager)):
            assert torch.equal(_bits(c), _bits(e)), (i, j)
        assert all(torch.isfinite(e).all() for e in eager[0::3] + eager[1::3])
        seen.add(tuple(eager[2].flatten().tolist()))
    assert len(seen) == 3           # the replays selected different joints: the selection is computed, not baked


def test_refusals_return_their_codes_and_write_nothing():
    lib, st = _lib()
    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    N = 2
    rows = torch.rand(N * 65, device="cuda")
    sel = torch.full((N * 65,), 0xFF, dtype=torch.uint8, device="cuda")
    sample = torch.full((N,), float("nan"), device="cuda").view(torch.int32).fill_(-1).view(torch.float32)          # 0xFF bytes
    mean = sample.new_empty(1).view(torch.int32).fill_(-1).view(torch.float32)
    p = lambda t: t.data_ptr()
    cases = [("K = 65", (p(rows), None, None, N, 65, 8, 1, p(sel), p(sample), p(mean)), ERR_UNSUPPORTED),
             ("topk = 0", (p(rows), None, None, N, 16, 0, 1, p(sel), p(sample), p(mean)), ERR_ARG),
             ("topk = K + 1", (p(rows), None, None, N, 16, 17, 1, p(sel), p(sample), p(mean)), ERR_ARG),
             ("null rows", (None, None, None, N, 16, 8, 1, p(sel), p(sample), p(mean)), ERR_ARG),
             ("null sel", (p(rows), None, None, N, 16, 8, 1, None, p(sample), p(mean)), ERR_ARG),
             ("null sample", (p(rows), None, None, N, 16, 8, 1, p(sel), None, p(mean)), ERR_ARG),
             ("N = 0", (p(rows), None, None, 0, 16, 8, 1, p(sel), p(sample), p(mean)), ERR_ARG),
             ("N * K > 1 << 22", (p(rows), None, None, (1 << 22) // 16 + 1, 16, 8, 1, p(sel), p(sample), p(mean)), ERR_ARG)]
    for name, args, want in cases:
        assert lib.udapose_topk_select(st, *args) == want, name
    thr = torch.empty(16, device="cuda").view(torch.int32).fill_(-1).view(torch.float32)
    pool = torch.rand(8 * 16, device="cuda")
    for name, (n_pool, K, k) in (("k = 0", (8, 16, 0)), ("k > n_pool", (8, 16, 9)), ("K = 0", (8, 0, 1))):
        assert lib.udapose_joint_kth_mask(st, p(pool), n_pool, K, k, None, p(pool), 8, p(thr), p(sel)) == ERR_ARG, name
    assert lib.udapose_thr_mask(st, None, None, 16, p(thr), p(sel)) == ERR_ARG
    assert lib.udapose_topk_sqdiff_bwd(st, p(rows), p(rows), None, p(sel), None, 2, 16, 4, 17, 1, p(rows)) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((sel == 0xFF).all()) and bool((sample.view(torch.int32) == -1).all()) and bool((mean.view(torch.int32) == -1).all())
    assert bool((thr.view(torch.int32) == -1).all())
    # the Python classes refuse the same before any launch
    big = torch.zeros(1, 65, 2, 2, device="cuda")
    with pytest.raises(ValueError):
        _L().JointsOHKMMSELoss(8)(big, big)
    with pytest.raises(ValueError):
        _L().ConsTopKLoss(17)(big[:, :16], big[:, :16])
    with pytest.raises(NotImplementedError):
        _L().JointsOHKMMSELoss(2, reduction='none')(big[:, :16].clone().requires_grad_(True), big[:, :16]).sum().backward()


# ---------------------------------------------------------------------------------------------- confidence masks
def _confidences(n, K, seed):
    g = torch.Generator().manual_seed(seed)
    act = torch.rand(n, K, generator=g)
    act[: n // 2, 1] = act[0, 1]                         # a column of duplicated values
    act[n // 3, 2] = act[n - 1, 2]
    return act


@pytest.mark.parametrize("n_pool,n_local,K", [(32, 32, 16), (7, 7, 17), (256, 32, 16)])
def test_per_joint_masks_equal_kthvalue_per_column_exactly(n_pool, n_local, K):
    from uda_poseestimation_amd import utils
    pool = _confidences(n_pool, K, seed=n_pool)
    lo = 64 if n_pool > n_local else 0                    # rows 64..95 of the pool: a rank's share of a global batch
    local = pool[lo:lo + n_local].contiguous()
    g = torch.Generator().manual_seed(1)
    tm = (torch.rand(n_local, K, generator=g) < 0.7).float()
    recon = torch.zeros(n_local, K, 2, 2, device="cuda")             # (unused: the confidences are given)
    checked = 0
    for with_nan in (False, True):
        if with_nan:
            pool = pool.clone()
            pool[lo + 1, 3] = float("nan")
            local = pool[lo:lo + n_local].contiguous()
        for ratio in (0.5, 1.0 / n_pool, 1.0):
            k = int(ratio * n_pool)
            assert k == {0.5: n_pool // 2, 1.0: n_pool}.get(ratio, 1)
            for tea_mask in (None, tm):
                gathered = None if n_pool == n_local else pool.reshape(-1).cuda()
                mask, act, thr = utils.confidence_mask(recon, ratio, None if tea_mask is None else tea_mask.cuda(), gathered, local.cuda(), mode="per_joint")
                want_thr = torch.kthvalue(pool, k, dim=0).values
                want = ((local if tea_mask is None else tea_mask * local) > want_thr[None, :])
                assert mask.dtype == torch.bool and tuple(mask.shape) == (n_local, K) and tuple(thr.shape) == (K,)
                assert torch.equal(_bits(thr.cpu()), _bits(want_thr)), (ratio, with_nan)          # an element of the input: the same bits (NaN included)
                assert torch.equal(mask.cpu(), want), (ratio, with_nan)
                checked += 1
        if with_nan:
            assert torch.isnan(want_thr[3]) and not want[:, 3].any()           # k = n_pool: the NaN is the column's largest value
    print(f"\nper-joint masks, pool {n_pool} local {n_local} K {K}: {checked} cases equal torch.kthvalue and `>` exactly")


def test_threshold_masks_equal_the_comparison_exactly():
    from uda_poseestimation_amd import utils
    act = _confidences(32, 16, seed=2)
    act[3, 4] = float("nan")
    tm = (torch.rand(32, 16, generator=torch.Generator().manual_seed(3)) < 0.7).float()
    recon = torch.zeros(32, 16, 2, 2, device="cuda")
    for v in (0.5, float(act[5, 5]), 0.0, 1.5):
        thr32 = torch.tensor(v, dtype=torch.float32)
        for tea_mask in (None, tm):
            m_f, _, t_f = utils.confidence_mask(recon, 0.5, None if tea_mask is None else tea_mask.cuda(), None, act.cuda(), mode="threshold", threshold=v)
            dev_thr = thr32.cuda()
            m_t, _, t_t = utils.confidence_mask(recon, 0.5, None if tea_mask is None else tea_mask.cuda(), None, act.cuda(), mode="threshold",
                                                threshold=dev_thr)
            want = (act if tea_mask is None else tea_mask * act) > thr32
            assert torch.equal(m_f.cpu(), want) and torch.equal(m_t.cpu(), want), v
            assert t_f.dim() == 0 and t_t.dim() == 0 and float(t_f) == float(thr32) == float(t_t) and t_t.data_ptr() == dev_thr.data_ptr()
    # the heat-maps' own maxima when no confidences are given
    hm = torch.rand(4, 16, 8, 8, generator=torch.Generator().manual_seed(4))
    m, a, _ = utils.confidence_mask(hm.cuda(), 0.0, mode="threshold", threshold=0.97)
    assert torch.equal(a.cpu(), hm.amax((2, 3))) and torch.equal(m.cpu(), hm.amax((2, 3)) > torch.tensor(0.97))


def test_global_mode_is_the_call_without_the_new_keywords():
    from uda_poseestimation_amd import utils
    hm = torch.rand(8, 16, 8, 8, generator=torch.Generator().manual_seed(5)).cuda()
    tm = (torch.rand(8, 16, generator=torch.Generator().manual_seed(6)) < 0.7).float().cuda()
    for ratio in (0.5, 0.25):
        a = utils.confidence_mask(hm, ratio, tm)
        b = utils.confidence_mask(hm, ratio, tm, mode="global")
        c = utils.confidence_mask(hm, ratio, tm, None, None, mode="global", threshold=0.3)            # (a threshold is not read in this mode)
        for x, y, z in zip(a, b, c):
            assert torch.equal(_bits(x), _bits(y)) and torch.equal(_bits(x), _bits(z))
        assert a[2].dim() == 0
        want_thr = torch.kthvalue(hm.amax((2, 3)).reshape(-1).cpu(), int(ratio * 128)).values
        assert float(a[2]) == float(want_thr)


# ---------------------------------------------------------------------------------------------- the step (tiny network)
N_, K_, S = 4, 16, 128


def _batches(seeds):
    from uda_poseestimation_amd import synthetic
    out = []
    for s in seeds:
        b = synthetic.mean_teacher_batch(N_, num_keypoints=K_, image_size=S, heatmap_size=S // 4, seed=s)
        g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
        out.append((g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"]))
    return out


def _trainer(nets, mode="per_joint", new_criteria=True, **kw):
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    L = _L()
    crit = dict(criterion=L.JointsOHKMMSELoss(8), con_criterion=L.ConsTopKLoss(4, largest=False)) if new_criteria else {}
    tr = MeanTeacherTrainer(*nets, lr=1e-4, image_size=S, heatmap_size=S // 4, precision="bf16", **crit, **kw)
    if mode is not None:
        tr.mask_mode = mode
    return tr


def _nets(base, seed):
    from test_gpu_steps import _tiny
    s_, t_ = _tiny(K_, seed=seed), _tiny(K_, seed=seed)
    s_.load_state_dict(base.state_dict())
    return s_.cuda(), t_.cuda()


def test_eager_step_with_the_new_criteria_and_per_joint_masks_equals_its_parts():
    from test_gpu_steps import _tiny
    from uda_poseestimation_amd import utils
    bt = _batches((31,))[0]
    tr = _trainer(_nets(_tiny(K_, seed=8), 8))
    out = tr.train_step(*bt)
    torch.cuda.synchronize()
    mask, act, thr = utils.confidence_mask(out["y_t_tea_recon"], tr.mask_ratio, mode="per_joint")
    assert torch.equal(out["tea_mask"], mask) and tuple(out["mask_thr"].shape) == (K_,) and torch.equal(_bits(out["mask_thr"]), _bits(thr))
    assert torch.equal(thr.cpu(), torch.kthvalue(act.cpu(), int(tr.mask_ratio * N_), dim=0).values)
    want = float(out["loss_s"]) + tr.lambda_c * float(out["loss_c"])
    assert abs(float(out["loss_all"]) - want) <= 1e-5 * abs(want)
    again = _L().JointsOHKMMSELoss(8)(out["y_s"], bt[1], bt[2])
    assert torch.equal(_bits(out["loss_s"].float()), _bits(again.float()))
    sel_s, sel_c = tr.criterion.last_selection, tr.con_criterion.last_selection
    print(f"\neager step: loss_s {float(out['loss_s']):.6e} loss_c {float(out['loss_c']):.6e}; joints per sample, supervised {sel_s.sum(1).tolist()} "
          f"consistency {sel_c.sum(1).tolist()}; mask {out['tea_mask'].sum(0).tolist()} per joint")
    assert bool((sel_s.sum(1) <= 8).all()) and bool((sel_c.sum(1) <= 4).all()) and not bool((sel_c & ~out["tea_mask"]).any())
    assert float(out["loss_s"]) > 0 and float(out["loss_c"]) > 0 and bool(out["tea_mask"].any())


def test_captured_steps_with_joint_selection_equal_eager_steps():
    """test_captured_steps_with_the_new_criteria_equal_eager_steps (tests/test_gpu_softmax_losses.py) with JointsOHKMMSELoss(8),
    ConsTopKLoss(4, largest=False) and per-joint masks: its assertions and bars."""
    from test_gpu_steps import _tiny
    from uda_poseestimation_amd.engine import GraphedTrainStep
    batches = _batches((31, 32, 33, 34))
    base = _tiny(K_, seed=8)
    for split in (False, True):
        nets = [_nets(base, 8), _nets(base, 8)]
        tr_g, tr_e = _trainer(nets[0]), _trainer(nets[1])
        p0 = [p.detach().clone() for p in nets[0][0].parameters()]
        gs = GraphedTrainStep(tr_g, *batches[0], warmup=1, split=split)       # the warm-up step IS step 1 (on batch 0)
        tr_e.train_step(*batches[0])
        for bt in batches[1:]:
            og = gs.step(*bt)
            oe = tr_e.train_step(*bt)
            print(f"split={split}: loss_all {float(og['loss_all']):.6e} / {float(oe['loss_all']):.6e}  loss_s {float(og['loss_s']):.6e}  "
                  f"loss_c {float(og['loss_c']):.4e} / {float(oe['loss_c']):.4e}")
            assert abs(float(og["loss_all"]) - float(oe["loss_all"])) <= 2e-3 * abs(float(oe["loss_all"]))
            assert abs(float(og["loss_c"]) - float(oe["loss_c"])) <= 5e-3 * abs(float(oe["loss_c"])) + 1e-7
            want = float(oe["loss_s"]) + float(oe["loss_c"])
            assert abs(float(oe["loss_all"]) - want) <= 1e-5 * abs(want)
            assert tuple(og["mask_thr"].shape) == (K_,)
        sg, se, tg, te = nets[0][0], nets[1][0], nets[0][1], nets[1][1]
        num = den = 0.0
        for pg, pe, q0 in zip(sg.parameters(), se.parameters(), p0):
            num += float(((pg.detach() - pe.detach()) ** 2).sum())
            den += float(((pe.detach() - q0) ** 2).sum())
        rel = (num / max(den, 1e-30)) ** 0.5
        print(f"split={split}: ||student(graph) - student(eager)|| / ||student(eager) - start|| = {rel:.3e} after {len(batches)} steps")
        assert den > 0 and rel < 0.2
        tn = sum(float(((a.detach() - c.detach()) ** 2).sum()) for a, c in zip(tg.parameters(), te.parameters()))
        td = sum(float(((c.detach() - q0) ** 2).sum()) for c, q0 in zip(te.parameters(), p0))
        assert (tn / max(td, 1e-30)) ** 0.5 < 0.1
        gs.release()


def test_two_captured_steps_with_joint_selection_agree_to_the_bit_after_five_steps():
    from test_gpu_steps import _tiny
    from uda_poseestimation_amd.engine import GraphedTrainStep
    batches = _batches(range(40, 45))
    base = _tiny(K_, seed=9)
    runs = []
    for _ in range(2):
        s_, t_ = _nets(base, 9)
        gs = GraphedTrainStep(_trainer((s_, t_)), *batches[0], warmup=1)
        losses = []
        for bt in batches[1:]:
            o = gs.step(*bt)
            losses.append(torch.stack([o[k].detach().float().reshape(()) for k in ("loss_all", "loss_s", "loss_c")]).clone())
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), [p.detach().cpu().clone() for p in s_.parameters()], [p.detach().cpu().clone() for p in t_.parameters()]))
        gs.release()
    (la, sa, ta), (lb, sb, tb) = runs
    print("\nlosses of the fifth step [all, s, c]:", la[-1].tolist())
    assert torch.isfinite(la).all() and torch.equal(_bits(la), _bits(lb))
    assert all(torch.equal(a, b) for a, b in zip(sa, sb)) and all(torch.equal(a, b) for a, b in zip(ta, tb))
    assert any(not torch.equal(a, p.detach()) for a, p in zip(sa, base.parameters()))          # it trained


def test_a_captured_step_follows_a_threshold_ramp_and_refuses_baked_changes():
    from test_gpu_steps import _tiny
    from uda_poseestimation_amd import utils
    from uda_poseestimation_amd.engine import GraphedTrainStep
    batches = _batches((51, 52, 53))
    tr = _trainer(_nets(_tiny(K_, seed=8), 8), mode="threshold")
    assert tr.mask_threshold == 0.5
    gs = GraphedTrainStep(tr, *batches[0], warmup=1)
    graph = gs.g_fb
    counts = []
    for bt, frac in zip(batches, (None, 0.3, 0.7)):
        if frac is not None:
            # a threshold inside the confidences of the last step, so that the mask is neither empty nor full
            tr.mask_threshold = float(torch.quantile(utils.heatmap_activations(gs.out["y_t_tea_recon"]).reshape(-1), frac))
        o = gs.step(*bt)
        torch.cuda.synchronize()
        thr32 = torch.tensor(tr.mask_threshold, dtype=torch.float32)
        act = utils.heatmap_activations(o["y_t_tea_recon"]).cpu()
        assert o["mask_thr"].dim() == 0 and float(o["mask_thr"]) == float(thr32)
        assert torch.equal(o["tea_mask"].cpu(), act > thr32)
        counts.append((float(thr32), int(o["tea_mask"].sum())))
    print(f"\nthreshold ramp through one captured graph: (threshold, joints above it of {N_ * K_}) = {counts}")
    assert gs.g_fb is graph and len({c[0] for c in counts}) == 3 and 0 < counts[1][1] < N_ * K_
    tr.mask_mode = "global"
    with pytest.raises(RuntimeError, match="mask_mode"):
        gs.step(*batches[0])
    tr.mask_mode = "threshold"
    tr.criterion.topk = 4
    with pytest.raises(RuntimeError, match=r"criterion\.topk"):
        gs.step(*batches[0])
    tr.criterion.topk = 8
    tr.con_criterion.largest = True
    with pytest.raises(RuntimeError, match=r"con_criterion\.largest"):
        gs.step(*batches[0])
    tr.con_criterion.largest = False
    gs.step(*batches[0])
    gs.release()


def test_the_default_step_is_untouched_by_the_new_attributes():
    from test_gpu_steps import _tiny
    batches = _batches((61, 62))
    base = _tiny(K_, seed=8)
    runs = []
    for touch in (False, True):
        s_, t_ = _nets(base, 8)
        tr = _trainer((s_, t_), mode=None, new_criteria=False)
        if touch:
            tr.mask_mode, tr.mask_threshold = "global", 0.25
        outs = [tr.train_step(*bt) for bt in batches]
        torch.cuda.synchronize()
        assert all("mask_thr" not in o for o in outs) and tr._mask_thr is None
        runs.append(([torch.stack([o[k].float() for k in ("loss_all", "loss_s", "loss_c")]).cpu() for o in outs],
                     [p.detach().cpu().clone() for p in s_.parameters()], outs[-1]["tea_mask"].cpu()))
    (la, pa, ma), (lb, pb, mb) = runs
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(la, lb)) and all(torch.equal(a, b) for a, b in zip(pa, pb)) and torch.equal(ma, mb)
