"""The student's gradient of one mean-teacher step is produced by several backward schedules: one stream or two
(MeanTeacherTrainer.concurrent), both passes' grouped weight gradients in one pair launch or not (merge_wgrad,
udapose_net_wgrad_pair), the backward cut after layer3 (overlap_allreduce), grouped or per-layer weight gradients, split
reductions as ordered partial tiles or fp32 atomics (policy wgrad_group / wgrad_det), bf16 / fp16 / 'strict', eager or captured.
They all compute the same function.  Here every schedule's gradient is checked against the plainest schedule's two passes taken
apart: g = g_S (source pass alone) + g_T (target pass alone), per tensor, to summation-order noise."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LAYERS, K, N, S = [2, 1, 2, 1], 16, 4, 128
PLAIN = {"wgrad_group": 0}


def _net(sd=None):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(5)
    m = pr._pose_resnet("t", K, pr.Bottleneck_default, LAYERS, False, False)
    if sd is not None:
        m.load_state_dict(sd)
    return m.cuda()


@pytest.fixture(scope="module")
def setup():
    from uda_poseestimation_amd import synthetic
    sd = {k: v.clone() for k, v in _net().cpu().state_dict().items()}
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=21)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    return sd, b, g


def _trainer(sd, prec, lam, concurrent=True, merge=True, overlap=False, policy=None, loss_scale=65536.0, lr=1e-4):
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    stu, tea = _net(sd), _net(sd)
    if policy:
        stu.policy = dict(policy)
    tr = MeanTeacherTrainer(stu, tea, lr=lr, image_size=S, heatmap_size=S // 4, lambda_c=lam, precision=prec, loss_scale_init=loss_scale)
    tr.concurrent, tr.merge_wgrad, tr.overlap_allreduce = concurrent, merge, overlap
    return tr


def _grad(sd, g, prec, lam, zero_weight_s=False, **kw):
    """One eager forward + backward with no optimizer step: (flat gradient, consistency mask, loss scale, student)."""
    from uda_poseestimation_amd import warp
    tr = _trainer(sd, prec, lam, **kw)
    w = torch.zeros_like(g["weight_s"]) if zero_weight_s else g["weight_s"]
    th_s = warp.recon_thetas(g["aug_param_stu"], N, tr.ratio, "cuda")
    th_t = [warp.recon_thetas(g["aug_param_tea"], N, tr.ratio, "cuda")]
    st = tr._forward_part(g["x_s"], g["label_s"], w, g["x_t_stu"], [g["x_t_tea"]], th_s, th_t)
    res = tr._loss_backward_part(st, None)
    tr._sync_grads()
    tr.student.finish_grads()
    torch.cuda.synchronize()
    sc = tr.stu_optimizer.loss_scale()
    return tr.student._flat_grad.clone(), res["tea_mask"].clone(), (1.0 if sc is None else float(sc)), tr.student


def _views(flat, stu):
    out, off = {}, 0
    for n_, p in stu.named_parameters():
        out[n_] = flat[off:off + p.numel()].as_strided(p.shape, p.stride())      # (the parameters' physical layout: channels-last)
        off += p.numel()
    assert off == flat.numel()
    return out


def _close(a, b):
    """The summation-order bar of tests/test_gpu_net.py::test_grouped_weight_gradients_equal_per_layer_launches, per tensor."""
    return float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()) + 1e-7


def _unsplit(n_):
    """Conv weights of layer3 / layer4: at 128x128 their pixel reductions fit one work-group (no split, plain stores at beta 0)."""
    return (".layer3." in n_ or ".layer4." in n_) and ("conv" in n_ or "downsample.0" in n_) and n_.endswith("weight")


def _norm(v, names):
    return math.sqrt(sum(float((v[n_].double() ** 2).sum()) for n_ in names))


_REF = {}


def _decomposition(setup, prec):
    """g_S (lambda_c = 0) and g_T (weight_s = 0) of the plainest schedule, and the lambda_c that makes the two passes comparable on the
    unsplit layers (a power of two: the ratio of their norms at lambda_c = 1, rounded)."""
    if prec in _REF:
        return _REF[prec]
    sd, b, g = setup
    if "lam" not in _REF:
        gs, _, _, stu = _grad(sd, g, "bf16", 0.0, concurrent=False, merge=False, policy=PLAIN)
        gt, _, _, _ = _grad(sd, g, "bf16", 1.0, zero_weight_s=True, concurrent=False, merge=False, policy=PLAIN)
        names = [n_ for n_, _ in stu.named_parameters() if _unsplit(n_)]
        r = _norm(_views(gs, stu), names) / _norm(_views(gt, stu), names)
        _REF["lam"] = 2.0 ** round(math.log2(r))
    lam = _REF["lam"]
    ls = 2.0 ** (16 - max(0, round(math.log2(lam))))       # (fp16 backward: keep lambda_c x loss scale at 2^16)
    gs, m_s, _, stu = _grad(sd, g, prec, 0.0, concurrent=False, merge=False, policy=PLAIN, loss_scale=ls)
    gt, m_t, _, _ = _grad(sd, g, prec, lam, zero_weight_s=True, concurrent=False, merge=False, policy=PLAIN, loss_scale=ls)
    assert torch.equal(m_s, m_t)                 # the teacher's mask depends on neither the student's weights nor weight_s
    assert torch.isfinite(gs).all() and torch.isfinite(gt).all()
    _REF[prec] = (gs, gt, m_s, lam, ls, stu)
    return _REF[prec]


def _check_against_sum(full, gs, gt, stu, tag):
    vf, vs, vt = _views(full, stu), _views(gs, stu), _views(gt, stu)
    bad = [n_ for n_ in vf if not _close(vf[n_], vs[n_] + vt[n_])]
    assert not bad, f"{tag}: {len(bad)} tensors differ from g_S + g_T, first {bad[0]}: " \
                    f"max|d| {float((vf[bad[0]] - vs[bad[0]] - vt[bad[0]]).abs().max()):.3e}, max|ref| {float((vs[bad[0]] + vt[bad[0]]).abs().max()):.3e}"


@pytest.mark.parametrize("prec", ["bf16", "fp16", "strict"])
def test_both_passes_carry_weight_on_the_unsplit_layers(setup, prec):
    """A1: with the chosen lambda_c, dropping either pass's share of the gradient moves the unsplit layers' gradient by at least 5 %
    (so that every schedule check below would fail by a wide margin if one pass were lost); the plainest schedule's full gradient equals
    g_S + g_T.  Measured: lambda_c = 0.5; |g_S| / |g_S + g_T| = 0.675 and |g_T| / |g_S + g_T| = 0.738 in bf16, 0.678 / 0.734 in fp16 and
    'strict', over the 11 unsplit conv weights."""
    sd, b, g = setup
    gs, gt, mask, lam, ls, stu = _decomposition(setup, prec)
    vs, vt = _views(gs, stu), _views(gt, stu)
    names = [n_ for n_ in vs if _unsplit(n_)]
    assert len(names) >= 10
    tot = {n_: vs[n_] + vt[n_] for n_ in names}
    ns, nt, nn = _norm(vs, names), _norm(vt, names), _norm(tot, names)
    print(f"{prec}: lambda_c {lam:g}, loss scale {ls:g}: |g_S| / |g_S + g_T| = {ns / nn:.3f}, |g_T| / |g_S + g_T| = {nt / nn:.3f} "
          f"over {len(names)} unsplit conv weights")
    assert ns >= 0.05 * nn and nt >= 0.05 * nn
    full, m, _, _ = _grad(sd, g, prec, lam, concurrent=False, merge=False, policy=PLAIN, loss_scale=ls)
    assert torch.equal(m, mask)
    _check_against_sum(full, gs, gt, stu, f"{prec} plain")


_BF16 = [(c, m, o, pol) for c in (True, False) for m in (True, False) for o in (False, True)
         for pol in ("default", "atomic", "per_layer", "short_split")]
_POL = {"default": None, "atomic": {"wgrad_det": 0}, "per_layer": {"wgrad_group": 0}, "short_split": {"wgrad_stages": 8}}


@pytest.mark.parametrize("concurrent,merge,overlap,pol", _BF16,
                         ids=[f"{'two' if c else 'one'}stream-{'merge' if m else 'nomerge'}-{'cut' if o else 'whole'}-{p}" for c, m, o, p in _BF16])
def test_bf16_schedule_equals_sum_of_passes(setup, concurrent, merge, overlap, pol):
    """A2, bf16: every schedule of the product one / two streams x pair launch or not x whole / cut backward x (deterministic grouped,
    atomic grouped, per-layer, and deterministic grouped with 8-stage splits - at 128x128 the production split length splits no layer,
    8 stages split layer1, layer2, the last deconvolution, the head and the stem into ordered partial tiles) weight gradients equals
    g_S + g_T per tensor.  (One stream with the pair launch is the configuration of
    bench.py's roofline sample: before the fix, its two passes shared one gradient buffer in one grid and the second pass's adds could
    land before the first pass's stores.)"""
    sd, b, g = setup
    gs, gt, mask, lam, ls, stu = _decomposition(setup, "bf16")
    full, m, _, _ = _grad(sd, g, "bf16", lam, concurrent=concurrent, merge=merge, overlap=overlap, policy=_POL[pol])
    assert torch.equal(m, mask)
    _check_against_sum(full, gs, gt, stu, f"bf16 concurrent={concurrent} merge={merge} overlap={overlap} {pol}")


@pytest.mark.parametrize("prec", ["fp16", "strict"])
@pytest.mark.parametrize("concurrent,merge", [(True, True), (True, False), (False, True), (False, False)])
def test_fp16_and_strict_schedules_equal_sum_of_passes(setup, prec, concurrent, merge):
    """A2, fp16 and 'strict' (the fp16 backward under the loss scale): the default policy with one / two streams x pair launch or not."""
    sd, b, g = setup
    gs, gt, mask, lam, ls, stu = _decomposition(setup, prec)
    full, m, _, _ = _grad(sd, g, prec, lam, concurrent=concurrent, merge=merge, loss_scale=ls)
    assert torch.equal(m, mask)
    _check_against_sum(full, gs, gt, stu, f"{prec} concurrent={concurrent} merge={merge}")


@pytest.mark.parametrize("pol", ["default", "short_split"])
def test_deterministic_schedules_give_the_same_bits(setup, pol):
    """A2: with the deterministic grouped weight gradients (wgrad_det = 1, the default) two runs of one schedule give the same bits; so do
    the four arrangements of one / two streams x pair launch or not.  Every per-pass tensor is computed by the same kernels in the same
    order whatever the streams; the passes meet in exactly one fp32 addition per element (g_A + g_B: the second pass's beta = 1 epilogue or
    split sum, the pair launch's second half, or the axpy of the second per-pass buffer), and fp32 addition commutes.  The whole / cut
    backward is not part of this claim: the cut regroups the weight-gradient launches (other work lists), whose split lengths may differ."""
    sd, b, g = setup
    lam = _decomposition(setup, "bf16")[3]
    first, _, _, _ = _grad(sd, g, "bf16", lam, policy=_POL[pol])
    again, _, _, _ = _grad(sd, g, "bf16", lam, policy=_POL[pol])
    assert torch.equal(first, again), "two runs of the deterministic default schedule differ"
    for c, m in ((True, False), (False, True), (False, False)):
        other, _, _, _ = _grad(sd, g, "bf16", lam, concurrent=c, merge=m, policy=_POL[pol])
        d = float((other - first).abs().max())
        assert torch.equal(other, first), f"concurrent={c} merge={m} differs from the default arrangement by {d:.3e}"


def _opt_state(tr):
    opt = tr.stu_optimizer
    out = []
    for p in tr.student.parameters():
        st = opt.state.get(p, {})
        out += [st[k].detach().clone() for k in ("exp_avg", "exp_avg_sq") if k in st]
    return out


def _rewind(tr, sd):
    """Model and optimizer back to the start state IN PLACE (the captured launches hold raw pointers)."""
    import copy
    tr.student.load_state_dict(sd)
    tr.teacher.load_state_dict(sd)
    opt = tr.stu_optimizer
    osd = copy.deepcopy(opt.state_dict())
    for st in osd["state"].values():
        for v in st.values():
            if torch.is_tensor(v):
                v.zero_()
    for gp in osd["param_groups"]:
        gp["step"] = 0
        if opt._scaler is not None:
            gp["loss_scale"], gp["growth_tracker"] = float(opt._scaler["init_scale"]), 0
    opt.load_state_dict(osd)
    torch.cuda.synchronize()


@pytest.mark.parametrize("concurrent", [True, False], ids=["twostream", "onestream"])
def test_captured_step_equals_eager_twin_to_the_bit(setup, concurrent):
    """A2, captured: GraphedTrainStep (one graph, the fused optimizer tail reading both per-pass buffers) against an eager twin that
    runs the same two steps from the same state, precision 'strict' (where tests/test_gpu_strict.py states captured == eager to the
    bit): parameters, Adam's two moments and the teacher agree to the bit, on one stream and on two."""
    from uda_poseestimation_amd.engine import GraphedTrainStep
    sd, b, g = setup
    lam, ls = _decomposition(setup, "strict")[3:5]
    args = (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])
    tr = _trainer(sd, "strict", lam, concurrent=concurrent, loss_scale=ls)
    gs = GraphedTrainStep(tr, *args, warmup=1)
    _rewind(tr, sd)
    for _ in range(2):
        gs.step(*args)
    torch.cuda.synchronize()
    tw = _trainer(sd, "strict", lam, concurrent=concurrent, loss_scale=ls)
    for _ in range(2):
        tw.train_step(*args)
    torch.cuda.synchronize()
    for (n_, pg), pe in zip(tr.student.named_parameters(), tw.student.parameters()):
        assert torch.equal(pg.detach(), pe.detach()), f"captured and eager {n_} differ"
    mg, me = _opt_state(tr), _opt_state(tw)
    assert len(mg) == len(me) > 0
    for a, e in zip(mg, me):
        assert torch.equal(a, e), "captured and eager Adam moments differ"
    for pg, pe in zip(tr.teacher.parameters(), tw.teacher.parameters()):
        assert torch.equal(pg.detach(), pe.detach())
    gs.release()


def test_strict_gradient_against_the_fp64_oracle(setup):
    """A3: the default schedule at precision 'strict' against oracle.step_ref.train_step_full_ref in fp64 (SGD at lr 0, so that .grad
    survives the step), on the same weights and inputs: the consistency mask element for element, and per tensor the cosine and the
    relative L2 distance of the gradient (loss scale divided out).  Measured over the 80 tensors with a gradient (lambda_c 0.5, loss
    scale 65536): worst cosine 0.99940 and worst relative L2 3.5e-2 (layer1's first block and its BatchNorms; the fp16 backward, not the
    fp32-grade forward, sets them).  Bars: cosine > 0.998 and relative L2 < 7e-2, twice the measured distance (tests/test_gpu_fp16.py's
    fp16 bar is cosine > 0.95)."""
    from oracle.pose_resnet_ref import PoseResNetRef
    from oracle.step_ref import train_step_full_ref
    sd, b, g = setup
    lam, ls0 = _decomposition(setup, "strict")[3:5]
    full, mask, ls, stu = _grad(sd, g, "strict", lam, loss_scale=ls0)
    torch.manual_seed(0)
    ref_s, ref_t = PoseResNetRef(LAYERS, K), PoseResNetRef(LAYERS, K)
    ref_s.load_state_dict(sd)
    ref_t.load_state_dict(sd)
    ref_s, ref_t = ref_s.double(), ref_t.double()
    opt = torch.optim.SGD(ref_s.parameters(), lr=0.0)
    d = lambda t: t.double()
    ref = train_step_full_ref(ref_s, ref_t, opt, d(b["x_s"]), d(b["label_s"]), d(b["weight_s"]), d(b["x_t_stu"]), d(b["x_t_tea"]),
                              b["aug_param_stu"], b["aug_param_tea"], lambda_c=lam, ratio=4.0)
    rm = ref["tea_mask"]
    assert torch.equal(mask.cpu().reshape(rm.shape).bool(), rm.bool()), "consistency mask differs from the oracle's"
    v = _views(full, stu)
    worst_cos, worst_rel, rows = 1.0, 0.0, []
    for n_, p in ref_s.named_parameters():
        if p.grad is None:
            continue
        a = v[n_].double().cpu() / ls
        r = p.grad.detach()
        cos = float((a * r).sum() / (a.norm() * r.norm()))
        rel = float((a - r).norm() / r.norm())
        rows.append((n_, cos, rel))
        worst_cos, worst_rel = min(worst_cos, cos), max(worst_rel, rel)
    rows.sort(key=lambda t: t[2])
    print(f"strict vs fp64 oracle over {len(rows)} tensors (lambda_c {lam:g}, loss scale {ls:g}): worst cosine {worst_cos:.6f}, "
          f"worst rel-L2 {worst_rel:.4e}; largest rel-L2: " + ", ".join(f"{n_} {c:.6f}/{r:.3e}" for n_, c, r in rows[-4:]))
    assert len(rows) >= 60
    assert worst_cos > 0.998 and worst_rel < 7e-2, (worst_cos, worst_rel)
