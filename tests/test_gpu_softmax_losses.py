"""The soft-max heat-map losses on the MI355X (csrc/softmax_loss.hip through lib.models.loss): JointsKLLoss, EntLoss, ConsSoftmaxLoss,
ConsKLLoss - values against what the reference's own classes returned, gradients against fp64 autograd of the plain-torch restatement
(tests/helpers/softmax_losses_fp64.py, pinned to the reference by tests/test_softmax_losses_cpu.py), capture and replay, and the
mean-teacher step with the new criteria.

THE BOUND of the value / gradient comparisons is measured, not chosen: the same restatement is evaluated in fp32 torch on the CPU (the
reference's arithmetic), its worst error against fp64 over the shapes of a test is taken per loss (value: relative; gradient: absolute,
divided by max|gradient|), and the device is allowed 4x that figure.  The device sums in double, so it should be better; the margin
absorbs an `expf` that differs by an ulp between libm and the device library.  Every test prints both figures.
"""
import os

import numpy as np
import pytest
import torch

from helpers import softmax_losses_fp64 as R64

pytestmark = pytest.mark.gpu
MARGIN = 4.0


def _losses():
    from uda_poseestimation_amd.lib.models import loss as L
    return L


def make_inputs(B, K, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    scale = 0.3 + 5.7 * torch.rand(B, K, 1, 1, generator=g)
    stu = torch.randn(B, K, H, W, generator=g) * scale
    tea = stu + 0.5 * torch.randn(B, K, H, W, generator=g) * scale
    label = torch.exp(-12 * torch.rand(B, K, H, W, generator=g))
    label[label < 0.02] = 0.0
    weight = (torch.rand(B, K, 1, generator=g) > 0.3).float()
    weight[0, 0] = 1.0
    tea_mask = torch.rand(B, K, generator=g) > 0.4
    tea_mask[0, 0] = True
    valid = torch.rand(B, H, W, generator=g) > 0.35
    return {"stu": stu, "tea": tea, "label": label, "weight": weight, "tea_mask": tea_mask, "valid": valid}


def entropy_threshold(stu):
    """A threshold between two rows' entropies (fp64), about half of the rows below it: no tie for fp32 rounding to break."""
    B, K = stu.shape[:2]
    lp = torch.log_softmax(stu.double().reshape(B * K, -1), -1)
    ent = (-(lp.exp() * lp).sum(-1) / np.log(lp.shape[-1])).sort().values
    n = ent.numel()
    return float((ent[n // 2 - 1] + ent[n // 2]) / 2) if n > 1 else 2.0 * float(ent[0])


# name -> (device loss, restatement); both take (x, inputs) with `inputs` on x's device / in x's dtype
def kinds(thr):
    L = _losses()
    return {
        "kl_w": (lambda x, d: L.JointsKLLoss(epsilon=1e-6)(x, d["label"], d["weight"]), lambda x, d: R64.joints_kl(x, d["label"], d["weight"], "mean", 1e-6)),
        "kl": (lambda x, d: L.JointsKLLoss(epsilon=1e-6)(x, d["label"]), lambda x, d: R64.joints_kl(x, d["label"], None, "mean", 1e-6)),
        "ent": (lambda x, d: L.EntLoss()(x), lambda x, d: R64.entropy(x)),
        "ent_thr": (lambda x, d: L.EntLoss()(x, thr), lambda x, d: R64.entropy(x, thr)),
        "csm": (lambda x, d: L.ConsSoftmaxLoss()(x, d["tea"]), lambda x, d: R64.cons_softmax(x, d["tea"])),
        "csm_mask": (lambda x, d: L.ConsSoftmaxLoss()(x, d["tea"], tea_mask=d["tea_mask"]), lambda x, d: R64.cons_softmax(x, d["tea"], tea_mask=d["tea_mask"])),
        "csm_valid": (lambda x, d: L.ConsSoftmaxLoss()(x, d["tea"], valid_mask=d["valid"]), lambda x, d: R64.cons_softmax(x, d["tea"], valid_mask=d["valid"])),
        "csm_both": (lambda x, d: L.ConsSoftmaxLoss()(x, d["tea"], d["valid"], d["tea_mask"]), lambda x, d: R64.cons_softmax(x, d["tea"], d["valid"], d["tea_mask"])),
        "ckl_lt": (lambda x, d: L.ConsKLLoss(log_target=True)(x, d["tea"]), lambda x, d: R64.cons_kl(x, d["tea"], log_target=True)),
        "ckl_lt_both": (lambda x, d: L.ConsKLLoss(log_target=True)(x, d["tea"], d["valid"], d["tea_mask"]),
                        lambda x, d: R64.cons_kl(x, d["tea"], d["valid"], d["tea_mask"], log_target=True)),
        # the reference's arithmetic as written: the value is NaN, the gradient (d/d log p = -t) is finite
        "ckl_ref_both": (lambda x, d: L.ConsKLLoss()(x, d["tea"], d["valid"], d["tea_mask"]), lambda x, d: R64.cons_kl(x, d["tea"], d["valid"], d["tea_mask"])),
    }


def _cast(d, dtype=None, device=None):
    out = {}
    for k, v in d.items():
        if v.dtype.is_floating_point and dtype is not None:
            v = v.to(dtype)
        out[k] = v.to(device) if device is not None else v
    return out


def _value_and_grad(fn, x, d):
    x = x.clone().requires_grad_(True)
    loss = fn(x, d)
    loss.backward()
    return loss.detach(), x.grad.detach()


def measure(d):
    """{kind: (device value error, fp32 value error, device gradient error, fp32 gradient error)} against fp64 on one set of inputs."""
    thr = entropy_threshold(d["stu"])
    d64, d32, dd = _cast(d, torch.float64), d, _cast(d, None, "cuda")
    out = {}
    for name, (dev_fn, ref_fn) in kinds(thr).items():
        l64, g64 = _value_and_grad(ref_fn, d64["stu"], d64)
        l32, g32 = _value_and_grad(ref_fn, d32["stu"], d32)
        ld, gd = _value_and_grad(dev_fn, dd["stu"], dd)
        ld, gd = ld.cpu(), gd.cpu()
        assert ld.dtype == torch.float32 and gd.dtype == torch.float32 and gd.shape == d["stu"].shape
        assert torch.isfinite(g64).all() and torch.isfinite(gd).all(), name
        assert bool(torch.isnan(ld)) == bool(torch.isnan(l64)), (name, float(ld), float(l64))
        if torch.isnan(l64):
            assert name == "ckl_ref_both"
            ev = (0.0, 0.0)
        else:
            ev = (abs(float(ld) - float(l64)) / abs(float(l64)), abs(float(l32) - float(l64)) / abs(float(l64)))
        gm = float(g64.abs().max())
        assert gm > 0, name
        out[name] = ev + (float((gd.double() - g64).abs().max()) / gm, float((g32.double() - g64).abs().max()) / gm)
    return out


def check_against_fp32_arithmetic(shapes, title):
    """Per loss: the device's error on every shape <= MARGIN x the fp32 restatement's worst error over the shapes."""
    res = {s: measure(make_inputs(*s, seed=7 + i)) for i, s in enumerate(shapes)}
    names = list(next(iter(res.values())))
    bad = []
    print(f"\n{title}: error against fp64 autograd, device | fp32 torch on the CPU (value: relative; gradient: max abs / max|grad|)")
    for n in names:
        v32 = max(r[n][1] for r in res.values())
        g32 = max(r[n][3] for r in res.values())
        vd = max(r[n][0] for r in res.values())
        gd = max(r[n][2] for r in res.values())
        print(f"  {n:13s} value {vd:.2e} | {v32:.2e}   gradient {gd:.2e} | {g32:.2e}")
        for s, r in res.items():
            if r[n][0] > MARGIN * v32:
                bad.append((n, s, "value", r[n][0], v32))
            if r[n][2] > MARGIN * g32:
                bad.append((n, s, "gradient", r[n][2], g32))
    assert not bad, bad


def test_forward_of_every_class_matches_what_the_reference_returned(golden_dir):
    """Every class / reduction / mask combination on the golden inputs.  The goldens are the reference's fp32 results: their own worst
    relative error against the fp64 restatement, per loss family, is the yardstick, and the device is held to 4x that against fp64.
    NaN where and only where the reference has NaN (an all-zero label row with epsilon = 0, an entropy threshold that selects nothing,
    ConsKLLoss as written)."""
    from test_softmax_losses_cpu import golden_cases, restated
    L = _losses()
    for pre, d in golden_cases(golden_dir):
        f = lambda a: torch.from_numpy(d[a]).cuda()
        stu, tea, w, tm, valid = f("stu"), f("tea"), f("weight"), f("tea_mask"), f("valid")
        got = {}
        for eps_name, eps, lab in (("eps", 1e-6, "label"), ("eps0", 0.0, "label"), ("eps0pos", 0.0, "label_pos")):
            for red in ("mean", "none"):
                got[f"kl_{eps_name}_{red}_w"] = L.JointsKLLoss(red, eps)(stu, f(lab), w)
                got[f"kl_{eps_name}_{red}"] = L.JointsKLLoss(red, eps)(stu, f(lab))
        for red in ("mean", "none"):
            got[f"ent_{red}"] = L.EntLoss(red)(stu)
            got[f"ent_{red}_some"] = L.EntLoss(red)(stu, float(d["thr_some"]))
            got[f"ent_{red}_none"] = L.EntLoss(red)(stu, float(d["thr_none"]))
        with pytest.warns(RuntimeWarning) if not L.ConsKLLoss._warned else _nullcontext():
            L.ConsKLLoss()(stu, tea)
        for cls, tag in ((L.ConsSoftmaxLoss, "csm"), (L.ConsKLLoss, "ckl")):
            got[f"{tag}_plain"] = cls()(stu, tea)
            got[f"{tag}_mask"] = cls()(stu, tea, tea_mask=tm)
            got[f"{tag}_valid"] = cls()(stu, tea, valid_mask=valid)
            got[f"{tag}_both"] = cls()(stu, tea, valid_mask=valid, tea_mask=tm)
        # masks in other storage: a float 0/1 mask and an integer valid_mask select the same elements
        assert torch.equal(L.ConsSoftmaxLoss()(stu, tea, valid_mask=valid.int(), tea_mask=tm.float()), got["csm_both"])
        assert L.JointsKLLoss("sum")(stu, f("label")) is None and L.EntLoss("sum")(stu) is None
        with pytest.raises(IndexError):
            L.ConsSoftmaxLoss()(stu, tea, valid_mask=tm)
        with pytest.raises(IndexError):
            L.ConsKLLoss(log_target=True)(stu, tea, valid_mask=tm)
        want64 = restated(d)
        assert set(want64) == set(got) and len(got) == 26
        rel = lambda a, b: float(np.max(np.abs(a - b)[np.isfinite(b)] / np.abs(b)[np.isfinite(b)])) if np.isfinite(b).any() else 0.0
        fam = {}
        for name in got:
            w64 = want64[name].numpy()
            fam.setdefault(name[:3], []).append(rel(d[name].astype(np.float64), w64))
        print(f"\n{pre}: golden (fp32 reference) worst relative error against fp64 per family: " + ", ".join(f"{k} {max(v):.2e}" for k, v in fam.items()))
        for name, v in got.items():
            g, ref, w64 = v.cpu().numpy(), d[name], want64[name].numpy()
            assert g.shape == ref.shape and g.dtype == np.float32, (name, g.shape, ref.shape)
            assert np.array_equal(np.isnan(g), np.isnan(ref)), (pre, name, g, ref)
            e, bar = rel(g.astype(np.float64), w64), MARGIN * max(fam[name[:3]])
            print(f"  {name:18s} device {e:.2e}  (bar {bar:.2e})")
            assert e <= bar, (pre, name, e, bar)


@pytest.mark.parametrize("n", [2, 7])
def test_a_tea_mask_that_does_not_have_one_entry_per_heatmap_is_refused_before_any_launch(n, monkeypatch):
    """The kernels index tea_mask by (b,k) row: a mask of another size (here 2 and 7 entries for B*K = 6) would be read out of bounds, so
    ConsLoss, ConsSoftmaxLoss and ConsKLLoss raise ValueError - and reach no library call on the way."""
    from uda_poseestimation_amd import heatmap_args
    L = _losses()
    stu, tea = torch.randn(2, 3, 4, 4, device="cuda"), torch.randn(2, 3, 4, 4, device="cuda")
    mask = torch.ones(n, dtype=torch.bool, device="cuda")

    def no_launch(*a, **k):
        raise AssertionError("a library call was reached")

    monkeypatch.setattr(L, "lib", no_launch)
    monkeypatch.setattr(heatmap_args, "lib", no_launch)
    for crit in (L.ConsLoss(), L.ConsSoftmaxLoss(), L.ConsKLLoss(log_target=True)):
        with pytest.raises(ValueError, match="tea_mask must have B\\*K elements"):
            crit(stu, tea, tea_mask=mask)
        with pytest.raises(ValueError, match="tea_mask must have B\\*K elements"):
            crit(stu, tea, valid_mask=torch.ones(2, 4, 4, dtype=torch.bool, device="cuda"), tea_mask=mask)


class _nullcontext:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def test_gradients_on_the_golden_shapes_match_fp64_autograd():
    check_against_fp32_arithmetic([(3, 5, 16, 16), (3, 5, 7, 9), (2, 3, 4, 4)], "golden shapes and B=2 K=3 4x4")


def test_gradients_on_ragged_shapes_match_fp64_autograd():
    """Pixel counts of 63 (odd, below one sweep), 960 (registers, a partly idle block), 3136 (registers, 56x56) and 6912 (above the 4096
    floats a block keeps in registers: re-read rows), with one key point and with 33."""
    shapes = [(2, K, H, W) for K in (1, 33) for (H, W) in ((7, 9), (24, 40), (56, 56), (96, 72))]
    check_against_fp32_arithmetic(shapes, "ragged shapes")


def test_gradients_at_the_product_size_match_fp64_autograd():
    check_against_fp32_arithmetic([(32, 16, 64, 64)], "product size B=32 K=16 64x64")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_16bit_inputs_return_gradients_in_the_input_dtype(dtype):
    d = make_inputs(3, 5, 16, 16, seed=3)
    d["stu"], d["tea"] = d["stu"].clamp(-30, 30), d["tea"].clamp(-30, 30)
    thr = entropy_threshold(d["stu"].to(dtype).float())
    d16 = _cast({k: (v.to(dtype) if k in ("stu", "tea", "label") else v) for k, v in d.items()}, None, "cuda")
    d32 = {k: (v.float() if v.dtype == dtype else v) for k, v in d16.items()}
    for name, (dev_fn, _) in kinds(thr).items():
        l16, g16 = _value_and_grad(dev_fn, d16["stu"], d16)
        l32, g32 = _value_and_grad(dev_fn, d32["stu"], d32)
        assert g16.dtype == dtype and l16.dtype == torch.float32, name
        # the operands are taken as fp32 rows: the same numbers as the fp32 call on the widened inputs, the gradient rounded once
        assert torch.equal(g16, g32.to(dtype)) and (torch.equal(l16, l32) or name == "ckl_ref_both"), name


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_loss_forward_and_backward_replayed_from_a_graph_equal_eager_bit_for_bit():
    """Loss + backward alone, captured into a hipGraph and replayed on fresh inputs: the same kernels in the same order and no atomics, so
    the results are the eager run's bits.  Two eager runs of one backward are bit-identical for the same reason."""
    B, K, H, W = 4, 16, 32, 32
    first = make_inputs(B, K, H, W, seed=20)
    thr = entropy_threshold(first["stu"]) * 1.02
    ks = kinds(thr)
    static = _cast(first, None, "cuda")
    x = static["stu"].clone().requires_grad_(True)
    scale = torch.tensor(3.0, device="cuda")

    def run(xx, dd):
        outs = []
        for name in ("kl_w", "ent", "ent_thr", "csm_both", "ckl_lt_both", "ckl_ref_both"):
            loss = ks[name][0](xx, dd)
            (g,) = torch.autograd.grad(loss * scale, xx)
            outs += [loss, g]
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
    for i in range(3):
        fresh = _cast(make_inputs(B, K, H, W, seed=21 + i), None, "cuda")
        for k, v in fresh.items():
            static[k].copy_(v)
        with torch.no_grad():
            x.copy_(fresh["stu"])
        graph.replay()
        xe = fresh["stu"].clone().requires_grad_(True)
        eager = run(xe, fresh)
        again = run(xe, fresh)
        torch.cuda.synchronize()
        assert len(captured) == len(eager) == 12
        for j, (c, e, a) in enumerate(zip(captured, eager, again)):
            assert torch.equal(_bits(c), _bits(e)), (i, j)
            assert torch.equal(_bits(e), _bits(a)), (i, j)
        assert all(torch.isfinite(e).all() for e in eager[:10]) and torch.isnan(eager[10]) and torch.isfinite(eager[11]).all()


# ---------------------------------------------------------------------------------------------- the step with the new criteria
N, K_, S = 4, 16, 128


def _new_criteria():
    L = _losses()
    return dict(criterion=L.JointsKLLoss(epsilon=1e-6), con_criterion=L.ConsSoftmaxLoss(), ent_criterion=L.EntLoss(), lambda_ent=0.1)


def _batches(seeds):
    from uda_poseestimation_amd import synthetic
    out = []
    for s in seeds:
        b = synthetic.mean_teacher_batch(N, num_keypoints=K_, image_size=S, heatmap_size=S // 4, seed=s)
        g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
        out.append((g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"]))
    return out


@pytest.mark.parametrize("precision", ["bf16", "strict"])
def test_captured_steps_with_the_new_criteria_equal_eager_steps(precision):
    """test_captured_steps_equal_eager_steps_from_identical_state_with_varying_batches (tests/test_gpu_steps.py) with
    JointsKLLoss / ConsSoftmaxLoss / EntLoss as the step's criteria: its assertions and bars, and loss_ent at the loss_c bar."""
    from test_gpu_steps import _tiny
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    batches = _batches((31, 32, 33, 34))
    base = _tiny(K_, seed=8)
    for split in (False, True):
        nets = []
        for _ in range(2):
            s_, t_ = _tiny(K_, seed=8), _tiny(K_, seed=8)
            s_.load_state_dict(base.state_dict())
            nets.append((s_.cuda(), t_.cuda()))
        tr_g = MeanTeacherTrainer(*nets[0], lr=1e-4, image_size=S, heatmap_size=S // 4, precision=precision, **_new_criteria())
        tr_e = MeanTeacherTrainer(*nets[1], lr=1e-4, image_size=S, heatmap_size=S // 4, precision=precision, **_new_criteria())
        p0 = [p.detach().clone() for p in nets[0][0].parameters()]
        gs = GraphedTrainStep(tr_g, *batches[0], warmup=1, split=split)       # the warm-up step IS step 1 (on batch 0)
        tr_e.train_step(*batches[0])
        for bt in batches[1:]:
            og = gs.step(*bt)
            oe = tr_e.train_step(*bt)
            print(f"{precision} split={split}: loss_all {float(og['loss_all']):.6e} / {float(oe['loss_all']):.6e}  loss_s {float(og['loss_s']):.6e}  "
                  f"loss_c {float(og['loss_c']):.4e} / {float(oe['loss_c']):.4e}  loss_ent {float(og['loss_ent']):.6e} / {float(oe['loss_ent']):.6e}")
            assert abs(float(og["loss_all"]) - float(oe["loss_all"])) <= 2e-3 * abs(float(oe["loss_all"]))
            assert abs(float(og["loss_c"]) - float(oe["loss_c"])) <= 5e-3 * abs(float(oe["loss_c"])) + 1e-7
            assert abs(float(og["loss_ent"]) - float(oe["loss_ent"])) <= 5e-3 * abs(float(oe["loss_ent"])) + 1e-7
            want = float(oe["loss_s"]) + float(oe["loss_c"]) + 0.1 * float(oe["loss_ent"])
            assert abs(float(oe["loss_all"]) - want) <= 1e-5 * abs(want)
        sg, se, tg, te = nets[0][0], nets[1][0], nets[0][1], nets[1][1]
        num = den = 0.0
        for pg, pe, q0 in zip(sg.parameters(), se.parameters(), p0):
            num += float(((pg.detach() - pe.detach()) ** 2).sum())
            den += float(((pe.detach() - q0) ** 2).sum())
        rel = (num / max(den, 1e-30)) ** 0.5
        print(f"{precision} split={split}: ||student(graph) - student(eager)|| / ||student(eager) - start|| = {rel:.3e} after {len(batches)} steps")
        assert den > 0 and rel < 0.2
        tn = sum(float(((a.detach() - c.detach()) ** 2).sum()) for a, c in zip(tg.parameters(), te.parameters()))
        td = sum(float(((c.detach() - q0) ** 2).sum()) for c, q0 in zip(te.parameters(), p0))
        assert (tn / max(td, 1e-30)) ** 0.5 < 0.1
        if not split:       # the deferred read-back carries the entropy term too
            m = gs.step_async(*batches[1])
            m = gs.flush_metrics()
            assert abs(m["loss_ent"] - float(gs.out["loss_ent"])) == 0.0 and abs(m["loss_c"] - float(gs.out["loss_c"])) == 0.0
        gs.release()


def test_two_captured_steps_with_the_new_criteria_agree_to_the_bit_after_ten_steps():
    from test_gpu_steps import _tiny
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    batches = _batches(range(40, 50))
    base = _tiny(K_, seed=9)
    runs = []
    for _ in range(2):
        s_, t_ = _tiny(K_, seed=9), _tiny(K_, seed=9)
        s_.load_state_dict(base.state_dict())
        s_, t_ = s_.cuda(), t_.cuda()
        tr = MeanTeacherTrainer(s_, t_, lr=1e-4, image_size=S, heatmap_size=S // 4, precision="bf16", **_new_criteria())
        gs = GraphedTrainStep(tr, *batches[0], warmup=1)
        losses = []
        for bt in batches[1:]:
            o = gs.step(*bt)
            losses.append(torch.stack([o[k].detach().float().reshape(()) for k in ("loss_all", "loss_s", "loss_c", "loss_ent")]).clone())
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), [p.detach().cpu().clone() for p in s_.parameters()], [p.detach().cpu().clone() for p in t_.parameters()]))
        gs.release()
    (la, sa, ta), (lb, sb, tb) = runs
    print("losses of the tenth step [all, s, c, ent]:", la[-1].tolist())
    assert torch.isfinite(la).all() and torch.equal(_bits(la), _bits(lb))
    assert all(torch.equal(a, b) for a, b in zip(sa, sb)) and all(torch.equal(a, b) for a, b in zip(ta, tb))
    assert any(not torch.equal(a, p.detach()) for a, p in zip(sa, base.parameters()))          # it trained


def test_strict_eager_step_with_the_new_criteria_matches_the_whole_step_oracle(monkeypatch):
    """precision='strict' (student forward and teacher at fp32 grade: the comparison tests the losses, not a 16-bit trunk): the eager step
    against oracle.step_ref.train_step_full_ref whose two loss functions are replaced, for this test, by the restatement - the mask element
    for element, loss_s within 1e-3 relative, loss_c within 5e-3 relative + 1e-7 (the bars of
    test_config2_eager_step_matches_whole_step_oracle)."""
    import oracle.step_ref as step_ref
    from oracle.pose_resnet_ref import PoseResNetRef
    from test_gpu_steps import _tiny
    from uda_poseestimation_amd import synthetic
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    L = _losses()
    monkeypatch.setattr(step_ref, "joints_mse_ref", lambda o, t, w=None: R64.joints_kl(o, t, w, "mean", 1e-6))
    monkeypatch.setattr(step_ref, "cons_loss_ref", lambda s, t, valid_mask=None, tea_mask=None: R64.cons_softmax(s, t, valid_mask, tea_mask))
    layers = [1, 1, 1, 1]
    torch.manual_seed(5)
    ref_s, ref_t = PoseResNetRef(layers, K_), PoseResNetRef(layers, K_)
    ref_t.load_state_dict(ref_s.state_dict())
    stu, tea = _tiny(K_, layers), _tiny(K_, layers)
    stu.load_state_dict(ref_s.state_dict())
    b = synthetic.mean_teacher_batch(N, num_keypoints=K_, image_size=S, heatmap_size=S // 4, seed=61)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    tr = MeanTeacherTrainer(stu.cuda(), tea.cuda(), lr=1e-4, image_size=S, heatmap_size=S // 4, precision="strict",
                            criterion=L.JointsKLLoss(epsilon=1e-6), con_criterion=L.ConsSoftmaxLoss())
    out = tr.train_step(g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])
    torch.cuda.synchronize()
    assert "loss_ent" not in out
    opt = torch.optim.Adam(ref_s.parameters(), lr=1e-4)
    ref = step_ref.train_step_full_ref(ref_s, ref_t, opt, b["x_s"], b["label_s"], b["weight_s"], b["x_t_stu"], b["x_t_tea"], b["aug_param_stu"],
                                       b["aug_param_tea"], ratio=4.0, image_size=S)
    ls, lr_, lc, lcr = float(out["loss_s"]), float(ref["loss_s"]), float(out["loss_c"]), float(ref["loss_c"])
    print(f"strict step, JointsKLLoss / ConsSoftmaxLoss: loss_s {ls:.6f} / oracle {lr_:.6f} ({abs(ls - lr_) / lr_:.2e}), "
          f"loss_c {lc:.4e} / oracle {lcr:.4e} ({abs(lc - lcr) / lcr:.2e})")
    assert torch.equal(out["tea_mask"].cpu().bool(), ref["tea_mask"].bool())
    assert abs(ls - lr_) <= 1e-3 * lr_, (ls, lr_)
    assert abs(lc - lcr) <= 5e-3 * lcr + 1e-7, (lc, lcr)
    # Adam and the EMA ran on the new losses' gradients: the teacher moved towards the student as the oracle's did
    dmax = max((a.detach().cpu() - r.detach()).abs().max().item() for a, r in zip(tea.parameters(), ref_t.parameters()))
    assert dmax < 1e-6 + 1e-3 * 1e-4 * 10, dmax


def test_default_trainer_issues_the_default_criteria():
    """No new keyword: JointsMSELoss / ConsLoss, no entropy term, the result dict as before (bit-identity of the default step with the
    parent commit is checked from outside, with bench.py --dump-outputs on both builds)."""
    from test_gpu_steps import _tiny
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    L = _losses()
    s_, t_ = _tiny(K_, seed=8).cuda(), _tiny(K_, seed=8).cuda()
    tr = MeanTeacherTrainer(s_, t_, lr=1e-4, image_size=S, heatmap_size=S // 4, precision="bf16")
    assert type(tr.criterion) is L.JointsMSELoss and type(tr.con_criterion) is L.ConsLoss and tr.ent_criterion is None
    out = tr.train_step(*_batches((31,))[0])
    assert sorted(out) == sorted(["loss_all", "loss_s", "loss_c", "y_s", "tea_mask", "y_t_tea_recon", "y_t_stu_recon"])
    assert float(out["loss_all"]) == float(out["loss_s"] + 1.0 * out["loss_c"])
