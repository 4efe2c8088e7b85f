"""The 'strict' training precision: an fp32-grade (f16x2) student FORWARD whose backward is the existing fp16 one.  The forward of a
mode-3 plan is the f16x2 forward, and its apply / pool / conversion launches also write the fp16 tensors the 16-bit backward reads.
Checked here: the forward equals the no-grad 'f16x2' forward to the bit and its fp16 tensors are roundings of the fp32-grade ones; the
gradients against fp32 CPU autograd (no worse than fp16's); the benchmarked step against the oracle at SURVEY.md 8(d)'s 1e-3 heat-map
bar; a 10-step trajectory; the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_fullsize import _args, _compare_with_oracle, _device_pair, _ema_bit_exact, _need_host_mem, _oracle_step, _rewind, _to_dev
from test_gpu_fullsize import keypoint_mean_teacher_batch

pytestmark = pytest.mark.gpu

LAYERS, K, N, S = [1, 1, 1, 1], 16, 4, 128


def _small(bias=False, seed=0):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(seed)
    return pr._pose_resnet("t", K, pr.Bottleneck_default, LAYERS, False, bias)


def _bufs(net):
    return [b.detach().clone() for b in net.buffers()]


def _set_bufs(net, bufs):
    with torch.no_grad():
        for b, v in zip(net.buffers(), bufs):
            b.copy_(v)


def _arena(act, off, name, nbytes, dtype):
    return act[off[name]:off[name] + nbytes].view(dtype)


@pytest.mark.parametrize("bias", [False, True], ids=["no_deconv_bias", "deconv_bias"])
def test_strict_forward_equals_f16x2_and_leaves_fp16_shadows(bias):
    from helpers.strict_layout import strict_layout
    from uda_poseestimation_amd import _hip
    net = _small(bias).cuda().train()
    if bias:
        with torch.no_grad():
            for m in net.upsampling.modules():
                if isinstance(m, torch.nn.ConvTranspose2d):
                    m.bias.normal_(0.0, 0.1)
    x = torch.randn(N, 3, S, S, generator=torch.Generator().manual_seed(1)).cuda()
    net.aux_lib_kind = "fp16"      # (the no-grad f16x2 plan in the strict plan's build, as MeanTeacherTrainer(precision='strict') places it)
    b0 = _bufs(net)
    net.precision = "strict"
    out = net(x)
    assert net._last_hd.precision == "strict" and out.grad_fn is not None
    torch.cuda.synchronize()
    bs = _bufs(net)
    act = out.grad_fn.act
    _set_bufs(net, b0)
    net.precision = "f16x2"
    with torch.no_grad():
        ref = net(x)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), ref), f"max|d| {(out.detach() - ref).abs().max().item():.3e}"
    for a, b in zip(bs, _bufs(net)):
        assert torch.equal(a, b), "running statistics differ"
    print(f"strict forward == no-grad f16x2 forward to the bit (heat-maps and {len(bs)} BN buffers), deconv bias {bias}")
    # the fp16 tensors of the 16-bit layout against the fp32-grade tensors they were rounded from
    off = strict_layout(LAYERS, K, N, S, S)
    x8 = _arena(act, off, "x8", N * S * S * 8 * 2, torch.float16).view(N, S, S, 8)
    exp = torch.zeros(N, S, S, 8, device=x.device)
    exp[..., :3] = x.permute(0, 2, 3, 1)
    assert torch.equal(x8, exp.half())
    Hu = S // 4            # the last deconvolution's y: its fp32 copy is the last tenant of slot Y
    nb = N * Hu * Hu * 256
    y16 = _arena(act, off, "up2.y", nb * 2, torch.float16)
    y32 = act[off["slot.Y"]:off["slot.Y"] + nb * 4].view(torch.float32)
    assert off["fslot.up2.y"] == "Y" and torch.equal(y16, y32.half())
    z16 = _arena(act, off, "up2.z", nb * 2, torch.float16)       # ... and its BN output: the h half of the split z, last in its slot
    sl = off["slot." + off["fslot.up2.z"]]
    zsp = act[sl:sl + nb * 4].view(torch.float16).view(-1, 2, 8)
    assert torch.equal(z16, zsp[:, 0, :].reshape(-1)) and (z16 >= 0).all()
    # block outputs: the ReLU bit mask of the fp16 z (where the 16-bit apply writes one)
    if _hip.policy().bn3_mask:
        Hc = S // 4
        for i, P in enumerate((64, 128, 256, 512)):
            Ho = Hc if i == 0 else Hc // 2
            n_el = N * Ho * Ho * 4 * P
            zb = _arena(act, off, f"block{i}.b3.z", n_el * 2, torch.float16)
            mk = act[off[f"block{i}.mask"]:off[f"block{i}.mask"] + n_el // 8]
            bits = ((mk.long().unsqueeze(1) >> torch.arange(8, device=mk.device)) & 1).reshape(-1).bool()
            assert torch.equal(bits, zb > 0), f"block {i}: mask"
            Hc = Ho
    # the stem's pooled fp16 map: the 3x3 s2 max of the stem's fp16 z, and the saved taps point at the winners
    Hs, Hp = S // 2, S // 4
    zs = _arena(act, off, "stem.z", N * Hs * Hs * 64 * 2, torch.float16).view(N, Hs, Hs, 64)
    pool = _arena(act, off, "pool", N * Hp * Hp * 64 * 2, torch.float16).view(N, Hp, Hp, 64)
    mp = torch.nn.functional.max_pool2d(zs.permute(0, 3, 1, 2).float(), 3, 2, 1).permute(0, 2, 3, 1).half()
    # (pool is the fp16 rounding of the pooled split VALUE h + l 2^-11, z's h the rounding of the exact fp32 z: where that value lies within
    # 2^-22 of a half-ulp boundary the two roundings differ by one ulp.  All values are >= 0 after the ReLU: ulps are integer steps of the bits)
    ulps = (pool.view(torch.int16).int() - mp.view(torch.int16).int()).abs()
    print(f"pooled fp16 map vs the 3x3 s2 max of the stem's fp16 z: {int((ulps == 0).sum())}/{ulps.numel()} identical, max {int(ulps.max())} ulp")
    assert int(ulps.max()) <= 1 and float((ulps == 0).float().mean()) > 0.999
    idx = act[off["poolidx"]:off["poolidx"] + N * Hp * Hp * 64].view(N, Hp, Hp, 64).long()
    ho = torch.arange(Hp, device=x.device).view(1, Hp, 1, 1) * 2 - 1 + idx // 3
    wo = torch.arange(Hp, device=x.device).view(1, 1, Hp, 1) * 2 - 1 + idx % 3
    assert (ho >= 0).all() and (wo >= 0).all() and (ho < Hs).all() and (wo < Hs).all()
    nn_ = torch.arange(N, device=x.device).view(N, 1, 1, 1).expand_as(idx)
    cc = torch.arange(64, device=x.device).view(1, 1, 1, 64).expand_as(idx)
    assert int((zs[nn_, ho, wo, cc].view(torch.int16).int() - pool.view(torch.int16).int()).abs().max()) <= 1
    print("fp16 shadows: image, deconv y / z, block masks, pooled map and taps all equal to roundings of the fp32-grade tensors")


def _trained_small(seed=3, steps=60):
    """A small network trained on the device for a few dozen fp16 steps (heat-maps with real peaks, BN statistics of real features)."""
    from uda_poseestimation_amd import optim as fused_optim
    from uda_poseestimation_amd import synthetic
    from uda_poseestimation_amd.lib.models.loss import JointsMSELoss
    net = _small(seed=seed).cuda().train()
    net.precision = "fp16"
    opt = fused_optim.FusedAdam(net.parameters(), lr=5e-4, dynamic_loss_scale=True, init_scale=1024.0)
    crit = JointsMSELoss()
    for it in range(steps):
        x, lab, wt = (t.cuda() for t in synthetic.keypoint_batch(8, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=2000 + it))
        opt.zero_grad()
        opt.scale_loss(crit(net(x), lab, wt)).backward()
        opt.step()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


@pytest.fixture(scope="module")
def small_sd():
    return _trained_small()


def test_strict_gradients_vs_fp32_autograd(small_sd):
    from oracle.pose_resnet_ref import PoseResNetRef
    from uda_poseestimation_amd import synthetic
    x, _, _ = synthetic.keypoint_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=77)
    G = torch.randn(N, K, S // 4, S // 4, generator=torch.Generator().manual_seed(5)) * 1e-2
    ref = PoseResNetRef(LAYERS, K)
    ref.load_state_dict(small_sd)
    ref.train()
    (ref(x) * G).sum().backward()
    names = [n for n, _ in ref.named_parameters()]
    gref = {n: p.grad.detach().clone() for n, p in ref.named_parameters() if p.grad is not None}
    scale = 1024.0          # (the fp16 backward needs the loss scaled, as under the trainer's scaler)
    grads, nets = {}, {}
    for prec in ("strict", "fp16"):
        net = _small().cuda().train()
        net.load_state_dict(small_sd)
        net.precision = prec
        ((net(x.cuda()) * G.cuda()).sum() * scale).backward()
        torch.cuda.synchronize()
        grads[prec] = {n: p.grad.detach().cpu() / scale for n, p in net.named_parameters() if p.grad is not None}
        nets[prec] = net
    assert set(grads["strict"]) == set(gref)
    rel = {}
    for prec in grads:
        num = sum(float(((grads[prec][n] - gref[n]).double() ** 2).sum()) for n in gref)
        den = sum(float((gref[n].double() ** 2).sum()) for n in gref)
        rel[prec] = (num / den) ** 0.5
    for n in names:
        if n in gref:
            cs = {p: float(torch.nn.functional.cosine_similarity(grads[p][n].flatten().double(), gref[n].flatten().double(), dim=0)) for p in grads}
            print(f"  {n:45s} cosine strict {cs['strict']:.6f}  fp16 {cs['fp16']:.6f}")
    print(f"global relative L2 error of the flat gradient vs fp32 autograd: strict {rel['strict']:.3e}, fp16 {rel['fp16']:.3e}")
    assert rel["strict"] <= rel["fp16"], rel
    # two backwards of the same forward state: the same bits
    net = nets["strict"]
    dout = (G.cuda() * scale).contiguous()
    net.zero_grad(set_to_none=True)
    out = net(x.cuda())
    act, hd, ws = out.grad_fn.act, out.grad_fn.hd, out.grad_fn.ws
    out.backward(dout)
    g1 = net._flat_grad.clone()
    with pytest.raises(RuntimeError):
        out.backward(dout)                  # a second .backward() of the same forward still raises
    net.zero_grad(set_to_none=True)
    net._run_backward(dout, act, hd, ws)
    torch.cuda.synchronize()
    assert torch.equal(g1, net._flat_grad), "two backwards of the same forward state differ"
    # the backward in two parts (data parallel's cut after layer3's first block) equals the whole backward
    net.zero_grad(set_to_none=True)
    net._flat_grad.fill_(float("nan"))
    net.split_backward = True
    net(x.cuda()).backward(dout)
    net.split_backward = False
    net.finish_backward()
    torch.cuda.synchronize()
    both = net._flat_grad
    assert torch.isfinite(both).all()
    assert float((both - g1).abs().max()) <= 1e-5 * float(g1.abs().max())
    print(f"two backwards of one forward: identical; two-part backward vs whole: max|d| {float((both - g1).abs().max()):.3e}")


@pytest.fixture(scope="module")
def config1_strict(trained_r101_k16):
    _need_host_mem(48)
    sd = trained_r101_k16[0]
    b = keypoint_mean_teacher_batch(32, seed=40)
    return sd, b, _oracle_step(sd, b, 16)


def test_strict_config1_full_size_captured_step_vs_oracle(config1_strict):
    """BASELINE.json configs[1] (PoseResNet-101, K = 16, N = 32, 256x256, one captured graph) with precision='strict' against the fp32 oracle
    step: the student's heat-maps meet SURVEY.md 8(d)'s 1e-3 bar."""
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    sd, b, ref = config1_strict
    g = _to_dev(b)
    burn = _to_dev(keypoint_mean_teacher_batch(32, seed=50))
    stu, tea = _device_pair(sd, 16)
    tr = MeanTeacherTrainer(stu, tea, lr=1e-4, precision="strict")
    assert stu.precision == "strict" and tea.precision == "f16x2" and tea.aux_lib_kind == "fp16" and tr.stu_optimizer._scaler is not None
    gs = GraphedTrainStep(tr, *_args(burn), warmup=1)
    assert gs.one_graph and not gs.split
    _rewind(tr, stu, tea, sd)
    out = dict(gs.step(*_args(g)))
    torch.cuda.synchronize()
    assert stu._last_hd.precision == "strict"
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}
    fig = _compare_with_oracle("configs[1] N=32 captured strict", out, ref, b["label_s"], stu, tea, sd, 1e-5, 1e-3, 1e-4, 1e-4, True)
    _ema_bit_exact(tea, sd, stu)
    names = [n for n, _ in stu.named_parameters()]
    agree = total = 0
    for n_, p_dev, p_ref in zip(names, stu.parameters(), ref["student_after"]):
        d_dev, d_ref = p_dev.detach().cpu() - sd[n_], p_ref - sd[n_]
        sel = d_ref.abs() > 5e-5
        agree += int((torch.sign(d_dev[sel]) == torch.sign(d_ref[sel])).sum())
        total += int(sel.sum())
    print(f"  strict: student heat-maps {fig['heatmap_max_abs']:.3e} (bar 1e-3); Adam sign agreement {agree / max(total, 1):.4f} over {total} entries")
    assert total > 1e7 and agree / total > 0.9
    # captured == eager twin, to the bit
    stu_e, tea_e = _device_pair(sd, 16)
    tr_e = MeanTeacherTrainer(stu_e, tea_e, lr=1e-4, precision="strict")
    out_e = tr_e.train_step(*_args(g))
    torch.cuda.synchronize()
    assert torch.equal(out_e["tea_mask"].cpu(), out["tea_mask"].cpu())
    for k_ in ("y_t_tea_recon", "y_s", "y_t_stu_recon"):
        assert torch.equal(out_e[k_].float(), out[k_].float()), f"captured and eager {k_} differ"
    for pg, pe in zip(list(stu.parameters()) + list(tea.parameters()), list(stu_e.parameters()) + list(tea_e.parameters())):
        assert torch.equal(pg.detach(), pe.detach())
    assert float(out["loss_all"]) == float(out_e["loss_all"])
    gs.release()


def test_strict_trajectory_10_steps_and_overflow(small_sd):
    """10 captured steps of a small network: the strict student's heat-maps stay at least as close to a 10-step fp32 oracle run as the fp16
    student's; captured == eager to the bit; an overflowing loss scale skips Adam and still runs the EMA."""
    from oracle.pose_resnet_ref import PoseResNetRef
    from oracle.step_ref import train_step_ref
    from uda_poseestimation_amd import synthetic
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    batches = [synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=300 + i) for i in range(10)]
    torch.set_num_threads(8)
    ref_s, ref_t = PoseResNetRef(LAYERS, K), PoseResNetRef(LAYERS, K)
    ref_s.load_state_dict(small_sd)
    ref_t.load_state_dict(small_sd)
    opt = torch.optim.Adam(ref_s.parameters(), lr=1e-4)
    y_ref = []
    for b in batches:
        r = train_step_ref(ref_s, ref_t, opt, b["x_s"], b["label_s"], b["weight_s"], b["x_t_stu"], b["x_t_tea"], b["aug_param_stu"],
                           b["aug_param_tea"], ratio=4.0)
        y_ref.append(r["y_s"].detach().clone())

    def pair():
        s_ = pr._pose_resnet("t", K, pr.Bottleneck_default, LAYERS, False, False)
        t_ = pr._pose_resnet("t", K, pr.Bottleneck_default, LAYERS, False, False)
        s_.load_state_dict(small_sd)
        t_.load_state_dict(small_sd)
        return s_.cuda(), t_.cuda()

    gb = [_to_dev(b) for b in batches]
    err, mx, ys = {}, {}, {}
    for prec in ("strict", "reference"):         # ('reference': the fp16 student next to the same f16x2 teacher)
        stu, tea = pair()
        tr = MeanTeacherTrainer(stu, tea, image_size=S, heatmap_size=S // 4, precision=prec)
        gs = GraphedTrainStep(tr, *_args(gb[0]), warmup=1)
        _rewind(tr, stu, tea, small_sd)
        ys[prec] = []
        for g in gb:
            ys[prec].append(gs.step(*_args(g))["y_s"].detach().float().clone())
        torch.cuda.synchronize()
        err[prec] = [float((y.cpu() - r).norm()) for y, r in zip(ys[prec], y_ref)]
        mx[prec] = [(y.cpu() - r).abs().max().item() for y, r in zip(ys[prec], y_ref)]
        if prec == "strict":
            p_cap = [p.detach().clone() for p in list(stu.parameters()) + list(tea.parameters())]
        gs.release()
    # (distance = the L2 norm of the heat-map difference over the batch; the max-abs element is printed as well - after the first step both
    #  students' weights have moved away from the oracle's by their fp16 gradients, and a single element's error is dominated by that drift)
    for name, e in (("||student heat-maps - oracle||_2", err), ("max|student heat-maps - oracle|", mx)):
        print(f"{name} per step:\n  strict " + " ".join(f"{v:.2e}" for v in e["strict"]) + "\n  fp16   " + " ".join(f"{v:.2e}" for v in e["reference"]))
    assert all(a <= b for a, b in zip(err["strict"], err["reference"])), err
    # captured == eager over the 10 steps
    stu, tea = pair()
    tr = MeanTeacherTrainer(stu, tea, image_size=S, heatmap_size=S // 4, precision="strict")
    for g, yc in zip(gb, ys["strict"]):
        assert torch.equal(tr.train_step(*_args(g))["y_s"].detach().float(), yc)
    for a, b in zip(list(stu.parameters()) + list(tea.parameters()), p_cap):
        assert torch.equal(a.detach(), b)
    # loss-scaler overflow: a scale that overflows fp16 skips Adam (weights and step counter untouched) and still runs the EMA
    stu, tea = pair()
    tr = MeanTeacherTrainer(stu, tea, image_size=S, heatmap_size=S // 4, precision="strict", loss_scale_init=2.0 ** 100)
    tr.train_step(*_args(gb[0]))
    torch.cuda.synchronize()
    st = tr.stu_optimizer.state_dict()["param_groups"][0]
    assert st["step"] == 0 and st["loss_scale"] == 2.0 ** 99, st
    for n_, p in stu.named_parameters():
        assert torch.equal(p.detach().cpu(), small_sd[n_]), n_
    _ema_bit_exact(tea, small_sd, stu)
    print("overflow: Adam skipped, scale backed off to 2^99, EMA ran")


def test_strict_abi():
    from uda_poseestimation_amd import _hip
    L = _hip.lib("fp16")
    arr = (C.c_int * 4)(*LAYERS)
    h = C.c_void_p()
    assert L.udapose_net_create(arr, K, N, S, S, 3, C.byref(h)) == 0
    L.udapose_net_destroy(h)
    assert L.udapose_net_create(arr, K, N, S, S, 3 | 0x200, C.byref(h)) != 0
    # udapose_net_backward on a mode-3 plan: OK
    net = _small().cuda().train()
    net.precision = "strict"
    x = torch.randn(N, 3, S, S, generator=torch.Generator().manual_seed(9)).cuda()
    out = net(x)
    act, hd, ws = out.grad_fn.act, out.grad_fn.hd, out.grad_fn.ws
    pa, ba, params = net._pointers()
    views = net._grad_views(params)
    gp = (C.c_void_p * len(views))(*[v.data_ptr() for v in views])
    assert hd.L.udapose_net_bind_grads(hd.h, gp) == 0
    dout = torch.randn_like(out) * 1e-2
    from uda_poseestimation_amd._hip import ptr
    rc = hd.L.udapose_net_backward(hd.h, _hip.stream(), ptr(dout), pa, ptr(hd.wpack), ptr(act), ptr(ws), gp, 0.0)
    torch.cuda.synchronize()
    assert rc == 0 and torch.isfinite(net._flat_grad).all() and float(net._flat_grad.abs().max()) > 0
    # the arena at N = 32, 256x256 (PoseResNet-101)
    r101 = (C.c_int * 4)(3, 4, 23, 3)
    sizes = {}
    for mode in (3, 0):
        assert L.udapose_net_create(r101, 16, 32, 256, 256, mode, C.byref(h)) == 0
        sizes[mode] = L.udapose_net_act_bytes(h)
        L.udapose_net_destroy(h)
    print(f"udapose_net_act_bytes at N=32, 256x256: strict {sizes[3] / 2 ** 20:.0f} MB, fp16 {sizes[0] / 2 ** 20:.0f} MB")
    assert sizes[3] < 1.5 * sizes[0]


def test_strict_pretrain_step_and_validate(small_sd):
    """pretrain_step (the source-only loop, train_human.py:262-289) in 'strict' moves the student like the fp16 student does, within the
    fp16 backward's reach of it; engine.validate on a strict model runs the no-grad f16x2 forward and equals validate on an 'f16x2' model."""
    from uda_poseestimation_amd import synthetic
    from uda_poseestimation_amd.engine import MeanTeacherTrainer, validate
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    x, lab, wt = (t.cuda() for t in synthetic.keypoint_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=91))
    moved = {}
    for prec in ("strict", "fp16"):
        s_ = pr._pose_resnet("t", K, pr.Bottleneck_default, LAYERS, False, False)
        t_ = pr._pose_resnet("t", K, pr.Bottleneck_default, LAYERS, False, False)
        s_.load_state_dict(small_sd)
        tr = MeanTeacherTrainer(s_.cuda(), t_.cuda(), image_size=S, heatmap_size=S // 4, precision=prec)
        losses = [float(tr.pretrain_step(x, lab, wt)["loss_s"]) for _ in range(2)]
        torch.cuda.synchronize()
        assert np.isfinite(losses).all()
        moved[prec] = torch.cat([(p.detach().cpu() - small_sd[n]).flatten() for n, p in s_.named_parameters()])
        if prec == "strict":
            assert s_._last_hd.precision == "strict"
            batches = [synthetic.keypoint_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=95 + i) for i in range(2)]
            batches = [tuple(t.cuda() for t in b) for b in batches]
            acc_s, loss_s = validate(batches, s_)
            assert s_._last_hd.precision == "f16x2" and s_.training
            ref = pr._pose_resnet("t", K, pr.Bottleneck_default, LAYERS, False, False).cuda()
            ref.load_state_dict(s_.state_dict())
            ref.precision, ref.aux_lib_kind = "f16x2", s_.aux_lib_kind
            acc_r, loss_r = validate(batches, ref)
            assert loss_s == loss_r and list(acc_s) == list(acc_r), (loss_s, loss_r)
    a, b = moved["strict"], moved["fp16"]
    cos = float(torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=0))
    print(f"pretrain_step x2: strict vs fp16 parameter update cosine {cos:.4f}; validate: strict model == f16x2 model")
    assert cos > 0.9
