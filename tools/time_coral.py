"""What GramCoralLoss costs on one MI355X at (N,K,H,W) = (32,16,64,64), coral_downsample 1 and 2.  Three parts, one process:
  kernels  udapose_coral_fwd (coral_gram_k + coral_sum_k + coral_finish_k) and udapose_coral_bwd (coral_bwd_k), 100 back-to-back launches between two
           device events each; the per-kernel split of the forward from torch's profiler over the same launches (device durations by name)
  torch    the same Gram form in plain torch on the device (torch.mm for the 2n x 2n Gram and for coef . Z, fp32), timed the same way
  step     BASELINE.json configs[1] (PoseResNet-101, bf16, captured GraphedTrainStep) without the criterion and with it at lambda_coral = 0.5,
           the trainers alternated in one process, median of --rounds
One JSON line per measurement; the committed copy is profiles/coral.txt.  The bytes-moved floors are arithmetic on the shapes: the forward reads
the inputs once and writes, then reads again, its fp64 partials; the backward reads the inputs and writes both gradients; floor_us = bytes over
HBM_TBPS, the 6.29 TB/s a float4 copy reaches on this part (of 8.0 TB/s nominal).
usage: python tools/time_coral.py [--parts kernels,torch,step] [--launches 100] [--steps 20] [--warmup 3] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uda_poseestimation_amd import _hip, synthetic  # noqa: E402
from uda_poseestimation_amd._hip import lib, ptr  # noqa: E402
from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer  # noqa: E402
from uda_poseestimation_amd.lib.models.loss import GramCoralLoss  # noqa: E402
import uda_poseestimation_amd.lib.models as models  # noqa: E402

N, K, H, W = 32, 16, 64, 64
HBM_TBPS = 6.29


def heatmaps(seed):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.arange(H).view(1, 1, H, 1).float(), torch.arange(W).view(1, 1, 1, W).float()
    cy, cx = torch.randint(0, H, (N, K, 1, 1), generator=g).float(), torch.randint(0, W, (N, K, 1, 1), generator=g).float()
    return (torch.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / 8.0) + 0.02 * torch.randn(N, K, H, W, generator=g)).cuda()


def timed(fn, launches):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches       # us per call


def down_torch(x, d):
    if d == 1:
        return x
    Ho, Wo = x.shape[2] // d, x.shape[3] // d
    b = x[..., :Ho * d, :Wo * d].reshape(x.shape[0], x.shape[1], Ho, d, Wo, d)
    if d % 2:
        return b[:, :, :, d // 2, :, d // 2]
    lo, hi = d // 2 - 1, d // 2
    return 0.25 * (b[:, :, :, lo, :, lo] + b[:, :, :, lo, :, hi] + b[:, :, :, hi, :, lo] + b[:, :, :, hi, :, hi])


def kernels_and_torch(d, launches, parts):
    L = lib()
    src, tgt = heatmaps(1), heatmaps(2)
    Dd = K * (H // d) * (W // d)
    read_mb = 2 * N * Dd * (4 if d % 2 == 0 else 1) * 4 / 1e6           # (even d reads four pixels per element)
    full_mb = 2 * N * K * H * W * 4 / 1e6
    if "kernels" in parts:
        ws = torch.empty(L.udapose_coral_ws_bytes(N, K, H, W, d) // 8, dtype=torch.float64, device="cuda")
        mp = (2 * N + 31) // 32 * 32
        coef = torch.empty(mp * mp, device="cuda")
        loss = torch.empty((), device="cuda")
        ds, dt = torch.empty_like(src), torch.empty_like(tgt)
        one = torch.ones(1, device="cuda")
        st = _hip.stream()
        fwd = lambda: L.udapose_coral_fwd(st, ptr(src), ptr(tgt), N, K, H, W, d, ptr(ws), ptr(coef), ptr(loss))
        bwd = lambda: L.udapose_coral_bwd(st, ptr(src), ptr(tgt), ptr(coef), ptr(one), N, K, H, W, d, ptr(ds), ptr(dt))
        part_mb = (ws.numel() * 8 - mp * mp * 8) / 1e6         # the partials and their sum: written once, read once
        rec = {"part": "kernels", "down": d, "launches": launches, "fwd_us": round(timed(fwd, launches), 2), "bwd_us": round(timed(bwd, launches), 2),
               "fwd_read_MB": round(read_mb, 2), "fwd_partials_written_MB": round(part_mb, 2), "fwd_partials_read_MB": round(part_mb, 2),
               "fwd_floor_us": round((read_mb + 2 * part_mb) / HBM_TBPS, 2), "bwd_read_MB": round(read_mb, 2), "bwd_written_MB": round(full_mb, 2),
               "bwd_floor_us": round((read_mb + full_mb) / HBM_TBPS, 2), "loss": float(loss)}
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(launches):
                    fwd()
                    bwd()
                torch.cuda.synchronize()
            for ev in prof.key_averages():
                for name in ("coral_gram_k", "coral_sum_k", "coral_finish_k", "coral_bwd_k"):
                    if name in ev.key:
                        rec[name + "_us"] = round(getattr(ev, "device_time_total", getattr(ev, "cuda_time_total", 0.0)) / max(ev.count, 1), 2)
        except Exception as e:      # (the split is a convenience: the event timings above stand without it)
            rec["profiler"] = f"unavailable: {type(e).__name__}"
        print(json.dumps(rec), flush=True)
    if "torch" in parts:
        n = N
        hc = torch.eye(n, device="cuda") - 1.0 / n
        state = {}

        def t_fwd():
            z = torch.cat([down_torch(src, d).reshape(n, -1), down_torch(tgt, d).reshape(n, -1)])
            g = z @ z.T
            gss, gst, gtt = hc @ g[:n, :n] @ hc, hc @ g[:n, n:] @ hc, hc @ g[n:, n:] @ hc
            s = ((gss ** 2).sum() - 2 * (gst ** 2).sum() + (gtt ** 2).sum()) / (n - 1) ** 2
            k = 1.0 / (2 * Dd ** 2 * s.sqrt() * (n - 1) ** 2)
            state["z"], state["coef"] = z, k * torch.cat([torch.cat([gss, -gst], 1), torch.cat([-gst.T, gtt], 1)])
            state["loss"] = s.sqrt() / (4 * Dd ** 2)

        def t_bwd():
            dz = (state["coef"] @ state["z"]).reshape(2 * n, K, H // d, W // d)
            if d == 1:
                state["d"] = dz
                return
            out = torch.zeros(2 * n, K, H, W, device="cuda")
            v = out[..., :H // d * d, :W // d * d].reshape(2 * n, K, H // d, d, W // d, d)
            if d % 2:
                v[:, :, :, d // 2, :, d // 2] = dz
            else:
                for a in (d // 2 - 1, d // 2):
                    for b in (d // 2 - 1, d // 2):
                        v[:, :, :, a, :, b] = 0.25 * dz
            state["d"] = out

        t_fwd()
        rec = {"part": "torch", "down": d, "launches": launches, "fwd_us": round(timed(t_fwd, launches), 2), "bwd_us": round(timed(t_bwd, launches), 2),
               "loss": float(state["loss"])}
        print(json.dumps(rec), flush=True)


def step_part(a):
    S = 256
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=0)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    args = (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])
    torch.manual_seed(0)
    sd = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False).state_dict()
    runs = {}
    for variant in ("default", "coral_d1", "coral_d2"):
        stu = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
        tea = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
        stu.load_state_dict(sd)
        tea.load_state_dict(sd)
        tr = MeanTeacherTrainer(stu.cuda(), tea.cuda(), lr=1e-4, precision="bf16")
        if variant != "default":
            tr.coral_criterion, tr.lambda_coral = GramCoralLoss(int(variant[-1])), 0.5
        runs[variant] = (GraphedTrainStep(tr, *args, warmup=a.warmup), [])
    for _ in range(a.rounds):
        for variant, (gs, times) in runs.items():
            for _ in range(a.warmup):
                gs.step(*args)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                gs.step(*args)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3 / a.steps)
    for variant, (gs, times) in runs.items():
        ms = sorted(times)[len(times) // 2]
        losses = {k: float(v) for k, v in gs.out.items() if k.startswith("loss")}
        print(json.dumps({"part": "step", "criteria": variant, "N": N, "res": S, "mode": "captured", "ms_per_step": round(ms, 3),
                          "rounds_ms": [round(t, 3) for t in times], "last_losses": losses}), flush=True)
        gs.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernels,torch,step")
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    parts = a.parts.split(",")
    for d in (1, 2):
        kernels_and_torch(d, a.launches, parts)
    if "step" in parts:
        step_part(a)


if __name__ == "__main__":
    main()
