"""What the skeleton prior costs on one MI355X at (B,K,H,W) = (32,16,64,64), both modes, with and without `multiply`.  Three parts, one process:
  kernels  udapose_prior_map alone (prior_map_k) and the whole utils.generate_prior_map call (arg-max decode + map), 100 back-to-back launches
           between two device events each
  torch    the reference's expression (utils.py:111-145) in plain torch on the device - the [B,K,K,H,W] distance, Gaussian and weighted product,
           summed over i - timed the same way, and its peak allocation
  step     BASELINE.json configs[1] (PoseResNet-101, bf16, captured GraphedTrainStep) without a prior and with one (default mode and v3), the trainers
           alternated in one process, median of --rounds
One JSON line per measurement; the committed copy is profiles/prior_map.txt.  The floor is issue arithmetic on the shape: per (i, j, pixel) term
one 8-cycle v_exp_f32 and four 4-cycle VALU instructions (subtract, square, scale, multiply-add), 24 issue cycles per wave of 64 pixels, over the
1024 SIMDs of the part at 2.4 GHz.  A per-kernel table comes from running the kernels part alone under `rocprofv3 --kernel-trace --stats`.
usage: python tools/time_prior_map.py [--parts kernels,torch,step] [--launches 100] [--steps 20] [--warmup 3] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uda_poseestimation_amd import _hip, synthetic, utils  # noqa: E402
from uda_poseestimation_amd._hip import lib, ptr  # noqa: E402
from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer  # noqa: E402
import uda_poseestimation_amd.lib.models as models  # noqa: E402

B, K, H, W = 32, 16, 64, 64
SIMDS, GHZ, CYCLES_PER_TERM = 1024, 2.4, 8 + 4 * 4


def heatmaps(seed):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.arange(H).view(1, 1, H, 1).float(), torch.arange(W).view(1, 1, 1, W).float()
    cy, cx = torch.randint(0, H, (B, K, 1, 1), generator=g).float(), torch.randint(0, W, (B, K, 1, 1), generator=g).float()
    return (torch.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / 8.0) + 0.02 * torch.randn(B, K, H, W, generator=g)).cuda()


def tables(seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(K, 2, generator=g) * torch.tensor([W, H]).float()
    mean = (pts[:, None] - pts[None]).norm(dim=-1)
    std = 0.3 + 3.7 * torch.rand(K, K, generator=g)
    return {"mean": mean.cuda(), "std": std.cuda()}


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


def torch_prior_map(prior, preds, gamma=2, sigma=2, epsilon=-10e10, v3=False):
    coords, conf = utils.get_max_preds_torch(preds)
    xx = torch.arange(W, device=preds.device).float().view(1, 1, 1, 1, W)
    yy = torch.arange(H, device=preds.device).float().view(1, 1, 1, H, 1)
    d = torch.sqrt((xx - coords[..., 0].view(B, K, 1, 1, 1)) ** 2 + (yy - coords[..., 1].view(B, K, 1, 1, 1)) ** 2)      # [B,K,1,H,W]
    t = torch.exp(-((d - prior["mean"].view(1, K, K, 1, 1)) ** 2) / (2 * sigma ** 2))                                    # [B,K,K,H,W]
    if v3:
        f = (1 / (1 + prior["std"])).view(1, K, K) * conf.view(B, K, 1)
        return (f.view(B, K, K, 1, 1) * t).sum(1)
    s = -prior["std"] / gamma
    s.fill_diagonal_(epsilon)
    return (torch.softmax(s, 0).view(1, K, K, 1, 1) * t).sum(1)


def kernels_and_torch(launches, parts):
    L = lib()
    preds, prior = heatmaps(1), tables(2)
    terms = B * K * K * H * W
    floor_us = terms / 64 * CYCLES_PER_TERM / SIMDS / (GHZ * 1e3)
    for v3 in (False, True):
        if "kernels" in parts:
            coords, conf = utils.get_max_preds_torch(preds)
            conf = conf.reshape(B, K).contiguous()
            mean_d, w = utils._prior_tables(prior, K, 2, -10e10, v3, preds.device)
            out = torch.empty_like(preds)
            st = _hip.stream()
            rec = {"part": "kernels", "v3": v3, "launches": launches, "terms": terms, "floor_us": round(floor_us, 2)}
            for mult in (False, True):
                k = lambda: L.udapose_prior_map(st, ptr(coords), ptr(conf), ptr(mean_d), ptr(w), ptr(preds) if mult else None, B, K, H, W, 2.0, int(v3), ptr(out))
                f = lambda: utils.generate_prior_map(prior, preds, v3=v3, multiply=mult)
                tag = "multiply" if mult else "map"
                rec[f"prior_map_k_{tag}_us"] = round(timed(k, launches), 2)
                rec[f"generate_prior_map_{tag}_us"] = round(timed(f, launches), 2)
            rec["over_floor"] = round(rec["prior_map_k_map_us"] / floor_us, 2)
            rec["out_MB"] = round(out.numel() * 4 / 1e6, 2)
            print(json.dumps(rec), flush=True)
        if "torch" in parts:
            f = lambda: torch_prior_map(prior, preds, v3=v3)
            want = utils.generate_prior_map(prior, preds, v3=v3)
            got = f()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            us = timed(f, max(launches // 5, 5))
            rec = {"part": "torch", "v3": v3, "launches": max(launches // 5, 5), "us": round(us, 2),
                   "peak_extra_MB": round((torch.cuda.max_memory_allocated() - base) / 1e6, 1),
                   "max_abs_diff_to_kernel": float((got - want).abs().max()), "max_abs": float(want.abs().max())}
            print(json.dumps(rec), flush=True)


def step_part(a):
    S = 256
    b = synthetic.mean_teacher_batch(B, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=0)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    args = (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])
    prior = utils.SkeletonPrior(K, "cuda").update(g["label_s"], g["weight_s"]).finalize()
    torch.manual_seed(0)
    sd = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False).state_dict()
    runs = {}
    for variant in ("default", "prior", "prior_v3"):
        stu = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
        tea = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
        stu.load_state_dict(sd)
        tea.load_state_dict(sd)
        tr = MeanTeacherTrainer(stu.cuda(), tea.cuda(), lr=1e-4, precision="bf16")
        if variant != "default":
            tr.skeleton_prior, tr.prior_v3 = prior, variant.endswith("v3")
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
        print(json.dumps({"part": "step", "prior": variant, "N": B, "res": S, "mode": "captured", "ms_per_step": round(ms, 3),
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
    if "kernels" in parts or "torch" in parts:
        kernels_and_torch(a.launches, parts)
    if "step" in parts:
        step_part(a)


if __name__ == "__main__":
    main()
