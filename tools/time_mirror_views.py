"""Dev tool: what mirrored views cost (profiles/mirror_views.txt).  One process, meant to run under a kernel trace without counters:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/time_mirror_views.py
    python tools/time_mirror_views.py --digest OUT
1. Launches: 20 calls each of the plain and the mirrored form (half the flags set, the "body16" permutation) of the nearest forward, the
   deterministic nearest backward, the bilinear forward and the bilinear backward at [32,16,64,64], and of udapose_aug_hflip_u8 at
   [32,256,256,3] beside udapose_aug_affine_u8 on the same bytes; their durations are read out of the trace (--digest: plain and mirrored forms are
   different kernels, so their rows are told apart by name).
2. The captured mean-teacher step (PoseResNet-101, bf16, N = 32, 256 x 256) built with trainer.flip_pairs = "body16" and replayed with half
   the flags set, against the same step built without: both captured once, alternating rounds of replays, device time by HIP events.
usage: python tools/time_mirror_views.py [--steps 30] [--rounds 3] [--skip-step] [--digest DIR]"""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("warp_chain_k", "warp_chain_bwd_det_k", "bilin_chain_lds_k", "aug_hflip_u8_k", "aug_affine_u8_k")


def digest(d):
    """Per kernel of part 1: the 20 calls after the first 3 of the process, out of the trace's own rows in start order - the captured step
    of part 2 launches the nearest kernels too (later in the run, beside other work), and the trace's statistics file mixes them in."""
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        print(f"no *kernel_trace.csv under {d}")
        return 1
    calls = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"]
            if any(k in name for k in KERNELS):
                calls.setdefault(name, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for name in sorted(calls):
        rows = sorted(calls[name])[3:23]
        us = [(e - s) / 1e3 for s, e in rows]
        print(f"{len(us)} calls (of {len(calls[name])} in the run)  mean {statistics.mean(us):8.2f} us  min {min(us):8.2f}  max {max(us):8.2f}  {name}")
    return 0


def launches():
    import torch
    from uda_poseestimation_amd import synthetic, warp
    from uda_poseestimation_amd.data_gpu import TargetViewPipeline, ViewConfig
    import numpy as np
    import random
    N, C, H = 32, 16, 64
    x = torch.randn(N, C, H, H, device="cuda")
    th = warp.recon_thetas(synthetic.aug_params(N, np.random.RandomState(0)), N, 4.0, "cuda")
    mirror = torch.tensor([i % 2 for i in range(N)], dtype=torch.uint8, device="cuda")
    perm = warp.mirror_perm("body16", C, "cuda")
    for mode in warp.MODES:
        for mir in (None, mirror):
            xg = x.clone().requires_grad_(True)
            for it in range(23):                   # 3 untimed, 20 for the statistics (the trace counts all 23)
                out = warp.warp_chain(xg, th, mode, mir, perm if mir is not None else None)
                out.backward(x)
            torch.cuda.synchronize()
            print(f"{mode} {'mirrored' if mir is not None else 'plain'}: 23 forward + backward calls done", flush=True)
    pipe = TargetViewPipeline(image_size=256, heatmap_size=64)
    base = torch.randint(0, 256, (N, 256, 256, 3), dtype=torch.uint8, device="cuda")
    rng = random.Random(0)
    params = [ViewConfig().draw_affine(rng, (256, 256)) for _ in range(N)]
    for _ in range(23):
        pipe.warp_images(pipe.hflip(base, [i % 2 for i in range(N)]), params)
    torch.cuda.synchronize()
    print("u8 flip + affine: 23 calls done", flush=True)


def step(steps_n, rounds):
    import torch
    import uda_poseestimation_amd.lib.models as models
    from uda_poseestimation_amd import synthetic
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    N, S, K = 32, 256, 16
    torch.manual_seed(0)
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=0)
    gd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    flags = torch.tensor([i % 2 for i in range(N)], dtype=torch.int64)
    plain = (gd["x_s"], gd["label_s"], gd["weight_s"], gd["x_t_stu"], gd["x_t_tea"], gd["aug_param_stu"], gd["aug_param_tea"])
    flagged = plain[:5] + (list(gd["aug_param_stu"]) + [flags], list(gd["aug_param_tea"]) + [1 - flags])
    sd = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False).state_dict()
    gs, args = {}, {False: plain, True: flagged}
    for on in (False, True):
        stu = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
        tea = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
        stu.load_state_dict(sd)
        tea.load_state_dict(sd)
        tr = MeanTeacherTrainer(stu.cuda(), tea.cuda(), lr=1e-4, precision="bf16")
        if on:
            tr.flip_pairs = "body16"
        gs[on] = GraphedTrainStep(tr, *plain, warmup=3)
        for _ in range(5):
            gs[on].step(*args[on])
        torch.cuda.synchronize()
        print(f"flip_pairs {'set' if on else 'unset'}: captured ({'one graph' if gs[on].one_graph else 'split'})", flush=True)
    res = {False: [], True: []}
    for _ in range(rounds):
        for on in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps_n):
                gs[on].step(*args[on])
            e1.record()
            torch.cuda.synchronize()
            res[on].append(e0.elapsed_time(e1) / steps_n)
    for on in (False, True):
        v = res[on]
        print(f"captured step, PoseResNet-101 bf16 N={N} {S}x{S}, {'flip_pairs=body16, half the flags set' if on else 'built without flip_pairs'}: "
              f"median {statistics.median(v):.3f} ms, min {min(v):.3f} ms over {rounds} alternating rounds of {steps_n} replays "
              f"({' '.join(f'{t:.3f}' for t in v)})", flush=True)
    print(f"mirrored - plain (medians): {statistics.median(res[True]) - statistics.median(res[False]):+.3f} ms per step", flush=True)
    for g in gs.values():
        g.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--digest", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.digest:
        return digest(a.digest)
    launches()
    if not a.skip_step:
        step(a.steps, a.rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
