"""ms per BASELINE.json configs[1] training step (PoseResNet-101, K = 16, N = 32, 256x256, bf16, captured GraphedTrainStep) with the
soft-max criteria - JointsKLLoss(epsilon=1e-6), ConsSoftmaxLoss(), EntLoss() at lambda_ent = 0.1 - next to the default JointsMSELoss /
ConsLoss step.  The two trainers live in one process and are timed in alternation, so that clocks and the machine's load affect them
alike.  One JSON line per variant.  For the new kernels' durations run one variant alone under the profiler:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/time_softmax_losses.py --variants softmax --rounds 1 --steps 5
usage: python tools/time_softmax_losses.py [--steps 20] [--warmup 3] [--rounds 3] [--variants default,softmax]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uda_poseestimation_amd import synthetic  # noqa: E402
from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer  # noqa: E402
from uda_poseestimation_amd.lib.models.loss import ConsSoftmaxLoss, EntLoss, JointsKLLoss  # noqa: E402
import uda_poseestimation_amd.lib.models as models  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--variants", default="default,softmax")
    a = ap.parse_args()
    N, K, S = a.N, 16, 256
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=0)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    args = (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])
    torch.manual_seed(0)
    sd = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False).state_dict()
    runs = {}
    for variant in a.variants.split(","):
        kw = {} if variant == "default" else dict(criterion=JointsKLLoss(epsilon=1e-6), con_criterion=ConsSoftmaxLoss(), ent_criterion=EntLoss(),
                                                  lambda_ent=0.1)
        stu = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
        tea = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
        stu.load_state_dict(sd)
        tea.load_state_dict(sd)
        tr = MeanTeacherTrainer(stu.cuda(), tea.cuda(), lr=1e-4, precision="bf16", **kw)
        runs[variant] = (GraphedTrainStep(tr, *args, warmup=a.warmup), [])
    for _ in range(a.rounds):
        for variant, (gs, times) in runs.items():
            for _ in range(a.warmup):
                gs.step(*args)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                out = gs.step(*args)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3 / a.steps)
    for variant, (gs, times) in runs.items():
        ms = sorted(times)[len(times) // 2]
        losses = {k: float(v) for k, v in gs.out.items() if k.startswith("loss")}
        print(json.dumps({"criteria": variant, "N": N, "res": S, "mode": "captured", "ms_per_step": round(ms, 3),
                          "img_per_s": round(N * 1e3 / ms, 1), "rounds_ms": [round(t, 3) for t in times], "last_losses": losses}), flush=True)
        gs.release()


if __name__ == "__main__":
    main()
