"""Dev tool: ms per step of the benched step (PoseResNet-101, bf16, N = 32, one hipGraph) under the tail's two switches, ONE variant per
process (variants captured side by side in one process do not time alike: the first graph built ran 0.25 ms faster than three later ones,
whatever their switches) - alternate the variants from the shell on one box.

usage: python tools/ab_tail_parts.py <wgrad_order 0|1> <sum_splits_in_tail 0|1> [rounds, default 3] [steps per round, default 60]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uda_poseestimation_amd.lib.models as models   # noqa: E402
from uda_poseestimation_amd import synthetic   # noqa: E402
from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer   # noqa: E402


def main():
    order, defer = int(sys.argv[1]), int(sys.argv[2])
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 60
    b = synthetic.mean_teacher_batch(32, num_keypoints=16, image_size=256, heatmap_size=64, sigma=2, seed=0)
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    g = (d["x_s"], d["label_s"], d["weight_s"], d["x_t_stu"], d["x_t_tea"], d["aug_param_stu"], d["aug_param_tea"])
    torch.manual_seed(0)
    stu = models.pose_resnet101(num_keypoints=16, pretrained_backbone=False).cuda()
    tea = models.pose_resnet101(num_keypoints=16, pretrained_backbone=False).cuda()
    stu.policy["wgrad_order"] = order
    tr = MeanTeacherTrainer(stu, tea, lr=1e-4, teacher_alpha=0.999, lambda_c=1.0, mask_ratio=0.5, sigma=2, image_size=256, heatmap_size=64, precision="bf16")
    tr.sum_splits_in_tail = bool(defer)
    gs = GraphedTrainStep(tr, *g)
    assert (stu.split_sums_deferred > 0) == bool(defer)
    for _ in range(150):          # clock ramp
        gs.step(*g)
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(steps):
            gs.step(*g)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    print(f"order {order} sum_in_sweep {defer}: " + " ".join(f"{m:.4f}" for m in ms) + f"  mean {sum(ms) / len(ms):.4f} ms/step", flush=True)


if __name__ == "__main__":
    main()
