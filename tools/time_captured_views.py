"""What k teacher views cost in the captured step against the eager step on one MI355X, at the shape of BASELINE.json configs[1]
(PoseResNet-101 student + teacher, N = 32, 256x256, K = 16, bf16): ms per step of GraphedTrainStep.step and of trainer.train_step at
k = 2 and k = 3, with trainer.view_merge off and "trimmed".  Every case builds its own networks; --rounds rounds of --steps steps each
between two device events, after --warm untimed steps; one JSON line per case with the median over the rounds and every round's figure.
usage: python tools/time_captured_views.py [--steps 30] [--rounds 3] [--k 2 3]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uda_poseestimation_amd.lib.models as models  # noqa: E402
from uda_poseestimation_amd import synthetic  # noqa: E402
from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer  # noqa: E402

N, K, S = 32, 16, 256


def batch(k):
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=0)
    g = {n: (v.cuda() if torch.is_tensor(v) else v) for n, v in b.items()}
    rs = np.random.RandomState(7)
    views = [g["x_t_tea"]] + [synthetic.images(N, S, 50 + i).cuda() for i in range(1, k)]
    augs = [g["aug_param_tea"]] + [synthetic.aug_params(N, rs) for _ in range(1, k)]
    return (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], views, g["aug_param_stu"], augs)


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--k", type=int, nargs="+", default=[2, 3])
    a = ap.parse_args()
    for k in a.k:
        b = batch(k)
        for merge in (None, "trimmed"):
            res = {}
            for form in ("captured", "eager"):
                torch.manual_seed(0)
                stu = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False).cuda()
                tea = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False).cuda()
                tr = MeanTeacherTrainer(stu, tea, lr=1e-4, image_size=S, heatmap_size=S // 4, precision="bf16")
                tr.view_merge, tr.view_min = merge, (2 if merge else None)
                if form == "captured":
                    gs = GraphedTrainStep(tr, *b)
                    fn = lambda: gs.step(None, None, None, None, None, b[5], b[6])      # noqa: E731  (the batch stays; the matrices are restaged)
                else:
                    fn = lambda: tr.train_step(*b)                                     # noqa: E731
                for _ in range(a.warm):
                    fn()
                torch.cuda.synchronize()
                rounds = [round(timed(fn, a.steps), 3) for _ in range(a.rounds)]
                res[form] = {"ms_per_step": round(statistics.median(rounds), 3), "rounds": rounds}
                del fn, tr, stu, tea
                if form == "captured":
                    gs.release()
                    del gs
                torch.cuda.empty_cache()
            print(json.dumps({"k": k, "view_merge": merge, **res}), flush=True)


if __name__ == "__main__":
    main()
