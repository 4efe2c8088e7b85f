"""ms per BASELINE.json configs[1] training step (PoseResNet-101, K = 16, N = 32, 256x256, bf16, captured GraphedTrainStep) with the SGD
optimizer (`--SGD`, train_human.py:136-137) and with the default Adam, A/B between two trees: this one and a baseline tree (a checkout of
the parent commit with its own built libraries, as tools/ab_tree.sh uses: tools/_ab/oldtree).  The code under test is never its own
baseline.  Every leg is a fresh child process that imports ONE tree, captures the step, warms up and times `--steps` replays; legs
alternate old / new for `--rounds` rounds on one box.  One JSON line per leg and optimizer, then a summary line per optimizer with the
medians, the difference and the run-to-run spread of each side.
usage: python tools/time_sgd_step.py --baseline tools/_ab/oldtree [--rounds 3] [--steps 300] [--warm 30] [--optimizers sgd,adam]
       (a single leg: python tools/time_sgd_step.py --leg --tree . --optimizers sgd)"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(a):
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    import torch
    from uda_poseestimation_amd import synthetic
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    import uda_poseestimation_amd.lib.models as models
    import uda_poseestimation_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(uda_poseestimation_amd.__file__))) == tree, "the leg imported another tree"
    N, K, S = a.N, 16, 256
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=0)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    args = (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])
    torch.manual_seed(0)
    sd = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False).state_dict()
    for which in a.optimizers.split(","):
        stu = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
        tea = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
        stu.load_state_dict(sd)
        tea.load_state_dict(sd)
        tr = MeanTeacherTrainer(stu.cuda(), tea.cuda(), lr=1e-4, precision="bf16", use_sgd=which == "sgd")
        gs = GraphedTrainStep(tr, *args, warmup=3)
        for _ in range(a.warm):
            gs.step(*args)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            gs.step(*args)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        print(json.dumps({"tree": a.tag or tree, "optimizer": which, "N": N, "res": S, "mode": "captured", "steps": a.steps,
                          "fused_tail": bool(tr.fused_last), "one_graph": bool(gs.one_graph), "ms_per_step": round(ms, 4),
                          "img_per_s": round(N * 1e3 / ms, 1)}), flush=True)
        gs.release()
        del gs, tr, stu, tea
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", default=os.path.join("tools", "_ab", "oldtree"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--optimizers", default="sgd,adam")
    ap.add_argument("--leg-timeout", type=int, default=300)
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    if not os.path.isdir(a.baseline):
        sys.exit(f"no baseline tree at {a.baseline}: check out the parent commit there and build its libraries")
    res = {}
    for r in range(a.rounds):
        for tag, tree in (("old", a.baseline), ("new", HERE)):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--tree", tree, "--tag", tag, "--steps", str(a.steps), "--warm", str(a.warm),
                   "--N", str(a.N), "--optimizers", a.optimizers]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
            if out.returncode != 0:         # (nothing more is started on the device after a leg that failed)
                sys.exit(f"leg {tag} round {r} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
            for line in out.stdout.splitlines():
                if line.startswith("{"):
                    d = json.loads(line)
                    d["round"] = r
                    print(json.dumps(d), flush=True)
                    res.setdefault((d["optimizer"], tag), []).append(d["ms_per_step"])
    med = lambda v: sorted(v)[len(v) // 2]
    for which in a.optimizers.split(","):
        o, n = res[(which, "old")], res[(which, "new")]
        print(json.dumps({"summary": which, "old_ms": o, "new_ms": n, "old_median": med(o), "new_median": med(n),
                          "new_minus_old_ms": round(med(n) - med(o), 4), "new_over_old": round(med(n) / med(o), 5),
                          "old_spread_ms": round(max(o) - min(o), 4), "new_spread_ms": round(max(n) - min(n), 4)}), flush=True)


if __name__ == "__main__":
    main()
