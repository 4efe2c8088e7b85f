"""Histogram-matching and colour-statistics style transfer against their byte time, and the captured BASELINE.json configs[2]-shaped step with them.

--kernels   udapose_pixel_summary over TWO batches and ONE udapose_pixel_transfer per mode at N x 3 x S x S (default 32 x 3 x 256 x 256), HIP events
            around the launches: `warm` = repeated back to back, `cold` = a 512 MB fill in front of every timed launch; medians of --reps, rounds
            alternate the cases, spread = max - min of the round medians.  Bytes that must move: the summary reads both batches once (2 N 3 S S 4),
            one transfer reads the content and writes the output (the same).  --images: `bytes` (uniform random bytes through the normalisation, the
            worst case for the LDS histogram) or `flat` (half of every image one level: the wave-aggregated add).  For per-kernel durations run this
            mode alone under `rocprofv3 --kernel-trace --stats -- python tools/time_pixel_style.py --kernels --reps 20 --rounds 1`.
--step      ms per captured step (PoseResNet-101, K = 16, N = 32, 256 x 256, bf16; both style directions forced on with alpha 0.5, adaptive occlusion on
            the device - bench.py's configs[2] leg) with style_net = PixelStyleNet(mode) for each --modes and FDANet(--beta), each built fresh, timed in
            alternation over --rounds rounds in one process.
usage: python tools/time_pixel_style.py [--kernels] [--step] [--modes hist meanstd cholesky] [--beta 0.01] [--reps 50] [--rounds 3] [--steps 50]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _images(a, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 256, (a.N, 3, a.res, a.res), generator=g)
    if a.images == "flat":
        b[:, :, : a.res // 2] = 0
    m, s = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    return ((b.float() / 255.0 - m) / s).cuda()


def kernels(a):
    import torch
    from uda_poseestimation_amd.lib.models import pixel_style as ps
    x_s, x_t = _images(a, 0), _images(a, 1)
    out = torch.empty_like(x_s)
    flush = torch.empty(128 << 20, dtype=torch.float32, device="cuda")
    nbytes = 4 * x_s.numel()
    nets = {m: ps.PixelStyleNet(m, MEAN, STD) for m in a.modes}
    first = nets[a.modes[0]]
    sum_s, sum_t = first.summary(x_s), first.summary(x_t)

    def summaries():
        first.summary(x_s, out=sum_s)
        first.summary(x_t, out=sum_t)
    cases = {"summary x2": (summaries, 2 * nbytes)}
    for m, net in nets.items():
        cases[f"transfer {m}"] = (lambda net=net: net.transfer(x_s, sum_s, sum_t, 0.5, out=out), 2 * nbytes)

    def median_us(fn, cold):
        ts = []
        for _ in range(a.reps):
            if cold:
                flush.fill_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return sorted(ts)[len(ts) // 2]

    for fn, _ in cases.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.rounds):
        for cold in (False, True):
            for name, (fn, _) in cases.items():
                res.setdefault((name, cold), []).append(median_us(fn, cold))
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({"N": a.N, "res": a.res, "images": a.images, "bytes_per_batch": nbytes, "reps": a.reps, "rounds": a.rounds}))
    for (name, cold), v in res.items():
        m = med(v)
        print(json.dumps({"case": name, "cache": "cold" if cold else "warm", "median_us": round(m, 2), "spread_us": round(max(v) - min(v), 2),
                          "bytes": cases[name][1], "GB_per_s": round(cases[name][1] / m / 1e3, 1), "round_medians_us": [round(x, 2) for x in v]}), flush=True)


def step(a):
    import numpy as np
    import torch
    from uda_poseestimation_amd import synthetic
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    from uda_poseestimation_amd.lib.models import fda, pixel_style as ps
    import uda_poseestimation_amd.lib.models as models
    N, K, S = a.N, 16, a.res
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=0)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    args = (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])
    torch.manual_seed(0)
    sd = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False).state_dict()
    lo, hi = torch.tensor([-2.1179, -2.0357, -1.8044]).cuda(), torch.tensor([2.2489, 2.4285, 2.64]).cuda()

    def style(which):
        return fda.FDANet(a.beta, MEAN, STD) if which == "fda" else ps.PixelStyleNet(which, MEAN, STD)

    legs = {}
    for _ in range(a.rounds):
        for which in list(a.modes) + ["fda"]:
            stu = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
            tea = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
            stu.load_state_dict(sd); tea.load_state_dict(sd)
            tr = MeanTeacherTrainer(stu.cuda(), tea.cuda(), lr=1e-4, image_size=S, heatmap_size=S // 4, precision="bf16", style_net=style(which),
                                    recover=(lo, hi), s2t_freq=1.0, t2s_freq=1.0, s2t_alpha=(0.5, 0.5), t2s_alpha=(0.5, 0.5),
                                    rng=np.random.RandomState(0), occlude_rate=0.5, occlude_thresh=0.9, occlude_size=10)
            tr.device_occlusion = True
            gs = GraphedTrainStep(tr, *args, warmup=3)
            for _ in range(10):
                gs.step(*args)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                gs.step(*args)
            torch.cuda.synchronize()
            legs.setdefault(which, []).append(round((time.perf_counter() - t0) * 1e3 / a.steps, 4))
            gs.release()
            del gs, tr, stu, tea
            torch.cuda.empty_cache()
    print(json.dumps({"captured_step_ms": legs, "N": N, "res": S, "steps": a.steps, "beta": a.beta,
                      "spread_ms": {k: round(max(v) - min(v), 4) for k, v in legs.items()},
                      "img_per_s": {k: round(N / (min(v) * 1e-3), 1) for k, v in legs.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--modes", nargs="+", default=["hist", "meanstd", "cholesky"], choices=["hist", "meanstd", "cholesky"])
    ap.add_argument("--images", default="bytes", choices=["bytes", "flat"])
    ap.add_argument("--beta", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    a = ap.parse_args()
    if a.kernels:
        kernels(a)
    if a.step:
        step(a)


if __name__ == "__main__":
    main()
