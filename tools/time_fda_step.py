"""Fourier-domain style transfer against its byte time, and the captured BASELINE.json configs[2]-shaped step with three style bridges.

--kernels   udapose_fda_spectrum over TWO batches and ONE udapose_fda_apply at N x 3 x S x S (default 32 x 3 x 256 x 256) for each --b, HIP events
            around the launches: `warm` = repeated back to back, `cold` = a 512 MB fill in front of every timed launch; medians of --reps, rounds
            alternate the cases, spread = max - min of the round medians.  Bytes that must move: the spectrum reads both batches once (2 N 3 S S 4),
            one apply reads the content and writes the output (the same).  For per-kernel durations run this mode alone under
            `rocprofv3 --kernel-trace --stats -- python tools/time_fda_step.py --kernels --reps 20 --rounds 1`.
--step      ms per captured step (PoseResNet-101, K = 16, N = 32, 256 x 256, bf16; both style directions forced on with alpha 0.5, adaptive occlusion on
            the device - bench.py's configs[2] leg) with style_net = FDANet(--beta), None, and the AdaIN Net (seeded random weights, 'bf16' as in that
            leg), each built fresh, timed in alternation over --rounds rounds in one process.
usage: python tools/time_fda_step.py [--kernels] [--step] [--b 2 23] [--beta 0.09] [--reps 50] [--rounds 3] [--steps 50]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def kernels(a):
    import torch
    from uda_poseestimation_amd.lib.models import fda
    N, S = a.N, a.res
    g = torch.Generator().manual_seed(0)
    x_s, x_t = torch.randn(N, 3, S, S, generator=g).cuda(), torch.randn(N, 3, S, S, generator=g).cuda()
    out = torch.empty_like(x_s)
    flush = torch.empty(128 << 20, dtype=torch.float32, device="cuda")
    nbytes = 4 * x_s.numel()
    cases = {}
    for b in a.b:
        sp_s, sp_t = fda.low_freq_spectrum(x_s, b), fda.low_freq_spectrum(x_t, b)
        net = fda.FDANet((b + 0.5) / S, MEAN, STD)
        assert net.window_of(x_s) == b

        def spectra(b=b, sp_s=sp_s, sp_t=sp_t):
            fda.low_freq_spectrum(x_s, b, out=sp_s)
            fda.low_freq_spectrum(x_t, b, out=sp_t)
        cases[f"spectrum x2 b={b}"] = (spectra, 2 * nbytes)
        cases[f"apply b={b}"] = (lambda net=net, sp_s=sp_s, sp_t=sp_t: net.transfer(x_s, sp_s, sp_t, 0.5, out=out), 2 * nbytes)

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
    print(json.dumps({"N": N, "res": S, "bytes_per_batch": nbytes, "reps": a.reps, "rounds": a.rounds}))
    for (name, cold), v in res.items():
        m = med(v)
        print(json.dumps({"case": name, "cache": "cold" if cold else "warm", "median_us": round(m, 2), "spread_us": round(max(v) - min(v), 2),
                          "bytes": cases[name][1], "GB_per_s": round(cases[name][1] / m / 1e3, 1), "round_medians_us": [round(x, 2) for x in v]}), flush=True)


def step(a):
    import numpy as np
    import torch
    from uda_poseestimation_amd import synthetic
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    from uda_poseestimation_amd.lib.models import Style_net, fda
    import uda_poseestimation_amd.lib.models as models
    N, K, S = a.N, 16, a.res
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=0)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    args = (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])
    torch.manual_seed(0)
    sd = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False).state_dict()
    lo, hi = torch.tensor([-2.1179, -2.0357, -1.8044]).cuda(), torch.tensor([2.2489, 2.4285, 2.64]).cuda()

    def style(which):
        if which == "none":
            return None
        if which == "fda":
            return fda.FDANet(a.beta, MEAN, STD)
        torch.manual_seed(1)
        Style_net.vgg.cuda(); Style_net.decoder.cuda()
        net = Style_net.Net(torch.nn.Sequential(*list(Style_net.vgg.children())[:31]), Style_net.decoder).cuda()
        net.precision = "bf16"
        return net

    legs = {}
    for _ in range(a.rounds):
        for which in ("fda", "none", "adain"):
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
    print(json.dumps({"captured_step_ms": legs, "N": N, "res": S, "steps": a.steps, "beta": a.beta, "b": fda.window(S, S, a.beta),
                      "img_per_s": {k: round(N / (min(v) * 1e-3), 1) for k, v in legs.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--b", type=int, nargs="+", default=[2, 23])
    ap.add_argument("--beta", type=float, default=0.09)
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
