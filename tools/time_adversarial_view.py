"""Dev tool: what the adversarial target view costs (profiles/adversarial_view.txt).  N = 32, 3 x 256 x 256.
Default: the captured mean-teacher step (PoseResNet-101, bf16) with trainer.adv_eps off and on (one probe), both captured once, alternating
rounds of replays in one process, device time by HIP events, no profiler.
--trace: the launches to read out of a kernel trace, in a run of its own -
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/time_adversarial_view.py --trace
20 calls each of udapose_perturb in its forms (l2 one-step; l2 projected around an x0; linf one launch; linf with gnorm) and 20 of
torch.add(x, g, out=out) on the same tensors (the add moves the bytes of the one-step apply launch: two streams in, one out).
usage: python tools/time_adversarial_view.py [--trace] [--steps 30] [--rounds 5] [--adv-steps 1]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--adv-steps", type=int, default=1)
    a = ap.parse_args()
    import torch
    import uda_poseestimation_amd.lib.models as models
    from uda_poseestimation_amd import adversarial, synthetic
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    N, S, K = 32, 256, 16
    eps = 0.05 * (3 * S * S) ** 0.5
    torch.manual_seed(0)
    if a.trace:
        x, g = torch.randn(N, 3, S, S, device="cuda"), torch.randn(N, 3, S, S, device="cuda")
        x0 = x - 0.01 * torch.randn_like(x)
        out = torch.empty_like(x)
        e, st = torch.tensor(eps, device="cuda"), torch.tensor(1.5 * eps, device="cuda")
        forms = {"l2 one-step": lambda: adversarial.perturb(x, g, e, "l2", out=out, want_norm=True),
                 "l2 projected": lambda: adversarial.perturb(x, g, e, "l2", x0=x0, step=st, out=out, want_norm=True),
                 "linf": lambda: adversarial.perturb(x, g, e, "linf", out=out),
                 "linf with gnorm": lambda: adversarial.perturb(x, g, e, "linf", out=out, want_norm=True),
                 "torch.add": lambda: torch.add(x, g, out=out)}
        for fn in forms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for name, fn in forms.items():
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            print(f"{name}: 20 calls done", flush=True)
        return
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=0)
    gd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    args = (gd["x_s"], gd["label_s"], gd["weight_s"], gd["x_t_stu"], gd["x_t_tea"], gd["aug_param_stu"], gd["aug_param_tea"])
    sd = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False).state_dict()
    steps = {}
    for on in (False, True):
        stu = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
        tea = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
        stu.load_state_dict(sd)
        tea.load_state_dict(sd)
        tr = MeanTeacherTrainer(stu.cuda(), tea.cuda(), lr=1e-4, precision="bf16")
        if on:
            tr.adv_eps, tr.adv_steps = eps, a.adv_steps
        steps[on] = GraphedTrainStep(tr, *args, warmup=3)
        for _ in range(10):
            steps[on].step(*args)
        torch.cuda.synchronize()
        print(f"adv_eps {'on' if on else 'off'}: captured ({'one graph' if steps[on].one_graph else 'split'})", flush=True)
    res = {False: [], True: []}
    for _ in range(a.rounds):
        for on in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                steps[on].step(*args)
            e1.record()
            torch.cuda.synchronize()
            res[on].append(e0.elapsed_time(e1) / a.steps)
    for on in (False, True):
        v = res[on]
        print(f"captured step, PoseResNet-101 bf16 N={N} {S}x{S}, adv_eps {'on (' + str(a.adv_steps) + ' probe(s))' if on else 'off'}: "
              f"median {statistics.median(v):.3f} ms, min {min(v):.3f} ms, spread {max(v) - min(v):.3f} ms over {a.rounds} alternating rounds of "
              f"{a.steps} replays ({' '.join(f'{t:.3f}' for t in v)})", flush=True)
    print(f"on - off (medians): {statistics.median(res[True]) - statistics.median(res[False]):+.3f} ms per step")
    for s_ in steps.values():
        s_.release()


if __name__ == "__main__":
    main()
