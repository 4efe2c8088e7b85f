"""ms per batch of engine.validate() with and without the flip test (PoseResNet-101, K = 16, N = 32, 256x256, 'auto' precision: the
f16x2 evaluation forward on forward-only plans, BatchNorm folded), on a synthetic list of device-resident batches:
    plain    validate(batches, model)                              (runs on a tree without the flip test as well: the yardstick)
    two      validate_flip(batches, model, "body16"), two forwards of N
    batched  the same with one forward of the 2N batch [x; mirror(x)]
The variants live in one process and are timed in alternation (host clock around a validate() call, which ends in its read-back), the
median of the rounds is reported.  --check first compares the heat-maps of the 2N forward, image for image and bit for bit, with two
forwards of N (at the timed shape and at the test shape: pose_resnet50, N = 2, 64x64).  --kernels times udapose_hflip_batch and
udapose_flip_merge alone (device events around a run of launches).  One JSON line per result.
usage: python tools/time_flip_test.py [--variants plain,two,batched] [--batches 8] [--rounds 5] [--warmup 1] [--check] [--kernels]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uda_poseestimation_amd import engine, synthetic  # noqa: E402
import uda_poseestimation_amd.lib.models as models  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def trained_stats(net, x):
    """Running statistics of one train-mode forward, so that the folded eval-mode BatchNorm is not the identity."""
    net.train()
    net.bn_momentum = 1.0
    with torch.no_grad():
        net(x)
    net.bn_momentum = 0.1
    net.eval()
    net._handles.clear()


def check_batched(arch, N, S, K=16):
    from uda_poseestimation_amd import ops
    torch.manual_seed(0)
    net = getattr(models, arch)(num_keypoints=K, pretrained_backbone=False).cuda()
    torch.nn.init.normal_(net.head.weight, std=0.05)
    x = synthetic.images(N, S, 5).cuda()
    trained_stats(net, x)
    with torch.no_grad():
        y, yf = net(x), net(ops.hflip_batch(x))
        y2 = net(ops.hflip_batch(x, keep_original=True))
    torch.cuda.synchronize()
    same = [bool(torch.equal(y2[i], y[i])) for i in range(N)] + [bool(torch.equal(y2[N + i], yf[i])) for i in range(N)]
    emit(check="2N forward vs two forwards, bit for bit", arch=arch, N=N, res=S, images_equal=sum(same), images=2 * N,
         max_abs_diff=float(torch.maximum((y2[:N] - y).abs().max(), (y2[N:] - yf).abs().max())), max_abs=float(y.abs().max()))
    return all(same)


def time_kernels(N, K, S):
    from uda_poseestimation_amd import ops
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    x = synthetic.images(N, S, 1).cuda()
    a, f = torch.randn(N, K, S // 4, S // 4, device="cuda"), torch.randn(N, K, S // 4, S // 4, device="cuda")
    perm = kd._perm_device("body16", K, a.device)
    calls = {"hflip_batch keep_original=0": lambda: ops.hflip_batch(x), "hflip_batch keep_original=1": lambda: ops.hflip_batch(x, True),
             "flip_merge mode 1 + decode": lambda: kd._flip_merge(a, f, perm, False, True, out=a),
             "flip_merge mode 1 + shift + decode": lambda: kd._flip_merge(a, f, perm, True, True, out=a),
             "heatmap_argmax (for scale)": lambda: kd._decode(a)}
    for name, fn in calls.items():
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                fn()
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) * 10.0)
        emit(kernel=name, N=N, K=K, res=S, us_per_call_incl_launch=round(sorted(runs)[2], 2), runs_us=[round(r, 2) for r in runs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="plain,two,batched")
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--arch", default="pose_resnet101")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    N, K, S = a.N, 16, a.res
    emit(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
    if a.check:
        check_batched("pose_resnet50", 2, 64)
        check_batched(a.arch, N, S)
    if a.kernels:
        time_kernels(N, K, S)
    variants = [v for v in a.variants.split(",") if v]
    if not variants:
        return
    torch.manual_seed(0)
    net = getattr(models, a.arch)(num_keypoints=K, pretrained_backbone=False).cuda()
    torch.nn.init.normal_(net.head.weight, std=0.05)
    batches = []
    for i in range(a.batches):
        b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=i)
        batches.append((b["x_s"].cuda(), b["label_s"].cuda(), b["weight_s"].cuda()))
    trained_stats(net, batches[0][0])

    def run(variant):
        if variant == "plain":
            return engine.validate(batches, net)
        engine.FLIP_FORWARD_FORM = variant
        return engine.validate_flip(batches, net, "body16")

    times, results, first = {v: [] for v in variants}, {}, {}
    for v in variants:          # (the first call of a variant creates its executor plan and uploads its tables: timed apart)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        results[v] = run(v)
        first[v] = ((time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated() / 2 ** 30)
    for _ in range(a.rounds):
        for v in variants:
            for _ in range(a.warmup):
                run(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run(v)
            times[v].append((time.perf_counter() - t0) * 1e3 / len(batches))
            assert out == results[v], f"{v}: validate() is not repeatable"
    for v in variants:
        ms = sorted(times[v])[len(times[v]) // 2]
        emit(variant=v, arch=a.arch, N=N, res=S, batches=len(batches), ms_per_batch=round(ms, 3), rounds_ms=[round(t, 3) for t in times[v]],
             first_call_ms=round(first[v][0], 1), peak_allocated_gb_first_call=round(first[v][1], 2),
             mean_pck=round(sum(results[v][0]) / K, 4), loss=results[v][1])
    if "two" in results and "batched" in results:
        emit(two_equals_batched=bool(results["two"] == results["batched"]))


if __name__ == "__main__":
    main()
