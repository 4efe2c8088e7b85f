"""ms per batch of engine.validate() and of engine.evaluate() (PoseResNet-101, K = 16, N = 32, 256x256, 'auto' precision: the f16x2
evaluation forward on forward-only plans, BatchNorm folded), on a synthetic list of device-resident batches:
    validate   validate(batches, model): PCK@0.05 as a batch-weighted mean   (runs on a tree without evaluate() as well: the yardstick)
    evaluate   evaluate(batches, model, groups="body16"): the 20-threshold curve, AUC, EPE and joint groups from one fused launch per batch
    unfused    evaluate(..., decode=<the arg-max as a callable>): the same report through two arg-max launches and the coordinate launch
The variants live in one process and are timed in alternation (host clock around a call, which ends in its read-back), the median of the
rounds is reported.  --kernels times the launches alone at [N,16,res/4,res/4] (device events around a run of 100 launches, so launch
overhead is in): udapose_heatmap_argmax x 2 + udapose_pck (what validate() issues per batch), udapose_pck_accumulate_heatmaps (what
evaluate() issues), udapose_pck_accumulate, and the Python calls around them (accuracy_device, PCKMeter.update).  One JSON line per result.
usage: python tools/time_eval_report.py [--variants validate,evaluate,unfused] [--batches 8] [--rounds 5] [--warmup 1] [--kernels]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uda_poseestimation_amd import _hip, engine, synthetic  # noqa: E402
from uda_poseestimation_amd.lib import keypoint_detection as kd  # noqa: E402
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


def time_kernels(N, K, S):
    H = W = S // 4
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=H, seed=0)
    t = b["label_s"].cuda().float().contiguous()
    o = (t + 0.1 * torch.randn_like(t)).contiguous()
    L, st, p = _hip.lib(), _hip.stream(), _hip.ptr
    pred, gt = torch.empty(N, K, 2, device="cuda"), torch.empty(N, K, 2, device="cuda")
    maxv, acc, avg_cnt = torch.empty(N, K, 1, device="cuda"), torch.empty(K, device="cuda"), torch.empty(2, device="cuda")

    def three():
        L.udapose_heatmap_argmax(st, p(o), N * K, H, W, p(maxv), None, p(pred), None, None, 0)
        L.udapose_heatmap_argmax(st, p(t), N * K, H, W, p(maxv), None, p(gt), None, None, 0)
        L.udapose_pck(st, p(pred), p(gt), N, K, H / 10.0, W / 10.0, 0.5, p(acc), p(avg_cnt))

    calls = {"heatmap_argmax x 2 + pck (validate's three launches)": three, "accuracy_device (Python call)": lambda: kd.accuracy_device(o, t)}
    if hasattr(kd, "PCKMeter"):
        for T in (1, 20, 64):
            thr = torch.tensor([0.05 * (j + 1) for j in range(T)], device="cuda")
            state = torch.zeros(K, T + 3, dtype=torch.int64, device="cuda")
            calls[f"pck_accumulate_heatmaps T={T} (evaluate's one launch)"] = \
                lambda thr=thr, state=state, T=T: L.udapose_pck_accumulate_heatmaps(st, p(o), p(t), None, N, K, H, W, p(thr), T, p(state), p(pred))
            calls[f"pck_accumulate T={T} (coordinates)"] = \
                lambda thr=thr, state=state, T=T: L.udapose_pck_accumulate(st, p(pred), p(gt), None, None, N, K, H / 10.0, W / 10.0, p(thr), T, p(state))
        meter = kd.PCKMeter(K)
        calls["PCKMeter.update argmax, heat-map targets (Python call)"] = lambda: meter.update(o, t)
        calls["PCKMeter.update quarter, heat-map targets (Python call)"] = lambda: meter.update(o, t, decode="quarter")
    three()
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
        emit(kernel=name, N=N, K=K, map=H, us_per_call_incl_launch=round(sorted(runs)[2], 2), runs_us=[round(r, 2) for r in runs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="validate,evaluate,unfused")
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--arch", default="pose_resnet101")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    N, K, S = a.N, 16, a.res
    emit(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
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
        if variant == "validate":
            acc, loss = engine.validate(batches, net)
            return {"pck@0.5": round(sum(acc) / K, 6), "loss": loss}
        rep = engine.evaluate(batches, net, groups="body16", decode="argmax" if variant == "evaluate" else kd._decode)
        return {"pck@0.5": round(float(rep["pck_mean"][9]), 6), "auc": round(rep["auc"], 6), "epe": round(rep["epe_mean"], 4), "loss": rep["loss"],
                "wrist@0.5": round(float(rep["groups"]["wrist"]["pck"][9]), 6)}

    times, results, first = {v: [] for v in variants}, {}, {}
    for v in variants:          # (the first call of a variant creates its executor plan and uploads its tables: timed apart)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        results[v] = run(v)
        first[v] = (time.perf_counter() - t0) * 1e3
    for _ in range(a.rounds):
        for v in variants:
            for _ in range(a.warmup):
                run(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run(v)
            times[v].append((time.perf_counter() - t0) * 1e3 / len(batches))
            assert out == results[v], f"{v}: not repeatable"
    for v in variants:
        ms = sorted(times[v])[len(times[v]) // 2]
        emit(variant=v, arch=a.arch, N=N, res=S, batches=len(batches), ms_per_batch=round(ms, 3), rounds_ms=[round(t, 3) for t in times[v]],
             first_call_ms=round(first[v], 1), **results[v])


if __name__ == "__main__":
    main()
