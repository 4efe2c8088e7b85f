"""What merging the teacher's views costs on one MI355X at B = 32, K = 16, 64x64 maps with k = 2 and 4 views: udapose_view_merge in mode
"mean" (one pass: peaks and the plain mean), in mode "trimmed" (two passes: peaks, then the mean of the inliers) and in mode "trimmed" with
the energy, beside udapose_mean_views, the launch it replaces (csrc/affine.hip, untouched by the merge).  The four calls alternate inside
every round, --rounds rounds of --launches back-to-back launches each between two device events (launch included); one JSON line per k with
the median over the rounds and every round's figure.  Kernel-only times: this script under `rocprofv3 --kernel-trace --stats`, in a run of
its own (kernel names view_merge_k<VEC, KM, U>, mean_views_k).
usage: python tools/time_view_merge.py [--launches 200] [--rounds 7]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uda_poseestimation_amd import _hip  # noqa: E402
from uda_poseestimation_amd._hip import lib, ptr  # noqa: E402


def heatmaps(B, K, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.arange(H).view(1, 1, H, 1).float(), torch.arange(W).view(1, 1, 1, W).float()
    cy, cx = 4 + torch.rand(B, K, 1, 1, generator=g) * (H - 9), 4 + torch.rand(B, K, 1, 1, generator=g) * (W - 9)
    return (torch.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / 8.0) + 0.02 * torch.randn(B, K, H, W, generator=g)).cuda()


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches       # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    L, st = lib(), _hip.stream()
    B, K, H, W = 32, 16, 64, 64
    R = B * K
    for k in (2, 4):
        views = [heatmaps(B, K, H, W, 10 * k + v) for v in range(k)]
        arr = (C.c_void_p * k)(*[v.data_ptr() for v in views])
        rad = torch.tensor(2.0, device="cuda")
        mean = torch.empty(B, K, H, W, device="cuda")
        peaks = torch.empty(k, R, 2, dtype=torch.int32, device="cuda")
        maxv = torch.empty(k, R, device="cuda")
        inl, n_in, spread = (torch.empty(R, dtype=torch.int32, device="cuda") for _ in range(3))
        agree, energy = torch.empty(R, device="cuda"), torch.empty(R, device="cuda")

        def merge(mode, want_energy):
            return L.udapose_view_merge(st, arr, k, R, H, W, mode, ptr(rad), k, ptr(mean), ptr(peaks), ptr(maxv), ptr(inl), ptr(n_in), ptr(spread),
                                        ptr(agree), ptr(energy) if want_energy else None)

        calls = {"mean_views_us": lambda: L.udapose_mean_views(st, arr, k, ptr(mean), mean.numel()),
                 "merge_mean_us": lambda: merge(0, False),
                 "merge_trimmed_us": lambda: merge(1, False),
                 "merge_trimmed_energy_us": lambda: merge(1, True)}
        for fn in calls.values():
            assert fn() == 0
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        runs = {name: [] for name in calls}
        for _ in range(a.rounds):
            for name, fn in calls.items():
                runs[name].append(round(timed(fn, a.launches), 2))
        rec = {"B": B, "K": K, "H": H, "W": W, "k": k, "launches": a.launches, "rounds": a.rounds, "views_MB": round(k * mean.numel() * 4 / 1e6, 2)}
        rec.update({name: round(statistics.median(v), 2) for name, v in runs.items()})
        rec["inlier_share"] = round(float(n_in.float().mean()) / k, 3)
        rec["runs_us"] = runs
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
