"""What the sub-pixel decodes cost on one MI355X at R = 512 maps of 64x64 (B = 32, K = 16): udapose_heatmap_argmax (the decode they replace),
udapose_refine_decode in quarter mode and in DARK mode (kernel 11; every arg-max of these maps is refinable, so every work-group blurs), and
DARK at 96x96 with kernel 17.  --launches back-to-back launches of each between two device events, one JSON line per measurement.  The
per-kernel table of profiles/dark_decode.txt comes from running this script under `rocprofv3 --kernel-trace --stats`, a run of its own.
usage: python tools/time_dark.py [--launches 100]"""
import argparse
import json
import os
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
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches       # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    a = ap.parse_args()
    L, st = lib(), _hip.stream()
    for (B, K, H, W, kernel) in ((32, 16, 64, 64, 11), (32, 16, 96, 96, 17)):
        hm = heatmaps(B, K, H, W, 1)
        R = B * K
        co, mv = torch.empty(R, 2, device="cuda"), torch.empty(R, device="cuda")
        ix = torch.empty(R, dtype=torch.int32, device="cuda")
        calls = {
            "heatmap_argmax_us": lambda: L.udapose_heatmap_argmax(st, ptr(hm), R, H, W, ptr(mv), ptr(ix), ptr(co), None, None, 0),
            "quarter_us": lambda: L.udapose_refine_decode(st, ptr(hm), R, H, W, 0, 0, 0.0, ptr(co), ptr(mv), ptr(ix)),
            "dark_us": lambda: L.udapose_refine_decode(st, ptr(hm), R, H, W, 1, kernel, 0.0, ptr(co), ptr(mv), ptr(ix)),
        }
        rec = {"R": R, "H": H, "W": W, "kernel": kernel, "launches": a.launches, "map_MB": round(hm.numel() * 4 / 1e6, 2)}
        for name, fn in calls.items():
            assert fn() == 0
            rec[name] = round(timed(fn, a.launches), 2)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
