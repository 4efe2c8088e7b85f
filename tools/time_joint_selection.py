"""Cost of the joint-selection kernels (csrc/select.hip) beside what they stand next to (profiles/joint_selection.txt).

  --case ohkm | mse           forward + backward of JointsOHKMMSELoss(8) | JointsMSELoss() at N = 32, K = 16, 64x64
  --case masks32 | masks256   utils.confidence_mask in its three modes on given confidences, local batch 32, pool 32 | 256
Each case alone under `rocprofv3 --kernel-trace --stats -- python tools/time_joint_selection.py --case ...` gives per-kernel durations
(the kernels' names are the stable part: sqdiff_rows_k, mean_rows_k, topk_select_k, sqdiff_bwd_k, kth_mask_k, joint_kth_mask_k, thr_mask_k).
  --events                    no profiler: HIP events around `reps` back-to-back calls of each of the above, alternated over `rounds`
                              rounds; us per call (median of the rounds, and max - min of them).  A call here is the whole Python call:
                              for kernels of a few microseconds the figure is the host's launch rate, not device time - it says what a
                              user of the eager classes pays, the kernel trace says what a captured step pays.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, K, H, W = 32, 16, 64, 64


def _loss_inputs():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(N, K, H, W, generator=g) * 0.5).cuda().requires_grad_(True)
    t = torch.rand(N, K, H, W, generator=g).cuda()
    w = (torch.rand(N, K, 1, generator=g) > 0.25).float().cuda()
    return x, t, w


def _loss_call(crit, x, t, w):
    def call():
        (g,) = torch.autograd.grad(crit(x, t, w), x)
        return g
    return call


def _mask_calls(n_pool):
    from uda_poseestimation_amd import utils
    g = torch.Generator().manual_seed(1)
    pool = torch.rand(n_pool, K, generator=g).cuda()
    local = pool[:N].contiguous()
    gathered = None if n_pool == N else pool.reshape(-1)
    recon = torch.zeros(N, K, 2, 2, device="cuda")
    thr = torch.tensor(0.5, device="cuda")
    return {f"mask global pool {n_pool}": lambda: utils.confidence_mask(recon, 0.5, None, gathered, local),
            f"mask per_joint pool {n_pool}": lambda: utils.confidence_mask(recon, 0.5, None, gathered, local, mode="per_joint"),
            f"mask threshold pool {n_pool}": lambda: utils.confidence_mask(recon, 0.5, None, None, local, mode="threshold", threshold=thr)}


def cases(which):
    from uda_poseestimation_amd.lib.models import loss as L
    out = {}
    if which in ("ohkm", "all"):
        out["JointsOHKMMSELoss(8) fwd+bwd"] = _loss_call(L.JointsOHKMMSELoss(8), *_loss_inputs())
    if which in ("mse", "all"):
        out["JointsMSELoss() fwd+bwd"] = _loss_call(L.JointsMSELoss(), *_loss_inputs())
    if which in ("masks32", "all"):
        out.update(_mask_calls(32))
    if which in ("masks256", "all"):
        out.update(_mask_calls(256))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["ohkm", "mse", "masks32", "masks256"])
    ap.add_argument("--events", action="store_true")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_joint_selection.py measures on the GPU: none found")
    if not a.events:
        if a.case is None:
            ap.error("--case or --events")
        for name, call in cases(a.case).items():
            for _ in range(a.reps):
                call()
            torch.cuda.synchronize()
            print(json.dumps({"case": name, "calls": a.reps}))
        return
    cs = cases("all")
    for call in cs.values():
        for _ in range(20):
            call()
    torch.cuda.synchronize()
    res = {k: [] for k in cs}
    for _ in range(a.rounds):
        for name, call in cs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    for name, v in res.items():
        s = sorted(v)
        print(json.dumps({"call": name, "us_per_call_median": round(s[len(s) // 2], 2), "spread_us": round(s[-1] - s[0], 2),
                          "rounds_us": [round(x, 2) for x in v], "reps": a.reps}))


if __name__ == "__main__":
    main()
