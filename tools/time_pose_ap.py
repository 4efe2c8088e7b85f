"""us per update and per compute() of the key-point AP meter (csrc/pose_ap.hip; profiles/pose_ap.txt).
  update   udapose_ap_match (three launches) at (M, G, F) = (64, 32, 8), (512, 256, 64), (4096, 2048, 512) with K = 17, the default ten
           thresholds, three area ranges and max_dets = 20: every frame holds M / F detections and G / F labels, three detections in four
           within reach of a label.  The counters are zeroed between runs of launches, so the records never pass the capacity.
  compute  udapose_ap_curve (two launches) and the whole compute() - the launches, the one read-back and the host report - at N = 4096 and
           65536 records.
Device events around runs of launches; the median of `reps` runs and every run.  One JSON line per result.
usage: python tools/time_pose_ap.py [--reps 5] [--iters 50]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uda_poseestimation_amd import _hip  # noqa: E402
from uda_poseestimation_amd.lib import keypoint_detection as kd  # noqa: E402

K = 17


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps, iters, before=None):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / iters)
    return sorted(runs)[len(runs) // 2], runs


def make_update(M, G, F, seed=0):
    """Detections and labels spread evenly over F frames: labels on a 200 px grid, a detection a jittered copy of a label of its frame
    (three in four) or a pose of its own."""
    rs = np.random.RandomState(seed)
    centre = np.stack([200.0 * (1 + np.arange(G) % 64), 200.0 * (1 + np.arange(G) // 64)], axis=1)
    gkp = centre[:, None, :] + rs.uniform(-40, 40, (G, K, 2))
    gframe = np.arange(G) % F
    frame = np.arange(M) % F
    per = max(G // F, 1)
    pick = (frame + F * (np.arange(M) // F % per)) % G            # a label of the detection's own frame
    kp = gkp[pick] + rs.uniform(-6, 6, (M, K, 2))
    own = np.arange(M) % 4 == 3
    kp[own] += 5000.0
    t = [kp.astype(np.float32), rs.uniform(0.1, 1.0, M).astype(np.float32), frame.astype(np.int32), gkp.astype(np.float32),
         (rs.uniform(0, 1, (G, K)) > 0.2).astype(np.float32), rs.uniform(20.0 ** 2, 150.0 ** 2, G).astype(np.float32), gframe.astype(np.int32)]
    return [torch.from_numpy(a).cuda() for a in t]


def time_updates(reps, iters):
    for M, G, F in ((64, 32, 8), (512, 256, 64), (4096, 2048, 512)):
        meter = kd.APMeter(K, device="cuda", capacity=1 << 18)
        t = make_update(M, G, F)

        def update():
            meter.update(*t, num_frames=F)
        update()
        torch.cuda.synchronize()
        records = int(meter.state()["counters"][0])
        us, runs = timed(update, reps, min(iters, (1 << 18) // max(records, 1)), before=meter.reset)
        emit(update=[M, G, F], K=K, records_per_update=records, update_us=round(us, 2), update_runs=[round(r, 2) for r in runs])


def time_compute(reps, iters):
    L, p = _hip.lib(), _hip.ptr
    for N in (4096, 65536):
        meter = kd.APMeter(K, device="cuda", capacity=65536)
        t = make_update(4096, 2048, 512)
        while int(meter.state()["counters"][0]) < N:
            meter.update(*t, num_frames=512)
        st = meter._st
        st["counters"][0] = N
        st["counters"][1] = 0      # (what the last update dropped past the capacity)
        T, A, R = 10, 3, 101
        ws = torch.empty(L.udapose_ap_curve_ws_bytes(meter.capacity, T, A) // 8 + 1, dtype=torch.int64, device="cuda")
        pr, sc, rc = (torch.empty(T, R, A, dtype=torch.float64, device="cuda"), torch.empty(T, R, A, device="cuda"),
                      torch.empty(T, A, dtype=torch.float64, device="cuda"))

        def curve():
            _hip.check(L.udapose_ap_curve(_hip.stream(), p(st["score"]), p(st["matched"]), p(st["ignored"]), meter.capacity, p(st["counters"]), T, A,
                                          p(st["rp"]), R, p(ws), p(pr), p(sc), p(rc)), "ap_curve")
        us, runs = timed(curve, reps, max(iters // 5, 3))
        meter.compute()
        t0 = time.perf_counter()
        for _ in range(5):
            rep = meter.compute()
        whole = (time.perf_counter() - t0) / 5 * 1e6
        emit(compute_records=N, curve_us=round(us, 1), curve_runs=[round(r, 1) for r in runs], compute_wall_us=round(whole, 1), AP=round(rep["AP"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    emit(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
    time_updates(a.reps, a.iters)
    time_compute(a.reps, a.iters)


if __name__ == "__main__":
    main()
