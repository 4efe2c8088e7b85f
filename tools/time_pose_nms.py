"""us per launch of the three kernels of csrc/pose_nms.hip and what nms adds to engine.predict (profiles/pose_nms.txt).
  kernels  udapose_pose_rescore, udapose_oks_matrix (self form, mask only, and with the fp32 matrix) and udapose_pose_nms_sweep (without and
           with suppressed_by) at M = 64, 512 and 4096 poses of K = 17 key points, and udapose_pose_nms, the three behind one entry.  The
           poses are triplets - a pose and two jittered copies on one of three frames - so about a third of the walk's steps keep a pose and
           OR a row; "sparse" rows time the walk where every pose is kept (poses far apart: every step ORs its row).  Device events around
           runs of launches.  sweep_us / M is set against one dependent global load (about 1 to 2 us on this part): a walk that
           waited for a row per step would cost M times that.
  predict  engine.predict (K = 17, 32 boxes of which half are shifted copies, input 256, arg-max decode) with nms=None and nms=True.
One JSON line per result.
usage: python tools/time_pose_nms.py [--kernels] [--predict] [--arch pose_resnet101] [--reps 5] [--iters 50]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uda_poseestimation_amd import _hip, engine  # noqa: E402
from uda_poseestimation_amd.lib import keypoint_detection as kd  # noqa: E402
import uda_poseestimation_amd.lib.models as models  # noqa: E402

K = 17


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / iters)
    return sorted(runs)[len(runs) // 2], runs


def make_poses(M, sparse, seed=0):
    """kp [M,K,2], conf [M,K], boxes [M,5], frame [M]: triplets of near copies (sparse: every pose on its own)."""
    rs = np.random.RandomState(seed)
    G = M if sparse else (M + 2) // 3
    centre = np.stack([200.0 * (1 + np.arange(G) % 64), 200.0 * (1 + np.arange(G) // 64)], axis=1)
    base = centre[:, None, :] + rs.uniform(-40, 40, (G, K, 2))
    g = np.arange(M) % G
    kp = base[g] + (0 if sparse else rs.uniform(-3, 3, (M, K, 2)))
    conf = rs.uniform(0.1, 0.95, (M, K))
    boxes = np.stack([kp[..., 0].mean(1), kp[..., 1].mean(1), np.full(M, 100.0), np.full(M, 100.0), np.zeros(M)], axis=1)
    return [torch.from_numpy(a.astype(np.float32)).cuda() for a in (kp, conf, boxes)] + [torch.from_numpy((g % 3).astype(np.int32)).cuda()]


def time_kernels(reps, iters):
    L, p, st = _hip.lib(), _hip.ptr, _hip.stream
    sg = kd._sigmas_device("coco17", K, "cuda")
    vthr, othr = kd.nms_threshold("vis_thr", 0.2, "cuda"), kd.nms_threshold("oks_thr", 0.9, "cuda")
    for M in (64, 512, 4096):
        for sparse in (False, True):
            kp, conf, boxes, frame = make_poses(M, sparse)
            W = (M + 63) // 64
            score, area = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
            order, sby = torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty(M, dtype=torch.int32, device="cuda")
            refused, keep = torch.empty(M, dtype=torch.uint8, device="cuda"), torch.empty(M, dtype=torch.uint8, device="cuda")
            n_keep = torch.empty(1, dtype=torch.int32, device="cuda")
            mask = torch.empty(M, W, dtype=torch.int64, device="cuda")
            ws = torch.empty(L.udapose_pose_nms_ws_bytes(M) // 8 + 1, dtype=torch.int64, device="cuda")
            mat = torch.empty(M, M, device="cuda") if M <= 512 else None

            def rescore():
                _hip.check(L.udapose_pose_rescore(st(), p(kp), p(conf), p(boxes), None, None, p(vthr), M, K, p(score), p(order), p(area),
                                                  p(refused)), "rescore")

            def matrix(out=None):
                _hip.check(L.udapose_oks_matrix(st(), p(kp), p(area), M, None, None, None, M, K, p(sg), p(frame), p(refused), p(othr), p(out),
                                                p(mask)), "oks_matrix")

            def sweep(s=None):
                _hip.check(L.udapose_pose_nms_sweep(st(), p(mask), p(order), p(refused), M, p(keep), p(n_keep), p(s)), "sweep")

            def whole():
                _hip.check(L.udapose_pose_nms(st(), p(kp), p(conf), p(boxes), p(frame), None, None, p(sg), p(vthr), p(othr), M, K, p(ws), p(score),
                                              p(order), p(keep), p(n_keep), p(sby), None), "pose_nms")
            rescore(); matrix(); sweep()
            torch.cuda.synchronize()
            row = {"M": M, "K": K, "sparse": sparse, "n_keep": int(n_keep.item())}
            for name, fn in (("rescore_us", rescore), ("mask_us", matrix), ("sweep_us", sweep), ("sweep_suppressed_by_us", lambda: sweep(sby)),
                             ("pose_nms_us", whole)) + ((("mask_and_matrix_us", lambda: matrix(mat)),) if mat is not None else ()):
                us, runs = timed(fn, reps, iters)
                row[name] = round(us, 2)
                row[name.replace("_us", "_runs")] = [round(r, 2) for r in runs]
            row["sweep_ns_per_step"] = round(row["sweep_us"] * 1e3 / M, 1)
            emit(**row)


def time_predict(arch, reps, iters):
    torch.manual_seed(0)
    net = getattr(models, arch)(num_keypoints=K, pretrained_backbone=False).cuda()
    torch.nn.init.normal_(net.head.weight, std=0.05)
    M, S, HS, WS = 32, 256, 1080, 1920
    rs = np.random.RandomState(0)
    frames = torch.randint(0, 256, (4, HS, WS, 3), dtype=torch.uint8, device="cuda")
    half = np.stack([WS / 2 + rs.uniform(-300, 300, M // 2), HS / 2 + rs.uniform(-150, 150, M // 2), np.full(M // 2, 400.0), np.full(M // 2, 400.0),
                     np.zeros(M // 2)], axis=1)
    boxes = np.concatenate([half, half + np.asarray([2.0, -1.0, 0, 0, 0])]).astype(np.float32)
    bd = torch.from_numpy(boxes).cuda()
    fi = torch.from_numpy((np.arange(M) % (M // 2) % 4).astype(np.int32)).cuda()
    bs = torch.from_numpy(rs.uniform(0.5, 1.0, M).astype(np.float32)).cuda()
    net.eval()
    res = {}
    for name, kw in (("plain", {}), ("nms", {"box_scores": bs, "nms": True})):
        def whole():
            return engine.predict(frames, bd, net, frame_idx=fi, batch=M, input_size=S, **kw)
        out = whole()
        torch.cuda.synchronize()
        us, runs = timed(whole, reps, iters)
        res[name] = (us, runs, out)
    emit(predict=arch, boxes=M, input=S, K=K, predict_us=round(res["plain"][0], 1), predict_nms_us=round(res["nms"][0], 1),
         added_us=round(res["nms"][0] - res["plain"][0], 1), runs_us=[round(r, 1) for r in res["plain"][1]],
         runs_nms_us=[round(r, 1) for r in res["nms"][1]], n_keep=int(res["nms"][2]["n_keep"].item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--predict", action="store_true")
    ap.add_argument("--arch", default="pose_resnet101")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    emit(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
    if a.kernels or not a.predict:
        time_kernels(a.reps, a.iters)
    if a.predict or not a.kernels:
        time_predict(a.arch, a.reps, max(a.iters // 5, 5))


if __name__ == "__main__":
    main()
