"""us per launch of udapose_box_crop and the cost of the crop inside engine.predict (profiles/box_crop.txt).
  kernel   32 crops of 256 x 256 from 32 frames of 1080 x 1920 at bw / Wo = 1, 2.5 and 6 (1, 3 x 3 and 6 x 6 samples per output pixel),
           upright and turned by 30 degrees, with and without the mirrored second half, fp32 NCHW output; device events around a run of
           launches.  Bytes = the boxes' source pixels inside the frame (3 B each, read once in the ideal) + the output written; the rate is
           set against the 6.0 TB/s DESIGN.md 3 measures for streaming kernels.  The work-groups that stage their footprint in LDS are
           counted on the host from the same geometry (tile corners, one pixel of margin, 8192 pixels of LDS image).
  predict  engine.predict (PoseResNet-101, K = 16, 32 boxes at bw / Wo = 2.5, input 256, arg-max decode) against the same evaluation forward and
           decode on crops made beforehand, each call followed by a device synchronisation as predict's saturation check is: what the crop,
           the way back and the bookkeeping add per call; both with and without the flip test.
One JSON line per result.
usage: python tools/time_box_crop.py [--kernel] [--predict] [--arch pose_resnet101] [--reps 5] [--iters 50]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uda_poseestimation_amd import data_gpu, engine  # noqa: E402
from uda_poseestimation_amd.lib import keypoint_detection as kd  # noqa: E402
import uda_poseestimation_amd.lib.models as models  # noqa: E402

HBM_TBS = 6.0
M, S, HS, WS = 32, 256, 1080, 1920


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


def make_boxes(ratio, rot, seed=0):
    rs = np.random.RandomState(seed)
    side = ratio * S
    return np.stack([WS / 2 + rs.uniform(-200, 200, M), HS / 2 + rs.uniform(-100, 100, M), np.full(M, side), np.full(M, side), np.full(M, rot)],
                    axis=1).astype(np.float32)


def source_bytes(boxes):
    """3 B per source pixel of every box that lies inside its frame (upright boxes exactly, turned ones by their area clipped as upright)."""
    w = np.minimum(boxes[:, 0] + boxes[:, 2] / 2, WS) - np.maximum(boxes[:, 0] - boxes[:, 2] / 2, 0)
    h = np.minimum(boxes[:, 1] + boxes[:, 3] / 2, HS) - np.maximum(boxes[:, 1] - boxes[:, 3] / 2, 0)
    return float((np.maximum(w, 0) * np.maximum(h, 0)).sum() * 3)


def staged_share(boxes, tw=32, th=8, lds_pixels=8192):
    """The share of work-groups whose footprint fits the LDS image: the kernel's own rule, restated."""
    fit = total = 0
    for cx, cy, bw, bh, rot in boxes.astype(np.float64):
        c, s = math.cos(math.radians(rot)), math.sin(math.radians(rot))
        sx, sy = bw / S, bh / S
        for v0 in range(0, S, th):
            for u0 in range(0, S, tw):
                xs, ys = [], []
                for u in (u0, min(u0 + tw, S)):
                    for v in (v0, min(v0 + th, S)):
                        dx, dy = (u - S / 2) * sx, (v - S / 2) * sy
                        xs.append(cx + c * dx - s * dy); ys.append(cy + s * dx + c * dy)
                xa, xb = max(math.floor(min(xs) - 0.5) - 1, -1), min(math.floor(max(xs) - 0.5) + 2, WS)
                ya, yb = max(math.floor(min(ys) - 0.5) - 1, -1), min(math.floor(max(ys) - 0.5) + 2, HS)
                total += 1
                fit += xb >= xa and yb >= ya and (xb - xa + 1) * (yb - ya + 1) <= lds_pixels
    return fit / total


def time_kernel(reps, iters):
    frames = torch.randint(0, 256, (M, HS, WS, 3), dtype=torch.uint8, device="cuda")
    fi = torch.arange(M, dtype=torch.int32, device="cuda")
    md, sd = data_gpu._norm_consts(frames.device, data_gpu.IMAGENET_MEAN, data_gpu.IMAGENET_STD)
    for ratio in (1.0, 2.5, 6.0):
        for rot in (0.0, 30.0):
            boxes = make_boxes(ratio, rot)
            bd = torch.from_numpy(boxes).cuda()
            for mirror in (False, True):
                us, runs = timed(lambda: data_gpu.box_crop_launch(frames, bd, fi, S, S, md, sd, mirror, True, False), reps, iters)
                moved = source_bytes(boxes) + M * (2 if mirror else 1) * 3 * S * S * 4
                emit(kernel="box_crop", crops=M, out=S, frame=[HS, WS], ratio=ratio, taps=int(min(max(math.ceil(ratio), 1), 8)) ** 2, rot=rot,
                     mirror=mirror, us_per_launch=round(us, 2), runs_us=[round(r, 2) for r in runs], mbytes=round(moved / 1e6, 2),
                     tb_per_s=round(moved / us / 1e6, 3), share_of_hbm_rate=round(moved / us / 1e6 / HBM_TBS, 3),
                     staged_share=round(staged_share(boxes), 3))


def time_predict(arch, reps, iters):
    torch.manual_seed(0)
    net = getattr(models, arch)(num_keypoints=16, pretrained_backbone=False).cuda()
    torch.nn.init.normal_(net.head.weight, std=0.05)
    frames = torch.randint(0, 256, (M, HS, WS, 3), dtype=torch.uint8, device="cuda")
    boxes = make_boxes(2.5, 0.0)
    bd, fi = torch.from_numpy(boxes).cuda(), torch.arange(M, dtype=torch.int32, device="cuda")
    # running statistics of one train-mode forward, so that the folded eval-mode BatchNorm is not the identity (and nothing saturates)
    net.train()
    net.bn_momentum = 1.0
    with torch.no_grad():
        net(data_gpu.box_crop(frames, bd, S, frame_idx=fi)[0])
    net.bn_momentum = 0.1
    net.eval()
    net._handles.clear()
    for flip in (None, "body16"):
        x, _ = data_gpu.box_crop(frames, bd, S, frame_idx=fi)

        def forward_only():
            with torch.no_grad():
                if flip:
                    perm = kd._perm_device(flip, 16, x.device)
                    engine._flip_forward(net, x, perm, False, True)
                else:
                    kd._decode_pred_max(net(x), "argmax")
            torch.cuda.synchronize()      # (predict ends in the saturation check's synchronisation: the same footing)

        def whole():
            return engine.predict(frames, bd, net, frame_idx=fi, flip_pairs=flip, batch=M, input_size=S)
        out = whole()
        torch.cuda.synchronize()
        fwd_us, _ = timed(forward_only, reps, iters)
        all_us, runs = timed(whole, reps, iters)
        emit(predict=arch, boxes=M, input=S, flip=bool(flip), forward_and_decode_us=round(fwd_us, 1), predict_us=round(all_us, 1),
             added_us=round(all_us - fwd_us, 1), added_share=round((all_us - fwd_us) / fwd_us, 4), runs_us=[round(r, 1) for r in runs],
             refused=int(out["status"].sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--predict", action="store_true")
    ap.add_argument("--arch", default="pose_resnet101")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    emit(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
    if a.kernel or not a.predict:
        time_kernel(a.reps, a.iters)
    if a.predict or not a.kernel:
        time_predict(a.arch, a.reps, max(a.iters // 5, 5))


if __name__ == "__main__":
    main()
