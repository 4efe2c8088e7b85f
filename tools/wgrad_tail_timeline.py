"""Dev tool: per-work-group timeline of the step's weight-gradient pair launch (both tile classes) on the benched plan, from the stamp hook
of wgrad_dma_group_kernel (udapose_policy.timeline): resident work-groups over time, each XCD's finish, the drain of each launch, the seam
between the two launches and what the last work-groups of each XCD were.

usage: python tools/wgrad_tail_timeline.py [wgrad_order, default: the policy's] [N, default 32] [file.npy: dump the raw stamps]
The stamped twins of the kernels run only inside this tool's one eager pair launch (after both gradient chains, as in the step)."""
import ctypes as C
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import uda_poseestimation_amd.lib.models as models   # noqa: E402
from uda_poseestimation_amd import _hip, synthetic, warp   # noqa: E402
from uda_poseestimation_amd.engine import MeanTeacherTrainer   # noqa: E402

STAMP_BLOCKS = 1 << 17     # (include/udapose.h: what a timeline buffer must hold)
TICK_US = 0.01             # s_memrealtime: 100 MHz


def residency(start, end, t0, t1, bin_ticks=1000):
    edges = np.arange(t0, t1 + bin_ticks, bin_ticks)
    mid = edges[:-1] + bin_ticks // 2
    return mid, np.array([int(((start <= m) & (end > m)).sum()) for m in mid])


def report(tag, rows, origin):
    start, end, xcd, stages = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 5] & 0xffffffff
    live = rows[:, 4].astype(np.int64) >= 0
    t0, t1 = int(start.min()), int(end.max())
    mid, res = residency(start[live], end[live], t0, t1)
    plateau = int(np.percentile(res, 90))
    below = np.nonzero(res >= 0.75 * plateau)[0]
    drain_from = mid[below[-1]] if len(below) else t0
    ramp_to = mid[below[0]] if len(below) else t0
    life = (end[live] - start[live]) * TICK_US
    print(f"{tag}: {int(live.sum())} work-groups ({len(rows) - int(live.sum())} padding), {(t0 - origin) * TICK_US:.1f} .. {(t1 - origin) * TICK_US:.1f} us "
          f"(length {(t1 - t0) * TICK_US:.1f} us); plateau {plateau} resident; ramp to 75 % {(ramp_to - t0) * TICK_US:.1f} us; "
          f"DRAIN (below 75 % of the plateau to the end) {(t1 - drain_from) * TICK_US:.1f} us; work-group lifetime mean {life.mean():.1f} max {life.max():.1f} us")
    print(f"  resident work-groups per 10 us bin: {' '.join(str(r) for r in res)}")
    fin = [(int(end[live & (xcd == k)].max()) - t0) * TICK_US if (live & (xcd == k)).any() else 0.0 for k in range(8)]
    print(f"  XCD finish times (us from the launch's start): {' '.join(f'{f:.1f}' for f in fin)}  (spread {max(fin) - min(fin):.1f} us)")
    for k in range(8):
        sel = np.nonzero(live & (xcd == k))[0]
        last = sel[np.argsort(end[sel])[-128:]]
        vals, cnt = np.unique(stages[last], return_counts=True)
        print(f"  XCD {k}: stages of its last 128 work-groups: " + ", ".join(f"{int(v)}x{int(c)}" for v, c in zip(vals, cnt)))
    # per form: time per stage of work-groups that ran at full residency (the middle half of the launch)
    midsel = live & (start > t0 + (t1 - t0) // 4) & (end < t1 - (t1 - t0) // 4)
    for name, bit in (("one-tap", 0), ("filter-row", 1), ("stem row-tap", 2)):
        form = (rows[:, 5] >> 32) & 3
        s = midsel & (form == bit)
        if s.sum() > 16:
            per = (end[s] - start[s]) * TICK_US / (stages[s] + 4)
            print(f"  {name}: {int(s.sum())} mid-launch work-groups, lifetime / (stages + 4) = {per.mean():.3f} us (std {per.std():.3f})")
    return t0, t1, mid, res, plateau


def main():
    order = int(sys.argv[1]) if len(sys.argv) > 1 else None
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    stu = models.pose_resnet101(num_keypoints=16, pretrained_backbone=False).to(dev)
    tea = models.pose_resnet101(num_keypoints=16, pretrained_backbone=False).to(dev)
    if order is not None:
        stu.policy["wgrad_order"] = order
    tr = MeanTeacherTrainer(stu, tea, lr=1e-4, teacher_alpha=0.999, lambda_c=1.0, mask_ratio=0.5, sigma=2, image_size=256, heatmap_size=64, precision="bf16")
    tr.sum_splits_in_tail = False
    b = synthetic.mean_teacher_batch(N, num_keypoints=16, image_size=256, heatmap_size=64, sigma=2, seed=0)
    g = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    for _ in range(3):
        tr.train_step(g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])
    torch.cuda.synchronize()
    buf = torch.zeros(STAMP_BLOCKS, 8, dtype=torch.int64, device=dev)
    orig = stu.finish_wgrad

    def stamped(**kw):
        hd = stu._pending_wg[0][0]
        pol = _hip.Policy()
        _hip.check(hd.L.udapose_net_get_policy(hd.h, C.byref(pol)), "get_policy")
        print(f"policy: wgrad_order {pol.wgrad_order}, wgrad_stages {pol.wgrad_stages}")
        pol.timeline = buf.data_ptr()
        _hip.check(hd.L.udapose_net_set_policy(hd.h, C.byref(pol)), "set_policy")
        try:
            return orig(**kw)
        finally:
            pol.timeline = None
            _hip.check(hd.L.udapose_net_set_policy(hd.h, C.byref(pol)), "set_policy")
    stu.finish_wgrad = stamped
    theta = lambda ap: warp.recon_thetas(ap, N, 4.0, "cuda")
    tr._forward_backward(g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], [g["x_t_tea"]], theta(g["aug_param_stu"]), [theta(g["aug_param_tea"])])
    torch.cuda.synchronize()
    stu.finish_wgrad = orig
    stu.finish_grads()
    rows = buf.cpu().numpy()
    rows = rows[rows[:, 1] != 0]
    if len(sys.argv) > 3:           # (the raw stamps, for offline fits of the deal's cost model)
        np.save(sys.argv[3], rows)
    big, small = rows[rows[:, 7] == 128], rows[rows[:, 7] == 64]
    origin = int(rows[:, 0].min())
    a = report("launch 1 (128x128 class)", big, origin)
    c = report("launch 2 (64x64 class)", small, origin)
    reach = c[2][np.nonzero(c[3] >= 0.75 * c[4])[0][0]]
    print(f"SEAM: end of launch 1 -> first work-group of launch 2 {(c[0] - a[1]) * TICK_US:.1f} us; -> launch 2 at 75 % of its plateau {(reach - a[1]) * TICK_US:.1f} us")
    print(f"both launches, first start to last end: {(c[1] - a[0]) * TICK_US:.1f} us")


if __name__ == "__main__":
    main()
