"""Dev tool: per-work-group timeline of the step's weight-gradient pair launch (both tile classes) on the benched plan, from the stamp hook
of wgrad_dma_group_kernel (udapose_policy.timeline): resident work-groups over time, each XCD's finish, the drain of each launch, the seam
between the two launches and what the last work-groups of each XCD were.

The per-stage cost is reported per loader form (fast2, filter-row, stride-2, transposed, stem row-tap) and tile class.

usage: python tools/wgrad_tail_timeline.py [wgrad_order, default: the policy's] [N, default 32] [file.npy: dump the raw stamps]
       [wgrad_fastgeo_strided: 0 / 1, default: the policy's]
       python tools/wgrad_tail_timeline.py --stamps file.npy [wgrad_fastgeo_strided of that run, default 1]: the report of dumped stamps again
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


LAYERS = (3, 4, 23, 3)     # pose_resnet101
FORMS = ("fast2", "filter-row", "stride-2 (general)", "transposed (general)", "stem row-tap (general)", "stride-2 (bit-field)",
         "transposed (bit-field)", "stem row-tap (bit-field)")


def plan_forms(layers, H, W, strided):
    """(tile class, problem) -> loader form of a whole-network plan's grouped weight gradients under the production policy on power-of-two
    maps: the table order of net.hip build_wg_group (head, stem, deconvolutions last to first, blocks last to first: conv3, conv2,
    downsample, conv1) and the class and form rules of wgrad.hip wgrad_group_plan.  strided: policy wgrad_fastgeo_strided."""
    how = "bit-field" if strided else "general"
    convs = [("head", 256, 64, 1, 1, H // 4, 0), ("stem", 8, 64, 7, 2, H, 0)]
    blocks, hc, cc = [], H // 4, 64
    for L, nb in enumerate(layers):
        for bi in range(nb):
            P, s = 64 << L, 2 if (bi == 0 and L > 0) else 1
            blk = [("c3", P, 4 * P, 1, 1, hc // s, 0), ("c2", P, P, 3, s, hc, 0)]
            if bi == 0:
                blk.append(("cd", cc, 4 * P, 1, s, hc, 0))
            blk.append(("c1", cc, P, 1, 1, hc, 0))
            blocks.append(blk)
            hc, cc = hc // s, 4 * P
    ups = []
    for i in range(3):
        ups.append(("up", cc, 256, 4, 2, hc, 1))
        hc, cc = 2 * hc, 256
    convs += ups[::-1] + [c for blk in blocks[::-1] for c in blk]
    forms, count = {}, [0, 0]
    for name, ci, co, k, s, hin, transposed in convs:
        row3 = k == 3 and s == 1 and 8 <= hin <= 64
        rdim, cdim = (ci, co) if transposed else (co, 64 if name == "stem" else ci)
        t = 0 if (rdim >= 128 and cdim >= 128 and not row3) else 1
        form = (f"stem row-tap ({how})" if name == "stem" else "filter-row" if row3 else f"transposed ({how})" if transposed else
                f"stride-2 ({how})" if s == 2 else "fast2")
        forms[(t, count[t])] = form
        count[t] += 1
    return forms


def residency(start, end, t0, t1, bin_ticks=1000):
    edges = np.arange(t0, t1 + bin_ticks, bin_ticks)
    mid = edges[:-1] + bin_ticks // 2
    return mid, np.array([int(((start <= m) & (end > m)).sum()) for m in mid])


def report(tag, rows, origin, forms, tile_class):
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
    # per loader form: time per stage of work-groups that ran at full residency (the middle half of the launch), and what the form would
    # save per step at the fast2 rate of its tile class: sum of its stages x (its us per stage - fast2's) / 1024 resident slots
    form = np.array([forms.get((tile_class, int(pr)), "?") if ok else "-" for pr, ok in zip(rows[:, 4].astype(np.int64), live)])
    bits = (rows[:, 5] >> 32) & 3
    assert ((bits == 1) == (form == "filter-row"))[live].all() and ((bits == 2) == np.char.startswith(form, "stem row-tap"))[live].all(), \
        "the tool's walk of the plan disagrees with the stamps' form bits"
    table = {}
    for name in FORMS:
        for cut, window in ((4, "middle half"), (10, "middle 80 %: too few in the middle half")):
            s = live & (form == name) & (start > t0 + (t1 - t0) // cut) & (end < t1 - (t1 - t0) // cut)
            if s.sum() > 16:
                per = (end[s] - start[s]) * TICK_US / (stages[s] + 4)
                table[name] = (int((form == name).sum()), int(stages[form == name].sum()), int(s.sum()), float(per.mean()), float(per.std()), window)
                break
    base = table.get("fast2", (0, 0, 0, 0.0, 0.0, ""))[3]
    total = 0.0
    for name, (n_wg, n_st, n_mid, mean, std, window) in table.items():
        line = f"  {name}: {n_wg} work-groups, {n_st} stages; {n_mid} mid-launch ({window}): lifetime / (stages + 4) = {mean:.3f} us (std {std:.3f})"
        if base and name != "fast2":
            save = n_st * (mean - base) / 1024.0
            line += f"; at the fast2 rate {base:.3f}: {save:+.1f} us per step"
            if name != "filter-row":
                total += save
        print(line)
    if base:
        print(f"  predicted saving of the strided / transposed / stem forms together: {total:.1f} us per step")
    return t0, t1, mid, res, plateau


def summary(rows, strided):
    big, small = rows[rows[:, 7] == 128], rows[rows[:, 7] == 64]
    origin = int(rows[:, 0].min())
    forms = plan_forms(LAYERS, 256, 256, strided)
    a = report("launch 1 (128x128 class)", big, origin, forms, 0)
    c = report("launch 2 (64x64 class)", small, origin, forms, 1)
    reach = c[2][np.nonzero(c[3] >= 0.75 * c[4])[0][0]]
    print(f"SEAM: end of launch 1 -> first work-group of launch 2 {(c[0] - a[1]) * TICK_US:.1f} us; -> launch 2 at 75 % of its plateau {(reach - a[1]) * TICK_US:.1f} us")
    print(f"both launches, first start to last end: {(c[1] - a[0]) * TICK_US:.1f} us")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--stamps":     # (the report of a dumped run again, no GPU: --stamps file.npy [wgrad_fastgeo_strided of that run])
        return summary(np.load(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 1)
    order = int(sys.argv[1]) if len(sys.argv) > 1 and int(sys.argv[1]) >= 0 else None     # (-1: the policy's)
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    stu = models.pose_resnet101(num_keypoints=16, pretrained_backbone=False).to(dev)
    tea = models.pose_resnet101(num_keypoints=16, pretrained_backbone=False).to(dev)
    if order is not None:
        stu.policy["wgrad_order"] = order
    if len(sys.argv) > 4:
        stu.policy["wgrad_fastgeo_strided"] = int(sys.argv[4])
    tr = MeanTeacherTrainer(stu, tea, lr=1e-4, teacher_alpha=0.999, lambda_c=1.0, mask_ratio=0.5, sigma=2, image_size=256, heatmap_size=64, precision="bf16")
    tr.sum_splits_in_tail = False
    b = synthetic.mean_teacher_batch(N, num_keypoints=16, image_size=256, heatmap_size=64, sigma=2, seed=0)
    g = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    for _ in range(3):
        tr.train_step(g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])
    torch.cuda.synchronize()
    buf = torch.zeros(STAMP_BLOCKS, 8, dtype=torch.int64, device=dev)
    orig = stu.finish_wgrad
    seen = {}

    def stamped(**kw):
        hd = stu._pending_wg[0][0]
        pol = _hip.Policy()
        _hip.check(hd.L.udapose_net_get_policy(hd.h, C.byref(pol)), "get_policy")
        seen["strided"] = int(getattr(pol, "wgrad_fastgeo_strided", 0))
        print(f"policy: wgrad_order {pol.wgrad_order}, wgrad_stages {pol.wgrad_stages}, wgrad_fastgeo_strided {seen['strided']}")
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
    summary(rows, seen.get("strided", 0))

if __name__ == "__main__":
    main()
