"""Device time of the gradient-clipping kernels against the loss scaler's found-inf check they replace, in ONE process over the SAME tables:
a PoseResNet-101 (K = 16) parameter list with synthetic gradients in two flat buffers (g and the second per-pass buffer g2), no forward.
  check2      udapose_grad_scaler_check2 (grad_check_k, the parent's kernel: reads g [+ g2], raises found_inf)
  sumsq+check udapose_grad_sumsq with a dev_state (grad_sumsq_k: the same read, the check, double sum of squares, one partial per block)
  sumsq       the same without a dev_state (bf16: no scaler)
  clip        udapose_grad_clip (one work-group over the partials) and udapose_grad_clip_restore
HIP events around one launch; `warm` = the launch repeated back to back (whatever of the 0.21 GB per buffer stays in the memory-side cache
stays), `cold` = a 512 MB fill in front of every timed launch.  Every figure is the median of --reps launches; the rounds alternate the
kernels, and the spread is max - min of a kernel's round medians (the margin the comparison is read against).
--step adds the BASELINE.json configs[1] captured step (N = 32, 256x256, bf16) with clipping off / on (max_grad_norm = inf: same update).
usage: python tools/time_grad_clip.py [--reps 50] [--rounds 5] [--step] [--steps 100]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--N", type=int, default=32)
    a = ap.parse_args()
    import torch
    from uda_poseestimation_amd import _hip
    from uda_poseestimation_amd.utils import _MultiTensorTable
    import uda_poseestimation_amd.lib.models as models
    L, ptr = _hip.lib(), _hip.ptr
    torch.manual_seed(0)
    net = models.pose_resnet101(num_keypoints=16, pretrained_backbone=False)
    sizes = [p.numel() for n, p in net.named_parameters() if not n.startswith("backbone.fc.")]
    total = sum(sizes)
    half = -(-total // 4) * 4
    flat = torch.randn(2 * half, device="cuda") * 0.05
    views, off = [], 0
    for n in sizes:
        views.append(flat[off:off + n])
        off += n
    delta = 4 * half
    tab = _MultiTensorTable([views])
    state = torch.tensor([0, 0, 0, 1e-3, 1.0 / 65536, 0, 65536.0, 0], dtype=torch.float32, device="cuda")
    part = torch.zeros(tab.nblocks, dtype=torch.float64, device="cuda")
    clip = torch.zeros(12, dtype=torch.float32, device="cuda")
    clip[0] = float("inf")
    one_state = (C.c_void_p * 1)(state.data_ptr())
    b0, b1 = (C.c_int * 1)(0), (C.c_int * 1)(tab.nblocks)
    tb = (ptr(tab.ptrs[0]), ptr(tab.sizes), ptr(tab.blk_t), ptr(tab.blk_o), tab.nblocks)
    s = lambda: _hip.stream()
    kernels = {}
    for name, d in (("g", 0), ("g+g2", delta)):
        kernels[f"check2 {name}"] = lambda d=d: L.udapose_grad_scaler_check2(s(), *tb, ptr(state), d)
        kernels[f"sumsq+check {name}"] = lambda d=d: L.udapose_grad_sumsq(s(), *tb, d, ptr(state), ptr(part))
        kernels[f"sumsq {name}"] = lambda d=d: L.udapose_grad_sumsq(s(), *tb, d, None, ptr(part))
    kernels["clip"] = lambda: L.udapose_grad_clip(s(), ptr(part), b0, b1, 1, one_state, ptr(clip))
    kernels["restore"] = lambda: L.udapose_grad_clip_restore(s(), 1, one_state, ptr(clip))
    flush = torch.empty(128 << 20, dtype=torch.float32, device="cuda")

    def median_us(fn, cold):
        ts = []
        for _ in range(a.reps):
            if cold:
                flush.fill_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _hip.check(fn(), "launch")
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return sorted(ts)[len(ts) // 2]

    for fn in kernels.values():             # warm-up: code objects loaded, tables resident
        for _ in range(10):
            _hip.check(fn(), "warm-up")
    torch.cuda.synchronize()
    res = {}
    for r in range(a.rounds):
        for cold in (False, True):
            for name, fn in kernels.items():
                res.setdefault((name, cold), []).append(median_us(fn, cold))
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({"parameters": total, "tensors": len(sizes), "blocks": tab.nblocks, "bytes_per_buffer": 4 * total, "reps": a.reps, "rounds": a.rounds}))
    for (name, cold), v in res.items():
        print(json.dumps({"kernel": name, "cache": "cold" if cold else "warm", "median_us": round(med(v), 2), "spread_us": round(max(v) - min(v), 2),
                          "round_medians_us": [round(x, 2) for x in v]}), flush=True)
    assert float(state[5]) == 0.0 and float(clip[2]) == 1.0
    del flush, flat
    torch.cuda.empty_cache()
    if not a.step:
        return
    from uda_poseestimation_amd import synthetic
    from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer
    N, K, S = a.N, 16, 256
    b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=0)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    args = (g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"])
    sd = net.state_dict()
    legs = {}
    for r in range(2):
        for clipv in (None, float("inf")):
            stu = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
            tea = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False)
            stu.load_state_dict(sd)
            tea.load_state_dict(sd)
            tr = MeanTeacherTrainer(stu.cuda(), tea.cuda(), lr=1e-4, precision="bf16")
            tr.max_grad_norm = clipv
            gs = GraphedTrainStep(tr, *args, warmup=3)
            for _ in range(20):
                gs.step(*args)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                gs.step(*args)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
            legs.setdefault("on" if clipv else "off", []).append(round(ms, 4))
            gs.release()
            del gs, tr, stu, tea
            torch.cuda.empty_cache()
    print(json.dumps({"captured_step_ms": legs, "N": N, "res": S, "steps": a.steps,
                      "on_minus_off_ms": round(min(legs["on"]) - min(legs["off"]), 4)}), flush=True)


if __name__ == "__main__":
    main()
