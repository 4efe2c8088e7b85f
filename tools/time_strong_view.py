"""What the strong student view's launches cost on one MI355X at N = 32, 256x256, beside one udapose_aug_color_op pass (csrc/augment.hip,
untouched by the feature): udapose_aug_point_op with every image on autocontrast / equalize / posterize / solarize, on a mix of the four, and
on equalize over constant images (every histogram atomic of an image on one LDS address per channel); udapose_aug_sharpness_u8;
udapose_aug_erase_f32 with boxes drawn like the reference draws them.  The calls alternate inside every round, --rounds rounds of
--launches back-to-back calls each between two device events (launch included); one JSON line per call with the median over the rounds.
Kernel-only times: this script under `rocprofv3 --kernel-trace --stats -d DIR -o sv --output-format csv`, in a run of its own with
--launches 1, then `--report DIR/..._kernel_trace.csv`: the trace's dispatches of the project's kernels are matched, in order, with
the sequence of calls below, and the median per (call, kernel) is printed.
usage: python tools/time_strong_view.py [--launches 100] [--rounds 7] | --report TRACE.csv [--rounds 7]"""
import argparse
import csv
import json
import os
import random
import statistics
import sys

# (call, kernels it launches in order)
SEQUENCE = [("color_op brightness", ["aug_gray_mean_k", "aug_color_op_k"]), ("color_op contrast", ["aug_gray_mean_k", "aug_color_op_k"]),
            ("color_op colour", ["aug_gray_mean_k", "aug_color_op_k"]),
            ("point_op autocontrast", ["point_table_k", "point_apply_k"]), ("point_op equalize", ["point_table_k", "point_apply_k"]),
            ("point_op posterize", ["point_table_k", "point_apply_k"]), ("point_op solarize", ["point_table_k", "point_apply_k"]),
            ("point_op mixed 4-7", ["point_table_k", "point_apply_k"]), ("point_op equalize, constant images", ["point_table_k", "point_apply_k"]),
            ("sharpness", ["sharp_copy_k", "sharpness_k"]), ("erase", ["erase_f32_k"])]
WARMUP = 3          # rounds of the sequence before the timed ones (both modes)


def report(path, rounds):
    names = sorted({k for _, ks in SEQUENCE for k in ks}, key=len, reverse=True)
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            k = next((n for n in names if n in r["Kernel_Name"]), None)
            if k is not None:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k))
    rows.sort()
    flat = [(call, k) for call, ks in SEQUENCE for k in ks]
    assert len(rows) == len(flat) * (WARMUP + rounds), (len(rows), len(flat), "the trace is not of a --launches 1 run with these --rounds")
    times = {ck: [] for ck in flat}
    for i, (t0, t1, k) in enumerate(rows):
        call, want = flat[i % len(flat)]
        assert k == want, (i, k, want)
        if i >= WARMUP * len(flat):
            times[(call, want)].append((t1 - t0) / 1e3)
    for (call, k), v in times.items():
        print(json.dumps({"call": call, "kernel": k, "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                          "dispatches": len(v)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--report", default=None)
    a = ap.parse_args()
    if a.report:
        return report(a.report, a.rounds)
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from uda_poseestimation_amd import _hip, data_gpu as D
    from uda_poseestimation_amd._hip import lib, ptr
    L, st = lib(), _hip.stream()
    N, H, W = 32, 256, 256
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    const = torch.full((N, H, W, 3), 93, dtype=torch.uint8).cuda()
    const[:, 0, 0] = 7                                  # (two filled bins: equalize builds a real table)
    tmp = torch.empty_like(img)
    x = torch.randn(N, 3, H, W, generator=g).cuda()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()
    ops = {c: i32([c] * N) for c in range(1, 9)}
    mixed = i32([4 + n % 4 for n in range(N)])
    factor = torch.full((N,), 1.27).cuda()
    iparam = {6: i32([4] * N), 7: i32([128] * N), 0: i32([4 if n % 4 == 2 else 128 for n in range(N)])}
    inv = torch.tensor(D.AUTOCONTRAST_SCALES, dtype=torch.float64).cuda()
    lut = torch.empty(N, 768, dtype=torch.uint8).cuda()
    mean = torch.empty(N, dtype=torch.int32).cuda()
    rng = random.Random(0)
    cfg = D.ViewConfig(erase=1.0)
    boxes = i32([cfg.draw_erase(rng, H, W) for _ in range(N)])
    color = lambda c: (lambda: L.udapose_aug_color_op(st, ptr(img), ptr(ops[c]), ptr(factor), ptr(mean), N, H * W))
    point = lambda o, p, t=img: (lambda: L.udapose_aug_point_op(st, ptr(t), ptr(o), ptr(p), ptr(inv), ptr(lut), N, H * W))
    fns = [color(1), color(2), color(3), point(ops[4], iparam[6]), point(ops[5], iparam[6]), point(ops[6], iparam[6]), point(ops[7], iparam[7]),
           point(mixed, iparam[0]), point(ops[5], iparam[6], const),
           lambda: L.udapose_aug_sharpness_u8(st, ptr(img), ptr(tmp), ptr(ops[8]), ptr(factor), N, H, W),
           lambda: L.udapose_aug_erase_f32(st, ptr(x), ptr(boxes), 0.4914, 0.4822, 0.4465, N, H, W)]
    calls = dict(zip([c for c, _ in SEQUENCE], fns))
    runs = {name: [] for name in calls}
    for rnd in range(WARMUP + a.rounds):
        for name, fn in calls.items():
            # (the image drifts under repeated in-place ops: fresh random bytes before every timed call keep the histograms full)
            if name != "erase" and "constant" not in name:
                img.copy_(torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8), non_blocking=False)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.launches):
                assert fn() == 0
            e1.record()
            torch.cuda.synchronize()
            if rnd >= WARMUP:
                runs[name].append(round(e0.elapsed_time(e1) * 1e3 / a.launches, 2))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "N": N, "H": H, "W": W, "launches": a.launches,
                      "rounds": a.rounds, "MB_per_batch": round(img.numel() / 1e6, 2)}))
    for name, v in runs.items():
        print(json.dumps({"call": name, "us_per_call_incl_launch": round(statistics.median(v), 2), "runs_us": v}), flush=True)


if __name__ == "__main__":
    main()
