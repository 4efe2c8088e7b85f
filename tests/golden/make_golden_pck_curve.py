"""Golden vectors of the evaluation report, made by RUNNING THE REFERENCE'S OWN lib.keypoint_detection.accuracy (pure numpy,
lib/keypoint_detection.py:65-94) and by reading the group tables off the reference's dataset classes.

    python tests/golden/make_golden_pck_curve.py

Writes next to this file (data only; the reference's modules are loaded by path at run time and none of their text is stored):
  pck_curve.npz      for every case of tests/helpers/pck_curve_ref.GOLDEN_CASES the seeded heat-map pair and, for each of the 20
                     thresholds of PCK_THRESHOLDS, the reference's acc [K], avg_acc and cnt
  joint_groups.json  the `keypoints_group` tables of Body16 / Hand21 / Animal18 / Animal14KeypointDataset
                     (lib/datasets/keypoint_dataset.py), in the reference's order of names; the classes are instantiated with no samples,
                     with empty stand-ins for the two drawing modules (cv2, webcolors) their file imports
The reference divides and compares in fp64, the device in fp32: the generator asserts that the fp32 restatement gives the reference's
numbers for every case and threshold (no case is left out), and prints the smallest relative gap |d - t| / t it met apart from the exact
ties d == t, which both precisions resolve as misses (12x20: d = 0.5 and d = 1.0).
"""
import json
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
from make_golden import load_by_path  # noqa: E402  (the reference checkout it reads is named there)
from helpers import pck_curve_ref as R  # noqa: E402

THRESHOLDS = tuple(0.05 * j for j in range(1, 21))      # lib.keypoint_detection.PCK_THRESHOLDS


def curves(ref):
    out, names = {}, []
    for name, shape, seed in R.GOLDEN_CASES:
        o, t = R.golden_inputs(shape, seed)
        H, W = shape[2:]
        acc, avg, cnt = [], [], []
        for thr in THRESHOLDS:
            a, av, c, _ = ref.accuracy(o.copy(), t.copy(), thr=thr)
            acc.append(a); avg.append(av); cnt.append(c)
        acc, avg, cnt = np.asarray(acc, dtype=np.float64), np.asarray(avg, dtype=np.float64), np.asarray(cnt, dtype=np.int64)
        # the fp32 restatement must give the same numbers: no fp32 / fp64 disagreement in the recorded cases
        s = R.state_fp32_heatmaps(o, t, np.asarray(THRESHOLDS, dtype=np.float32))
        T = len(THRESHOLDS)
        mine = np.where((s[:, T] > 0)[:, None], s[:, :T] / np.maximum(s[:, T], 1)[:, None], -1.0).T
        assert np.abs(mine - acc).max() <= 1e-12, name
        seen = s[:, T] > 0
        assert (cnt == seen.sum()).all() and np.abs(mine[:, seen].mean(1) - avg).max() <= 1e-12, name
        assert (~seen).any() and ((s[:, T] > 0) & (s[:, T] < shape[0])).any(), name      # joints hidden everywhere / in some samples
        d, _, vis = R.distances_fp64(R.argmax_preds(o), R.argmax_preds(t), np.float32(H / 10.0), np.float32(W / 10.0))
        gap = np.abs(d[vis][:, None] - np.asarray(THRESHOLDS)) / np.asarray(THRESHOLDS)
        ties = int((gap == 0).sum())
        print(f"{name}: {int(vis.sum())} visible pairs, smallest relative gap {gap[gap > 0].min():.2e}, exact ties {ties}, "
              f"PCK@0.5 mean {avg[9]:.4f}, cnt {int(cnt[0])}")
        assert gap[gap > 0].min() > 1e-5, name
        out.update({name + "/output": o, name + "/target": t, name + "/acc": acc, name + "/avg_acc": avg, name + "/cnt": cnt})
        names.append(name)
    out["names"] = np.array(names)
    out["thresholds"] = np.asarray(THRESHOLDS, dtype=np.float64)
    path = os.path.join(OUT, "pck_curve.npz")
    np.savez_compressed(path, **out)
    print("pck_curve.npz written:", os.path.getsize(path), "bytes")


def groups():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    if "webcolors" not in sys.modules:
        wc = types.ModuleType("webcolors")
        wc.name_to_rgb = None
        sys.modules["webcolors"] = wc
    ds = load_by_path("ref_keypoint_dataset", "lib/datasets/keypoint_dataset.py")
    tables = {}
    for key, cls in (("body16", ds.Body16KeypointDataset), ("hand21", ds.Hand21KeypointDataset), ("animal18", ds.Animal18KeypointDataset),
                     ("animal14", ds.Animal14KeypointDataset)):
        tables[key] = {name: [int(i) for i in idx] for name, idx in cls(None, []).keypoints_group.items()}
    path = os.path.join(OUT, "joint_groups.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in tables.items()) + "\n}\n")
    print("joint_groups.json written:", {k: list(v) for k, v in tables.items()})


if __name__ == "__main__":
    curves(load_by_path("ref_kd", "lib/keypoint_detection.py"))
    groups()
