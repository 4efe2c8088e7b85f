"""Golden vectors of the soft-max heat-map losses, made by RUNNING THE REFERENCE'S OWN lib/models/loss.py on the CPU.

    python tests/golden/make_golden_softmax_losses.py

Writes softmax_losses.npz next to this file: seeded inputs and the reference's results (data only; the reference's module is
loaded by path at run time and none of its text is stored).  Two map sizes, 16x16 (HW % 4 == 0) and 7x9 (ragged); the
inputs hold a zero target_weight, an all-zero label row (finite with epsilon > 0, NaN with epsilon = 0), masked (b,k) rows, a
(b,h,w) valid_mask, logits of magnitude 80, and entropy thresholds that select some rows and none.
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import load_by_path  # noqa: E402  (the reference checkout it reads is named there)

SIZES = ((16, 16), (7, 9))
B, K = 3, 5


def inputs(H, W, seed):
    rs = np.random.RandomState(seed)
    scale = rs.uniform(0.3, 6.0, size=(B, K, 1, 1))              # rows from nearly flat to peaked: entropies spread over (0, 1)
    stu = (rs.randn(B, K, H, W) * scale).astype(np.float32)
    tea = (rs.randn(B, K, H, W) * scale + 0.3 * rs.randn(B, K, H, W)).astype(np.float32)
    stu[1, 2] = rs.choice([-80.0, 80.0], size=(H, W)).astype(np.float32) + rs.randn(H, W).astype(np.float32)
    tea[2, 0] = (80.0 * rs.randn(H, W)).astype(np.float32)
    label = np.exp(-rs.uniform(0, 12, size=(B, K, H, W))).astype(np.float32)
    label[label < 0.02] = 0.0                                     # exact zeros: xlogy(0, 0) = 0 with epsilon = 0
    label[0, 3] = 0.0                                             # an all-zero label row
    weight = (rs.rand(B, K, 1) > 0.2).astype(np.float32)
    weight[2, 1] = 0.0
    weight[0, 0] = 1.0
    tea_mask = rs.rand(B, K) > 0.4
    tea_mask[1, 1], tea_mask[1, 2] = False, True
    valid = rs.rand(B, H, W) > 0.35
    return stu, tea, label, weight, tea_mask, valid


def main():
    ref = load_by_path("ref_loss", "lib/models/loss.py")
    out = {"sizes": np.array(SIZES)}
    T = torch.from_numpy
    for ci, (H, W) in enumerate(SIZES):
        stu, tea, label, weight, tea_mask, valid = inputs(H, W, 40 + ci)
        pre = f"c{ci}_"
        out.update({pre + "stu": stu, pre + "tea": tea, pre + "label": label, pre + "weight": weight, pre + "tea_mask": tea_mask,
                    pre + "valid": valid})

        def rec(name, v):
            out[pre + name] = np.asarray(v.detach().numpy(), dtype=np.float32)

        label_pos = label.copy()
        label_pos[0, 3] = label[0, 2]                             # (no all-zero row: epsilon = 0 stays finite)
        for eps_name, eps, lab in (("eps", 1e-6, label), ("eps0", 0.0, label), ("eps0pos", 0.0, label_pos)):
            for red in ("mean", "none"):
                rec(f"kl_{eps_name}_{red}_w", ref.JointsKLLoss(red, eps)(T(stu), T(lab), T(weight)))
                rec(f"kl_{eps_name}_{red}", ref.JointsKLLoss(red, eps)(T(stu), T(lab)))
        out[pre + "label_pos"] = label_pos
        assert ref.JointsKLLoss("sum")(T(stu), T(label)) is None
        ent = ref.EntLoss("none")
        rows = -(torch.softmax(T(stu).reshape(B, K, -1), -1) * torch.log_softmax(T(stu).reshape(B, K, -1), -1)).sum(-1) / np.log(H * W)
        srt = np.sort(rows.numpy().reshape(-1))
        thr_some, thr_none = float((srt[6] + srt[7]) / 2), float(srt[0] / 2)   # between two rows' values: no tie to break
        out[pre + "thr_some"], out[pre + "thr_none"] = np.float64(thr_some), np.float64(thr_none)
        for red in ("mean", "none"):
            rec(f"ent_{red}", ref.EntLoss(red)(T(stu)))
            rec(f"ent_{red}_some", ref.EntLoss(red)(T(stu), thr_some))
            rec(f"ent_{red}_none", ref.EntLoss(red)(T(stu), thr_none))
        assert ent(T(stu)).shape == (B,)
        for cls, tag in ((ref.ConsSoftmaxLoss, "csm"), (ref.ConsKLLoss, "ckl")):
            rec(f"{tag}_plain", cls()(T(stu).clone(), T(tea).clone()))
            rec(f"{tag}_mask", cls()(T(stu).clone(), T(tea).clone(), tea_mask=T(tea_mask)))
            rec(f"{tag}_valid", cls()(T(stu).clone(), T(tea).clone(), valid_mask=T(valid)))
            rec(f"{tag}_both", cls()(T(stu).clone(), T(tea).clone(), valid_mask=T(valid), tea_mask=T(tea_mask)))
        # the reference's ConsKLLoss on inputs of more than one pixel: recorded as found
        print(f"{H}x{W}: ConsKLLoss ->", [float(out[pre + f'ckl_{n}']) for n in ("plain", "mask", "valid", "both")],
              "| EntLoss thresholds", thr_some, thr_none, "| kl eps0:", float(out[pre + "kl_eps0_mean"]), float(out[pre + "kl_eps0pos_mean"]))
    np.savez_compressed(os.path.join(OUT, "softmax_losses.npz"), **out)
    print("softmax_losses.npz written:", os.path.getsize(os.path.join(OUT, "softmax_losses.npz")), "bytes")


if __name__ == "__main__":
    main()
