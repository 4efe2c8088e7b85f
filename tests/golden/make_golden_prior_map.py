"""Golden vectors of the skeleton prior, made by RUNNING THE REFERENCE'S OWN utils.generate_prior_map (utils.py:111-145) on the CPU.

    python tests/golden/make_golden_prior_map.py

Writes prior_map.npz next to this file: seeded inputs (tests/helpers/prior_map_fp64.case_inputs) and the reference's fp32 results in both modes
(data only; the reference's module is loaded by path at run time and none of its text is stored).  The function sends its tables and its grid
to the device with .cuda(); for this run torch.Tensor.cuda is the identity.  Cases: five map shapes with H != W among them at the default
(gamma, sigma), two at another setting, one std with infinite entries, one plane whose maximum is negative.
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
from make_golden import load_by_path  # noqa: E402  (the reference checkout it reads is named there)
from helpers import prior_map_fp64 as P64  # noqa: E402


def main():
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        ref = load_by_path("ref_utils", "utils.py")
        out, names = {}, []
        for name, shape, seed, gamma, sigma, inf_std, neg in P64.golden_cases():
            preds, mean, std = P64.case_inputs(shape, seed, inf_std, neg)
            pre = name + "/"
            out.update({pre + "preds": preds, pre + "mean": mean, pre + "std": std, pre + "gamma": np.float64(gamma), pre + "sigma": np.float64(sigma)})
            for v3 in (False, True):
                prior = {"mean": torch.from_numpy(mean.copy()), "std": torch.from_numpy(std.copy())}
                got = ref.generate_prior_map(prior, torch.from_numpy(preds.copy()), gamma=gamma, sigma=sigma, v3=v3)
                assert got.dtype == torch.float32 and tuple(got.shape) == shape and bool(torch.isfinite(got).all()), name
                out[pre + ("v3" if v3 else "default")] = got.numpy()
            names.append(name)
            print(f"{name}: max default {float(out[pre + 'default'].max()):.4f}, max v3 {float(out[pre + 'v3'].max()):.4f}")
        out["names"] = np.array(names)
    finally:
        torch.Tensor.cuda = real_cuda
    path = os.path.join(OUT, "prior_map.npz")
    np.savez_compressed(path, **out)
    print("prior_map.npz written:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
