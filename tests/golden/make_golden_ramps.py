"""Golden values of the four ramp functions, made by RUNNING THE REFERENCE'S OWN utils.sigmoid_rampup / cosine_rampdown / rev_sigmoid /
sigmoid (utils.py:28-52) on the CPU.

    python tests/golden/make_golden_ramps.py

Writes ramps.npz next to this file: the grid and the reference's float64 results (data only; the reference's module is loaded by path at run
time and none of its text is stored).  Grid: lengths 0, 1, 7 and 40, `current` from -2 to length + 2 in steps of 0.5; `progress` from -0.5
to 1.5 in steps of 0.05.  cosine_rampdown at length 0 is the reference's 0 / 0: NaN, recorded as such.
"""
import os
import sys
import warnings

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import load_by_path  # noqa: E402  (the reference checkout it reads is named there)

LENGTHS = (0, 1, 7, 40)


def grid():
    """-> ({length: current values}, progress values): exact binary fractions / the same np.arange expression on both sides."""
    current = {L: np.arange(-2.0, L + 2.0 + 0.25, 0.5) for L in LENGTHS}
    progress = np.arange(-10, 31) * 0.05
    return current, progress


def main():
    ref = load_by_path("ref_utils", "utils.py")
    current, progress = grid()
    out = {"lengths": np.array(LENGTHS, np.int64), "progress": progress}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # (0 / 0 at length 0)
        for L in LENGTHS:
            out[f"current/{L}"] = current[L]
            out[f"sigmoid_rampup/{L}"] = np.array([ref.sigmoid_rampup(float(c), L) for c in current[L]], np.float64)
            out[f"cosine_rampdown/{L}"] = np.array([ref.cosine_rampdown(float(c), L) for c in current[L]], np.float64)
    out["rev_sigmoid"] = np.array([ref.rev_sigmoid(float(p)) for p in progress], np.float64)
    out["sigmoid"] = np.array([ref.sigmoid(float(p)) for p in progress], np.float64)
    path = os.path.join(OUT, "ramps.npz")
    np.savez_compressed(path, **out)
    print("ramps.npz written:", os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
