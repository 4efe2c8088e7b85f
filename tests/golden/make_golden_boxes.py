"""Golden vectors of the box helpers, made by RUNNING THE REFERENCE'S OWN get_bounding_box, scale_box and get_transform
(lib/datasets/util.py:87-123, 289-316; pure numpy / Python).

    python tests/golden/make_golden_boxes.py

Writes boxes.npz next to this file (data only; the reference's module is loaded by path at run time, with an empty stand-in for the cv2
module its file imports, and none of its text is stored):
  kp [N,K,2], image_wh [N,2]      seeded key points and frame sizes: people in the middle of the frame and people pushed against each of
                                  its four edges, where scale_box(pad=False) moves the square back inside
  bbox [N,4]                      get_bounding_box(kp[n])
  scaled [N,4]                    scale_box(bbox[n], width, height, 1.5) = (left, upper, right, lower), inclusive pixel indices
  center [N,2], scale [N], rot [N], res [N,2], matrix [N,3,3]
                                  get_transform(center, scale, res, rot) with rot cycling through {0, 30, -45, 90} and res = (rows, cols)
"""
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import load_by_path  # noqa: E402  (the reference checkout it reads is named there)

N, K = 40, 16
ROTS = (0, 30, -45, 90)
EDGES = ("middle", "left", "right", "top", "bottom")


def main():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    ref = load_by_path("ref_dutil", "lib/datasets/util.py")
    rs = np.random.RandomState(17)
    kp = np.zeros((N, K, 2))
    wh = np.zeros((N, 2), np.int64)
    bbox, scaled = np.zeros((N, 4)), np.zeros((N, 4))
    center, scale, rot, res, matrix = np.zeros((N, 2)), np.zeros(N), np.zeros(N), np.zeros((N, 2), np.int64), np.zeros((N, 3, 3))
    moved = {e: 0 for e in EDGES}
    for n in range(N):
        w, h = int(rs.randint(200, 1000)), int(rs.randint(200, 1000))
        ext = rs.uniform(0.1, 0.5, 2) * (w, h)                    # the person's extent
        edge = EDGES[n % len(EDGES)]
        lo = np.array([rs.uniform(0.3, 0.5) * (w - ext[0]), rs.uniform(0.3, 0.5) * (h - ext[1])])
        if edge == "left":
            lo[0] = rs.uniform(0, 3)
        elif edge == "right":
            lo[0] = w - 1 - ext[0] - rs.uniform(0, 3)
        elif edge == "top":
            lo[1] = rs.uniform(0, 3)
        elif edge == "bottom":
            lo[1] = h - 1 - ext[1] - rs.uniform(0, 3)
        p = lo + rs.uniform(0, 1, (K, 2)) * ext
        p[0], p[1] = lo, lo + ext                                  # the extremes are reached
        kp[n], wh[n] = p, (w, h)
        bbox[n] = ref.get_bounding_box(p)
        scaled[n] = ref.scale_box(tuple(bbox[n]), w, h, 1.5)
        side = scaled[n, 2] - scaled[n, 0] + 1
        free = (round((bbox[n, 0] + bbox[n, 2]) / 2 - side / 2), round((bbox[n, 1] + bbox[n, 3]) / 2 - side / 2))
        if (scaled[n, 0], scaled[n, 1]) != free:
            moved[edge] += 1
        center[n] = ((bbox[n, 0] + bbox[n, 2]) / 2, (bbox[n, 1] + bbox[n, 3]) / 2)
        scale[n] = max(bbox[n, 2] - bbox[n, 0], bbox[n, 3] - bbox[n, 1]) / 200.0 * 1.25
        rot[n] = ROTS[n % len(ROTS)]
        res[n] = (256, 256) if n % 3 else (64, 64)
        matrix[n] = ref.get_transform(center[n], scale[n], [int(res[n, 0]), int(res[n, 1])], rot=rot[n])
    print("boxes that scale_box moved back inside the frame, by the edge the person is pushed against:", moved)
    assert all(moved[e] > 0 for e in EDGES[1:]), moved
    path = os.path.join(OUT, "boxes.npz")
    np.savez_compressed(path, kp=kp, image_wh=wh, bbox=bbox, scaled=scaled, center=center, scale=scale, rot=rot, res=res, matrix=matrix)
    print("boxes.npz written:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
