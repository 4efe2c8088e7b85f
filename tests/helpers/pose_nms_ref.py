"""A numpy restatement of the instance layer (include/udapose.h: udapose_pose_rescore, udapose_oks_matrix,
udapose_pose_nms_sweep), and the construction of the GPU tests' inputs.

Rescoring, areas, refusals and the order are sequential fp32, the device's own operations in the device's order: they compare bit for
bit.  OKS is float64 on the fp32 inputs; the device's fp32 value is within `oks_tolerance(K)` of it.

The tolerance, from the expression (u = 2^-24, the unit round-off of fp32; every input is an fp32 number, so the float64 value is exact
up to ~1e-16):
  dx = x_i - x_j                      one rounding: relative error u                      (the same for dy)
  dx * dx, dy * dy                    2 u from dx, u of the product: 3 u
  d2 = dx * dx + dy * dy              a sum of non-negative terms keeps 3 u, u of the sum: 4 u
  v_k = (2 s_k) * (2 s_k)             2 s_k is exact, the product rounds: u
  A = (a_i + a_j) * 0.5f + eps        the sum u, the halving exact, the sum with eps u: 2 u (positive terms); a_j + eps alone: u
  e_k = d2 / v_k / A * 0.5f           4 u + u + u (the quotient) + 2 u + u (the quotient), the halving exact: 9 u; first order, so
                                      10 u covers the second-order terms by far
  exp(-e (1 + d)) - exp(-e)           at most e |d| exp(-e) <= |d| / 2.718: 10 u / 2.718 < 3.7 u absolute
  expf                                the device library's expf, at most 3 ulp (the bound OpenCL sets for exp, which the ROCm device
                                      library is built to); a term is <= 1, an ulp of it <= 2 u: 6 u absolute
  one term                            < 9.7 u absolute: 10 u
  K additions in ascending k          every partial sum is <= K: at most u K per addition, but the k-th partial sum is <= k: u K (K + 1) / 2
  / K (or / the visible count n, where K stands for n <= K below)   (10 u K + u K (K + 1) / 2) / K + u of the quotient
  total                               (11 + (K + 1) / 2) u            K = 17: 20 u = 1.2e-6; K = 64: 43.5 u = 2.6e-6
Nothing here was measured on the kernel.  Decisions (oks > oks_thr) are compared exactly instead: the constructed inputs keep every
same-frame pair at least 1e-3 from the threshold (asserted in float64), four hundred times the tolerance."""
import numpy as np

F32 = np.float32
FLT_EPSILON = float(np.finfo(np.float32).eps)
U = 2.0 ** -24


def oks_tolerance(K):
    return (11.0 + (K + 1) / 2.0) * U


def rescore_ref(conf, box_score=None, vis_thr=0.2):
    """score [M] fp32: the confidences above fp32(vis_thr) added in ascending k in fp32, divided by their count (0 for none), times
    box_score."""
    conf = np.asarray(conf, F32)
    M, K = conf.shape
    thr = F32(vis_thr)
    out = np.zeros(M, F32)
    with np.errstate(all="ignore"):
        for m in range(M):
            s, n = F32(0), 0
            for k in range(K):
                if conf[m, k] > thr:
                    s = F32(s + conf[m, k])
                    n += 1
            ks = F32(s / F32(n)) if n else F32(0)
            out[m] = F32(ks * (F32(1) if box_score is None else F32(box_score[m])))
    return out


def area_ref(boxes):
    b = np.asarray(boxes, F32)
    with np.errstate(all="ignore"):
        return (b[:, 2] * b[:, 3]).astype(F32)


def refused_ref(kp, area, score, status=None):
    kp = np.asarray(kp, F32)
    bad = ~np.isfinite(kp).all(axis=(1, 2)) | ~np.isfinite(area) | ~(area > 0) | ~np.isfinite(score)
    if status is not None:
        bad |= np.asarray(status) != 0
    return bad


def order_ref(score, refused):
    """Descending score, equal scores by ascending index; refused poses last, by ascending index."""
    idx = np.arange(len(score))
    good = sorted(idx[~refused], key=lambda m: (-float(score[m]), m))
    return np.asarray(good + list(idx[refused]), np.int32)


def _sig2(sigmas):
    s = np.asarray(sigmas, F32).astype(np.float64)
    return (2.0 * s) ** 2


def oks_self_ref(kp, area, sigmas):
    """[M,M] float64: mean_k exp(-d2_k / v_k / ((a_i + a_j) / 2 + eps) / 2); NaN where an operand is not finite."""
    kp = np.asarray(kp, F32).astype(np.float64)
    a = np.asarray(area, F32).astype(np.float64)
    v = _sig2(sigmas)
    M, K = kp.shape[:2]
    A = (a[:, None] + a[None, :]) * 0.5 + FLT_EPSILON
    acc = np.zeros((M, M))
    with np.errstate(all="ignore"):
        for k in range(K):
            d2 = (kp[:, None, k, 0] - kp[None, :, k, 0]) ** 2 + (kp[:, None, k, 1] - kp[None, :, k, 1]) ** 2
            acc += np.exp(-(d2 / v[k] / A * 0.5))
    return acc / K


def oks_rect_ref(kp_a, kp_b, area_b, visible_b, sigmas):
    """[Ma,Mb] float64, COCO's convention: the label's area, the mean over the label's visible joints, 0 for a label without one."""
    a = np.asarray(kp_a, F32).astype(np.float64)
    b = np.asarray(kp_b, F32).astype(np.float64)
    ar = np.asarray(area_b, F32).astype(np.float64) + FLT_EPSILON
    v = _sig2(sigmas)
    K = a.shape[1]
    vis = np.ones((b.shape[0], K), bool) if visible_b is None else np.asarray(visible_b) > 0
    acc = np.zeros((a.shape[0], b.shape[0]))
    for k in range(K):
        d2 = (a[:, None, k, 0] - b[None, :, k, 0]) ** 2 + (a[:, None, k, 1] - b[None, :, k, 1]) ** 2
        acc += np.exp(-(d2 / v[k] / ar[None, :] * 0.5)) * vis[None, :, k]
    n = vis.sum(1)
    return np.where(n[None, :] > 0, acc / np.maximum(n, 1)[None, :], 0.0)


def same_frame_oks(kp, area, sigmas, frame, refused):
    """{frame: (indices, their oks_self_ref)} over the poses that are not refused: all the walk needs, and all M = 4096 affords."""
    frame = np.zeros(len(area), np.int64) if frame is None else np.asarray(frame)
    out = {}
    for f in np.unique(frame):
        idx = np.nonzero((frame == f) & ~refused)[0]
        if idx.size:
            out[int(f)] = (idx, oks_self_ref(np.asarray(kp)[idx], np.asarray(area)[idx], sigmas))
    return out


def min_margin(blocks, oks_thr):
    """The smallest |oks - fp32(oks_thr)| over the same-frame pairs i != j."""
    thr = float(F32(oks_thr))
    best = np.inf
    for idx, o in blocks.values():
        if idx.size > 1:
            off = ~np.eye(idx.size, dtype=bool)
            best = min(best, float(np.abs(o[off] - thr).min()))
    return best


def walk_ref(blocks, order, refused, oks_thr, M):
    """The greedy walk -> (keep [M] uint8, n_keep, suppressed_by [M] int32)."""
    thr = float(F32(oks_thr))
    where = {}
    for f, (idx, o) in blocks.items():
        for r, m in enumerate(idx):
            where[int(m)] = (f, r)
    keep, removed, sby = np.zeros(M, np.uint8), np.zeros(M, bool), np.full(M, -1, np.int32)
    for m in order:
        m = int(m)
        if refused[m] or removed[m]:
            continue
        keep[m] = 1
        f, r = where[m]
        idx, o = blocks[f]
        hit = idx[(o[r] > thr) & (idx != m)]
        new = hit[~removed[hit]]
        sby[new] = m
        removed[hit] = True
    return keep, int(keep.sum()), sby


def nms_ref(kp, conf, boxes, frame=None, status=None, box_score=None, sigmas=None, oks_thr=0.9, vis_thr=0.2):
    """Everything udapose_pose_nms returns, and the margin of the decisions."""
    score = rescore_ref(conf, box_score, vis_thr)
    area = area_ref(boxes)
    refused = refused_ref(kp, area, score, status)
    order = order_ref(score, refused)
    blocks = same_frame_oks(kp, area, sigmas, frame, refused)
    keep, n_keep, sby = walk_ref(blocks, order, refused, oks_thr, len(score))
    return {"score": score, "area": area, "refused": refused, "order": order, "keep": keep, "n_keep": n_keep, "suppressed_by": sby,
            "margin": min_margin(blocks, oks_thr)}


# ------------------------------------------------------------------------------------------------------------------------ constructed inputs
SIGMA = 0.0669          # uniform (lib.keypoint_detection.OKS_UNIFORM_SIGMA)
SIDE = 100.0            # every box is SIDE x SIDE: equal areas
PITCH = 80.0            # the grid of base poses: oks of two bases = exp(-PITCH^2 / (2 v A)) = exp(-17.9) - far below 0.05, and a 0.80
#                         duplicate of one base is still PITCH - 2 r(0.80) = 62 px from any pose of another: oks <= exp(-10.8)


def offset_length(q, sigma=SIGMA, area=SIDE * SIDE):
    """r with exp(-r^2 / (2 v A)) = q, v = (2 sigma)^2, A = area + eps: a duplicate whose every joint is r away has oks q."""
    v = (2.0 * float(F32(sigma))) ** 2
    return float(np.sqrt(-2.0 * v * (area + FLT_EPSILON) * np.log(q)))


def joint_layout(K):
    """The base pose's joints round its centre: the same for every base, so two bases differ by their grid displacement in every joint."""
    k = np.arange(K)
    return np.stack([30.0 * np.cos(2.4 * k), 30.0 * np.sin(2.4 * k)], axis=1)


def base_pose(g, K, cols=40):
    return np.asarray([PITCH * (1 + g % cols), PITCH * (1 + g // cols)])[None, :] + joint_layout(K)


def duplicate(pose, q, twist=0.0):
    """pose + a per-joint offset of length offset_length(q), its direction turning with the joint."""
    k = np.arange(pose.shape[0])
    ang = 0.7 * k + twist
    return pose + offset_length(q) * np.stack([np.cos(ang), np.sin(ang)], axis=1)


def grouped_case(M, K, frames=3):
    """M poses in G = ceil(M / 3) groups of base, 0.95 duplicate, 0.80 duplicate: pose m has role m // G of group m % G, which lies on
    frame (m % G) % frames - the members of a group are G indices apart (other mask words for G > 21), the frames interleave.
    Confidences are one value per pose from a fixed scramble of [0.3, 0.9] (so who leads a group varies), with every fifth joint at 0.05:
    all at least 0.05 from vis_thr = 0.2.  Returns fp32 arrays kp, conf, boxes and int32 frame."""
    G = (M + 2) // 3
    kp, conf, boxes, frame = np.zeros((M, K, 2)), np.zeros((M, K)), np.zeros((M, 5)), np.zeros(M, np.int32)
    for m in range(M):
        role, g = m // G, m % G
        base = base_pose(g, K)
        kp[m] = base if role == 0 else duplicate(base, 0.95 if role == 1 else 0.80, twist=0.4 * role)
        c = 0.3 + 0.6 * ((m * 0.6180339887) % 1.0)
        conf[m] = c
        conf[m, (np.arange(K) + m) % 5 == 0] = 0.05
        boxes[m] = (kp[m, :, 0].mean(), kp[m, :, 1].mean(), SIDE, SIDE, 0.0)
        frame[m] = g % frames
    return kp.astype(F32), conf.astype(F32), boxes.astype(F32), frame
