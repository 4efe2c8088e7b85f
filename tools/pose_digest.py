"""Dev tool: one SHA-256 per output tensor of every instance-layer entry point (csrc/pose_nms.hip, csrc/pose_ap.hip) on
fixed, seeded inputs - to `diff` between two builds of the library (this tree's and a git worktree's of another commit) on ONE box in one
session, as tools/bn_forms_digest.py does for the BatchNorm forms.  Every kernel here is deterministic (fixed summation orders, integer
atomics only), so a refactor must leave every line identical; the digests are not expected values and belong in no test.  Unlike the tests'
inputs, these hold equal scores, refused entries and OKS values at and next to the thresholds (a threshold is one of the matrix's own values).

    python tools/pose_digest.py [LIBRARY] > digest.txt     # LIBRARY: the libudapose_hip.so to load (default: this tree's)

Line: <case>[<output>] <sha256 or integer>."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uda_poseestimation_amd import _hip  # noqa: E402

if len(sys.argv) > 1:
    _hip.LIB_PATHS["bf16"] = os.path.abspath(sys.argv[1])      # (the instance layer is fp32: both builds export identical code)
L, p, st = _hip.lib(), _hip.ptr, _hip.stream
SIGMA = 0.0669


def emit(case, outs):
    for name, t in outs.items():
        if isinstance(t, int):
            print(f"{case}[{name}] {t}", flush=True)
        else:
            print(f"{case}[{name}] {hashlib.sha256(t.contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()}", flush=True)


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def zeros(shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def call(code, what):
    assert code == 0, (what, code)


def poses(M, K, seed):
    """Groups of four near copies on three frames, confidences from five levels (equal scores), and refused poses of every kind."""
    rs = np.random.RandomState(seed)
    G = (M + 3) // 4
    base = np.stack([300.0 * (1 + np.arange(G) % 8), 300.0 * (1 + np.arange(G) // 8)], axis=1)[:, None, :] + rs.uniform(-60, 60, (G, K, 2))
    g = np.arange(M) % G
    kp = base[g] + rs.uniform(-6, 6, (M, K, 2)) * (np.arange(M) // G > 0)[:, None, None]
    conf = np.asarray([0.1, 0.3, 0.5, 0.5, 0.9])[rs.randint(0, 5, (M, K))] * (rs.uniform(0, 1, (M, 1)) > 0.3) + 0.25 * (np.arange(M) % 2)[:, None]
    boxes = np.stack([kp[..., 0].mean(1), kp[..., 1].mean(1), np.full(M, 90.0), 80.0 + 10.0 * (np.arange(M) % 3), np.zeros(M)], axis=1)
    status = (np.arange(M) % 13 == 7).astype(np.uint8)
    if M > 4:
        kp[3, K // 2, 1] = np.nan
        boxes[4, 2] = 0.0
    if M > 40:
        boxes[37, 3] = np.inf
        conf[40] = np.nan
    return dev(kp), dev(conf), dev(boxes), dev(g % 3, np.int32), dev(status, np.uint8), dev(0.5 + 0.25 * (np.arange(M) % 3))


def nms_cases():
    vthr = dev([0.2])
    for M in (1, 17, 64, 65, 257, 1030):
        for K in (1, 17, 64):
            case = f"M{M}_K{K}"
            kp, conf, boxes, frame, status, bscore = poses(M, K, 1000 * K + M)
            sg = dev(np.full(K, SIGMA) * (1 + 0.1 * (np.arange(K) % 4)))
            W = (M + 63) // 64
            score, area, order, refused = zeros(M), zeros(M), zeros(M, torch.int32), zeros(M, torch.uint8)
            call(L.udapose_pose_rescore(st(), p(kp), p(conf), p(boxes), p(status), p(bscore), p(vthr), M, K, p(score), p(order), p(area), p(refused)),
                 "rescore")
            emit(f"rescore_{case}", {"score": score, "order": order, "area": area, "refused": refused})
            a = torch.nan_to_num(area, nan=1.0, posinf=1.0).clamp_min(1.0)
            out = zeros((M, M))
            call(L.udapose_oks_matrix(st(), p(kp), p(a), M, None, None, None, M, K, p(sg), None, None, None, p(out), None), "oks self")
            same = (frame[:, None] == frame[None, :]) & ~torch.eye(M, dtype=torch.bool, device="cuda") & ~torch.isnan(out)
            vals = out[same].sort().values
            othr = vals[(3 * vals.numel()) // 4].reshape(1).clone() if vals.numel() else dev([0.9])      # one of the matrix's own values
            mask, out2, mask2 = zeros((M, W), torch.int64), zeros((M, M)), zeros((M, W), torch.int64)
            call(L.udapose_oks_matrix(st(), p(kp), p(a), M, None, None, None, M, K, p(sg), p(frame), p(refused), p(othr), None, p(mask)), "oks mask")
            call(L.udapose_oks_matrix(st(), p(kp), p(a), M, None, None, None, M, K, p(sg), p(frame), p(refused), p(othr), p(out2), p(mask2)), "oks both")
            emit(f"oks_self_{case}", {"matrix": out, "thr": othr, "mask": mask, "matrix_with_mask": out2, "mask_with_matrix": mask2})
            Mb = max(1, (2 * M) // 3)
            kb, ab = kp[:Mb].flip(0).contiguous() + 2.0, a[:Mb].flip(0).contiguous()
            vis = dev(np.random.RandomState(M + K).uniform(-0.5, 1.0, (Mb, K)) * (np.arange(Mb) % 5 != 2)[:, None])
            r1, r2 = zeros((M, Mb)), zeros((M, Mb))
            call(L.udapose_oks_matrix(st(), p(kp), None, M, p(kb), p(ab), None, Mb, K, p(sg), None, None, None, p(r1), None), "oks rect")
            call(L.udapose_oks_matrix(st(), p(kp), None, M, p(kb), p(ab), p(vis), Mb, K, p(sg), None, None, None, p(r2), None), "oks rect vis")
            emit(f"oks_rect_{case}", {"all_joints": r1, "visible": r2})
            keep, n_keep, sby = zeros(M, torch.uint8), zeros(1, torch.int32), zeros(M, torch.int32)
            call(L.udapose_pose_nms_sweep(st(), p(mask), p(order), p(refused), M, p(keep), p(n_keep), None), "sweep")
            emit(f"sweep_{case}", {"keep": keep, "n_keep": int(n_keep.item())})
            keep.zero_()
            call(L.udapose_pose_nms_sweep(st(), p(mask), p(order), p(refused), M, p(keep), p(n_keep), p(sby)), "sweep sby")
            emit(f"sweep_sby_{case}", {"keep": keep, "n_keep": int(n_keep.item()), "suppressed_by": sby})
            ws = zeros(L.udapose_pose_nms_ws_bytes(M) // 8 + 1, torch.int64)
            score, order, keep, sby, full = zeros(M), zeros(M, torch.int32), zeros(M, torch.uint8), zeros(M, torch.int32), zeros((M, M))
            call(L.udapose_pose_nms(st(), p(kp), p(conf), p(boxes), p(frame), p(status), p(bscore), p(sg), p(vthr), p(othr), M, K, p(ws), p(score),
                                    p(order), p(keep), p(n_keep), p(sby), p(full)), "pose_nms")
            emit(f"pose_nms_{case}", {"score": score, "order": order, "keep": keep, "n_keep": int(n_keep.item()), "suppressed_by": sby, "oks": full})


def ap_update(M, G, F, K, seed):
    """Labels on a grid, detections jittered copies of a label of their frame (oks spread over the thresholds) or poses of their own; scores
    from eight levels; refused detections and labels of every kind."""
    rs = np.random.RandomState(seed)
    gkp = np.stack([300.0 * (1 + np.arange(G) % 16), 300.0 * (1 + np.arange(G) // 16)], axis=1)[:, None, :] + rs.uniform(-50, 50, (G, K, 2))
    gframe, frame = rs.randint(0, F, G), rs.randint(0, F, M)
    pick = rs.randint(0, G, M)
    near = np.flatnonzero(rs.uniform(0, 1, M) < 0.8)
    for m in near:
        mine = np.flatnonzero(gframe == frame[m])
        if mine.size:
            pick[m] = mine[rs.randint(0, mine.size)]
    kp = gkp[pick] + rs.uniform(-1, 1, (M, K, 2)) * rs.choice([2.0, 5.0, 9.0, 14.0], (M, 1, 1))
    kp[rs.uniform(0, 1, M) < 0.15] += 4000.0
    score = 0.2 + 0.1 * rs.randint(0, 8, M)
    valid, garea = np.ones(M, np.uint8), rs.choice([20.0 ** 2, 31.0 ** 2, 33.0 ** 2, 60.0 ** 2, 95.0 ** 2, 97.0 ** 2, 140.0 ** 2], G)
    gvis = (rs.uniform(0, 1, (G, K)) > 0.25) * (np.arange(G) % 9 != 4)[:, None]
    if M > 8:
        valid[5], score[6], frame[7], kp[8, 0, 0] = 0, np.nan, F, np.inf
        gframe[G // 2] = -1
    return [dev(kp), dev(score), dev(frame, np.int32), dev(valid, np.uint8), dev(gkp), dev(gvis), dev(garea), dev(gframe, np.int32),
            dev(np.arange(G) % 7 == 3, np.uint8)]


def ap_cases():
    thr, ranges = dev(np.linspace(0.5, 0.95, 10)), dev([[0, 1e10], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]])
    rp = dev(np.linspace(0.0, 1.0, 101), np.float64)
    T, A, R, cap = len(thr), len(ranges), len(rp), 8192
    runs = [("M40_G12_F3_K17", [(40, 12, 3, 17, 1)]), ("M40_G12_F3_K1", [(40, 12, 3, 1, 2)]), ("M40_G12_F3_K64", [(40, 12, 3, 64, 3)]),
            ("M300_G90_F22_K17", [(300, 90, 22, 17, 4)]), ("sequence_K17", [(300, 90, 22, 17, 10 + i) for i in range(18)] + [(40, 12, 3, 17, 5)])]
    for case, updates in runs:
        K = updates[0][3]
        sg = dev(np.full(K, SIGMA) * (1 + 0.1 * (np.arange(K) % 4)))
        rs_, rm, ri = zeros(cap + 1), zeros(cap + 1, torch.int64), zeros(cap + 1, torch.int64)
        cnt = zeros(6 + A, torch.int64)
        for n, (M, G, F, _, seed) in enumerate(updates):
            kp, score, frame, valid, gkp, gvis, garea, gframe, gign = ap_update(M, G, F, K, seed)
            ws = zeros(L.udapose_ap_match_ws_bytes(M, G, F) // 8 + 1, torch.int64)
            call(L.udapose_ap_match(st(), p(kp), p(score), p(frame), p(valid), None, M, p(gkp), p(gvis), p(garea), p(gframe), p(gign), G, K, F, p(sg),
                                    p(thr), T, p(ranges), A, 20, p(ws), p(rs_), p(rm), p(ri), cap, p(cnt)), "ap_match")
            if n in (0, len(updates) - 1):
                emit(f"ap_match_{case}_update{n}", {"order": ws.view(torch.int32)[:M], "counters": cnt})
        N = int(cnt[0].item())
        emit(f"ap_match_{case}", {"records": N, "score": rs_[:N], "matched": rm[:N], "ignored": ri[:N], "counters": cnt})
        ws = zeros(L.udapose_ap_curve_ws_bytes(cap, T, A) // 8 + 1, torch.int64)
        pr, sc, rc = zeros((T, R, A), torch.float64), zeros((T, R, A)), zeros((T, A), torch.float64)
        call(L.udapose_ap_curve(st(), p(rs_), p(rm), p(ri), cap, p(cnt), T, A, p(rp), R, p(ws), p(pr), p(sc), p(rc)), "ap_curve")
        emit(f"ap_curve_{case}", {"precision": pr, "scores": sc, "recall": rc, "sorted_score": ws.view(torch.float32)[:N]})


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU"
    nms_cases()
    ap_cases()
