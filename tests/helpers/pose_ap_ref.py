"""A numpy restatement of the key-point AP meter (include/udapose.h: udapose_ap_match, udapose_ap_curve): cocoapi's
evaluateImg + accumulate for key points, as this project states them.

OKS is float64 on the fp32 inputs (pose_nms_ref.oks_rect_ref, imported); the device's fp32 value is within pose_nms_ref.oks_tolerance(K) of
it, so a decision `oks < best` against a threshold is the same on both sides when every pair is further from every threshold than that:
`min_margin` returns the smallest distance, and the GPU tests assert it is >= 1e-3 on their constructed inputs.  Everything else - areas,
refusals, orders, the walk, the record words, the counts, the curves in fp64 - is exact and compares with array_equal."""
import numpy as np

from helpers.pose_nms_ref import F32, oks_rect_ref

THRESHOLDS = np.linspace(.5, .95, 10)
AREA_RANGES = {"all": (0, 1e10), "medium": (32 ** 2, 96 ** 2), "large": (96 ** 2, 1e10)}
RECALL_POINTS = np.linspace(.0, 1.00, int(np.round(1.00 / .01)) + 1)
MAX_LABELS = 64
COUNT_NAMES = ("records", "dropped", "refused", "cut", "overflow_frames", "bad_labels")


def det_area_ref(kp):
    """cocoapi loadRes for key-point results, in fp32: (max x - min x) * (max y - min y) over all K joints."""
    kp = np.asarray(kp, F32)
    with np.errstate(all="ignore"):
        return ((kp[:, :, 0].max(1) - kp[:, :, 0].min(1)).astype(F32) * (kp[:, :, 1].max(1) - kp[:, :, 1].min(1)).astype(F32)).astype(F32)


class APRef:
    def __init__(self, num_keypoints, sigmas, thresholds=THRESHOLDS, area_ranges=AREA_RANGES, max_dets=20, recall_points=RECALL_POINTS,
                 capacity=65536):
        self.K = int(num_keypoints)
        self.sigmas = tuple(float(s) for s in sigmas)
        self.thr = np.asarray(thresholds, np.float64).astype(F32)
        self.names = tuple(area_ranges)
        self.ranges = np.asarray([area_ranges[n] for n in self.names], np.float64).astype(F32).reshape(-1, 2)
        self.max_dets, self.capacity = int(max_dets), int(capacity)
        self.rp = np.asarray(recall_points, np.float64)
        self.T, self.A = len(self.thr), len(self.ranges)
        self.score, self.matched, self.ignored = [], [], []
        self.npig = np.zeros(self.A, np.int64)
        self.counts = dict.fromkeys(COUNT_NAMES, 0)
        self.margin = np.inf

    def update(self, keypoints, score, frame_idx, gt_keypoints, gt_visible, gt_area, gt_frame, *, num_frames, area=None, valid=None, gt_ignore=None):
        kp, score, frame = np.asarray(keypoints, F32), np.asarray(score, F32), np.asarray(frame_idx).astype(np.int64)
        gkp, garea, gframe = np.asarray(gt_keypoints, F32), np.asarray(gt_area, F32), np.asarray(gt_frame).astype(np.int64)
        gvis = np.ones(gkp.shape[:2], F32) if gt_visible is None else np.asarray(gt_visible, F32)
        gign = np.zeros(len(garea), bool) if gt_ignore is None else np.asarray(gt_ignore) != 0
        F, T, A = int(num_frames), self.T, self.A
        refused = ~np.isfinite(score) | ~np.isfinite(kp).all(axis=(1, 2)) | (frame < 0) | (frame >= F)
        if valid is not None:
            refused |= np.asarray(valid) == 0
        if area is not None:
            darea = np.asarray(area, F32)
            refused |= ~np.isfinite(darea)
        else:
            darea = det_area_ref(kp)
        self.counts["refused"] += int(refused.sum())
        bad = (gframe < 0) | (gframe >= F)
        self.counts["bad_labels"] += int(bad.sum())
        thr64 = self.thr.astype(np.float64)
        for f in range(F):
            labels = np.nonzero((gframe == f) & ~bad)[0]
            dets = sorted(np.nonzero((frame == f) & ~refused)[0], key=lambda m: (-float(score[m]), m))
            if len(labels) > MAX_LABELS:
                self.counts["overflow_frames"] += 1
                continue
            self.counts["cut"] += max(0, len(dets) - self.max_dets)
            if len(dets) and len(labels):      # (the margin covers the detections that are cut as well)
                every = oks_rect_ref(kp[dets], gkp[labels], garea[labels], gvis[labels], self.sigmas)
                self.margin = min(self.margin, float(np.abs(every[:, :, None] - thr64[None, None, :]).min()))
            dets = dets[:self.max_dets]
            oks = oks_rect_ref(kp[dets], gkp[labels], garea[labels], gvis[labels], self.sigmas) if len(dets) and len(labels) else None
            no_joint = ~(gvis[labels] > 0).any(axis=1) if len(labels) else np.zeros(0, bool)
            m_words, i_words = np.zeros(len(dets), np.uint64), np.zeros(len(dets), np.uint64)
            for a in range(A):
                lo, hi = self.ranges[a]
                ign = gign[labels] | no_joint | (garea[labels] < lo) | (garea[labels] > hi)
                walk = [j for j in range(len(labels)) if not ign[j]] + [j for j in range(len(labels)) if ign[j]]
                self.npig[a] += int((~ign).sum())
                for t in range(T):
                    taken = set()
                    bit = np.uint64(1) << np.uint64(a * T + t)
                    for di, d in enumerate(dets):
                        best, m = float(self.thr[t]), -1
                        for j in walk:
                            if j in taken:
                                continue
                            if m > -1 and not ign[m] and ign[j]:
                                break
                            if oks[di, j] < best:
                                continue
                            best, m = oks[di, j], j
                        if m > -1:
                            taken.add(m)
                            m_words[di] |= bit
                            if ign[m]:
                                i_words[di] |= bit
                        elif darea[d] < lo or darea[d] > hi:
                            i_words[di] |= bit
            for di, d in enumerate(dets):
                if len(self.score) < self.capacity:
                    self.score.append(score[d])
                    self.matched.append(m_words[di])
                    self.ignored.append(i_words[di])
                else:
                    self.counts["dropped"] += 1
        self.counts["records"] = len(self.score)

    def records(self):
        return np.asarray(self.score, F32), np.asarray(self.matched, np.uint64), np.asarray(self.ignored, np.uint64)

    def tables(self):
        """precision [T,R,A] fp64, scores [T,R,A] fp32, recall [T,A] fp64 - cocoapi's accumulate."""
        T, A, R = self.T, self.A, len(self.rp)
        score, matched, ignored = self.records()
        N = len(score)
        order = np.argsort(-score, kind="mergesort")
        score, matched, ignored = score[order], matched[order], ignored[order]
        precision, scores, recall = -np.ones((T, R, A)), -np.ones((T, R, A), F32), -np.ones((T, A))
        for a in range(A):
            if self.npig[a] == 0:
                continue
            for t in range(T):
                bit = np.uint64(a * T + t)
                m = ((matched >> bit) & np.uint64(1)).astype(bool)
                g = ((ignored >> bit) & np.uint64(1)).astype(bool)
                tp = np.cumsum(m & ~g).astype(np.float64)
                fp = np.cumsum(~m & ~g).astype(np.float64)
                rc = tp / self.npig[a]
                pr = tp / (fp + tp + np.spacing(1))
                recall[t, a] = rc[-1] if N else 0
                pr = pr.tolist()
                for i in range(N - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                inds = np.searchsorted(rc, self.rp, side="left")
                q, ss = np.zeros(R), np.zeros(R, F32)
                for ri, pi in enumerate(inds):
                    if pi < N:
                        q[ri], ss[ri] = pr[pi], score[pi]
                precision[t, :, a], scores[t, :, a] = q, ss
        return precision, scores, recall

    def counters(self):
        return np.asarray([self.counts[n] for n in COUNT_NAMES] + list(self.npig), np.int64)


def min_margin(ref):
    """The smallest |oks - fp32(thr_t)| over all same-frame (detection, label) pairs and all t that the updates of `ref` met."""
    return ref.margin
