"""Plain-torch CPU restatement of the flip test's heat-map side (csrc/flip.hip, udapose_flip_merge), written from the formulas in
include/udapose.h: fb[n][k][y][x] = f[n][perm[k]][y][W-1-x]; s = fb, or fb moved one pixel to the right with column 0 kept; out = s or
(a + s) * 0.5.  The merge is one fp32 add and an exact halving, so the device must agree bit for bit."""
import torch


def perm_from_pairs(pairs, K):
    """perm[i] = j, perm[j] = i for every pair; the identity elsewhere."""
    perm = list(range(K))
    for i, j in pairs:
        perm[i], perm[j] = j, i
    return perm


def guard(perm, K):
    """The kernel's table rule: an entry outside [0, K) counts as k itself."""
    return [p if 0 <= p < K else k for k, p in enumerate(perm)]


def flip_back(f, perm, shift=False):
    fb = torch.flip(f, [3])[:, guard(list(perm), f.shape[1])]
    if shift:
        s = fb.clone()
        s[..., 1:] = fb[..., :-1]
        return s
    return fb.contiguous()


def flip_merge(a, f, perm, shift=False):
    return (a + flip_back(f, perm, shift)) * 0.5
