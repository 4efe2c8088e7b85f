"""Dev tool: one SHA-256 per output tensor of the entry points whose kernels changed their instruction text when the block sum moved into
csrc/common.h (block_sum) and that tools/plan_digest.py, step_digest.py, bn_forms_digest.py and conv_forms_digest.py do not reach:
udapose_grad_sumsq / udapose_grad_clip, udapose_perturb (its two sum-of-squares launches), udapose_feat_mse_fwd, udapose_style_stat_loss,
the heat-map row sums (udapose_joints_mse_fwd, udapose_cons_loss_valid_fwd, udapose_mask_count) and the contrast mean of udapose_aug_color_op.
Both builds, seeded CPU-generated inputs, millisecond shapes: per entry point one whose element count is no multiple of the block's stride
and one smaller than a wave.  Every kernel here is deterministic (fixed summation orders, no atomics), so every line must be identical between
two trees; the digests are not expected values and belong in no test.

    python tools/pointwise_digest.py [--tree ROOT] > digest.txt     # ROOT: the tree whose package and libraries are loaded (default: this one)

Line: <build> <case>[<output>] <sha256>."""
import argparse
import ctypes as C
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402
from uda_poseestimation_amd import _hip  # noqa: E402
from uda_poseestimation_amd.utils import _MultiTensorTable  # noqa: E402

ELEM = {"bf16": torch.bfloat16, "fp16": torch.float16}
ptr, check, stream = _hip.ptr, _hip.check, _hip.stream


def emit(build, case, outs):
    for name, t in outs.items():
        if t is not None:
            print(f"{build} {case}[{name}] {hashlib.sha256(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()}", flush=True)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).cuda()


def grad_clip(build, L):
    """two parameter groups of a few tensors each; a group's gradients lie in row 0 of one [2][total] buffer and the second per-pass buffer
    in row 1, 4 * total bytes behind (g2 = 1; 36000 bytes: the 16-byte loads, 20164: the scalar ones)"""
    for name, sizes in (("ragged", ((5003, 37, 1), (9000,))), ("small", ((37,), (5,)))):
        for g2 in (0, 1):
            g = gen(11 + g2)
            bufs, tables, states, deltas = [], [], [], []
            for gi, group in enumerate(sizes):
                total = sum(group)
                flat = randn((2, total), g, 0.1 * (gi + 1))
                views, o = [], 0
                for n in group:
                    views.append(flat[0, o:o + n])
                    o += n
                bufs.append(flat)
                tables.append(_MultiTensorTable([views]))
                deltas.append(4 * total if g2 else 0)
                states.append(torch.tensor([0, 0, 0, 0, 0.5 * (gi + 1), 0, 2.0, 0], dtype=torch.float32, device="cuda"))
            part = torch.zeros(sum(t.nblocks for t in tables), dtype=torch.float64, device="cuda")
            begin, end, b = [], [], 0
            for t, st, delta in zip(tables, states, deltas):
                check(L.udapose_grad_sumsq(stream(), ptr(t.ptrs[0]), ptr(t.sizes), ptr(t.blk_t), ptr(t.blk_o), t.nblocks, delta, ptr(st),
                                           part.data_ptr() + 8 * b), "grad_sumsq")
                begin.append(b)
                b += t.nblocks
                end.append(b)
            clip = torch.zeros(12, dtype=torch.float32, device="cuda")
            clip[0] = 0.25
            n = len(tables)
            sp = (C.c_void_p * n)(*[s.data_ptr() for s in states])
            check(L.udapose_grad_clip(stream(), ptr(part), (C.c_int * n)(*begin), (C.c_int * n)(*end), n, sp, ptr(clip)), "grad_clip")
            emit(build, f"grad_clip_{name}_g2{g2}", {"partials": part, "clip": clip, "state0": states[0], "state1": states[1]})


def perturb(build, L):
    """HW % 4 == 0: the 16-byte kernels, otherwise the scalar ones; one step (one norm launch) and the projected form (two)"""
    for N, Cc, HW in ((2, 3, 1372), (2, 3, 1371), (3, 1, 20), (3, 1, 15), (1, 4, 70001)):
        g = gen(N * 100 + HW)
        x, gr, x0 = randn((N, Cc, HW), g), randn((N, Cc, HW), g, 3.0), randn((N, Cc, HW), g)
        eps, step = torch.tensor(0.7, device="cuda"), torch.tensor(0.4, device="cuda")
        ws = torch.zeros(max(L.udapose_perturb_ws_bytes(N, Cc, HW) // 4, 1), dtype=torch.float32, device="cuda")
        for form, a0, st in (("one_step", None, None), ("projected", x0, step)):
            out, gn = torch.zeros_like(x), torch.zeros(N, dtype=torch.float32, device="cuda")
            ws.zero_()
            check(L.udapose_perturb(stream(), ptr(x), ptr(gr), ptr(a0), N, Cc, HW, 0, ptr(eps), ptr(st), None, None, ptr(ws), ptr(out), ptr(gn)),
                  "perturb")
            emit(build, f"perturb_{form}_{N}x{Cc}x{HW}", {"out": out, "gnorm": gn, "ws": ws})


def style_losses(build, L):
    dt = ELEM[build]
    ws = torch.zeros(L.udapose_feat_mse_ws_bytes() // 4, dtype=torch.float32, device="cuda")
    for n8 in (131072 + 333, 1000, 5):          # past the grid's stride of 512 x 256 groups, a ragged last block, less than a wave
        g = gen(n8)
        a, b = randn((n8 * 8,), g).to(dt), randn((n8 * 8,), g).to(dt)
        out = torch.zeros((), dtype=torch.float32, device="cuda")
        check(L.udapose_feat_mse_fwd(stream(), ptr(a), ptr(b), n8 * 8, ptr(out), ptr(ws)), "feat_mse_fwd")
        emit(build, f"feat_mse_{n8}", {"out": out, "parts": ws})
    for R in (300, 7):
        stats = randn((R, 4), gen(R))
        for acc in (0, 1):
            out = torch.full((), 0.125, dtype=torch.float32, device="cuda")
            check(L.udapose_style_stat_loss(stream(), ptr(stats), R, ptr(out), acc), "style_stat_loss")
            emit(build, f"style_stat_loss_R{R}_acc{acc}", {"out": out})


def heatmap_rows(build, L):
    B, K = 3, 5
    for HW in (4100, 4097, 20, 15):             # 16-byte and scalar row sums
        g = gen(HW)
        p, t = randn((B * K, HW), g), randn((B * K, HW), g)
        w = torch.rand(B * K, generator=g).cuda()
        rows, mean = torch.zeros(B * K, dtype=torch.float32, device="cuda"), torch.zeros((), dtype=torch.float32, device="cuda")
        check(L.udapose_joints_mse_fwd(stream(), ptr(p), ptr(t), ptr(w), B * K, HW, ptr(rows), ptr(mean)), "joints_mse_fwd")
        emit(build, f"joints_mse_{HW}", {"rows": rows, "mean": mean})
        valid = (torch.rand(B, HW, generator=g) < 0.3).to(torch.uint8).cuda()
        mask = (torch.rand(B * K, generator=g) < 0.7).to(torch.uint8).cuda()
        cnt = torch.zeros((), dtype=torch.float32, device="cuda")
        check(L.udapose_mask_count(stream(), ptr(valid), valid.numel(), ptr(cnt)), "mask_count")
        rows, mean = torch.zeros(B * K, dtype=torch.float32, device="cuda"), torch.zeros((), dtype=torch.float32, device="cuda")
        check(L.udapose_cons_loss_valid_fwd(stream(), ptr(p), ptr(t), ptr(mask), ptr(valid), ptr(cnt), B * K, K, HW, ptr(rows), ptr(mean)),
              "cons_loss_valid_fwd")
        emit(build, f"cons_valid_{HW}", {"count": cnt, "rows": rows, "mean": mean})


def contrast_mean(build, L):
    for HW in (1000, 50):
        g = gen(HW)
        N = 4
        img = torch.randint(0, 256, (N, HW, 3), generator=g, dtype=torch.uint8).cuda()
        op = torch.tensor([2, 1, 2, 3], dtype=torch.int32, device="cuda")
        f = torch.tensor([1.4, 0.8, 0.6, 1.2], dtype=torch.float32, device="cuda")
        mean = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        check(L.udapose_aug_color_op(stream(), ptr(img), ptr(op), ptr(f), ptr(mean), N, HW), "aug_color_op")
        emit(build, f"aug_color_op_{HW}", {"mean": mean, "img": img})


if __name__ == "__main__":
    print(f"# tree {os.path.abspath(args.tree)}", file=sys.stderr)
    for build in ELEM:
        L = _hip.lib(build)
        grad_clip(build, L)
        perturb(build, L)
        style_losses(build, L)
        heatmap_rows(build, L)
        contrast_mean(build, L)
    torch.cuda.synchronize()
