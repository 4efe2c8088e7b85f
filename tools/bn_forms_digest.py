"""Dev tool: one SHA-256 per output tensor of every training-mode BatchNorm and max-pool kernel form of csrc/pointwise.hip, driven through the
`_ex` entry points of ops.py in both builds on seeded CPU-generated inputs - to `diff` between two trees (this one and a git worktree of
another commit with its own built libraries) on ONE box in one session, as tools/plan_digest.py does for whole plans.  plan_digest.py's plans
(N = 2 at 64 x 64) reach only the streaming forms; this tool reaches the chunked, pre-reduced, XCD-mapped, split and 'strict' forms as well.
Every kernel here is deterministic (fixed summation orders, no atomics), so a refactor of these kernels must leave every line identical; the
digests are not expected values and belong in no test.

    python tools/bn_forms_digest.py [--tree ROOT] > digest.txt     # ROOT: the tree whose package and libraries are loaded (default: this one)
    python tools/bn_forms_digest.py --fold digest.txt              # no GPU: one line per (build, form) = SHA-256 over its tensors' lines

Line: <build> <case>[<output>] <sha256>, with the library's form code (bit 0: chunked form, bit 1: XCD mapping) as the output `code`."""
import argparse
import hashlib
import os
import struct
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--fold", metavar="FILE", help="fold an output of this tool: per build and form, the count and one SHA-256 over the lines' values in order")
args = ap.parse_args()
if args.fold:
    groups = {}
    for line in open(args.fold):
        build, what, value = line.split()
        t = what.split("_")
        groups.setdefault((build, "_".join(t[:2]) if t[0] in ("fwd", "stem") else t[0].split("[")[0]), []).append(value)
    for (build, form), vals in groups.items():
        print(f"{build} {form} x{len(vals)} {hashlib.sha256(' '.join(vals).encode()).hexdigest()}")
    sys.exit(0)
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402
from uda_poseestimation_amd import _hip, ops  # noqa: E402

ELEM = {"bf16": torch.bfloat16, "fp16": torch.float16}
KINDS = {"bf16": ("16bit", "f32", "split"), "fp16": ("16bit", "f32", "split", "strict")}
B29, B30 = 1 << 29, 1 << 30
ptr, check, stream = _hip.ptr, _hip.check, _hip.stream


def emit(build, case, outs):
    for name, t in outs.items():
        if t is None:
            continue
        if isinstance(t, int):
            print(f"{build} {case}[{name}] {t}", flush=True)
        else:
            print(f"{build} {case}[{name}] {hashlib.sha256(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()}", flush=True)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, g, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=g) * scale + shift


def zeros(shape, dt):
    return torch.zeros(shape, dtype=dt, device="cuda")


def slab_of(a, b, rows):
    """[rows][2][C] fp32 partial sums of the columns of a and of b over `rows` interleaved pixel sets (rows past the pixel count stay zero)."""
    npix, C = a.shape
    rid = torch.arange(npix) % rows
    s = torch.zeros(rows, 2, C, dtype=torch.float64)
    s[:, 0].index_add_(0, rid, a.double())
    s[:, 1].index_add_(0, rid, b.double())
    return s.float().cuda()


# ---- forward: finalize + apply --------------------------------------------------------------------------------------------------------
def forward(build, npix, C, rows, policy, xcd_rows, pre_bias=False):
    g = gen(npix * 7 + C + rows)
    dt = ELEM[build]
    y32, res32 = randn((npix, C), g, 1.5, 0.3), randn((npix, C), g)
    gamma, beta, pb = (torch.rand(C, generator=g) + 0.5).cuda(), randn((C,), g, 0.3).cuda(), randn((C,), g, 0.5).cuda()
    rm0, rv0 = randn((C,), g), torch.rand(C, generator=g) + 0.5
    for kind in KINDS[build]:
        y = y32.to(dt).cuda() if kind == "16bit" else y32.cuda()
        res = res32.to(dt).cuda() if kind == "16bit" else (res32.cuda() if kind == "f32" else ops.f32_to_split(res32.cuda()))
        slab = slab_of(y.float().cpu(), y.float().cpu() ** 2, rows)
        masked = kind in ("16bit", "strict")
        for on in (1, 0):          # residual + ReLU on and off
            zdt = {"16bit": dt, "f32": torch.float32}.get(kind, torch.int32)
            o = {"z": zeros((npix, C), zdt), "scale": zeros((C,), torch.float32), "shift": zeros((C,), torch.float32), "save": zeros((3, C), torch.float32),
                 "rm": rm0.clone().cuda(), "rv": rv0.clone().cuda(), "nbt": torch.tensor([7], device="cuda"),
                 "mask": zeros((npix * C // 8,), torch.uint8) if masked else None,
                 "y16": zeros((npix, C), torch.float16) if kind == "strict" else None, "z16": zeros((npix, C), torch.float16) if kind == "strict" else None}
            o["code"] = ops.bn_train_fwd_ex(kind, y, o["z"], slab, gamma, beta, o["scale"], o["shift"], o["save"], res=res if on else None,
                                            pre_bias=pb if pre_bias else None, running_mean=o["rm"], running_var=o["rv"], nbt=o["nbt"], relu=bool(on),
                                            fwd_chunked=policy, xcd_rows=xcd_rows, mask=o["mask"], y16=o["y16"], z16=o["z16"], build=build)
            emit(build, f"fwd_{kind}_{npix}x{C}_rows{rows}_policy{policy}_xcd{xcd_rows}_bias{int(pre_bias)}_resrelu{on}", o)


# ---- backward -------------------------------------------------------------------------------------------------------------------------
class Bwd:
    def __init__(self, build, npix, C):
        g = gen(npix * 3 + C)
        dt = ELEM[build]
        self.npix, self.C, self.dt = npix, C, dt
        y = randn((npix, C), g, 1.5, 0.3).to(dt)
        mean, invstd = randn((C,), g, 0.2, 0.3), torch.rand(C, generator=g) * 0.5 + 0.4
        gamma, beta = torch.rand(C, generator=g) + 0.5, randn((C,), g, 0.3)
        sc = gamma * invstd
        z = torch.relu(y.float() * sc + (beta - mean * sc) + randn((npix, C), g)).to(dt)        # (any stored z serves as a mask source)
        dz = randn((npix, C), g, 1.0, 0.5)
        self.y, self.z, self.mean, self.invstd, self.gamma, self.beta = y.cuda(), z.cuda(), mean.cuda(), invstd.cuda(), gamma.cuda(), beta.cuda()
        self.dz = {"f32": dz.cuda(), "16bit": dz.to(dt).cuda()}
        self.old = (randn((C,), g).cuda(), randn((C,), g).cuda())


def backward(build, npix, C):
    c = Bwd(build, npix, C)
    rows = _hip.lib().udapose_bn_bwd_rows(npix)
    for dzk in ("16bit", "f32"):
        for relu in (0, 1, 2):
            for acc in (0.0, 0.5):
                o = {"dy": zeros((npix, C), c.dt), "gout": zeros((npix, C), c.dt), "slab": zeros((rows, 2, C), torch.float32), "coef": zeros((3, C), torch.float32),
                     "dgamma": c.old[0].clone(), "dbeta": c.old[1].clone()}
                o["code"] = ops.bn_bwd_ex(c.dz[dzk], c.z if relu == 1 else None, c.y, o["dy"], c.gamma, c.mean, c.invstd, o["slab"], o["coef"], o["dgamma"],
                                          o["dbeta"], relu=relu, gout=o["gout"], beta=c.beta if relu == 2 else None, beta_acc=acc, chunked=1)
                emit(build, f"bwd_{npix}x{C}_dz{dzk}_relu{relu}_acc{acc}", o)


def backward_pre(build, npix, C, rows, sel, legacy=0):
    c = Bwd(build, npix, C)
    xhat = ((c.y.double() - c.mean.double()) * c.invstd.double()).cpu()
    for gk in ("16bit", "f32"):
        g = torch.where(c.z > 0, c.dz[gk], torch.zeros_like(c.dz[gk]))
        slab = slab_of(g.cpu(), g.cpu().double() * xhat, rows)
        for acc in (0.0, 0.5):
            o = {"dy": zeros((npix, C), c.dt), "coef": zeros((3, C), torch.float32), "dgamma": c.old[0].clone(), "dbeta": c.old[1].clone()}
            o["code"] = ops.bn_bwd_pre_ex(g, c.y, o["dy"], c.gamma, c.mean, c.invstd, slab, o["coef"], o["dgamma"], o["dbeta"], beta_acc=acc, chunked=sel,
                                          legacy=legacy)
            emit(build, f"pre_{npix}x{C}_rows{rows}_sel{sel & ~(3 << 29)}_bits{sel >> 29}_legacy{legacy}_g{gk}_acc{acc}", o)


# ---- stem and pools -------------------------------------------------------------------------------------------------------------------
def stem(build, N, H, W, C):
    c = Bwd(build, N * H * W, C)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    scale = c.gamma * c.invstd
    shift = c.beta - c.mean * scale
    y4 = c.y.reshape(N, H, W, C)
    o = {"pooled": zeros((N, Ho, Wo, C), c.dt), "idx": zeros((N, Ho, Wo, C), torch.uint8)}
    ops.bn_relu_maxpool3x3s2(y4, o["pooled"], o["idx"], scale, shift)
    emit(build, f"stem_fwd_{N}x{H}x{W}x{C}", o)
    pdy = randn((N, Ho, Wo, C), gen(H * W + C), 1.0, 0.5).to(c.dt).cuda()
    rows = _hip.lib().udapose_bn_bwd_rows(c.npix)
    b = {"dy": zeros((c.npix, C), c.dt), "slab": zeros((rows, 2, C), torch.float32), "coef": zeros((3, C), torch.float32), "dgamma": c.old[0].clone(),
         "dbeta": c.old[1].clone()}
    ops.bn_bwd_pooled(pdy, o["idx"], y4, b["dy"], c.gamma, c.mean, c.invstd, c.beta, b["slab"], b["coef"], b["dgamma"], b["dbeta"], beta_acc=0.5)
    emit(build, f"stem_bwd_{N}x{H}x{W}x{C}", b)


def pools(build):
    dt = ELEM[build]
    L = _hip.lib(build)
    N, H, W, C = 2, 9, 11, 16
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x32 = (torch.randn((N, H, W, C), generator=gen(5)).bfloat16().float() * 0.5).cuda()      # (few distinct values: ties inside windows)
    idx16 = None
    for kind in KINDS[build]:
        x = x32.to(dt) if kind == "16bit" else (x32 if kind == "f32" else ops.f32_to_split(x32))
        zdt = {"16bit": dt, "f32": torch.float32}.get(kind, torch.int32)
        o = {"y": zeros((N, Ho, Wo, C), zdt), "idx": zeros((N, Ho, Wo, C), torch.uint8), "y16": zeros((N, Ho, Wo, C), torch.float16) if kind == "strict" else None}
        ops.maxpool3x3s2_fwd_ex(kind, x, o["y"], o["idx"], y16=o["y16"], build=build)
        emit(build, f"pool3x3_fwd_{kind}", o)
        if kind == "16bit":
            idx16 = o["idx"]
    dy = randn((N, Ho, Wo, C), gen(6)).to(dt).cuda()
    dx = zeros((N, H, W, C), dt)
    check(L.udapose_maxpool3x3s2_bwd(stream(), ptr(dy), ptr(idx16), ptr(dx), N, H, W, C), "maxpool3x3s2_bwd")
    emit(build, "pool3x3_bwd", {"dx": dx})
    x32 = (torch.randn((2, 7, 9, 8), generator=gen(7)).bfloat16().float() * 0.5).cuda()
    for kind in ("16bit", "f32", "split"):
        x = x32.to(dt) if kind == "16bit" else (x32 if kind == "f32" else ops.f32_to_split(x32))
        y = zeros((2, 4, 5, 8), x.dtype)
        fn = {"16bit": L.udapose_maxpool2x2_ceil, "f32": L.udapose_maxpool2x2_ceil_f32, "split": L.udapose_maxpool2x2_ceil_split}[kind]
        check(fn(stream(), ptr(x), ptr(y), 2, 7, 9, 8), "maxpool2x2_ceil")
        emit(build, f"pool2x2_{kind}", {"y": y})


def coefficients(build):
    L = _hip.lib(build)
    layers = []
    for C in (8, 2048):
        g = gen(C)
        gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), randn((C,), g, 0.3).cuda()
        rm0, rv0 = randn((C,), g).cuda(), (torch.rand(C, generator=g) + 0.5).cuda()
        save = torch.stack([randn((C,), g, 0.5, 0.2), torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5]).cuda()
        o = {"scale": zeros((C,), torch.float32), "shift": zeros((C,), torch.float32)}
        check(L.udapose_bn_eval_coeff(stream(), C, ptr(gamma), ptr(beta), ptr(rm0), ptr(rv0), 1e-5, ptr(o["scale"]), ptr(o["shift"])), "bn_eval_coeff")
        emit(build, f"eval_coeff_C{C}", o)
        o = {"rm": rm0.clone(), "rv": rv0.clone(), "nbt": torch.tensor([7], device="cuda")}
        check(L.udapose_bn_running_update(stream(), ptr(save), C, ptr(o["rm"]), ptr(o["rv"]), ptr(o["nbt"]), 0.1), "bn_running_update")
        emit(build, f"running_update_C{C}", o)
        layers.append((C, save, rm0, rv0))
    # both layers in one launch: the saved statistics in one arena at 256-byte offsets, as the executor keeps them
    offs, total = [], 0
    for C, *_ in layers:
        offs.append(total)
        total += -(-3 * C * 4 // 256) * 256
    act = zeros((total,), torch.uint8)
    outs, table = [], b""
    for (C, save, rm0, rv0), off in zip(layers, offs):
        act[off:off + 3 * C * 4].view(torch.float32).view(3, C).copy_(save)
        o = {"rm": rm0.clone(), "rv": rv0.clone(), "nbt": torch.tensor([7], device="cuda")}
        outs.append((C, o))
        table += struct.pack("<QQQQii", off, o["rm"].data_ptr(), o["rv"].data_ptr(), o["nbt"].data_ptr(), C, 0)     # (size_t, three pointers, int C, int pad)
    jobs = torch.frombuffer(bytearray(table), dtype=torch.uint8).cuda()
    check(L.udapose_bn_running_update_multi(stream(), ptr(jobs), len(layers), 2048, ptr(act), 0.1), "bn_running_update_multi")
    for C, o in outs:
        emit(build, f"running_update_multi_C{C}", o)


if __name__ == "__main__":
    print(f"# tree {os.path.abspath(args.tree)}", file=sys.stderr)
    for build in ELEM:
        # streaming finalize + apply: the 1-, 4- and 8-row loops of the finalize, G = 1 / 3 / 8 / 256; then the XCD request, engaged and refused
        for C, rows, pb in ((8, 1, False), (24, 97, False), (64, 129, True), (2048, 257, False)):
            forward(build, 33, C, rows, 0, 1, pb)
        for npix in (1000, 1031):
            forward(build, npix, 64, 37, 0, 2)
        # chunked: the prelude's loops, then ragged pixel ranges under three work-group targets with the XCD remap off and on
        for rows in (1, 9, 33, 65, 128):
            forward(build, 1024, 256, rows, 1, 1)
        for policy in (1, 64, 4096):
            for xcd in (0, 1):
                forward(build, 1031, 320, 37, policy, xcd)
        for npix, C in ((1031, 8), (1031, 64), (1031, 2048), (1023, 256), (1024, 256), (1031, 256), (1200, 2048)):
            backward(build, npix, C)
        for rows in (1, 57, 128):
            for sel in (1, 1 | B30):
                backward_pre(build, 1200, 256, rows, sel)
        for npix in (1000, 1031):
            backward_pre(build, npix, 64, 37, 1 | B29)
        backward_pre(build, 1031, 64, 37, 1, legacy=1)
        for C in (8, 64):
            stem(build, 2, 9, 11, C)
        pools(build)
        coefficients(build)
    torch.cuda.synchronize()
