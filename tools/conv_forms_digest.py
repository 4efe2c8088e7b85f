"""Dev tool: one SHA-256 per output tensor of every convolution kernel form, to `diff` between two trees (this one and a git worktree of another
commit with its own built libraries) on ONE box in one session, as tools/bn_forms_digest.py does for the BatchNorm and max-pool kernels.

The forms are the forced-form matrix of tests/test_gpu_conv_forms.py part (A) - every geometry of IGEMM_SHAPES under every variant of _variants():
fprop with its fused statistics and epilogues, the data gradient, the data gradient with the BatchNorm epilogue, the exact-fp32 and f16x2
forwards per tile id; every geometry of WGRAD_SHAPES under every variant of _wgrad_variants(), with the two accumulating calls - and the
patch-staged forms of tests/test_gpu_patchconv_forms.py (co16, ci8 small and persistent, the trunk cases; with patch_conv = 0 as well), in both
builds.  The case and variant lists are IMPORTED from those modules (always this tree's tests/: the lists, not the code under test), operands are
generated as the tests generate them; nothing is compared with fp64 here.

Every kernel but one family has a fixed summation order: its lines must be identical between two trees that claim the same arithmetic.  The
exception: weight gradients that split the pixel range or accumulate add with fp32 atomics, so their bits change from run to run.  Run the
reference tree TWICE and let --compare skip what it does not reproduce itself.  The digests are not expected values and belong in no test.

    python tools/conv_forms_digest.py [--tree ROOT] > digest.txt      # ROOT: the tree whose package and libraries are loaded (default: this one)
    python tools/conv_forms_digest.py --fold digest.txt               # no GPU: one line per (build, family, variant) = SHA-256 over its lines
    python tools/conv_forms_digest.py --compare A1.txt A2.txt B.txt   # no GPU: every line A1 and A2 agree on must be identical in B; exit 1 if not

Line: <build> <family>:<variant>:<shape>[<output>] <sha256>."""
import argparse
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=HERE)
ap.add_argument("--fold", metavar="FILE")
ap.add_argument("--compare", nargs=3, metavar=("A1", "A2", "B"))
args = ap.parse_args()


def read(path):
    return dict(line.rsplit(None, 1) for line in open(path) if line.strip() and not line.startswith("#"))


if args.fold:
    groups = {}
    for key, value in read(args.fold).items():
        build, what = key.split(None, 1)
        groups.setdefault((build, ":".join(what.split(":")[:2])), []).append(value)
    for (build, form), vals in groups.items():
        print(f"{build} {form} x{len(vals)} {hashlib.sha256(' '.join(vals).encode()).hexdigest()}")
    sys.exit(0)
if args.compare:
    a1, a2, b = (read(p) for p in args.compare)
    stable = [k for k in a1 if a2.get(k) == a1[k]]
    missing = [k for k in a1 if k not in b] + [k for k in b if k not in a1]
    bad = [k for k in stable if k in b and b[k] != a1[k]]
    print(f"{len(a1)} lines; the reference reproduces {len(stable)} of them itself ({len(a1) - len(stable)} not: atomics); of those {len(bad)} differ in the "
          f"other tree; {len(missing)} lines exist in one file only")
    for k in (bad + missing)[:40]:
        print("  " + k)
    sys.exit(1 if bad or missing else 0)

sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402
import test_gpu_conv_forms as T  # noqa: E402
import test_gpu_patchconv_forms as P  # noqa: E402
from uda_poseestimation_amd import _hip, ops  # noqa: E402


def emit(build, case, outs):
    for name, t in outs.items():
        if t is not None:
            print(f"{build} {case}[{name}] {hashlib.sha256(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()}", flush=True)


def attempt(build, case, fn):
    """A form the library refuses prints its error instead of digests (the refusal must be the same in both trees)."""
    try:
        emit(build, case, fn())
    except RuntimeError as e:
        print(f"{build} {case}[refused] {str(e).split()[-1]}", flush=True)


def igemm():
    for name, N, H, W, Ci, Co, K, s, p, tr, refl, up in T.IGEMM_SHAPES:
        d0 = ops.conv_desc(N, H, W, Ci, Co, K, s, p, transposed=tr, reflect=refl, upsample=up, policy=_hip.policy(patch_conv=0))
        dgrad_ok = Co % 64 == 0 and not (refl or up or Ci == 8)
        for build, dt in T.ELEM.items():
            case = T.Case(d0, dt, seed=len(name) * 7 + Co)
            gen = torch.Generator(device="cuda").manual_seed(5)
            bias = torch.randn(Co, device="cuda", generator=gen)
            res = torch.randn(case.dy.shape, device="cuda", generator=gen).to(dt)
            bn = case.bn_operands(9)
            f32_out = Co % 8 != 0
            for vname, pol in T._variants():
                d = ops.with_policy(d0, _hip.policy(**dict(pol, patch_conv=0)))

                def fwd():
                    y, st = ops.conv2d_fwd(case.x, case.wf, d, want_stats=True, out_f32=f32_out)
                    yf, stf = ops.conv2d_fwd(case.x, case.wf, d, out_f32=True, want_stats=True)
                    o = {"y": y, "stats": st, "y_f32": yf, "stats_f32": stf, "y_bias_f32": ops.conv2d_fwd(case.x, case.wf, d, bias=bias, out_f32=True)}
                    if Co % 8 == 0:
                        o["y_res_bias_relu"] = ops.conv2d_fwd(case.x, case.wf, d, res=res, bias=bias, relu=True)
                    return o

                def bwd():
                    gq, slab = ops.conv2d_bwd_data_bn(case.dy, case.wb, d, bn[0], bn[1], bn[2], bn_gamma=bn[3], bn_beta=bn[4])
                    return {"dx": ops.conv2d_bwd_data(case.dy, case.wb, d), "dx_f32": ops.conv2d_bwd_data(case.dy, case.wb, d, out_f32=True), "bn_g": gq, "bn_slab": slab}
                attempt(build, f"fprop:{vname}:{name}", fwd)
                if dgrad_ok:
                    attempt(build, f"dgrad:{vname}:{name}", bwd)
            if build == "bf16" and (Ci % 32 == 0 or Ci == 8):
                gen = torch.Generator(device="cuda").manual_seed(3)
                xf = torch.randn(N, H, W, Ci, device="cuda", generator=gen)
                if Ci == 8:
                    xf[..., 3:] = 0
                wf = case.wp.float() if not tr else case.wp.float().permute(2, 1, 0).contiguous()
                for split in (False, True):
                    x, w = (ops.f32_to_split(xf), ops.f32_to_split(wf)) if split else (xf, wf)
                    for vname, pol in [(f"tile{t}", {"igemm_tile": t}) for t in T.TILES[:5]] + [("default", {})]:
                        d = ops.with_policy(d0, _hip.policy(**dict(pol, patch_conv=0)))

                        def fwd32():
                            y, st = ops.conv2d_fwd(x, w, d, out_f32=True, want_stats=True)
                            return {"y": y, "stats": st, "y_split": ops.conv2d_fwd(x, w, d) if split and Co % 8 == 0 else None}
                        attempt("split" if split else "f32", f"fprop:{vname}:{name}", fwd32)
            del case
        torch.cuda.empty_cache()


def wgrad():
    for name, N, H, W, Ci, Co, K, s, p, tr in T.WGRAD_SHAPES:
        for build, dt in T.ELEM.items():
            d0 = ops.conv_desc(N, H, W, Ci, Co, K, s, p, transposed=tr)
            case = T.Case(d0, dt, seed=len(name) + Ci, with_dgrad=False)
            variants = T._wgrad_variants(Ci == 8)
            outs = {}
            for vname, pol in variants:
                d = ops.with_policy(d0, _hip.policy(**pol))

                def one():
                    outs[vname] = ops.conv2d_bwd_weight(case.dy, case.x, d)
                    return {"dw": outs[vname]}
                attempt(build, f"wgrad:{vname}:{name}", one)
            for vname in ("default", "ksplit4" if Ci == 8 else "tile-1_ks4"):
                if vname in outs:
                    d = ops.with_policy(d0, _hip.policy(**dict(variants)[vname]))
                    attempt(build, f"wgrad_accumulate:{vname}:{name}", lambda: {"dw": ops.conv2d_bwd_weight(case.dy, case.x, d, dw=outs[vname].clone())})
            del case, outs


def patch(family, name, op, pol, out_f32=False, epilogues=P.ALL_EPILOGUES):
    g = op.g
    for pc in (pol, dict(pol, patch_conv=0)):
        d = ops.conv_desc(g.N, g.Hi, g.Wi, g.Ci, g.Co, 3, 1, 1, reflect=True, upsample=g.upsample, policy=_hip.policy(**pc))
        for with_bias, relu in epilogues:
            tag = f"{family}{'_igemm' if pc.get('patch_conv', 2) == 0 else ''}:bias{int(with_bias)}_relu{int(relu)}:{name}"
            attempt(op.kind, tag, lambda: {"y": P._conv(op.x, op.w, d, out_f32, op.bias if with_bias else None, relu)[0]})


def patchconv():
    for name, N, H, W in P.CO16_SHAPES:
        for Co in (1, 3, 13, 16):
            for kind in P.KINDS:
                patch("co16", f"{name}_Co{Co}", P.Operands(kind, N, H, W, 64, Co, False, seed=H * 31 + W + Co), {}, out_f32=True)
    for kind in P.KINDS:
        for name, N, H, W in (("single_tile", 1, 4, 64), ("8_tiles", 2, 8, 128)):
            patch("ci8", name, P.Operands(kind, N, H, W, 8, 64, False, seed=H * 17 + W), {})
        for N in (30, 60):
            patch("ci8", f"{N * 26}_tiles", P.Operands(kind, N, 52, 128, 8, 64, False, seed=N), {}, epilogues=P.BIAS_RELU)
        for name, N, Hi, Wi, Ci, Co, up, pc in P.TRUNK_CASES:
            patch("trunk", name, P.Operands(kind, N, Hi, Wi, Ci, Co, up, seed=Hi * 13 + Wi + Ci + Co), {"patch_conv": pc})
        torch.cuda.empty_cache()


if __name__ == "__main__":
    print(f"# tree {os.path.abspath(args.tree)}", file=sys.stderr)
    _hip.lib("bf16"), _hip.lib("fp16")
    igemm()
    wgrad()
    patchconv()
    torch.cuda.synchronize()
