"""Dev tool: one SHA-256 per tensor of what three training steps leave behind, for every form of the step the engine has and fixed seeds -
to `diff` between two trees (this one and a git worktree of another commit with its own built libraries) on ONE box in one session.
Host-side refactors of uda_poseestimation_amd/engine.py must leave every line of a form that reproduces itself identical; the digests are
not expected values and belong in no test.  (The twins of tests/test_gpu_steps.py compare captured with eager inside ONE tree: a change to
both passes them.  The stem's fp32 atomics make some forms differ between two runs of the SAME tree: run the old tree twice first.)

    python tools/step_digest.py [--tree ROOT] > digest.txt        # ROOT: the tree whose package and libraries are loaded (default: this one)
    python tools/step_digest.py --fold digest.txt                 # no GPU: one line per (form, tensor kind) = SHA-256 over its tensors' lines

The tiny network of tests/test_gpu_steps.py (_tiny: one bottleneck per stage, K = 16), N = 4, 128 x 128, a new batch per step.  Forms: eager;
one graph; single_graph=False; overlap forced - eager, captured, captured with split=True; AdaIN style with device occlusion, captured
(BASELINE.json configs[2]'s form); FDA style, captured; precision='strict', captured; FusedSGD, captured.  Per form: student and teacher
parameters, the optimizer's state, every tensor of the last step's `out`, and the metric vector of a captured step."""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--fold", metavar="FILE", help="fold an output of this tool: per form and tensor kind, the count and one SHA-256 over the tensors' digests in order")
args = ap.parse_args()
if args.fold:
    groups = {}
    for line in open(args.fold):
        tag, what, value = line.split()
        groups.setdefault((tag, what.split("[")[0]), []).append(value)
    for (tag, what), vals in groups.items():
        print(f"{tag} {what} x{len(vals)} {hashlib.sha256(' '.join(vals).encode()).hexdigest() if len(vals) > 1 else vals[0]}")
    sys.exit(0)
sys.path.insert(0, os.path.abspath(args.tree))
sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "tests", "golden"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import uda_poseestimation_amd.lib.models.pose_resnet as pr  # noqa: E402
from uda_poseestimation_amd import synthetic  # noqa: E402
from uda_poseestimation_amd.engine import GraphedTrainStep, MeanTeacherTrainer  # noqa: E402

K, N, S, STEPS = 16, 4, 128, 3
pr.PoseResNet.default_precision = "bf16"        # (as the step tests set it; 'strict' below names its own)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def tiny(seed):
    torch.manual_seed(seed)
    return pr._pose_resnet("t", K, pr.Bottleneck_default, [1, 1, 1, 1], False, False)


def batches():
    out = []
    for s in range(31, 31 + STEPS):
        b = synthetic.mean_teacher_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=s)
        g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
        out.append((g["x_s"], g["label_s"], g["weight_s"], g["x_t_stu"], g["x_t_tea"], g["aug_param_stu"], g["aug_param_tea"]))
    return out


def adain_net():
    from seeded import fill_style_weights
    from uda_poseestimation_amd.lib.models import Style_net
    fill_style_weights(Style_net.vgg, 11)
    fill_style_weights(Style_net.decoder, 12)
    Style_net.vgg.cuda()
    Style_net.decoder.cuda()
    net = Style_net.Net(torch.nn.Sequential(*list(Style_net.vgg.children())[:31]), Style_net.decoder).cuda()
    net.compute_losses = False
    return net


def fda_net():
    from uda_poseestimation_amd.lib.models import fda
    return fda.FDANet(0.05, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def run(tag, captured, style=None, attrs=None, graph_kw=None, **trainer_kw):
    stu, tea = tiny(7).cuda(), tiny(8).cuda()
    if style is not None:
        lo, hi = torch.tensor([-2.1179, -2.0357, -1.8044]).cuda(), torch.tensor([2.2489, 2.4285, 2.64]).cuda()
        trainer_kw.update(style_net=style(), recover=(lo, hi), s2t_freq=0.5, t2s_freq=0.5, rng=np.random.RandomState(123), occlude_rate=0.5,
                          occlude_thresh=-1e9, occlude_size=10)
    tr = MeanTeacherTrainer(stu, tea, lr=1e-3, teacher_alpha=0.9, image_size=S, heatmap_size=S // 4, **trainer_kw)
    tr.device_occlusion = style is not None
    for k, v in (attrs or {}).items():
        setattr(tr, k, v)
    bs = batches()
    gs = None
    if captured:
        gs = GraphedTrainStep(tr, *bs[0], warmup=1, **(graph_kw or {}))          # (the warm-up step IS step 1, on batch 0)
        for b in bs[1:]:
            out = gs.step(*b)
    else:
        for b in bs:
            out = tr.train_step(*b)
    torch.cuda.synchronize()
    for name, m in (("student", stu), ("teacher", tea)):
        for i, p in enumerate(m.parameters()):
            print(f"{tag} {name}_param[{i}] {sha(p)}", flush=True)
        for i, b in enumerate(m.buffers()):
            print(f"{tag} {name}_buffer[{i}] {sha(b)}", flush=True)
    i = 0
    for g in tr.stu_optimizer.param_groups:
        for p in g["params"]:
            for k, v in sorted((tr.stu_optimizer.state.get(p) or {}).items()):
                if torch.is_tensor(v):
                    print(f"{tag} optimizer_{k}[{i}] {sha(v)}", flush=True)
            i += 1
    for k in sorted(out):
        if torch.is_tensor(out[k]):
            print(f"{tag} out.{k} {sha(out[k])}", flush=True)
    if gs is not None:
        print(f"{tag} mvec {sha(gs._mvec)}", flush=True)
        print(f"{tag} form split={int(gs.split)},one_graph={int(gs.one_graph)},overlap={int(gs.overlap)},g_lb2={int(gs.g_lb2 is not None)},"
              f"fused_tail={int(gs._fused_tail)}", flush=True)


if __name__ == "__main__":
    print(f"# tree {os.path.abspath(args.tree)}", file=sys.stderr)
    run("eager", False)
    run("one_graph", True)
    run("two_graphs", True, attrs={"single_graph": False})
    run("overlap_eager", False, attrs={"overlap_allreduce": True})
    run("overlap_graph", True, attrs={"overlap_allreduce": True})
    run("overlap_graph_split", True, attrs={"overlap_allreduce": True}, graph_kw={"split": True})
    run("adain_occlusion_graph", True, style=adain_net)
    run("fda_occlusion_graph", True, style=fda_net)
    run("strict_graph", True, precision="strict")
    run("sgd_graph", True, use_sgd=True)
