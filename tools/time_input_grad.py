"""Dev tool: what an input gradient through PoseResNet costs (profiles/input_grad.txt).  PoseResNet-101, bf16, N = 32, 256x256.
Default: forward + JointsMSE + backward with and without x.requires_grad, alternating rounds in one process, device events, no profiler.
--trace: the launches to read out of a kernel trace, in a run of its own -
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/time_input_grad.py --trace
20 calls of the stem's forward convolution alone (udapose_conv2d_fwd with the fused statistics, the launch conv_bn_fwd issues) and 20 of
udapose_stem_dgrad on operands of the same shapes - the same tensors in opposite roles - then three network steps with x.requires_grad."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import uda_poseestimation_amd.lib.models as models
from uda_poseestimation_amd import ops, synthetic
from uda_poseestimation_amd.lib.models.loss import JointsMSELoss

N, S, K = 32, 256, 16
trace = "--trace" in sys.argv
torch.manual_seed(0)
net = models.pose_resnet101(num_keypoints=K, pretrained_backbone=False).cuda().train()
net.precision = "bf16"
x, lab, wt = (t.cuda() for t in synthetic.keypoint_batch(N, num_keypoints=K, image_size=S, heatmap_size=S // 4, seed=1))
crit = JointsMSELoss()


def step(xreq):
    for p in net.parameters():
        p.grad = None
    xin = x.detach().requires_grad_(xreq)
    (crit(net(xin), lab, wt) * 1024.0).backward()
    return xin.grad


for r in (False, True, False, True):
    step(r)
torch.cuda.synchronize()

if trace:
    d = ops.conv_desc(N, S, S, 8, 64, 7, 2, 3)
    w = torch.randn(64, 3, 7, 7, device="cuda") * 147 ** -0.5
    x8 = torch.randn(N, S, S, 8, device="cuda")
    x8[..., 3:] = 0
    x8 = x8.bfloat16()
    wf = ops.pack_weight(w, d, "fwd")
    dy = torch.randn(N, S // 2, S // 2, 64, device="cuda").bfloat16()
    dx = torch.empty(N, 3, S, S, device="cuda")
    for _ in range(20):
        ops.conv2d_fwd(x8, wf, d, want_stats=True)
    torch.cuda.synchronize()
    for _ in range(20):
        ops.stem_dgrad(dy, w, dx=dx)
    torch.cuda.synchronize()
    for _ in range(3):
        step(True)
    torch.cuda.synchronize()
    print("trace run done")
    sys.exit(0)

REP, ROUNDS = 10, 7
res = {False: [], True: []}
for rnd in range(ROUNDS):
    for xreq in (False, True):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(REP):
            step(xreq)
        b.record()
        torch.cuda.synchronize()
        res[xreq].append(a.elapsed_time(b) / REP)
for xreq in (False, True):
    v = res[xreq]
    print(f"PoseResNet-101 bf16 N={N} {S}x{S} forward + JointsMSE + backward, x.requires_grad={xreq}: median {statistics.median(v):.3f} ms, "
          f"min {min(v):.3f} ms over {ROUNDS} alternating rounds of {REP} steps ({' '.join(f'{t:.3f}' for t in v)})")
