"""ms per AdaIN decoder training step (uda_poseestimation_amd.adain: three encoder passes, decoder, backward, torch.optim.Adam step),
eager and captured (the whole step in one graph on one stream, replayed), bf16 and fp16, N = 4 and N = 16 at 256x256.  One JSON line per
configuration.  usage: python tools/time_adain_train.py [--steps 10] [--warmup 3] [--sizes 4,16] [--precisions bf16,fp16] [--modes eager,captured]"""
import argparse
import copy
import json
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uda_poseestimation_amd.adain import net as anet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="4,16")
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--precisions", default="bf16,fp16")
    ap.add_argument("--modes", default="eager,captured")
    a = ap.parse_args()
    for prec in a.precisions.split(","):
        for N, mode in [(int(s), m) for s in a.sizes.split(",") for m in a.modes.split(",")]:
            torch.manual_seed(0)
            dec = copy.deepcopy(anet.decoder).cuda()
            net = anet.Net(nn.Sequential(*list(copy.deepcopy(anet.vgg).children())[:31]).cuda(), dec)
            net.precision = prec
            opt = torch.optim.Adam(dec.parameters(), lr=1e-5, capturable=(mode == "captured"))
            c = torch.rand(N, 3, a.res, a.res, device="cuda")
            s = torch.rand(N, 3, a.res, a.res, device="cuda")

            def step():
                opt.zero_grad(set_to_none=False)
                lc, ls, _ = net(c, s)
                loss = lc + 0.1 * ls
                loss.backward()
                opt.step()
                return loss
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(a.warmup):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            run = step
            if mode == "captured":
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    sloss = step()

                def run():
                    graph.replay()
                    return sloss
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = run()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
            print(json.dumps({"precision": prec, "N": N, "res": a.res, "mode": mode, "ms_per_step": round(ms, 3),
                              "img_per_s": round(N * 1e3 / ms, 2), "loss": float(loss.item())}), flush=True)


if __name__ == "__main__":
    main()
