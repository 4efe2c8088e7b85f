"""Golden vectors of the AdaIN decoder's training step, made by RUNNING THE REFERENCE'S OWN adain/net.py (CPU, fp32).

Run in the build container only (needs the reference checkout; it does not exist on the GPU box):
    python tests/golden/make_golden_adain.py
Writes adain_train.npz next to this file: data only (seeded inputs and the reference's outputs).  Network: the reference's vgg cut to
31 children and its decoder, weights from seeded.fill_style_weights (vgg seed 11, decoder seed 12); N = 2, 64x64 images; loss =
loss_c + 0.1 * loss_s; torch.optim.Adam(decoder.parameters(), lr=1e-4) stepped 3 times on the same pair.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from seeded import fill_style_weights  # noqa: E402

SEED_ENC, SEED_DEC, SEED_IMG, SEED_IDX, N, S, STEPS, LR, SW = 11, 12, 7, 3, 2, 64, 3, 1e-4, 0.1
SMALL = 4096        # tensors up to this size are stored whole


def load_ref_net():
    sys.path.insert(0, os.path.join(REF, "adain"))          # adain/net.py imports `function` as a top-level module
    spec = importlib.util.spec_from_file_location("ref_adain_net", os.path.join(REF, "adain", "net.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sample_index(numel, k=64):
    return np.random.RandomState(SEED_IDX + numel).choice(numel, size=min(k, numel), replace=False)


def grad_record(dec, out, prefix):
    for name, p in dec.named_parameters():
        g = p.grad.detach().double().flatten().numpy()
        out[f"{prefix}/{name}/norm"] = np.float64(np.linalg.norm(g))
        out[f"{prefix}/{name}/sum"] = np.float64(g.sum())
        if g.size <= SMALL:
            out[f"{prefix}/{name}/values"] = g.astype(np.float32)
        else:
            idx = sample_index(g.size)
            out[f"{prefix}/{name}/idx"] = idx.astype(np.int64)
            out[f"{prefix}/{name}/values"] = g[idx].astype(np.float32)


def main():
    torch.set_num_threads(16)
    ref = load_ref_net()
    vgg, dec = ref.vgg, ref.decoder
    fill_style_weights(vgg, SEED_ENC)
    fill_style_weights(dec, SEED_DEC)
    net = ref.Net(nn.Sequential(*list(vgg.children())[:31]), dec)
    g = torch.Generator().manual_seed(SEED_IMG)
    content, style = torch.rand(N, 3, S, S, generator=g), torch.rand(N, 3, S, S, generator=g)
    out = {"content": content.numpy(), "style": style.numpy(), "seeds": np.array([SEED_ENC, SEED_DEC, SEED_IMG, SEED_IDX]),
           "lr": np.float64(LR), "style_weight": np.float64(SW)}
    opt = torch.optim.Adam(dec.parameters(), lr=LR)
    losses = []
    for step in range(STEPS + 1):
        loss_c, loss_s, g_t = net(content, style)
        loss = loss_c + SW * loss_s
        opt.zero_grad()
        loss.backward()
        losses.append([loss_c.item(), loss_s.item()])
        if step == 0:
            out["g_t"] = g_t.detach().numpy()
            grad_record(dec, out, "step0")
        if step == STEPS:
            grad_record(dec, out, f"step{STEPS}")     # gradient at the weights after STEPS Adam steps
            break
        opt.step()
    out["losses"] = np.array(losses, dtype=np.float64)      # [STEPS + 1][loss_c, loss_s]: before each Adam step, and after the last
    np.savez_compressed(os.path.join(OUT, "adain_train.npz"), **out)
    print("adain_train.npz written:", os.path.getsize(os.path.join(OUT, "adain_train.npz")), "bytes; losses", losses)


if __name__ == "__main__":
    main()
