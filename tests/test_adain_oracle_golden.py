"""CPU: the test-side oracle of the AdaIN decoder's training step (tests/helpers/adain_oracle.py) against golden vectors made by running
the reference's own adain/net.py (tests/golden/make_golden_adain.py -> adain_train.npz): losses, g_t, every decoder gradient at the
initial weights and after 3 torch.optim.Adam steps."""
import os

import numpy as np
import torch
import torch.nn as nn

from helpers.adain_oracle import make_nets, step_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adain_train.npz")


def _check_grads(dec, z, prefix, tol):
    """tol: relative bar of the sampled values; after Adam steps last-bit differences of two fp32 implementations in near-zero gradient
    entries become whole-size differences of those entries' updates (Adam normalises each entry), so the later bars are wider"""
    for name, p in dec.named_parameters():
        g = p.grad.detach().double().flatten().numpy()
        ref = z[f"{prefix}/{name}/values"].astype(np.float64)
        got = g[z[f"{prefix}/{name}/idx"]] if f"{prefix}/{name}/idx" in z else g
        scale = float(z[f"{prefix}/{name}/norm"]) / np.sqrt(g.size)
        assert np.abs(got - ref).max() <= tol * np.abs(ref).max() + tol * 0.1 * scale, name
        assert abs(np.linalg.norm(g) - float(z[f"{prefix}/{name}/norm"])) <= tol * 0.1 * float(z[f"{prefix}/{name}/norm"]), name
        assert abs(g.sum() - float(z[f"{prefix}/{name}/sum"])) <= tol * np.abs(g).sum() + 1e-12, name


def test_oracle_matches_reference_adain_net():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    z = np.load(GOLDEN)
    seeds = z["seeds"]
    vgg, dec = make_nets(int(seeds[0]), int(seeds[1]))
    vgg31 = nn.Sequential(*list(vgg.children())[:31])
    c, s = torch.from_numpy(z["content"]), torch.from_numpy(z["style"])
    sw, lr = float(z["style_weight"]), float(z["lr"])
    opt = torch.optim.Adam(dec.parameters(), lr=lr)
    losses = z["losses"]
    steps = len(losses) - 1
    for step in range(steps + 1):
        lc, ls, g_t = step_ref(vgg31, dec, c, s)
        opt.zero_grad()
        (lc + sw * ls).backward()
        assert abs(lc.item() - losses[step, 0]) <= 1e-4 * losses[step, 0]
        assert abs(ls.item() - losses[step, 1]) <= 1e-4 * losses[step, 1]
        if step == 0:
            assert np.abs(g_t.detach().numpy() - z["g_t"]).max() <= 1e-4 * np.abs(z["g_t"]).max()
            _check_grads(dec, z, "step0", 1e-3)
        if step == steps:
            _check_grads(dec, z, f"step{steps}", 1e-2)
            break
        opt.step()
