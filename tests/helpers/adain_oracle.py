"""CPU fp32 autograd oracle of the AdaIN decoder's training step (mean/std style loss, reference adain/net.py:102-162), built from
oracle.style_ref's VGG and decoder layer lists.  Test-only."""
import torch

from oracle.style_ref import adain_ref, calc_mean_std_ref, make_decoder_ref, make_vgg_ref

# vgg[:31] split of the reference's Net: relu1_1, relu2_1, relu3_1, relu4_1
SPLITS = [(0, 4), (4, 11), (11, 18), (18, 31)]


def make_nets(seed_enc=11, seed_dec=12):
    from seeded import fill_style_weights
    vgg, dec = make_vgg_ref(), make_decoder_ref()
    fill_style_weights(vgg, seed_enc)
    fill_style_weights(dec, seed_dec)
    return vgg, dec


def encode_with_intermediate(vgg, x):
    ch = list(vgg.children())
    out = []
    for a, b in SPLITS:
        for m in ch[a:b]:
            x = m(x)
        out.append(x)
    return out


def step_ref(vgg, dec, content, style, alpha=1.0):
    """(loss_c, loss_s, g_t); gradients flow into dec's parameters only"""
    for p in vgg.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        sf = encode_with_intermediate(vgg, style)
        cf = encode_with_intermediate(vgg, content)[-1]
        t = adain_ref(cf, sf[-1])
        t = alpha * t + (1 - alpha) * cf
    g_t = dec(t)
    gf = encode_with_intermediate(vgg, g_t)
    loss_c = torch.nn.functional.mse_loss(gf[-1], t)
    loss_s = 0.0
    for a, b in zip(gf, sf):
        ma, sa = calc_mean_std_ref(a)
        mb, sb = calc_mean_std_ref(b)
        loss_s = loss_s + torch.nn.functional.mse_loss(ma, mb) + torch.nn.functional.mse_loss(sa, sb)
    return loss_c, loss_s, g_t
