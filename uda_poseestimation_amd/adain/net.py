"""API mirror of the reference's adain/net.py (decoder, vgg, Net) with a DIFFERENTIABLE forward: the AdaIN decoder's pre-training
step (adain/train/train_human.py:182-213) on MI355X kernels.

`decoder` and `vgg` have the reference's child indices and state_dict keys (the same layer lists as lib/models/Style_net.py, as new
module instances).  `Net(vgg, decoder)` keeps the reference's enc_1..enc_4 split of vgg[:31] (frozen) and returns
(loss_c, loss_s, g_t) with the mean/std style loss (adain/net.py:137-146):

    loss_c = MSE(relu4_1(g_t), t)
    loss_s = sum over relu1_1 .. relu4_1 of MSE(mean, mean_style) + MSE(std, std_style),  std = sqrt(unbiased var + 1e-5)

`forward` is one torch.autograd.Function: it runs the three encoder passes, AdaIN and the decoder per op on NHWC activations of the
16-bit element type (fp32 accumulation) and keeps what the backward needs (the decoder's step inputs, the g_t pass's step outputs).
`loss.backward()` then fills `.grad` of the decoder's parameters (fp32, torch layout) and nothing else: the gradient runs through the
frozen encoder into g_t and through the decoder; t and the style statistics carry none.  A gradient arriving on g_t is added at the
decoder output.  The upstream scalars (d loss / d loss_c, d loss / d loss_s) are read on the device: no host synchronisation.

`Net.precision`: 'bf16' (default) or 'fp16' (the fp16 build of the library).
"""
import torch
import torch.nn as nn

from .. import _hip, ops
from ..lib.models import Style_net
from ..lib.models.Style_net import _compile

decoder = nn.Sequential(*Style_net._decoder_layers())
vgg = nn.Sequential(*Style_net._vgg_layers())

_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _c64(c):
    return (c + 63) // 64 * 64


class _StyleStepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, content, style, alpha, *params):
        loss_c, loss_s, g_t, saved = net._forward_impl(content, style, alpha)
        ctx.net, ctx.saved = net, saved
        return loss_c, loss_s, g_t

    @staticmethod
    def backward(ctx, grad_c, grad_s, grad_g):
        if ctx.saved is None:
            raise RuntimeError("adain.net.Net: the step's activations are released by its first backward; a second backward through the "
                               "same forward (retain_graph=True) is not supported - run the forward again")
        grads = ctx.net._backward_impl(ctx.saved, grad_c, grad_s, grad_g)
        ctx.saved = None
        return (None, None, None, None) + tuple(grads)


class Net(nn.Module):
    def __init__(self, encoder, decoder):
        super(Net, self).__init__()
        enc_layers = list(encoder.children())
        self.enc_1 = nn.Sequential(*enc_layers[:4])  # input -> relu1_1
        self.enc_2 = nn.Sequential(*enc_layers[4:11])  # relu1_1 -> relu2_1
        self.enc_3 = nn.Sequential(*enc_layers[11:18])  # relu2_1 -> relu3_1
        self.enc_4 = nn.Sequential(*enc_layers[18:31])  # relu3_1 -> relu4_1
        self.decoder = decoder
        self.mse_loss = nn.MSELoss()
        for name in ['enc_1', 'enc_2', 'enc_3', 'enc_4']:
            for param in getattr(self, name).parameters():
                param.requires_grad = False
        self.precision = 'bf16'
        # constant scale of the 16-bit gradients inside the backward (undone in the fp32 weight / bias gradients): the loss gradients
        # of this network are ~1e-7 per element, fp16's subnormal range (a power of two: exact in both directions).  Measured with
        # seeded weights on [0, 1) images; there is no overflow check: with networks whose relu4_1 features are orders of magnitude larger
        # lower it (fp16 saturates at 65504), or check the decoder's .grad with torch.isfinite
        self.grad_scale = 4096.0
        self._esteps = _compile(enc_layers[:31])
        self._dsteps = _compile(list(decoder.children()))
        self._dec_ids = {id(st.conv) for st in self._dsteps}
        self._taps = Style_net.Net._stage_ends([len(list(getattr(self, f"enc_{i}").children())) for i in range(1, 5)], enc_layers[:31])
        for k in self._taps[:3]:
            assert self._esteps[k].kind == "conv" and self._esteps[k + 1].kind == "conv"
        self._packs = {}
        self._bufs = {}
        self._pol = None

    # ---- packed weights.  The frozen encoder's packs are cached per parameter version; the decoder's are re-packed on every call (device
    # kernels, ~3.5 M parameters): a captured step then re-packs from the weights its own optimizer step just wrote on every replay, where a
    # cache decided on the host would replay stale packs
    def _policy(self):
        if self._pol is None:
            self._pol = _hip.policy(**Style_net._SeqRunner.policy_overrides)
        return self._pol

    @staticmethod
    def _folded(st):
        w, b = st.conv.weight.detach().float(), st.conv.bias.detach().float()
        if st.pre1x1 is not None:     # the 1x1 colour conv folded into the first 3x3 conv (reflection commutes with it)
            w1 = st.pre1x1.weight.detach().float().reshape(st.pre1x1.out_channels, st.pre1x1.in_channels)
            b = b + torch.einsum("omhw,m->o", w, st.pre1x1.bias.detach().float())
            w = torch.einsum("omhw,mc->ochw", w, w1)
        return w, b

    def _packed(self, st, d, direction, dt):
        conv = st.conv
        if id(conv) in self._dec_ids:
            return self._pack(st, d, direction, dt)
        ver = (conv.weight._version, conv.bias._version, conv.weight.data_ptr(),
               None if st.pre1x1 is None else (st.pre1x1.weight._version, st.pre1x1.bias._version))
        key = (id(conv), direction, dt, d.Ci, d.Co)
        hit = self._packs.get(key)
        if hit is None or hit[0] != ver:
            hit = (ver,) + self._pack(st, d, direction, dt)
            self._packs[key] = hit
        return hit[1], hit[2]

    def _pack(self, st, d, direction, dt):
        w, b = self._folded(st)
        if direction == "bwd" and (w.shape[0] != d.Co or w.shape[1] != d.Ci):   # zero-padded 3-channel end layers
            wp = torch.zeros(d.Co, d.Ci, 3, 3, dtype=torch.float32, device=w.device)
            wp[:w.shape[0], :w.shape[1]] = w
            w = wp
        return ops.pack_weight(w.contiguous(), d, direction, dtype=dt), b.contiguous()

    def _fdesc(self, N, H, W, Ci, Co, up):
        return ops.conv_desc(N, H, W, Ci, Co, 3, 1, 1, reflect=True, upsample=up, policy=self._policy())

    @staticmethod
    def _bdesc(N, H, W, Ci, Co, up):
        return ops.conv_desc(N, H, W, _c64(Ci), _c64(Co), 3, 1, 1, reflect=True, upsample=up)

    def _run(self, steps, x, dt, final_f32=False):
        """every step's output (the list the backward walks)"""
        outs = []
        for si, st in enumerate(steps):
            if st.kind == "pool":
                x = ops.maxpool2x2_ceil(x)
            else:
                N, H, W, Ci = x.shape
                d = self._fdesc(N, H, W, Ci, st.conv.out_channels, st.upsample)
                w, b = self._packed(st, d, "fwd", dt)
                x = ops.conv2d_fwd(x, w, d, bias=b, relu=st.relu, out_f32=(final_f32 and si == len(steps) - 1))
            outs.append(x)
        return outs

    def _bwd_buffers(self, N, H, W, dt, dev, gouts, dins):
        """workspaces of the backward, allocated on the first call for a shape (and the tap tables built) - reused afterwards"""
        key = (N, H, W, dt)
        b = self._bufs.get(key)
        if b is not None:
            return b
        descs = []
        for i, st in enumerate(self._esteps):
            if st.kind == "conv":
                xi = (N, H, W, 8) if i == 0 else tuple(gouts[i - 1].shape)
                descs.append(self._bdesc(xi[0], xi[1], xi[2], xi[3], st.conv.out_channels, False))
        for j, st in enumerate(self._dsteps):
            s = dins[j].shape
            descs.append(self._bdesc(s[0], s[1], s[2], s[3], st.conv.out_channels, st.upsample))
        for d in descs:
            ops.conv_bwd_prepare(d, dt)
        ws = max(ops.conv_bwd_ws_bytes(d) for d in descs)
        bws = max(ops.bias_grad_ws_bytes(N * (H + 1) * (W + 1), _c64(st.conv.out_channels)) for st in self._dsteps)
        b = dict(ws=torch.empty(ws, dtype=torch.uint8, device=dev), bws=torch.empty(bws, dtype=torch.uint8, device=dev),
                 mws=torch.empty(ops.feat_mse_ws_bytes(), dtype=torch.uint8, device=dev),
                 zero=torch.zeros((), dtype=torch.float32, device=dev))
        self._bufs[key] = b
        return b

    def _forward_impl(self, content, style, alpha):
        _hip.require_cuda(content, style)
        if self.precision not in _DTYPES:
            raise ValueError("precision must be 'bf16' or 'fp16'")
        dt = _DTYPES[self.precision]
        N, _, H, W = content.shape
        s_outs = self._run(self._esteps, ops.to_nhwc_bf16(style.detach().float().contiguous(), 8, dtype=dt), dt)
        c_last = self._run(self._esteps, ops.to_nhwc_bf16(content.detach().float().contiguous(), 8, dtype=dt), dt)[-1]
        t = ops.adain(c_last, s_outs[-1], alpha=alpha if torch.is_tensor(alpha) else float(alpha))
        d_outs = self._run(self._dsteps, t, dt, final_f32=True)
        g_t = ops.to_nchw_f32(d_outs[-1], 3)
        g_outs = self._run(self._esteps, ops.to_nhwc_bf16(g_t, 8, dtype=dt), dt)
        dins = [t] + d_outs[:-1]
        bufs = self._bwd_buffers(N, H, W, dt, content.device, g_outs, dins)
        stats = [ops.adain(g_outs[k], s_outs[k], stats_only=True) for k in self._taps]
        loss_s = torch.empty((), dtype=torch.float32, device=content.device)
        for i, st in enumerate(stats):
            ops.style_stat_loss(st, loss_s, accumulate=i > 0)
        loss_c = ops.feat_mse(g_outs[-1], t, bufs["mws"])
        saved = dict(dt=dt, t=t, dins=dins, g_outs=g_outs, stats=stats, bufs=bufs, N=N, H=H, W=W)
        return loss_c, loss_s, g_t, saved

    def _backward_impl(self, sv, grad_c, grad_s, grad_g):
        dt, bufs, g_outs, stats, t = sv["dt"], sv["bufs"], sv["g_outs"], sv["stats"], sv["t"]
        N, H, W = sv["N"], sv["H"], sv["W"]
        ws = bufs["ws"]
        gs_c = bufs["zero"] if grad_c is None else grad_c.detach().float().contiguous()
        gs_s = bufs["zero"] if grad_s is None else grad_s.detach().float().contiguous()
        gadd = None if grad_g is None else grad_g.detach().float().contiguous()

        def padded(d):
            n = d.N * ((d.Hi << d.upsample) + 2) * ((d.Wi << d.upsample) + 2) * d.Ci
            return ws[:n * 2].view(dt).view(d.N, (d.Hi << d.upsample) + 2, (d.Wi << d.upsample) + 2, d.Ci)

        # ---- encoder (the g_t pass), relu4_1 back to the image
        steps, tap_of = self._esteps, {k: i for i, k in enumerate(self._taps)}
        L = len(steps) - 1
        y = g_outs[L]
        dz = torch.empty_like(y)
        S = self.grad_scale
        ops.reflect_fold(dz, x=y, relu_mask=True, stats=stats[tap_of[L]], gscale_s=gs_s, t=t, gscale_c=gs_c, c_scale=2.0 / y.numel(), term_scale=S)
        i = L
        while True:
            st = steps[i]
            xs = (N, H, W, 8) if i == 0 else tuple(g_outs[i - 1].shape)
            d = self._bdesc(xs[0], xs[1], xs[2], xs[3], st.conv.out_channels, False)
            w_bwd, _ = self._packed(st, d, "bwd", dt)
            dP = ops.conv2d_bwd_data_reflect_padded(dz, w_bwd, d, padded(d))
            if i == 0:     # d g_t: 3 real channels of 64 (the rest exactly zero): the decoder's last layer's padded dy
                dy = torch.empty(N, H, W, 64, dtype=dt, device=dz.device)
                ops.reflect_fold(dy, dP=dP, add_nchw=gadd, term_scale=S)
                break
            yp = g_outs[i - 1]
            if steps[i - 1].kind == "pool":
                dpool = ops.reflect_fold(torch.empty_like(yp), dP=dP)
                dz = ops.maxpool2x2_ceil_bwd(g_outs[i - 2], dpool, relu_mask=True)
                i -= 2
            else:
                k = tap_of.get(i - 1)
                dz = ops.reflect_fold(torch.empty_like(yp), dP=dP, x=yp, relu_mask=True, stats=None if k is None else stats[k], gscale_s=gs_s,
                                       term_scale=S)
                i -= 1

        # ---- decoder, last layer back to the first: weight + bias gradients, and the data gradient below every layer but the first
        grads = {}
        dins = sv["dins"]
        for j in range(len(self._dsteps) - 1, -1, -1):
            st, xj = self._dsteps[j], dins[j]
            Co = st.conv.out_channels
            d = self._bdesc(xj.shape[0], xj.shape[1], xj.shape[2], xj.shape[3], Co, st.upsample)
            grads[id(st.conv.weight)] = ops.conv2d_bwd_weight_reflect(dy, xj, d, ws, co_valid=Co, out_scale=1.0 / S)
            grads[id(st.conv.bias)] = ops.bias_grad(dy, bufs["bws"], c_valid=Co, out_scale=1.0 / S)
            if j > 0:
                w_bwd, _ = self._packed(st, d, "bwd", dt)
                dP = ops.conv2d_bwd_data_reflect_padded(dy, w_bwd, d, padded(d))
                dy = ops.reflect_fold(torch.empty_like(xj), dP=dP, upsample=st.upsample, x=xj, relu_mask=True)
        return [grads.get(id(p)) for p in self._dec_params()]

    def _dec_params(self):
        out = []
        for st in self._dsteps:
            out += [st.conv.weight, st.conv.bias]
        return out

    def forward(self, content, style, alpha=1.0):
        if not torch.is_tensor(alpha):
            assert 0 <= alpha <= 1
        return _StyleStepFn.apply(self, content, style, alpha, *self._dec_params())
