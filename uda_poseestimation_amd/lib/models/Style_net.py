"""AdaIN style-transfer network (API mirror of the reference's lib/models/Style_net.py:4-177) on MI355X kernels.

`vgg` and `decoder` are module-level nn.Sequential singletons with the reference's exact child indices, so the
training script's `Style_net.decoder.load_state_dict(...)`, `Style_net.vgg.load_state_dict(...)`,
`nn.Sequential(*list(vgg.children())[:31])` and `Style_net.Net(vgg, decoder)` (train_human.py:120-131) work unchanged.
The children are parameter containers: `Net.forward` walks them and issues one fused kernel per
[ReflectionPad2d -> Conv2d -> ReLU] group (reflection, nearest x2 upsample, bias and ReLU live inside the conv
kernel), the ceil-mode max-pools, and the AdaIN kernel, on NHWC activations.

Three precisions (`Net.precision`):
  'f16x2' (default): the fast fp32-grade mode - the loop runs the style net OUTSIDE autocast, in fp32 (train_human.py:347-356).
                    Activations and weights as fp16 pairs (h, l), three fp16 MFMAs per K step, fp32 accumulation, fp32 AdaIN
                    statistics: g_t within ~5e-6 * max of the reference's output (tests/test_gpu_f16x2.py), 2.5x the speed of
                    the exact mode.  Range of activations: |x| <= 65504 (saturating).
  'fp32':           fp32 storage and the exact fp32 MFMA (v_mfma_f32_16x16x4_f32); ~5x slower than bf16.
  'bf16':           bf16 storage, bf16 MFMA, fp32 accumulation - the fastest mode; g_t within ~8e-2 * max of the fp32 result
                    after 19 un-normalised conv layers (tests/test_gpu_hotpath.py).

`forward` returns (loss_c, loss_s, g_t) like the reference.  The training loop consumes only [2] (train_human.py:275,350,355)
and the two losses cost a third encoder pass plus eight Gram matrices, so they are computed only when
`Net.compute_losses = True`; otherwise they are NaN (not a silent zero): a caller that does use them notices at once.
"""
import torch
import torch.nn as nn

from ... import _hip, ops
from ... import heatmap_args as ha
from .loss import _cons_fwd


def _nchw_feat(feat):
    assert feat.dim() == 4
    _hip.require_cuda(feat)
    return feat.detach().float().contiguous()


def calc_mean_std(feat, eps=1e-5):
    """Per-(n,c) mean and sqrt(unbiased var + eps) over H*W (Style_net.py:4-12), from the AdaIN kernel's fp32 statistics."""
    size = feat.size()
    assert (len(size) == 4)
    N, C = size[:2]
    x = ops.to_nhwc_f32(_nchw_feat(feat), (C + 63) // 64 * 64)
    st = ops.adain(x, x, alpha=0.0, eps=eps, stats_only=True)
    return st[:, :C, 0].reshape(N, C, 1, 1).to(feat.dtype), st[:, :C, 1].reshape(N, C, 1, 1).to(feat.dtype)


def adain(content_feat, style_feat):
    """(content - mean_c) / std_c * std_s + mean_s (Style_net.py:21-29); NCHW fp32 in/out at the API boundary, fp32 inside."""
    assert (content_feat.size()[:2] == style_feat.size()[:2])
    N, C, H, W = content_feat.shape
    Cp = (C + 63) // 64 * 64
    out = ops.adain(ops.to_nhwc_f32(_nchw_feat(content_feat), Cp), ops.to_nhwc_f32(_nchw_feat(style_feat), Cp), alpha=1.0)
    return ops.to_nchw_f32(out, C).to(content_feat.dtype)


def gram_matrix(y):
    """features @ features^T / (ch*h*w) per image (Style_net.py:14-19).  One exact-fp32 MFMA launch per image: the NCHW
    feature map of an image IS the [ch][h*w] matrix F, and F F^T is the 1x1 "convolution" of F (ch pixels, h*w channels)
    with F itself as the weight."""
    f = _nchw_feat(y)
    b, ch, h, w = f.shape
    if (h * w) % 64 or ch % 8:
        raise NotImplementedError("gram_matrix on the device needs h*w % 64 == 0")
    d = ops.conv_desc(1, ch, 1, h * w, ch, 1)
    out = torch.empty(b, ch, ch, dtype=torch.float32, device=f.device)
    for n in range(b):
        g = ops.conv2d_fwd(f[n].reshape(1, ch, 1, h * w), f[n].reshape(ch, 1, h * w), d)
        out[n] = g.reshape(ch, ch)
    return out / (ch * h * w)


def _mse(a, b):
    """nn.MSELoss() of two equally shaped fp32 tensors on the device (one sweep)."""
    assert a.shape == b.shape
    return _cons_fwd(ha.f32c(a), ha.f32c(b))[1]      # (ConsLoss's forward without a mask: the mean of (a - b)^2 over everything)


# decoder (Style_net.py:32-62): mirror of the encoder; 'U' = nearest x2 upsample; the last conv has no ReLU
_DECODER_CFG = [(512, 256), 'U', (256, 256), (256, 256), (256, 256), (256, 128), 'U', (128, 128), (128, 64), 'U', (64, 64), (64, 3)]


def _decoder_layers():
    mods = []
    for i, v in enumerate(_DECODER_CFG):
        if v == 'U':
            mods.append(nn.Upsample(scale_factor=2, mode='nearest'))
        else:
            mods += [nn.ReflectionPad2d((1, 1, 1, 1)), nn.Conv2d(v[0], v[1], (3, 3))]
            if i != len(_DECODER_CFG) - 1:
                mods.append(nn.ReLU())
    return mods


decoder = nn.Sequential(*_decoder_layers())


def _vgg_layers():
    cfg = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512]
    mods = [nn.Conv2d(3, 3, (1, 1))]
    cin = 3
    for v in cfg:
        if v == 'M':
            mods.append(nn.MaxPool2d((2, 2), (2, 2), (0, 0), ceil_mode=True))
        else:
            mods += [nn.ReflectionPad2d((1, 1, 1, 1)), nn.Conv2d(cin, v, (3, 3)), nn.ReLU()]
            cin = v
    return mods


vgg = nn.Sequential(*_vgg_layers())


class _Step:
    __slots__ = ("kind", "conv", "pre1x1", "relu", "upsample")

    def __init__(self, kind, conv=None, pre1x1=None, relu=False, upsample=False):
        self.kind, self.conv, self.pre1x1, self.relu, self.upsample = kind, conv, pre1x1, relu, upsample


def _compile(children):
    """Group a child list into fused device steps."""
    steps, i, pend_up, pend_1x1 = [], 0, False, None
    ch = list(children)
    while i < len(ch):
        m = ch[i]
        if isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1):
            pend_1x1 = m          # 3->3 colour transform: folded into the next 3x3 conv (reflection pad commutes with it)
            i += 1
        elif isinstance(m, nn.Upsample):
            pend_up = True
            i += 1
        elif isinstance(m, nn.ReflectionPad2d):
            conv = ch[i + 1]
            assert isinstance(conv, nn.Conv2d) and conv.kernel_size == (3, 3), "expected ReflectionPad2d -> Conv2d(3x3)"
            relu = i + 2 < len(ch) and isinstance(ch[i + 2], nn.ReLU)
            steps.append(_Step("conv", conv, pend_1x1, relu, pend_up))
            pend_up, pend_1x1 = False, None
            i += 3 if relu else 2
        elif isinstance(m, nn.MaxPool2d):
            steps.append(_Step("pool"))
            i += 1
        else:
            raise NotImplementedError(f"unsupported style-net child {type(m).__name__}")
    assert pend_1x1 is None and not pend_up
    return steps


class _SeqRunner:
    """Runs a compiled step list on NHWC tensors (bf16 or fp32: the input's dtype decides); packed weights are cached per
    precision until a parameter changes."""

    # dispatch policy of the style convolutions: they run alone on one stream over 32x32 .. 256x256 maps (hundreds of thousands of
    # rows), where 128x128 tiles pay (profiles/r3_ab_runs.txt) - unlike in the three-stream pose step, whose policy stays the default
    policy_overrides = {"igemm_big_min": 1024}

    def __init__(self, children):
        self.steps = _compile(children)
        self._packs = {}
        self._pol = None

    def policy(self):
        if self._pol is None:
            self._pol = _hip.policy(**self.policy_overrides)
        return self._pol

    def _packed(self, st, d, f32):
        """f32: False (16-bit element type), True (fp32) or 'split' (f16x2)"""
        conv = st.conv
        ver = (conv.weight._version, conv.bias._version, conv.weight.data_ptr(),
               None if st.pre1x1 is None else (st.pre1x1.weight._version, st.pre1x1.bias._version))
        hit = self._packs.get((id(conv), f32))
        if hit is None or hit[0] != ver:
            w, b = conv.weight.detach().float(), conv.bias.detach().float()
            if st.pre1x1 is not None:
                w1 = st.pre1x1.weight.detach().float().reshape(st.pre1x1.out_channels, st.pre1x1.in_channels)
                b1 = st.pre1x1.bias.detach().float()
                b = b + torch.einsum("omhw,m->o", w, b1)
                w = torch.einsum("omhw,mc->ochw", w, w1)
            if not f32:
                wp = ops.pack_weight(w.contiguous(), d, "fwd")
            elif d.Ci == 8:
                # [Co][KH][KWp = 8][8] fp32: three real channels, three real column taps, zero elsewhere
                wp = torch.zeros(d.Co, d.KH, ops.kwp(d), 8, dtype=torch.float32, device=w.device)
                wp[:, :, :d.KW, :w.shape[1]] = w.permute(0, 2, 3, 1)
            else:
                wp = w.permute(0, 2, 3, 1).contiguous()             # [Co][KH][KW][Ci] = the GEMM layout [Co][taps][Ci]
            if f32 == 'split':
                wp = ops.f32_to_split(wp)                           # the same layout, every 8 values as [8 h][8 l]
            hit = (ver, wp, b.contiguous())
            self._packs[(id(conv), f32)] = hit
        return hit[1], hit[2]

    def run(self, x, taps=None, final_f32=False):
        """x NHWC bf16 or fp32.  `taps`: step indices after which to record the activation (encode_with_intermediate)."""
        outs = []
        f32 = 'split' if x.dtype == ops.SPLIT else x.dtype == torch.float32
        for si, st in enumerate(self.steps):
            if st.kind == "pool":
                x = ops.maxpool2x2_ceil(x)
            else:
                N, H, W, Cin = x.shape
                d = ops.conv_desc(N, H, W, Cin, st.conv.out_channels, 3, 1, 1, reflect=True, upsample=st.upsample, policy=self.policy())
                w, b = self._packed(st, d, f32)
                last = si == len(self.steps) - 1
                x = ops.conv2d_fwd(x, w, d, bias=b, relu=st.relu, out_f32=(final_f32 and last))
            if taps is not None and si in taps:
                outs.append(x)
        return (x, outs) if taps is not None else x


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
        self.precision = 'f16x2'          # fp32-grade: the reference runs this network in fp32 (module docstring); 'bf16' is the fast mode
        self.compute_losses = False       # True: loss_c / loss_s as in Style_net.py:151-177 (a third encoder pass + Gram matrices)
        self._enc = _SeqRunner(enc_layers[:31])
        self._dec = _SeqRunner(list(decoder.children()))
        # step indices that end enc_1..enc_4 (relu1_1, relu2_1, relu3_1, relu4_1)
        self._enc_taps = self._stage_ends([len(list(getattr(self, f"enc_{i}").children())) for i in range(1, 5)], enc_layers[:31])

    @staticmethod
    def _stage_ends(stage_child_counts, children):
        ends, acc, steps_seen, i = [], 0, 0, 0
        bounds = []
        for c in stage_child_counts:
            acc += c
            bounds.append(acc)
        ch = list(children)
        si = -1
        out = []
        for b in bounds:
            while i < b:
                m = ch[i]
                if isinstance(m, nn.ReflectionPad2d):
                    relu = i + 2 < len(ch) and isinstance(ch[i + 2], nn.ReLU)
                    si += 1
                    i += 3 if relu else 2
                elif isinstance(m, nn.MaxPool2d):
                    si += 1
                    i += 1
                else:
                    i += 1
            out.append(si)
        return out

    def _image_in(self, img):
        _hip.require_cuda(img)
        if self.precision not in ('bf16', 'fp32', 'f16x2'):
            raise ValueError("precision must be 'f16x2', 'fp32' or 'bf16'")
        x = img.detach().float().contiguous()
        if self.precision == 'f16x2':
            return ops.to_nhwc_split(x, 8)
        return ops.to_nhwc_f32(x, 8) if self.precision == 'fp32' else ops.to_nhwc_bf16(x, 8)

    def _intermediate(self, x_nhwc):
        """(relu4_1 NHWC, [relu1_1 .. relu4_1] as NCHW fp32)"""
        last, feats = self._enc.run(x_nhwc, taps=set(self._enc_taps))
        return last, [ops.to_nchw_f32(f) for f in feats]

    def encode_with_intermediate(self, input):
        """relu1_1, relu2_1, relu3_1, relu4_1 as NCHW fp32 tensors (Style_net.py:136-142)."""
        return self._intermediate(self._image_in(input))[1]

    def encode(self, input):
        return ops.to_nchw_f32(self._enc.run(self._image_in(input)))

    def calc_content_loss(self, input, target):
        assert (input.size() == target.size())
        assert (target.requires_grad is False)
        return _mse(input, target)

    def calc_style_loss(self, input, target):
        assert (input.size() == target.size())
        assert (target.requires_grad is False)
        return _mse(gram_matrix(input), gram_matrix(target))

    # ---- the two halves of forward(), for callers that transfer in BOTH directions between the same two batches (the loop's s2t and
    # t2s passes, train_human.py:347-356, encode x_s and x_t twice each): encode once, transfer twice - same kernels on the same
    # inputs, so the results are bit-identical to two forward() calls
    def encode_features(self, img):
        """relu4_1 of `img` as the internal NHWC tensor of this network's precision (input of transfer_from_features)."""
        with torch.no_grad():
            return self._enc.run(self._image_in(img))

    def transfer_from_features(self, content_feat, style_feat, alpha=1.0, clamp=None):
        """g_t (NCHW fp32) of forward(content, style, alpha, clamp)[2] from the two images' encode_features()."""
        if not torch.is_tensor(alpha):
            assert 0 <= alpha <= 1
        with torch.no_grad():
            t = ops.adain(content_feat, style_feat, alpha=alpha if torch.is_tensor(alpha) else float(alpha))
            g = self._dec.run(t, final_f32=True)
            lo, hi = (None, None) if clamp is None else (clamp[0].float().contiguous(), clamp[1].float().contiguous())
            return ops.to_nchw_f32(g, 3, lo, hi)

    def forward(self, content, style, alpha=1.0, clamp=None):
        """-> (loss_c, loss_s, g_t) (Style_net.py:163-177).  `clamp=(lo[3], hi[3])` fuses the loop's recover clamp
        (train_human.py:351) into the output conversion (the losses, when computed, see the unclamped g_t like the reference).
        `alpha` may be a one-element fp32 CUDA tensor: the blend factor is then read on the device when the kernel runs."""
        if not torch.is_tensor(alpha):
            assert 0 <= alpha <= 1
        with torch.no_grad():
            if self.compute_losses:
                sf, style_feats = self._intermediate(self._image_in(style))
            else:
                sf = self._enc.run(self._image_in(style))
            cf = self._enc.run(self._image_in(content))
            t = ops.adain(cf, sf, alpha=alpha if torch.is_tensor(alpha) else float(alpha))              # alpha-blend fused (Style_net.py:167-168)
            g = self._dec.run(t, final_f32=True)                    # [N,H,W,3] fp32
            lo, hi = (None, None) if clamp is None else (clamp[0].float().contiguous(), clamp[1].float().contiguous())
            g_t = ops.to_nchw_f32(g, 3, lo, hi)
            if not self.compute_losses:
                nan = torch.full((), float("nan"), device=g_t.device)
                return nan, nan.clone(), g_t
            g_plain = g_t if clamp is None else ops.to_nchw_f32(g, 3)
            g_t_feats = self.encode_with_intermediate(g_plain)
            loss_c = self.calc_content_loss(g_t_feats[-1], ops.to_nchw_f32(t))
            loss_s = self.calc_style_loss(g_t_feats[0], style_feats[0])
            for i in range(1, 4):
                loss_s = loss_s + self.calc_style_loss(g_t_feats[i], style_feats[i])
        return loss_c, loss_s, g_t
