"""Float64 reference of the stem's data gradient (csrc/stem_dgrad.hip, udapose_stem_dgrad): the adjoint of Conv2d(3, 64, 7, stride 2, pad 3)
through tests/helpers/fp64_conv.py's tap loops, in the kernel's layouts - dy NHWC [N][H/2][W/2][64], w in torch's [64][3][7][7], dx NCHW
[N][3][H][W].  tests/test_input_grad_cpu.py checks it against torch.autograd of F.conv2d in float64."""
import torch

from helpers import fp64_conv
from helpers.fp64_conv import Geom, phys_weight


def stem_geom(N, H, W):
    """The stem as the library's plans describe it: 3 input channels padded to 8, 7 filter columns padded to 8."""
    return Geom(N, H, W, 8, 64, 7, 7, 2, 3)


def stem_dgrad(dy, w):
    """(ref, absref) float64 NCHW [N, 3, H, W]: dx = conv^T(dy, w), and the same on |dy|, |w| (the scale of fp64_conv.check's bars)."""
    N, Ho, Wo, Co = dy.shape
    assert Co == 64 and tuple(w.shape) == (64, 3, 7, 7)
    g = stem_geom(N, 2 * Ho, 2 * Wo)
    assert (g.Ho, g.Wo) == (Ho, Wo)
    ref, absref = fp64_conv.dgrad(g, dy, phys_weight(w, g))
    return ref[..., :3].permute(0, 3, 1, 2).contiguous(), absref[..., :3].permute(0, 3, 1, 2).contiguous()


def round_to(t, dtype):
    """t rounded to the element type (round to nearest even, as the kernels' conversions), back in float32."""
    return t.float().to(dtype).float()
