"""Input gradients through PoseResNet, the host side (no GPU): the float64 reference the GPU tests measure csrc/stem_dgrad.hip against
(tests/helpers/stem_dgrad_fp64.py) is the adjoint torch.autograd gives for the stem convolution, and the two entry points are declared,
bound, defined and documented."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from helpers import fp64_conv
from helpers import stem_dgrad_fp64 as S64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,H,W", [(1, 16, 24), (2, 40, 24), (1, 8, 8)])
def test_reference_is_autograd_of_conv2d_in_float64(N, H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn(N, 3, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(64, 3, 7, 7, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, stride=2, padding=3)
    assert tuple(y.shape) == (N, 64, H // 2, W // 2)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (dx,) = torch.autograd.grad(y, x, dy)
    ref, absref = S64.stem_dgrad(dy.permute(0, 2, 3, 1).contiguous(), w)
    assert ref.shape == dx.shape == absref.shape
    assert float((ref - dx).abs().max()) < 1e-12 * float(dx.abs().max())
    assert bool((absref >= ref.abs() * (1 - 1e-12)).all())
    # the forward the adjoint belongs to: F.conv2d agrees with the helper's own direct convolution for this geometry
    geom = S64.stem_geom(N, H, W)
    x8 = torch.zeros(N, H, W, 8, dtype=torch.float64)
    x8[..., :3] = x.detach().permute(0, 2, 3, 1)
    yf, _ = fp64_conv.fprop(geom, x8, fp64_conv.phys_weight(w, geom))
    assert float((yf.permute(0, 3, 1, 2) - y.detach()).abs().max()) < 1e-12 * float(y.detach().abs().max())


def test_entry_points_are_declared_bound_defined_and_documented():
    import ctypes as C
    from uda_poseestimation_amd import _hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "udapose.h")).read(), flags=re.S)
    assert re.search(r"^int udapose_stem_dgrad\(void\* stream, const void\* dy, const float\* w, int N, int H, int W, float\* dx\);", hdr, flags=re.M)
    assert re.search(r"^int udapose_net_input_grad\(udapose_net_t net, void\* stream, const void\* const\* h_params, void\* ws, float\* dx\);", hdr,
                     flags=re.M)
    vp, ci = C.c_void_p, C.c_int
    assert _hip._SIGS["udapose_stem_dgrad"] == (ci, [vp, vp, vp, ci, ci, ci, vp])
    assert _hip._SIGS["udapose_net_input_grad"] == (ci, [vp, vp, vp, vp, vp])
    assert {"udapose_stem_dgrad", "udapose_net_input_grad"} <= set(_hip.EXPORTS)
    csrc = os.path.join(ROOT, "uda_poseestimation_amd", "csrc")
    capi = open(os.path.join(csrc, "capi.hip")).read()
    assert "int udapose_stem_dgrad(" in capi and "int udapose_net_input_grad(" in capi
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "stem_dgrad.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "udapose_stem_dgrad" in text and "udapose_net_input_grad" in text, doc
    assert "4.15" in open(os.path.join(ROOT, "DESIGN.md")).read()
