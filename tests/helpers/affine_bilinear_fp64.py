"""torchvision's tensor `affine` (zero fill) restated with a dtype and an interpolation mode: the reference of the bilinear re-warp.

The grid construction is oracle/affine_ref.py's (_gen_affine_grid: base grid at half-integers, theta / (0.5 * [W, H]); then
grid_sample(padding_mode="zeros", align_corners=False)), with two differences: the inverse matrix comes in as its six fp32 VALUES - what
the kernel receives - and the grid and the sampling run in `dtype`.  With float32 and "nearest" it is the oracle bit for bit
(tests/test_warp_bilinear_cpu.py); with float64 it is the reference the device is held to, with float32 the yardstick of that comparison
(torch's own fp32 arithmetic on the CPU).  Everything is differentiable with respect to the image.
"""
import torch
import torch.nn.functional as F


def affine_ref(img, m6, dtype=torch.float64, mode="bilinear"):
    """img [C,H,W] -> [C,H,W] in `dtype`; m6: the six fp32 values of the inverse affine matrix (row-major 2x3)."""
    C, H, W = img.shape
    theta = torch.as_tensor(m6, dtype=torch.float32).reshape(1, 2, 3).to(dtype)
    xs = torch.linspace(-W * 0.5 + 0.5, W * 0.5 - 0.5, W, dtype=dtype)
    ys = torch.linspace(-H * 0.5 + 0.5, H * 0.5 - 0.5, H, dtype=dtype)
    base = torch.empty(1, H, W, 3, dtype=dtype)
    base[..., 0] = xs[None, None, :]
    base[..., 1] = ys[None, :, None]
    base[..., 2] = 1
    resc = theta.transpose(1, 2) / torch.tensor([0.5 * W, 0.5 * H], dtype=dtype)
    grid = base.reshape(1, H * W, 3).bmm(resc).reshape(1, H, W, 2)
    return F.grid_sample(img[None].to(dtype), grid, mode=mode, padding_mode="zeros", align_corners=False)[0]


def chain_ref(img, thetas, dtype=torch.float64, mode="bilinear"):
    """img [N,C,H,W], thetas [N,S,6] fp32 -> [N,C,H,W] in `dtype`: S sequential warps per sample, stage 0 first."""
    thetas = torch.as_tensor(thetas, dtype=torch.float32).cpu()
    out = []
    for n in range(img.shape[0]):
        t = img[n]
        for s in range(thetas.shape[1]):
            t = affine_ref(t, thetas[n, s], dtype, mode)
        out.append(t)
    return torch.stack(out)
