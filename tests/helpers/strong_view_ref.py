"""The strong student view's references (test-only): the PIL calls themselves - ImageOps.autocontrast / equalize / posterize / solarize,
ImageEnhance.Sharpness, and the chain of several ops - and plain-numpy restatements of the arithmetic the device performs
(csrc/strong_aug.hip): the autocontrast and equalize tables from a histogram, the SMOOTH stencil in float32, the blend.
tests/test_strong_view_cpu.py ties every restatement to PIL; tests/test_gpu_strong_view.py compares the device with PIL directly and, where
PIL would be too slow (the exhaustive autocontrast batch), with the restatement."""
import math

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

# 255.0 / d for d = 1 .. 255 as Python computes it: the table data_gpu uploads (the device never divides in fp64)
SCALE_TABLE = np.array([255.0 / d for d in range(1, 256)], dtype=np.float64)


def solarize_cut(threshold):
    """`i < threshold` for an integer i = `i < ceil(threshold)`: the integer cut data_gpu hands to the device, clipped to [0, 256]."""
    return int(min(256, max(0, math.ceil(threshold))))


# ---------------------------------------------------------------------------------------------------------------- PIL itself
def pil_op(img_u8, code, param=None):
    """One op of data_gpu.STRONG_OPS on an [H,W,3] uint8 image, by PIL."""
    im = Image.fromarray(np.ascontiguousarray(img_u8))
    if code == 0:
        out = im
    elif code in (1, 2, 3):
        out = {1: ImageEnhance.Brightness, 2: ImageEnhance.Contrast, 3: ImageEnhance.Color}[code](im).enhance(param)
    elif code == 4:
        out = ImageOps.autocontrast(im)
    elif code == 5:
        out = ImageOps.equalize(im)
    elif code == 6:
        out = ImageOps.posterize(im, int(param))
    elif code == 7:
        out = ImageOps.solarize(im, param)
    elif code == 8:
        out = ImageEnhance.Sharpness(im).enhance(param)
    else:
        raise ValueError(code)
    return np.array(out)


def pil_chain(img_u8, codes, params):
    for c, p in zip(codes, params):
        img_u8 = pil_op(img_u8, c, p)
    return img_u8


def pil_smooth(img_u8):
    from PIL import ImageFilter
    return np.array(Image.fromarray(np.ascontiguousarray(img_u8)).filter(ImageFilter.SMOOTH))


# ---------------------------------------------------------------------------------------------------------------- restatements
def histograms(img_u8):
    """[3][256] int64 counts of an [H,W,3] image"""
    return np.stack([np.bincount(img_u8[..., c].reshape(-1), minlength=256) for c in range(3)])


def autocontrast_table(h, scale_table=SCALE_TABLE):
    """One channel's table from its 256 counts: lo / hi = first / last non-empty bin; identity when hi <= lo; else
    int(ix * scale + offset) in float64 - product and sum rounded separately - truncated toward zero, clipped to 0..255, with
    scale = scale_table[hi - lo - 1] and offset = -lo * scale."""
    nz = np.nonzero(h)[0]
    ident = np.arange(256, dtype=np.int64)
    if len(nz) == 0 or nz[-1] <= nz[0]:
        return ident
    return autocontrast_table_lo_hi(int(nz[0]), int(nz[-1]), scale_table)


def autocontrast_table_lo_hi(lo, hi, scale_table=SCALE_TABLE):
    scale = np.float64(scale_table[hi - lo - 1])
    offset = np.float64(-lo) * scale
    v = np.arange(256, dtype=np.float64) * scale + offset          # (numpy rounds the product, then the sum: no fused form)
    return np.clip(np.trunc(v), 0, 255).astype(np.int64)


def equalize_table(h):
    """One channel's table, integers only: step = (total - last non-zero count) // 255; identity when at most one bin is filled or
    step == 0; else entry i = (step // 2 + sum(h[:i])) // step, which can be 256 and is clipped to 255 (as Image.point does)."""
    h = np.asarray(h, dtype=np.int64)
    nz = h[h != 0]
    ident = np.arange(256, dtype=np.int64)
    if len(nz) <= 1:
        return ident
    step = (int(nz.sum()) - int(nz[-1])) // 255
    if step == 0:
        return ident
    before = np.concatenate([[0], np.cumsum(h)[:-1]])
    return np.minimum((step // 2 + before) // step, 255)


def posterize_table(bits):
    return np.arange(256, dtype=np.int64) & ~(2 ** (8 - int(bits)) - 1) & 0xFF


def solarize_table(cut):
    i = np.arange(256, dtype=np.int64)
    return np.where(i < int(cut), i, 255 - i)


def apply_tables(img_u8, tables):
    """tables [3][256] -> the image through them, channel by channel"""
    return np.stack([np.asarray(tables[c], dtype=np.uint8)[img_u8[..., c]] for c in range(3)], axis=-1)


def point_op_np(img_u8, code, param=None):
    """Ops 4-7 as the device computes them (table from the histogram / the parameter, then a look-up)."""
    if code == 4:
        t = [autocontrast_table(h) for h in histograms(img_u8)]
    elif code == 5:
        t = [equalize_table(h) for h in histograms(img_u8)]
    elif code == 6:
        t = [posterize_table(param)] * 3
    elif code == 7:
        t = [solarize_table(solarize_cut(param))] * 3
    else:
        raise ValueError(code)
    return apply_tables(img_u8, t)


def _clip8(v):
    """libImaging's clip8 on float32: <= 0 -> 0, >= 255 -> 255, else truncation"""
    return np.where(v <= 0, 0, np.where(v >= 255, 255, np.trunc(v))).astype(np.uint8)


def smooth_np(img_u8, bottom_up=False):
    """ImageFilter.SMOOTH = the 3x3 kernel (1,1,1, 1,5,1, 1,1,1) / 13 in float32: coefficients float32(k / 13), the sum starts at 0.5f,
    each row's three products are added left to right and the row's sum is then added; clip8; the one-pixel border is copied, and an image
    with a side below 3 is returned as it is.  bottom_up adds the rows in the other order (the centre row second either way)."""
    H, W, _ = img_u8.shape
    out = img_u8.copy()
    if H < 3 or W < 3:
        return out
    f = np.float32
    k1, k5 = f(1.0 / 13.0), f(5.0 / 13.0)
    x = img_u8.astype(np.float32)
    def row(r, kc):          # r: [H-2, W, 3] rows -> the row's sum at the interior columns
        return (r[:, :-2] * k1 + r[:, 1:-1] * kc) + r[:, 2:] * k1
    top, mid, bot = row(x[:-2], k1), row(x[1:-1], k5), row(x[2:], k1)
    ss = np.full(top.shape, 0.5, dtype=np.float32)
    for r in ((bot, mid, top) if bottom_up else (top, mid, bot)):
        ss = ss + r
    assert ss.dtype == np.float32
    out[1:-1, 1:-1] = _clip8(ss)
    return out


def blend_np(d_u8, v_u8, factor):
    """Image.blend(degenerate, image, factor) as ImageEnhance calls it: float32 d + f * (v - d), clipped, truncated."""
    d, v = d_u8.astype(np.float32), v_u8.astype(np.float32)
    return _clip8(d + np.float32(factor) * (v - d))


def sharpness_np(img_u8, factor, bottom_up=False):
    return blend_np(smooth_np(img_u8, bottom_up), img_u8, factor)


# ---------------------------------------------------------------------------------------------------------------- crafted images
def lut256_image():
    """The 16x32 image whose equalize table holds 256: 511 pixels below 200 and one pixel of 255 -> step 2, lut[255] = 256."""
    rs = np.random.RandomState(256)
    img = rs.randint(0, 200, (16, 32, 3)).astype(np.uint8)
    img[15, 31] = 255
    return img


def erase_np(x, box, value):
    """RandomErasing's write on one [3,H,W] float32 tensor: box = (top, left, h, w)"""
    out = x.copy()
    top, left, h, w = box
    for c in range(3):
        out[c, top:top + h, left:left + w] = np.float32(value[c])
    return out
