"""A numpy restatement of the box crop and its coordinate maps (csrc/box_crop.hip), parameterised by dtype: float64 is the
truth, float32 the yardstick - the same formulas in the device's precision and order, whose distance e32 from the truth is what the
device is allowed a small multiple of (the rule of DESIGN.md 4.9).  numpy rounds every operation separately: no fused multiply-add.

Geometry: pixel i of a frame covers [i, i + 1); box = (cx, cy, bw, bh, rot_deg); sx = bw / Wo, sy = bh / Ho; tx = clamp(ceil(sx), 1, 8);
sample (i, j) of output pixel (u, v): dx = ((u + (i + 0.5) / tx) - Wo / 2) * sx, dy likewise, X = cx + c dx - s dy, Y = cy + s dx + c dy;
x0 = floor(X - 0.5), weight X - 0.5 - x0 on x0 + 1; a tap outside the frame contributes 0; samples added j-major, divided by tx * ty.
The boxes are fp32 values (the device's type) in every dtype."""
import numpy as np

# the six dyadic boxes of the exact cases (cx, cy, bw, bh, rot): sx, sy in {1/2, 1, 2, 4, 8} at 16 x 16 and 32 x 16, centres multiples of 1/8
DYADIC_BOXES = ((20.5, 17.25, 32, 16, 0), (60, 40, 64, 64, 90), (10.125, 8.5, 8, 8, 0), (31.5, 24, 128, 64, 180), (5, 5, 32, 32, 270),
                (33.375, 20.625, 16, 128, 90))


def trig(rot, dtype):
    """(cos, sin) of rot degrees as `dtype`: exact for multiples of 90, else the fp64 value rounded to dtype."""
    rot = float(np.float32(rot))
    r = np.fmod(rot, 360.0)
    if r < 0:
        r += 360.0
    table = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}
    c, s = table[r] if r in table else (np.cos(rot * (np.pi / 180.0)), np.sin(rot * (np.pi / 180.0)))
    return dtype(c), dtype(s)


def taps(scale):
    return int(min(max(np.ceil(np.float32(scale)), 1), 8))


def box_ok(box, fidx, F):
    b = np.asarray(box, dtype=np.float32)
    return bool(np.isfinite(b).all() and b[2] > 0 and b[3] > 0 and 0 <= fidx < F)


def crop_values(frames_u8, frame_idx, boxes, size, dtype=np.float64):
    """-> (values [M,Ho,Wo,3] of `dtype` ahead of rounding / normalisation, status [M] uint8)."""
    Ho, Wo = size
    F, Hs, Ws, _ = frames_u8.shape
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 5)
    M = boxes.shape[0]
    out = np.zeros((M, Ho, Wo, 3), dtype)
    status = np.zeros(M, np.uint8)
    f = dtype
    half = f(0.5)
    for m in range(M):
        if not box_ok(boxes[m], frame_idx[m], F):
            status[m] = 1
            continue
        img = frames_u8[frame_idx[m]].astype(dtype)
        cx, cy, bw, bh = (f(v) for v in boxes[m, :4])
        sx, sy = bw / f(Wo), bh / f(Ho)
        # the tap counts come from the fp32 ratio in every dtype (the device's decision)
        tx, ty = taps(np.float32(boxes[m, 2]) / np.float32(Wo)), taps(np.float32(boxes[m, 3]) / np.float32(Ho))
        c, s = trig(boxes[m, 4], dtype)
        u = np.arange(Wo, dtype=dtype)[None, :]
        v = np.arange(Ho, dtype=dtype)[:, None]
        acc = np.zeros((Ho, Wo, 3), dtype)
        for j in range(ty):
            dy = ((v + (f(j) + half) / f(ty)) - f(Ho) / f(2)) * sy
            for i in range(tx):
                dx = ((u + (f(i) + half) / f(tx)) - f(Wo) / f(2)) * sx
                X = cx + c * dx - s * dy
                Y = cy + s * dx + c * dy
                fx0, fy0 = np.floor(X - half), np.floor(Y - half)
                wx, wy = (X - half - fx0)[..., None], (Y - half - fy0)[..., None]
                x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)

                def tap(xx, yy):
                    inside = (xx >= 0) & (xx < Ws) & (yy >= 0) & (yy < Hs)
                    p = img[np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)]
                    return np.where(inside[..., None], p, f(0))
                one = f(1)
                top = (one - wx) * tap(x0, y0) + wx * tap(x0 + 1, y0)
                bot = (one - wx) * tap(x0, y0 + 1) + wx * tap(x0 + 1, y0 + 1)
                acc = acc + ((one - wy) * top + wy * bot)
        out[m] = acc / f(tx * ty)
        assert out[m].dtype == dtype
    return out, status


def to_u8(values):
    return np.minimum(255, np.floor(values + values.dtype.type(0.5))).astype(np.uint8)


def normalise(values, mean, std):
    """(value / 255 - mean) / std in fp32, torch's order: [M,H,W,3] values -> [M,3,H,W] float32."""
    x = values.astype(np.float32) / np.float32(255)
    x = (x - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def to_tensor(img_u8, mean, std):
    """ToTensor + Normalize of a uint8 image batch."""
    assert img_u8.dtype == np.uint8
    return normalise(img_u8, mean, std)


def to_crop_coords(kp_img, boxes, size, dtype=np.float64):
    """R(rot)^T (kp - (cx, cy)) / (sx, sy) + (Wo / 2, Ho / 2): [M,K,2] pixels of the frame -> pixels of the crop."""
    Ho, Wo = size
    f = dtype
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 5)
    kp = np.asarray(kp_img, dtype=dtype)
    out = np.zeros_like(kp)
    for m in range(boxes.shape[0]):
        cx, cy, bw, bh = (f(v) for v in boxes[m, :4])
        c, s = trig(boxes[m, 4], dtype)
        dx, dy = kp[m, :, 0] - cx, kp[m, :, 1] - cy
        out[m, :, 0] = (c * dx + s * dy) / (bw / f(Wo)) + f(Wo) / f(2)
        out[m, :, 1] = (-s * dx + c * dy) / (bh / f(Ho)) + f(Ho) / f(2)
    return out


def to_image_coords(coords_hm, boxes, input_size, heatmap_size, dtype=np.float64):
    """(cx, cy) + R(rot) (((x, y) * stride - (Wo / 2, Ho / 2)) * (sx, sy)): [M,K,2] heat-map pixels of the crop -> pixels of the frame.  The
    strides are formed in Python floats and rounded to fp32 first, as the device receives them."""
    Ho, Wo = input_size
    Hh, Wh = heatmap_size
    f = dtype
    stx, sty = f(np.float32(Wo / Wh)), f(np.float32(Ho / Hh))
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 5)
    co = np.asarray(coords_hm, dtype=np.float32).astype(dtype)
    out = np.zeros_like(co)
    for m in range(boxes.shape[0]):
        cx, cy, bw, bh = (f(v) for v in boxes[m, :4])
        c, s = trig(boxes[m, 4], dtype)
        dx = (co[m, :, 0] * stx - f(Wo) / f(2)) * (bw / f(Wo))
        dy = (co[m, :, 1] * sty - f(Ho) / f(2)) * (bh / f(Ho))
        out[m, :, 0] = cx + c * dx - s * dy
        out[m, :, 1] = cy + s * dx + c * dy
    return out


def general_boxes(n=64, seed=11):
    """The seeded general boxes of the GPU test for frames of 48 x 64: centres in [-5, 70] x [-5, 55], sides in [6, 90], any angle; at
    16 x 16 and 32 x 16 outputs that is 1 to 6 taps an axis, many boxes partly outside the frame."""
    rs = np.random.RandomState(seed)
    b = np.stack([rs.uniform(-5, 70, n), rs.uniform(-5, 55, n), rs.uniform(6, 90, n), rs.uniform(6, 90, n), rs.uniform(-180, 180, n)], axis=1)
    return b.astype(np.float32)
