"""Top-down inference geometry on the CPU: the host box helpers against the reference's own functions (tests/golden/
boxes.npz), the forward map against the recorded get_transform matrices, and the properties of the numpy restatement
(tests/helpers/box_crop_ref.py) that the GPU tests hold the kernel to."""
import os

import numpy as np
import pytest
import torch

from helpers import box_crop_ref as R
from uda_poseestimation_amd import data_gpu
from uda_poseestimation_amd.lib import keypoint_detection as kd


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "boxes.npz"))


def test_human_boxes_match_scale_box(golden):
    kp, wh = golden["kp"], golden["image_wh"]
    assert kp.shape[0] >= 40
    for n in range(kp.shape[0]):
        w, h = int(wh[n, 0]), int(wh[n, 1])
        np.testing.assert_array_equal(golden["bbox"][n], [kp[n, :, 0].min(), kp[n, :, 1].min(), kp[n, :, 0].max(), kp[n, :, 1].max()])
        b = kd.boxes_from_keypoints(kp[n], None, (h, w), style="human")[0]
        left, upper, right, lower = golden["scaled"][n]
        side = right - left + 1
        assert lower - upper + 1 == side
        # pixels left .. right inclusive are [left, right + 1) on the continuous axis
        assert tuple(b) == (left + side / 2, upper + side / 2, side, side, 0.0), (n, b, golden["scaled"][n])
        # crop + resize move key points by (kp - left) * S / w
        got = kd.to_crop_coords(kp[n][None], b[None], 256)[0]
        np.testing.assert_allclose(got, (kp[n] - (left, upper)) * 256 / side, rtol=0, atol=1e-10)
    # visible joints only
    vis = np.ones(kp.shape[1]); vis[0] = 0
    b = kd.boxes_from_keypoints(kp[3], vis[None], (int(wh[3, 1]), int(wh[3, 0])))[0]
    assert b[2] <= kd.boxes_from_keypoints(kp[3], None, (int(wh[3, 1]), int(wh[3, 0])))[0][2]


def test_to_crop_coords_is_get_transform(golden):
    kp = golden["kp"]
    worst = 0.0
    for n in range(kp.shape[0]):
        box = kd.boxes_from_center_scale(golden["center"][n], golden["scale"][n], golden["rot"][n])
        assert box.shape == (1, 5) and box[0, 2] == box[0, 3] == 200 * golden["scale"][n]
        res = (int(golden["res"][n, 0]), int(golden["res"][n, 1]))
        got = kd.to_crop_coords(kp[n][None], box, res)[0]
        want = (golden["matrix"][n] @ np.concatenate([kp[n], np.ones((kp.shape[1], 1))], axis=1).T).T[:, :2]
        worst = max(worst, np.abs(got - want).max())
    print(f"to_crop_coords against get_transform: max |difference| {worst:.2e} px")
    assert worst <= 1e-12
    assert set(golden["rot"].tolist()) == {0.0, 30.0, -45.0, 90.0}


def test_animal_boxes_follow_the_clip_and_scale():
    rs = np.random.RandomState(2)
    H, W = 225, 400
    kp = rs.uniform(1, 1, (3, 18, 2)) * 0
    kp[0] = rs.uniform((5, 5), (395, 220), (18, 2))           # widened past every edge: clipped
    kp[1] = rs.uniform((150, 80), (250, 140), (18, 2))        # inside
    kp[2] = kp[1]; kp[2, :4] = 0                               # absent joints (0, 0) do not count
    b = kd.boxes_from_keypoints(kp, None, (H, W), style="animal")
    for m in range(3):
        xs, ys = kp[m, kp[m, :, 0] > 0, 0], kp[m, kp[m, :, 1] > 0, 1]
        x0, x1 = max(xs.min() - 15, 0.0), min(xs.max() + 15, float(W))
        y0, y1 = max(ys.min() - 15, 0.0), min(ys.max() + 15, float(H))
        s = max(x1 - x0, y1 - y0) / 200.0 * 1.25
        np.testing.assert_array_equal(b[m], kd.boxes_from_center_scale(((x0 + x1) / 2, (y0 + y1) / 2), s)[0])
    assert b[0, 2] > min(H, W)                                 # such a box leaves the frame
    np.testing.assert_array_equal(b[2], kd.boxes_from_keypoints(kp[1, 4:][None], None, (H, W), style="animal")[0])
    with pytest.raises(ValueError, match="no joint"):
        kd.boxes_from_keypoints(np.zeros((1, 4, 2)), None, (H, W), style="animal")
    with pytest.raises(ValueError, match="style"):
        kd.boxes_from_keypoints(kp, None, (H, W), style="hand")


def test_restatement_round_trip():
    boxes = np.concatenate([np.asarray(R.DYADIC_BOXES, np.float32), R.general_boxes(16)])
    rs = np.random.RandomState(3)
    kp = rs.uniform(-10, 80, (boxes.shape[0], 7, 2))
    for size, hm in (((16, 16), (4, 4)), ((32, 16), (8, 4))):
        crop = R.to_crop_coords(kp, boxes, size)
        stride = (size[1] / hm[1], size[0] / hm[0])
        back = R.to_image_coords((crop / stride).astype(np.float64), boxes, size, hm)
        # (to_image_coords takes fp32 heat-map coordinates, the decodes' type: the round trip is good to fp32's rounding of them)
        scale = np.maximum(boxes[:, 2] / size[1], boxes[:, 3] / size[0])[:, None, None]
        assert (np.abs(back - kp) <= 2.0 ** -23 * 4 * (np.abs(crop).max() + 1) * scale + 1e-9).all()
        # the product's host map is the restatement's
        np.testing.assert_allclose(kd.to_crop_coords(kp, boxes, size), crop, rtol=0, atol=1e-10)


def test_restatement_identity_and_quarter_turns():
    rs = np.random.RandomState(0)
    fr = rs.randint(0, 256, (2, 48, 64, 3)).astype(np.uint8)
    for dt in (np.float64, np.float32):
        v, st = R.crop_values(fr, [1], [(32, 24, 64, 48, 0)], (48, 64), dt)
        assert st[0] == 0 and np.array_equal(v[0], fr[1])
        v, _ = R.crop_values(fr, [0], [(32, 24, 64, 48, 180)], (48, 64), dt)
        assert np.array_equal(v[0], fr[0][::-1, ::-1])
        v, _ = R.crop_values(fr, [0], [(24, 24, 48, 48, 90)], (48, 48), dt)
        assert np.array_equal(v[0], np.rot90(fr[0][:, :48], 1))
        v, _ = R.crop_values(fr, [0], [(24, 24, 48, 48, -270)], (48, 48), dt)
        assert np.array_equal(v[0], np.rot90(fr[0][:, :48], 1))
    # exact in fp32 on the dyadic boxes
    for size in ((16, 16), (32, 16)):
        fi = [m % 2 for m in range(len(R.DYADIC_BOXES))]
        v64, _ = R.crop_values(fr, fi, R.DYADIC_BOXES, size, np.float64)
        v32, _ = R.crop_values(fr, fi, R.DYADIC_BOXES, size, np.float32)
        assert np.array_equal(v64, v32.astype(np.float64))
    # refusals
    _, st = R.crop_values(fr, [0, 0, 2, 1], [(np.nan, 1, 2, 2, 0), (1, 1, 0, 2, 0), (8, 8, 4, 4, 0), (8, 8, 4, 4, 0)], (4, 4))
    assert st.tolist() == [1, 1, 1, 0]


def test_python_layer_argument_errors():
    good = [(8.0, 8.0, 4.0, 4.0, 0.0), (9.0, 8.0, 4.0, 6.0, 30.0)]
    assert kd.check_boxes(good).shape == (2, 5)
    for bad, row in (([good[0], (np.nan, 1, 2, 2, 0)], "box 1"), ([(1, 1, 0, 2, 0)], "box 0"), ([good[0], good[1], (1, 1, 2, -1, 0)], "box 2"),
                     ([(1, 1, np.inf, 2, 0)], "box 0"), ([(1, 1, 1e39, 2, 0)], "box 0")):
        with pytest.raises(ValueError, match=row):
            kd.check_boxes(bad)
    with pytest.raises(ValueError, match="M,5"):
        kd.check_boxes(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="M,K,2"):
        kd.to_crop_coords(np.zeros((3, 4, 2)), good, 16)
    with pytest.raises(ValueError, match="size"):
        kd.to_crop_coords(np.zeros((2, 4, 2)), good, (0, 16))
    with pytest.raises(ValueError, match="M,K,2"):
        kd.to_image_coords(np.zeros((2, 4)), good, 16, 4)
    with pytest.raises(ValueError, match="box 1"):
        kd.to_image_coords(np.zeros((2, 4, 2), np.float32), [good[0], (1, 1, 0, 1, 0)], 16, 4)
    # the crop refuses CPU frames (there is no CPU path), and a bad output kind before anything else
    with pytest.raises(RuntimeError, match="MI355X"):
        data_gpu.box_crop(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), good, 16)
    with pytest.raises(ValueError, match="out must be"):
        data_gpu.box_crop(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), good, 16, out="f16")
    with pytest.raises(ValueError, match="1024"):
        data_gpu.box_crop(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), good, 2048)
    from uda_poseestimation_amd import engine
    with pytest.raises(ValueError, match="batch"):
        engine.predict(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), good, None, batch=0)
