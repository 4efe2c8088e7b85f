"""engine.predict on the MI355X: pictures and boxes in, key points in the pictures' pixels out.

Geometry, with a stub network whose heat-maps are the device's own label maps drawn at lib.keypoint_detection.to_crop_coords(known key
points): the arg-max of quantised labels is within half a heat-map pixel per axis of the position, which the way back scales by
stride * max(sx, sy): the bound is 0.5 * stride * max(sx, sy) * sqrt(2); sub-pixel labels under the DARK decode are within the 0.01
heat-map pixels that tests/test_gpu_dark.py holds for that pairing (64 x 64 maps, sigma 2, centres 4 px inside), scaled the same way.
Composition, with PoseResNet-50: predict is, to the bit, the crop, the evaluation forward, the decode and the way back done by hand per
chunk; with flip_pairs it is flip_forward on the hand-made crops; the result does not depend on the chunk size; a captured call follows new
box values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
K = 16


def _mods():
    from uda_poseestimation_amd import data_gpu, engine
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    return data_gpu, engine, kd


class LabelStub(torch.nn.Module):
    """Ignores the pixels: a call returns the label maps of the boxes of the chunk predict() is at (the last chunk padded with repeats of
    its first row, as predict pads), followed, for a flip-test batch of twice the size, by what a network would give for the mirrored crops:
    columns reversed, left / right channels swapped."""

    def __init__(self, labels, batch, perm=None):
        super().__init__()
        self.num_keypoints = labels.shape[1]
        self.labels, self.batch, self.perm, self.at, self.calls = labels, batch, perm, 0, 0

    def forward(self, x):
        M = self.labels.shape[0]
        n = min(self.batch, M - self.at)
        rows = list(range(self.at, self.at + n)) + [self.at] * (self.batch - n)
        self.at = (self.at + n) % M
        self.calls += 1
        y = self.labels[rows]
        if x.shape[0] == 2 * self.batch:
            return torch.cat([y, torch.flip(y[:, self.perm], [3])]).contiguous()
        assert x.shape[0] == self.batch
        return y.contiguous()


def _stub_case():
    """Frames 96 x 128, five boxes - turned, non-square, two of them leaving the frame - and key points whose crop positions lie 4 heat-map
    pixels inside the 64 x 64 map."""
    dg, engine, kd = _mods()
    boxes = np.asarray([(64, 48, 100, 100, 0), (20, 30, 90, 120, 30), (110, 80, 140, 80, -45), (64, 40, 60, 60, 90), (5, 90, 110, 70, 200)],
                       np.float64)
    fi = np.asarray([0, 1, 1, 0, 0])
    rs = np.random.RandomState(8)
    centres = 4 + rs.rand(5, K, 2) * (63 - 8)                    # heat-map pixels of the crop
    # their image positions, by the forward map's inverse in fp64
    c, s = kd.box_rotation(boxes[:, 4])
    d = (centres * 4.0 - 128.0) * (boxes[:, None, 2:4] / 256.0)
    kp = np.stack([boxes[:, None, 0] + c[:, None] * d[..., 0] - s[:, None] * d[..., 1],
                   boxes[:, None, 1] + s[:, None] * d[..., 0] + c[:, None] * d[..., 1]], axis=-1)
    crop = kd.to_crop_coords(kp, boxes, 256)
    assert np.abs(crop / 4.0 - centres).max() < 1e-9
    frames = torch.from_numpy(rs.randint(0, 256, (2, 96, 128, 3)).astype(np.uint8)).cuda()
    return boxes, fi, kp, crop, frames


@pytest.mark.parametrize("flip", [False, True])
def test_stub_model_geometry(flip):
    dg, engine, kd = _mods()
    boxes, fi, kp, crop, frames = _stub_case()
    scale = np.maximum(boxes[:, 2], boxes[:, 3]) / 256.0           # max(sx, sy)
    perm = kd.flip_perm("body16", K).cuda().long()
    vis = np.ones((5, K, 1), np.float32)
    for decode, subpixel, hm_bound in (("argmax", False, 0.5 * np.sqrt(2.0)), ("dark", True, 0.01)):
        labels, _ = dg.TargetViewPipeline(image_size=256, heatmap_size=64, sigma=2, subpixel_labels=subpixel).labels(crop, vis, "cuda")
        stub = LabelStub(labels, 2, perm)
        out = engine.predict(frames, boxes, stub, frame_idx=fi, flip_pairs="body16" if flip else None, decode=decode, batch=2, input_size=256,
                             return_heatmaps=True)
        assert stub.calls == 3 and stub.at == 0
        assert out["keypoints"].shape == (5, K, 2) and out["confidence"].shape == (5, K) and out["status"].tolist() == [0] * 5
        assert out["keypoints"].is_cuda and out["confidence"].is_cuda and out["status"].is_cuda
        assert torch.equal(out["heatmaps"], labels)                                # (the flip merge of a map with itself is the map)
        assert torch.equal(out["confidence"], labels.amax((2, 3)))
        err = np.linalg.norm(out["keypoints"].cpu().numpy().astype(np.float64) - kp, axis=-1)
        bound = hm_bound * 4.0 * scale
        print(f"stub, flip={flip}, {decode}: max error per box {np.round(err.max(1), 4).tolist()} px, bounds {np.round(bound, 4).tolist()}")
        assert (err <= bound[:, None]).all()


@pytest.fixture(scope="module")
def r50_case():
    import uda_poseestimation_amd.lib.models as models
    torch.manual_seed(0)
    model = models.pose_resnet50(K, pretrained_backbone=False).cuda()
    rs = np.random.RandomState(9)
    frames = torch.from_numpy(rs.randint(0, 256, (2, 96, 128, 3)).astype(np.uint8)).cuda()
    boxes = np.asarray([(64, 48, 96, 96, 0), (30, 30, 80, 100, 20), (100, 70, 120, 90, -60), (64, 40, 64, 64, 90), (10, 85, 90, 70, 170)], np.float32)
    fi = np.asarray([0, 1, 1, 0, 1], np.int32)
    return model, frames, boxes, fi


def _by_hand(model, frames, boxes, fi, batch, flip_pairs=None):
    dg, engine, kd = _mods()
    bd, fd = torch.from_numpy(boxes).cuda(), torch.from_numpy(fi).cuda()
    kps, conf = [], []
    model.eval()
    for i0 in range(0, len(boxes), batch):
        n = min(batch, len(boxes) - i0)
        rows = list(range(i0, i0 + n)) + [i0] * (batch - n)
        b, f = bd[rows].contiguous(), fd[rows].contiguous()
        x, st = dg.box_crop(frames, b, 64, frame_idx=f)
        assert not st.any()
        with torch.no_grad():
            y = engine.flip_forward(model, x, flip_pairs) if flip_pairs else model(x)
        preds, maxv = kd.get_max_preds(y)
        kps.append(kd.to_image_coords(preds, b, 64, tuple(y.shape[2:]))[:n])
        conf.append(maxv[:n, :, 0])
    return torch.cat(kps), torch.cat(conf)


def test_predict_is_its_pieces(r50_case):
    dg, engine, kd = _mods()
    model, frames, boxes, fi = r50_case
    for flip_pairs in (None, "body16"):
        want_kp, want_conf = _by_hand(model, frames, boxes, fi, 2, flip_pairs)
        model.train()
        out = engine.predict(frames, boxes, model, frame_idx=fi, flip_pairs=flip_pairs, batch=2, input_size=64)
        assert model.training                                       # the mode is restored
        model.eval()
        assert torch.equal(out["keypoints"], want_kp) and torch.equal(out["confidence"], want_conf)
        assert out["status"].tolist() == [0] * 5
        assert bool(torch.isfinite(out["keypoints"]).all()) and out["keypoints"].unique(dim=0).shape[0] > 1
        for batch in (1, 5):                                        # the result does not depend on the chunk size
            other = engine.predict(frames, boxes, model, frame_idx=fi, flip_pairs=flip_pairs, batch=batch, input_size=64)
            assert not model.training
            assert torch.equal(other["keypoints"], out["keypoints"]) and torch.equal(other["confidence"], out["confidence"])
    # device boxes: a refused box is reported, its neighbours are what they were
    bad = torch.from_numpy(boxes).cuda()
    bad[2, 2] = float("nan")
    res = engine.predict(frames, bad, model, frame_idx=torch.from_numpy(fi).cuda(), batch=2, input_size=64)
    assert res["status"].tolist() == [0, 0, 1, 0, 0]
    keep = [0, 1, 3, 4]
    assert torch.equal(res["keypoints"][keep], engine.predict(frames, boxes, model, frame_idx=fi, batch=2, input_size=64)["keypoints"][keep])
    with pytest.raises(ValueError, match="box 2"):
        engine.predict(frames, bad.cpu().numpy(), model, frame_idx=fi, batch=2, input_size=64)


def test_captured_predict_follows_new_boxes(r50_case):
    """Nothing is read back or uploaded with device boxes: the call can be captured, and a replay follows new values in the boxes tensor."""
    dg, engine, kd = _mods()
    model, frames, boxes, fi = r50_case
    model.eval()
    moved = boxes.copy()
    moved[:, 0] += 7.5
    moved[:, 4] += 11.0
    fd = torch.from_numpy(fi).cuda()
    eager = [engine.predict(frames, torch.from_numpy(b).cuda(), model, frame_idx=fd, batch=2, input_size=64) for b in (boxes, moved)]
    assert not torch.equal(eager[0]["keypoints"], eager[1]["keypoints"])
    static = torch.from_numpy(boxes).cuda()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = engine.predict(frames, static, model, frame_idx=fd, batch=2, input_size=64)
    for want, src in ((eager[1], moved), (eager[0], boxes)):
        static.copy_(torch.from_numpy(src))
        out["keypoints"].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["keypoints"], want["keypoints"]) and torch.equal(out["confidence"], want["confidence"])
