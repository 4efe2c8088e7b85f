"""Box crops and their coordinate maps on the MI355X (csrc/box_crop.hip through data_gpu.box_crop and lib.keypoint_detection.
to_image_coords), against the numpy restatement of tests/helpers/box_crop_ref.py (checked on the CPU by tests/test_box_crop_cpu.py).

Exact cases: on the dyadic boxes (bw / Wo, bh / Ho in {1/2, 1, 2, 4, 8}, centres multiples of 1/8, quarter turns) every fp32 operation of
the kernel is exact, so the device must give the fp64 restatement's bits.  General boxes: e32 = the largest distance of the fp32
restatement from the fp64 one on the same inputs, computed here; the device's values must lie within 4 * e32 of fp64 (DESIGN.md 4.9's
rule: the factor covers fused multiply-adds and another association), and its uint8 output must be floor(fp64 + 0.5) except where fp64
lies within 4 * e32 of a rounding boundary.  Frames are 48 x 64: outputs of 16 x 16 and 32 x 16 take one 32 x 8 tile row partly filled and
several tile rows; the identity crop takes 2 x 6 tiles.  The footprints of these frames always fit the LDS image, so the gather path has
cases of its own: a frame base that is not dword-aligned (the same bits as the staged path) and a footprint larger than the LDS image."""
import numpy as np
import pytest
import torch

from helpers import box_crop_ref as R

pytestmark = pytest.mark.gpu
SIZES = ((16, 16), (32, 16))
IDENTITY = (32.0, 24.0, 64.0, 48.0, 0.0)
ZERO3, ONE3 = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _mods():
    from uda_poseestimation_amd import data_gpu
    from uda_poseestimation_amd.lib import keypoint_detection as kd
    return data_gpu, kd


@pytest.fixture(scope="module")
def frames():
    fr = np.random.RandomState(0).randint(0, 256, (2, 48, 64, 3)).astype(np.uint8)
    return fr, torch.from_numpy(fr).cuda()


@pytest.fixture(scope="module")
def general(frames):
    """The 64 seeded boxes with, per output size, the fp64 values, e32 and the frame indices: computed once."""
    fr, _ = frames
    boxes = R.general_boxes(64)
    fi = (np.arange(64) * 7 % 2).astype(np.int32)
    ref = {}
    for size in SIZES:
        v64, st = R.crop_values(fr, fi, boxes, size, np.float64)
        v32, _ = R.crop_values(fr, fi, boxes, size, np.float32)
        assert not st.any()
        ref[size] = (v64, float(np.abs(v64 - v32.astype(np.float64)).max()))
    return boxes, fi, ref


def _values(dg, fr_d, boxes, size, fi, **kw):
    """The device's values ahead of the normalisation: mean 0, std 1 leave value / 255."""
    x = dg.box_crop(fr_d, boxes, size, frame_idx=fi, mean=ZERO3, std=ONE3, out="f32", **kw)
    return x.cpu().numpy().astype(np.float64).transpose(0, 2, 3, 1) * 255.0


@pytest.mark.parametrize("size", SIZES)
def test_exact_on_dyadic_boxes(frames, size):
    dg, _ = _mods()
    fr, fr_d = frames
    boxes = np.asarray(R.DYADIC_BOXES, np.float32)
    for fi in ([0, 1, 0, 0, 1, 1], [1, 0, 1, 1, 0, 0]):          # two boxes on one frame; the permuted assignment
        want, st = R.crop_values(fr, fi, boxes, size, np.float64)
        assert not st.any()
        want_u8 = R.to_u8(want)
        whole = np.ascontiguousarray((want == np.floor(want)).transpose(0, 3, 1, 2))      # values that are integers (NCHW)
        assert whole.any() and not whole.all()
        u8 = dg.box_crop(fr_d, boxes, size, frame_idx=fi, out="u8", mirror=True)
        x = dg.box_crop(fr_d, boxes, size, frame_idx=np.asarray(fi), mean=MEAN, std=STD, out="f32", mirror=True)
        M = len(fi)
        assert u8.shape == (2 * M, size[0], size[1], 3) and x.shape == (2 * M, 3, size[0], size[1])
        assert np.array_equal(u8[:M].cpu().numpy(), want_u8)
        # the normalised output: the restatement's bits everywhere (the values are exact in fp32), to_tensor(out_u8)'s where they are integers
        xb = x[:M].cpu().numpy().view(np.int32)
        assert np.array_equal(xb, R.normalise(want, MEAN, STD).view(np.int32))
        assert np.array_equal(xb[whole], R.to_tensor(want_u8, MEAN, STD).view(np.int32)[whole])
        # the mirror half is the flip of the plain half, to the bit
        assert torch.equal(u8[M:], torch.flip(u8[:M], [2])) and torch.equal(x[M:].view(torch.int32), torch.flip(x[:M], [3]).view(torch.int32))
        # to_tensor of the device's own uint8 crop: the pipeline's kernel gives the same bits there
        pipe = dg.TargetViewPipeline(image_size=size[0], mean=MEAN, std=STD)
        tb = pipe.to_tensor(u8[:M].contiguous()).cpu().numpy().view(np.int32)
        assert np.array_equal(tb[whole], xb[whole])
    nz = (want_u8 != 0).mean()
    print(f"{size}: {nz:.1%} of the dyadic outputs are non-zero")
    assert nz > 0.5


def test_exact_values_that_are_not_integers(frames):
    """Halving boxes (bw / Wo = 2) average 2 x 2 samples: values with fractions, exact in fp32; uint8 = floor(value + 0.5)."""
    dg, _ = _mods()
    fr, fr_d = frames
    boxes = np.asarray([(20.5, 17.25, 32, 16, 0), (10.125, 8.5, 8, 8, 0)], np.float32)
    want, _ = R.crop_values(fr, [0, 1], boxes, (16, 16), np.float64)
    assert (want != np.floor(want)).any()
    got = _values(dg, fr_d, boxes, (16, 16), [0, 1])
    # value / 255 is rounded once by the kernel: one fp32 rounding of a value below 256
    assert np.abs(got - want).max() <= 256 * 2.0 ** -23
    assert np.array_equal(dg.box_crop(fr_d, boxes, (16, 16), frame_idx=[0, 1], out="u8").cpu().numpy(), R.to_u8(want))


def test_identity_half_turn_quarter_turn(frames):
    dg, _ = _mods()
    fr, fr_d = frames
    u8 = dg.box_crop(fr_d, [IDENTITY, IDENTITY], (48, 64), out="u8")
    assert torch.equal(u8, fr_d)
    u8 = dg.box_crop(fr_d, [IDENTITY[:4] + (180.0,)], (48, 64), frame_idx=[1], out="u8")
    assert torch.equal(u8[0], torch.flip(fr_d[1], [0, 1]))
    u8 = dg.box_crop(fr_d, [(24.0, 24.0, 48.0, 48.0, 90.0)], (48, 48), frame_idx=[0], out="u8")
    assert np.array_equal(u8[0].cpu().numpy(), np.rot90(fr[0][:, :48], 1))
    # a buffer whose size is no multiple of 4: its last, partial dword is read byte by byte
    small = np.random.RandomState(4).randint(0, 256, (1, 5, 7, 3)).astype(np.uint8)
    u8 = dg.box_crop(torch.from_numpy(small).cuda(), [(3.5, 2.5, 7.0, 5.0, 0.0)], (5, 7), out="u8")
    assert np.array_equal(u8.cpu().numpy(), small)


@pytest.mark.parametrize("size", SIZES)
def test_general_boxes_within_4_e32(frames, general, size):
    dg, _ = _mods()
    fr, fr_d = frames
    boxes, fi, ref = general
    v64, e32 = ref[size]
    got = _values(dg, fr_d, boxes, size, fi)
    err = float(np.abs(got - v64).max())
    tx = np.clip(np.ceil(boxes[:, 2] / np.float32(size[1])), 1, 8)
    ty = np.clip(np.ceil(boxes[:, 3] / np.float32(size[0])), 1, 8)
    print(f"{size}: e32 = {e32:.3e} grey levels, device max |difference| from fp64 {err:.3e} (bar {4 * e32:.3e}); taps {int(min(tx.min(), ty.min()))}"
          f" .. {int(max(tx.max(), ty.max()))}")
    assert e32 > 0 and err <= 4 * e32
    want_u8 = R.to_u8(v64)
    nonzero = want_u8 != 0
    assert nonzero.mean() >= 1 / 3, nonzero.mean()
    u8 = dg.box_crop(fr_d, boxes, size, frame_idx=fi, out="u8").cpu().numpy()
    frac = (v64 + 0.5) - np.floor(v64 + 0.5)                      # distance of fp64 + 0.5 above the last integer
    near = (np.minimum(frac, 1 - frac) <= 4 * e32) & (v64 > 0)
    assert np.array_equal(u8[~near], want_u8[~near])
    assert (np.abs(u8[near].astype(np.int64) - want_u8[near]) <= 1).all()
    share = near.sum() / nonzero.sum()
    print(f"{size}: {near.sum()} of {nonzero.sum()} non-zero outputs ({share:.2%}) lie within 4 e32 of a rounding boundary; "
          f"{(u8 != want_u8).sum()} of them round the other way on the device; {nonzero.mean():.1%} of the outputs are non-zero")
    assert share < 0.02
    # many boxes leave the frame: a corner of theirs lies outside it
    c, s = np.cos(np.deg2rad(boxes[:, 4])), np.sin(np.deg2rad(boxes[:, 4]))
    outside = np.zeros(64, bool)
    for ax, ay in ((-0.5, -0.5), (0.5, -0.5), (-0.5, 0.5), (0.5, 0.5)):
        x = boxes[:, 0] + c * ax * boxes[:, 2] - s * ay * boxes[:, 3]
        y = boxes[:, 1] + s * ax * boxes[:, 2] + c * ay * boxes[:, 3]
        outside |= (x < 0) | (x > 64) | (y < 0) | (y > 48)
    assert 16 < outside.sum() < 64


def test_gather_path_gives_the_staged_bits(frames, general):
    """A frames tensor whose base address is not dword-aligned takes every tap from global memory: same samples, same order, same bits."""
    dg, _ = _mods()
    _, fr_d = frames
    boxes, fi, _ = general
    n = fr_d.numel()
    buf = torch.empty(n + 8, dtype=torch.uint8, device="cuda")
    odd = buf[1:1 + n].view(fr_d.shape)
    odd.copy_(fr_d)
    assert odd.data_ptr() % 4 != 0 and odd.is_contiguous()
    for size in SIZES:
        a = dg.box_crop(fr_d, boxes, size, frame_idx=fi, mean=MEAN, std=STD)
        b = dg.box_crop(odd, boxes, size, frame_idx=fi, mean=MEAN, std=STD)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    d = np.asarray(R.DYADIC_BOXES, np.float32)
    assert torch.equal(dg.box_crop(fr_d, d, (16, 16), frame_idx=[0, 1, 0, 0, 1, 1], out="u8"),
                       dg.box_crop(odd, d, (16, 16), frame_idx=[0, 1, 0, 0, 1, 1], out="u8"))


def test_footprint_larger_than_the_lds_image():
    """One 32 x 8 tile at 8 x reduction covers 258 x 66 source pixels, more than the 8192 of the LDS image: those tiles gather; a small box
    on the same frame stages.  Exact on the dyadic boxes, within 4 e32 on the turned one."""
    dg, _ = _mods()
    fr = np.random.RandomState(5).randint(0, 256, (1, 72, 300, 3)).astype(np.uint8)
    fr_d = torch.from_numpy(fr).cuda()
    boxes = np.asarray([(150, 36, 256, 64, 0), (150.5, 36.25, 256, 64, 180), (100, 30, 32, 8, 0), (140, 30, 200, 60, 33)], np.float32)
    fi = [0, 0, 0, 0]
    v64, _ = R.crop_values(fr, fi, boxes, (8, 32), np.float64)
    v32, _ = R.crop_values(fr, fi, boxes, (8, 32), np.float32)
    assert np.array_equal(v64[:3], v32[:3].astype(np.float64))
    e32 = float(np.abs(v64[3] - v32[3]).max())
    got = _values(dg, fr_d, boxes, (8, 32), fi)
    print(f"large footprint: e32 = {e32:.3e}, device max |difference| on the turned box {np.abs(got[3] - v64[3]).max():.3e}")
    assert np.abs(got[:3] - v64[:3]).max() <= 256 * 2.0 ** -23 and np.abs(got[3] - v64[3]).max() <= 4 * e32
    u8 = dg.box_crop(fr_d, boxes[:3], (8, 32), frame_idx=fi[:3], out="u8").cpu().numpy()
    assert np.array_equal(u8, R.to_u8(v64[:3]))


def test_refusals_and_status(frames):
    dg, _ = _mods()
    fr, fr_d = frames
    good = np.asarray(R.DYADIC_BOXES[:5], np.float32)
    clean, st = dg.box_crop(fr_d, torch.from_numpy(good).cuda(), (16, 16), frame_idx=torch.tensor([0, 1, 0, 1, 0], dtype=torch.int32).cuda(),
                            out="u8")
    assert st.tolist() == [0] * 5 and st.dtype == torch.uint8
    bad = good.copy()
    bad[1, 0] = np.nan          # a NaN field
    bad[3, 2] = 0.0             # bw = 0
    fi = torch.tensor([0, 1, 0, 1, 2], dtype=torch.int32).cuda()          # row 4 names frame F
    for out in ("u8", "f32"):
        crops, st = dg.box_crop(fr_d, torch.from_numpy(bad).cuda(), (16, 16), frame_idx=fi, out=out, mean=ZERO3, std=ONE3, mirror=True)
        assert st.tolist() == [0, 1, 0, 1, 1]
        crops = crops.float()
        for m in (1, 3, 4):
            assert not crops[m].any() and not crops[5 + m].any()          # zero pixel values, the mirror image too
        if out == "u8":
            for m in (0, 2):
                assert torch.equal(crops[m], clean[m].float())              # the neighbours are intact
    # a negative index, an infinite centre, a negative side
    bad = good.copy()
    bad[0, 1] = np.inf
    bad[2, 3] = -4.0
    _, st = dg.box_crop(fr_d, torch.from_numpy(bad).cuda(), (16, 16), frame_idx=torch.tensor([0, -1, 0, 1, 0], dtype=torch.int32).cuda())
    assert st.tolist() == [1, 1, 1, 0, 0]
    # host boxes are checked before any launch
    for boxes, fidx, row in ((bad, [0, 1, 0, 1, 0], "box 0"), (good, [0, 1, 0, 1, 2], "box 4"), (good, [0, 1, -1, 1, 0], "box 2")):
        with pytest.raises(ValueError, match=row):
            dg.box_crop(fr_d, boxes, (16, 16), frame_idx=fidx)
    with pytest.raises(ValueError, match="frame_idx"):
        dg.box_crop(fr_d, good, (16, 16))                                  # 5 boxes, 2 frames, no frame_idx


def test_launcher_argument_errors(frames):
    from uda_poseestimation_amd import _hip
    _, fr_d = frames
    lib, p, s = _hip.lib(), _hip.ptr, _hip.stream()
    boxes = torch.tensor([IDENTITY], dtype=torch.float32).cuda()
    fi = torch.zeros(1, dtype=torch.int32).cuda()
    ms = torch.ones(3).cuda()
    of, ou, st = torch.empty(2, 3, 8, 8).cuda(), torch.empty(2, 8, 8, 3, dtype=torch.uint8).cuda(), torch.empty(1, dtype=torch.uint8).cuda()

    def call(frames=fr_d, F=2, Hs=48, Ws=64, fi=fi, boxes=boxes, M=1, Ho=8, Wo=8, mean=ms, std=ms, mirror=0, of=of, ou=ou, st=st):
        return lib.udapose_box_crop(s, p(frames), F, Hs, Ws, p(fi), p(boxes), M, Ho, Wo, p(mean), p(std), mirror, p(of), p(ou), p(st))
    assert call() == 0 and call(of=None) == 0 and call(ou=None) == 0 and call(mirror=1) == 0 and call(of=None, mean=None, std=None) == 0
    for kw in (dict(frames=None), dict(fi=None), dict(boxes=None), dict(st=None), dict(of=None, ou=None), dict(mean=None), dict(std=None),
               dict(M=0), dict(M=-1), dict(Ho=0), dict(Wo=0), dict(Ho=1025), dict(Wo=1025), dict(Hs=0), dict(Ws=0), dict(Hs=8193), dict(Ws=8193),
               dict(F=0), dict(mirror=2)):
        assert call(**kw) == -1, kw
    co, out = torch.zeros(1, 4, 2).cuda(), torch.empty(1, 4, 2).cuda()

    def back(co=co, boxes=boxes, M=1, K=4, Ho=8, Wo=8, out=out):
        return lib.udapose_coords_to_image(s, p(co), p(boxes), M, K, 4.0, 4.0, Ho, Wo, p(out))
    assert back() == 0
    for kw in (dict(co=None), dict(boxes=None), dict(out=None), dict(M=0), dict(K=0), dict(Ho=0), dict(Wo=0)):
        assert back(**kw) == -1, kw
    torch.cuda.synchronize()


def test_to_image_coords(frames):
    _, kd = _mods()
    rs = np.random.RandomState(6)
    # exact on the dyadic boxes: heat-map coordinates that are multiples of 1/4, stride 4
    boxes = np.asarray(R.DYADIC_BOXES, np.float32)
    for size, hm in (((16, 16), (4, 4)), ((32, 16), (8, 4))):
        co = (rs.randint(-8, 40, (6, 5, 2)) / 4.0).astype(np.float32)
        want = R.to_image_coords(co, boxes, size, hm, np.float64)
        assert np.array_equal(R.to_image_coords(co, boxes, size, hm, np.float32).astype(np.float64), want)
        got = kd.to_image_coords(co, boxes, size, hm)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
        got_t = kd.to_image_coords(torch.from_numpy(co).cuda(), torch.from_numpy(boxes).cuda(), size, hm)
        assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), got)
        # the inverse of to_crop_coords / stride (exact here: every step is)
        stride = (size[1] / hm[1], size[0] / hm[0])
        assert np.array_equal(kd.to_crop_coords(want, boxes, size) / stride, co.astype(np.float64))
    # general boxes: within 4 e32 of fp64, and the inverse of the forward map
    boxes = R.general_boxes(64)
    for size, hm in (((16, 16), (4, 4)), ((32, 16), (8, 4)), ((256, 192), (64, 48))):
        kp = rs.uniform(-10, 80, (64, 9, 2))
        stride = (size[1] / hm[1], size[0] / hm[0])
        co = (kd.to_crop_coords(kp, boxes, size) / stride).astype(np.float32)
        want = R.to_image_coords(co, boxes, size, hm, np.float64)
        e32 = float(np.abs(R.to_image_coords(co, boxes, size, hm, np.float32).astype(np.float64) - want).max())
        got = kd.to_image_coords(co, boxes, size, hm).astype(np.float64)
        err = float(np.abs(got - want).max())
        # back to the key points: fp64's own distance from them is the fp32 rounding of the heat-map coordinates, which the test made
        back = float(np.abs(want - kp).max())
        print(f"to_image_coords {size}: e32 = {e32:.3e} px, device max |difference| from fp64 {err:.3e}, fp64 round trip {back:.3e}")
        assert e32 > 0 and err <= 4 * e32
        assert np.abs(got - kp).max() <= back + 4 * e32
