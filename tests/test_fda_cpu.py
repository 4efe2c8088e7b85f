"""Fourier-domain style transfer without a GPU: the low-rank formulation the kernels compute against the textbook FFT pipeline in float64,
its raw-space DC variant, its exactness properties, the window sizes, the ABI's three prototypes and the module's refusals."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import fda_fp64 as ff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (shape, b): the shapes of tests/test_gpu_fda.py
CASES = [((2, 3, 16, 16), 1), ((1, 3, 16, 16), 0), ((1, 3, 16, 16), 7), ((1, 3, 12, 20), 1), ((1, 1, 15, 17), 2), ((1, 3, 64, 64), 5),
         ((1, 3, 256, 256), 23), ((1, 3, 384, 384), 34)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.mark.parametrize("shape,b", CASES)
def test_low_rank_form_is_the_fft_pipeline(shape, b):
    seed = ff.pick_seed(shape, b)
    c, s = ff.inputs(shape, seed)
    assert ff.condition(c, b) >= ff.MIN_CONDITION and ff.condition(s, b) >= ff.MIN_CONDITION
    for alpha in (1.0, 0.37):
        d = float(np.abs(ff.low_rank(c, s, b, alpha) - ff.fft_form(c, s, b, alpha)).max())
        print(f"{shape} b={b} alpha={alpha} seed={seed}: low-rank vs FFT {d:.2e}; condition {ff.condition(c, b):.1e}")
        assert d <= 1e-12
    # the spectrum is the FFT's window
    f = np.fft.fft2(c.astype(np.float64), axes=(-2, -1))
    H, W = shape[-2:]
    g = ff.spectrum(c, b)
    for u in range(-b, b + 1):
        assert np.abs(g[:, :, u + b, :] - f[:, :, u % H, :b + 1]).max() <= 1e-12 * np.abs(c).sum()


def test_raw_space_variant_is_fda_of_the_denormalised_images():
    shape, b = (2, 3, 16, 16), 1
    rng = np.random.RandomState(3)
    # normalised images whose raw means straddle the dataset mean: the DC coefficients differ in sign
    c = ((0.30 + 0.1 * rng.standard_normal(shape)) - np.reshape(MEAN, (1, 3, 1, 1))) / np.reshape(STD, (1, 3, 1, 1))
    s = ((0.65 + 0.1 * rng.standard_normal(shape)) - np.reshape(MEAN, (1, 3, 1, 1))) / np.reshape(STD, (1, 3, 1, 1))
    for alpha in (1.0, 0.37):
        got = ff.low_rank(c, s, b, alpha, MEAN, STD)
        assert np.abs(got - ff.raw_reference(c, s, b, alpha, MEAN, STD)).max() <= 1e-12
        assert np.abs(got - ff.low_rank(c, s, b, alpha)).max() > 0.1          # plain FDA on the normalised tensors is another function


def test_alpha_zero_is_the_identity_and_b_zero_moves_only_the_mean():
    shape = (1, 3, 16, 16)
    c, s = ff.inputs(shape, 0)
    assert np.array_equal(ff.low_rank(c, s, 3, 0.0), c.astype(np.float64))
    assert np.array_equal(ff.low_rank(c, c, 3, 1.0), c.astype(np.float64))
    d = ff.low_rank(c, s, 0, 1.0) - c
    assert np.abs(d - d.mean(axis=(2, 3), keepdims=True)).max() <= 1e-14 and np.abs(d).min() > 1e-3
    # all-zero content: the phase is 1, the output is the style's amplitudes as cosines
    z = np.zeros(shape, dtype=np.float32)
    assert np.abs(ff.low_rank(z, s, 2, 1.0) - ff.fft_form(z, s, 2, 1.0)).max() <= 1e-12
    assert np.abs(ff.transfer_bar(z, s, 2, 1.0)).max() < 1e-3


def test_window_values():
    from uda_poseestimation_amd.lib.models import fda
    for H, W, beta, b in ((256, 256, 0.01, 2), (256, 256, 0.09, 23), (384, 384, 0.09, 34), (12, 20, 0.09, 1), (512, 512, 0.09, 46)):
        assert fda.window(H, W, beta) == b == ff.window(H, W, beta)
    assert fda.MAX_B >= 46


def test_prototypes_exist_in_the_header_and_in_sigs():
    from uda_poseestimation_amd import _hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "udapose.h")).read(), flags=re.S)
    for name, ret in (("udapose_fda_ws_bytes", "long long"), ("udapose_fda_spectrum", "int"), ("udapose_fda_apply", "int")):
        assert re.search(r"^" + ret + r"\s+" + name + r"\s*\(", hdr, flags=re.M), name
        assert name in _hip._SIGS
    assert _hip._SIGS["udapose_fda_ws_bytes"][0] is _hip.ll
    from uda_poseestimation_amd.lib.models import fda
    full = open(os.path.join(ROOT, "include", "udapose.h")).read()
    assert int(re.search(r"#define\s+UDAPOSE_FDA_MAX_B\s+(\d+)", full).group(1)) == fda.MAX_B
    assert int(re.search(r"#define\s+UDAPOSE_FDA_MAX_DIM\s+(\d+)", full).group(1)) == fda.MAX_DIM
    mk = open(os.path.join(ROOT, "uda_poseestimation_amd", "csrc", "Makefile")).read()
    assert "fda.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()


def test_host_size_query_and_refusals_need_no_gpu():
    from uda_poseestimation_amd import _hip
    from uda_poseestimation_amd.lib.models import fda
    lib = _hip.lib()
    assert lib.udapose_fda_ws_bytes(96, 256, 256, 23) == 96 * 8 * 47 * 24 * 8
    assert lib.udapose_fda_ws_bytes(1, 16, 16, 7) == 15 * 8 * 8
    for planes, H, W, b in ((1, 16, 16, 8), (1, 16, 16, -1), (0, 16, 16, 1), (1, 0, 16, 0), (1, 16, 0, 0), (1, 256, 256, fda.MAX_B + 1),
                            (1, fda.MAX_DIM + 1, 256, 2)):
        assert lib.udapose_fda_ws_bytes(planes, H, W, b) in (-1, -3), (planes, H, W, b)
    # refused before anything touches the device (null stream and pointers are never read)
    assert lib.udapose_fda_spectrum(None, None, 1, 16, 16, 8, None, None) in (-1, -3)
    assert lib.udapose_fda_apply(None, None, None, None, None, 1, 1, 16, 16, fda.MAX_B + 1, 1.0, None, None, None, None, None) in (-1, -3)


def test_cpu_tensors_are_refused():
    from uda_poseestimation_amd.lib.models import fda
    x = torch.zeros(1, 3, 16, 16)
    net = fda.FDANet(0.1)
    assert list(net.parameters()) == [] and list(net.buffers()) == [] and not hasattr(net, "precision")
    for call in (lambda: fda.fda_transfer(x, x, 0.1), lambda: fda.low_freq_spectrum(x, 1), lambda: net(x, x), lambda: net.spectrum(x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="go together"):
        fda.FDANet(0.1, mean=MEAN)


def test_drop_in_import():
    import subprocess
    import sys
    code = f'''
import sys
sys.path.insert(0, {os.path.join(ROOT, "uda_poseestimation_amd")!r})
import _dropin; _dropin.alias()
from lib.models import fda
from lib.models.fda import FDANet, fda_transfer, low_freq_spectrum, window
import uda_poseestimation_amd.lib.models.fda as real
assert fda is real and FDANet is real.FDANet and window(256, 256, 0.09) == 23
print("DROPIN-OK")
'''
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DROPIN-OK" in r.stdout, r.stdout + r.stderr
