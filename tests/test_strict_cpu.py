"""The 'strict' training precision on the host (no GPU): how PoseResNet resolves it, and the executor plan it creates (C ABI mode 3) -
refused where it cannot exist, sized as DESIGN.md 2 describes (the 16-bit arena plus one set of f16x2 scratch slots)."""
import ctypes as C

import pytest


def _small(K=16):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    return pr._pose_resnet("t", K, pr.Bottleneck_default, [1, 1, 1, 1], False, False)


def test_strict_resolves_to_strict_for_differentiable_and_f16x2_for_no_grad_forwards():
    net = _small()
    net.precision = "strict"
    assert net.resolved_precision(True) == "strict"
    assert net.resolved_precision(False) == "f16x2"
    for p in ("bf16", "fp16", "f16x2", "fp32"):          # (every existing value resolves as before)
        net.precision = p
        assert net.resolved_precision(True) == p and net.resolved_precision(False) == p
    net.precision = "auto"
    assert net.resolved_precision(False) == "f16x2"
    net.precision = "strict32"
    with pytest.raises(ValueError):
        net.resolved_precision(True)


def test_strict_plan_modes_and_arena_layout():
    from uda_poseestimation_amd import _hip
    from helpers.strict_layout import strict_layout
    L16, L = _hip.lib("fp16"), _hip.lib("bf16")

    def create(lib, layers, K, N, H, W, mode):
        h = C.c_void_p()
        rc = lib.udapose_net_create((C.c_int * 4)(*layers), K, N, H, W, mode, C.byref(h))
        return rc, h

    r101 = (3, 4, 23, 3)
    rc, h = create(L16, r101, 16, 32, 256, 256, 3)
    assert rc == 0
    rc0, h0 = create(L16, r101, 16, 32, 256, 256, 0)
    assert rc0 == 0
    a3, a0 = L16.udapose_net_act_bytes(h), L16.udapose_net_act_bytes(h0)
    print(f"activation arena at N=32, 256x256: strict {a3 / 2 ** 20:.0f} MB, fp16 {a0 / 2 ** 20:.0f} MB ({a3 / a0:.3f}x)")
    assert a3 < 1.5 * a0
    L16.udapose_net_destroy(h)
    L16.udapose_net_destroy(h0)
    assert create(L16, r101, 16, 32, 256, 256, 3 | 0x200)[0] != 0       # strict is differentiable by definition
    assert create(L, r101, 16, 32, 256, 256, 3)[0] != 0                 # its backward is the fp16 build's
    assert create(L16, r101, 16, 32, 256, 256, 4)[0] != 0
    # the tests' host mirror of the layout (tests/helpers/strict_layout.py) adds up to the plan's arena
    for layers, K, N, H, W in (((1, 1, 1, 1), 16, 4, 128, 128), (r101, 16, 32, 256, 256), ((2, 1, 2, 1), 18, 3, 96, 64)):
        for bias in (0, 0x100):
            rc, h = create(L16, layers, K, N, H, W, 3 | bias)
            assert rc == 0
            assert L16.udapose_net_act_bytes(h) == strict_layout(layers, K, N, H, W)["act_bytes"]
            L16.udapose_net_destroy(h)
