"""udapose_net_ws_bytes where a device exists: the workspace INCLUDING the partial tiles of the split weight-gradient reductions, which a dry walk
of the grouped table's builder (net.hip build_wg_group, sizing mode) adds up layer by layer under the plan's policy of that moment - head, stem,
deconvolutions 2..0, blocks from last to first as c3, c2, cd, c1.  The walk needs the layers' tap plans, which live in device memory: without a
device it gives up and the answer is the workspace without partial tiles (what tests/test_plan_layout_cpu.py pins).  A layer dropped from the
walk, or sized under another policy, changes these figures.

The policies: the default (deterministic splits, 128-stage split length), wgrad_det = 0 (atomics: no partial tiles), and split lengths of 64, 8
and 2 stages, at which more and more layers of these small plans are split; wgrad_group_stem = 0 takes the stem out of the walk.

The table was recorded on an MI355X from the build of the commit BEFORE net.hip's layer walks were unified (its parent).  To regenerate it
after a deliberate change, on a machine with the GPU:

    python tests/test_gpu_plan_workspace.py --record [--tree ROOT]      # ROOT: another tree whose built libraries answer (default: this one)

rewrites the lines between the two RECORDED markers of this file.  The ORDER of the table entries does not show in a size; it is pinned by the
bit comparisons of tests/test_gpu_wgrad_pair.py and tests/test_gpu_tail_order.py (pair launch against per-pass launches, work orders) and read
back from the stamps in tests/test_gpu_wgrad_strided_loader.py."""
import ctypes as C
import itertools
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYERS = ((1, 1, 1, 1), (2, 1, 2, 1), (3, 4, 23, 3))
SHAPES = ((16, 2, 64, 64), (21, 1, 96, 64), (17, 4, 128, 128))          # (K, N, H, W)
MODES = {"bf16": (0, 0x100), "fp16": (0, 0x100, 3)}
POLICIES = ({}, {"wgrad_det": 0}, {"wgrad_stages": 64}, {"wgrad_stages": 8}, {"wgrad_stages": 2}, {"wgrad_stages": 8, "wgrad_group_stem": 0})
CASES = [(k, l, s, m) for k in MODES for l, s in itertools.product(LAYERS, SHAPES) for m in MODES[k]]

# fmt: off
# ---- RECORDED (python tests/test_gpu_plan_workspace.py --record) ----
TABLE = {
    ('bf16', (1, 1, 1, 1), (16, 2, 64, 64), 0): (39043072, 38928384, 39043072, 39387136, 42532864, 38928384),
    ('bf16', (1, 1, 1, 1), (16, 2, 64, 64), 256): (39043072, 38928384, 39043072, 39387136, 42532864, 38928384),
    ('bf16', (1, 1, 1, 1), (21, 1, 96, 64), 0): (37738496, 37623808, 37738496, 37967872, 40342528, 37623808),
    ('bf16', (1, 1, 1, 1), (21, 1, 96, 64), 256): (37738496, 37623808, 37738496, 37967872, 40342528, 37623808),
    ('bf16', (1, 1, 1, 1), (17, 4, 128, 128), 0): (75685888, 75456512, 75915264, 94863360, 176676864, 91193344),
    ('bf16', (1, 1, 1, 1), (17, 4, 128, 128), 256): (75685888, 75456512, 75915264, 94863360, 176676864, 91193344),
    ('bf16', (2, 1, 2, 1), (16, 2, 64, 64), 0): (39534592, 39419904, 39534592, 39878656, 44138496, 39419904),
    ('bf16', (2, 1, 2, 1), (16, 2, 64, 64), 256): (39534592, 39419904, 39534592, 39878656, 44138496, 39419904),
    ('bf16', (2, 1, 2, 1), (21, 1, 96, 64), 0): (38107136, 37992448, 38107136, 38336512, 41546752, 37992448),
    ('bf16', (2, 1, 2, 1), (21, 1, 96, 64), 256): (38107136, 37992448, 38107136, 38336512, 41546752, 37992448),
    ('bf16', (2, 1, 2, 1), (17, 4, 128, 128), 0): (79618048, 79388672, 79847424, 101023744, 198434816, 97353728),
    ('bf16', (2, 1, 2, 1), (17, 4, 128, 128), 256): (79618048, 79388672, 79847424, 101023744, 198434816, 97353728),
    ('bf16', (3, 4, 23, 3), (16, 2, 64, 64), 0): (42680320, 42565632, 42680320, 43024384, 48398336, 42565632),
    ('bf16', (3, 4, 23, 3), (16, 2, 64, 64), 256): (42680320, 42565632, 42680320, 43024384, 48398336, 42565632),
    ('bf16', (3, 4, 23, 3), (21, 1, 96, 64), 0): (40466432, 40351744, 40466432, 40695808, 44741632, 40351744),
    ('bf16', (3, 4, 23, 3), (21, 1, 96, 64), 256): (40466432, 40351744, 40466432, 40695808, 44741632, 40351744),
    ('bf16', (3, 4, 23, 3), (17, 4, 128, 128), 0): (104783872, 104554496, 105013248, 135102464, 446423040, 131432448),
    ('bf16', (3, 4, 23, 3), (17, 4, 128, 128), 256): (104783872, 104554496, 105013248, 135102464, 446423040, 131432448),
    ('fp16', (1, 1, 1, 1), (16, 2, 64, 64), 0): (39043072, 38928384, 39043072, 39387136, 42532864, 38928384),
    ('fp16', (1, 1, 1, 1), (16, 2, 64, 64), 256): (39043072, 38928384, 39043072, 39387136, 42532864, 38928384),
    ('fp16', (1, 1, 1, 1), (16, 2, 64, 64), 3): (39043072, 38928384, 39043072, 39387136, 42532864, 38928384),
    ('fp16', (1, 1, 1, 1), (21, 1, 96, 64), 0): (37738496, 37623808, 37738496, 37967872, 40342528, 37623808),
    ('fp16', (1, 1, 1, 1), (21, 1, 96, 64), 256): (37738496, 37623808, 37738496, 37967872, 40342528, 37623808),
    ('fp16', (1, 1, 1, 1), (21, 1, 96, 64), 3): (37738496, 37623808, 37738496, 37967872, 40342528, 37623808),
    ('fp16', (1, 1, 1, 1), (17, 4, 128, 128), 0): (75685888, 75456512, 75915264, 94863360, 176676864, 91193344),
    ('fp16', (1, 1, 1, 1), (17, 4, 128, 128), 256): (75685888, 75456512, 75915264, 94863360, 176676864, 91193344),
    ('fp16', (1, 1, 1, 1), (17, 4, 128, 128), 3): (75685888, 75456512, 75915264, 94863360, 176676864, 91193344),
    ('fp16', (2, 1, 2, 1), (16, 2, 64, 64), 0): (39534592, 39419904, 39534592, 39878656, 44138496, 39419904),
    ('fp16', (2, 1, 2, 1), (16, 2, 64, 64), 256): (39534592, 39419904, 39534592, 39878656, 44138496, 39419904),
    ('fp16', (2, 1, 2, 1), (16, 2, 64, 64), 3): (39534592, 39419904, 39534592, 39878656, 44138496, 39419904),
    ('fp16', (2, 1, 2, 1), (21, 1, 96, 64), 0): (38107136, 37992448, 38107136, 38336512, 41546752, 37992448),
    ('fp16', (2, 1, 2, 1), (21, 1, 96, 64), 256): (38107136, 37992448, 38107136, 38336512, 41546752, 37992448),
    ('fp16', (2, 1, 2, 1), (21, 1, 96, 64), 3): (38107136, 37992448, 38107136, 38336512, 41546752, 37992448),
    ('fp16', (2, 1, 2, 1), (17, 4, 128, 128), 0): (79618048, 79388672, 79847424, 101023744, 198434816, 97353728),
    ('fp16', (2, 1, 2, 1), (17, 4, 128, 128), 256): (79618048, 79388672, 79847424, 101023744, 198434816, 97353728),
    ('fp16', (2, 1, 2, 1), (17, 4, 128, 128), 3): (79618048, 79388672, 79847424, 101023744, 198434816, 97353728),
    ('fp16', (3, 4, 23, 3), (16, 2, 64, 64), 0): (42680320, 42565632, 42680320, 43024384, 48398336, 42565632),
    ('fp16', (3, 4, 23, 3), (16, 2, 64, 64), 256): (42680320, 42565632, 42680320, 43024384, 48398336, 42565632),
    ('fp16', (3, 4, 23, 3), (16, 2, 64, 64), 3): (42680320, 42565632, 42680320, 43024384, 48398336, 42565632),
    ('fp16', (3, 4, 23, 3), (21, 1, 96, 64), 0): (40466432, 40351744, 40466432, 40695808, 44741632, 40351744),
    ('fp16', (3, 4, 23, 3), (21, 1, 96, 64), 256): (40466432, 40351744, 40466432, 40695808, 44741632, 40351744),
    ('fp16', (3, 4, 23, 3), (21, 1, 96, 64), 3): (40466432, 40351744, 40466432, 40695808, 44741632, 40351744),
    ('fp16', (3, 4, 23, 3), (17, 4, 128, 128), 0): (104783872, 104554496, 105013248, 135102464, 446423040, 131432448),
    ('fp16', (3, 4, 23, 3), (17, 4, 128, 128), 256): (104783872, 104554496, 105013248, 135102464, 446423040, 131432448),
    ('fp16', (3, 4, 23, 3), (17, 4, 128, 128), 3): (104783872, 104554496, 105013248, 135102464, 446423040, 131432448),
}
# ---- END RECORDED ----
# fmt: on


def _ws_bytes(kind, layers, shape, mode):
    """udapose_net_ws_bytes of one plan under each of POLICIES"""
    from uda_poseestimation_amd import _hip
    lib = _hip.lib(kind)
    h = C.c_void_p()
    assert lib.udapose_net_create((C.c_int * 4)(*layers), *shape, mode, C.byref(h)) == 0
    try:
        out = []
        for over in POLICIES:
            p = _hip.Policy()
            lib.udapose_policy_default(C.byref(p))
            for k, v in over.items():
                setattr(p, k, v)
            assert lib.udapose_net_set_policy(h, C.byref(p)) == 0
            out.append(lib.udapose_net_ws_bytes(h))
        return tuple(out)
    finally:
        lib.udapose_net_destroy(h)


@pytest.mark.parametrize("kind,layers,shape,mode", CASES, ids=lambda v: hex(v) if isinstance(v, int) else "-".join(map(str, v)) if isinstance(v, tuple) else v)
def test_workspace_with_partial_tiles_is_the_recorded_one(kind, layers, shape, mode):
    got = _ws_bytes(kind, layers, shape, mode)
    print(f"{kind} {layers} {shape} mode {mode:#x}: ws_bytes per policy {got}")
    assert got == TABLE[(kind, layers, shape, mode)]


def test_recorded_table_holds_partial_tiles():
    """The table was recorded with a device: every deterministic policy carries partial tiles (at least the stem's, which is always split),
    wgrad_det = 0 none, and taking the stem out of the grouped launch takes its partial tiles out."""
    assert set(TABLE) == set(CASES)
    for case, (default, atomic, s64, s8, s2, s8_nostem) in TABLE.items():
        assert atomic < min(default, s64, s8, s2) and atomic <= s8_nostem < s8, case


if __name__ == "__main__":
    if "--tree" in sys.argv:
        ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
    sys.path.insert(0, ROOT)
    assert "--record" in sys.argv
    rows = [f"    {c!r}: {_ws_bytes(*c)!r},\n" for c in CASES]
    src = open(__file__).read().split("\n")
    lo = next(i for i, l in enumerate(src) if l.startswith("# ---- RECORDED"))
    hi = next(i for i, l in enumerate(src) if l.startswith("# ---- END RECORDED"))
    open(__file__, "w").write("\n".join(src[:lo + 1]) + "\nTABLE = {\n" + "".join(rows) + "}\n" + "\n".join(src[hi:]))
    print(f"recorded {len(rows)} plans from {ROOT}")
