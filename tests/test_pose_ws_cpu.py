"""The workspace layouts of the instance layer (csrc/pose_ws.h) without a GPU: a small host program prints every
struct's byte count and region offsets; the counts are the formulas the launchers have always reported, every region lies inside the count,
none overlaps another, and each is aligned for the type the kernels read it as (the base is 8-byte aligned, as the launchers require)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = r"""
#include <stdio.h>
#include "pose_ws.h"
static char* const BASE = (char*)(uintptr_t)0x100008;      /* 8-byte aligned and no more; never read */
#define OFF(p) (long long)((char*)(p) - BASE)
int main() {
    const int Ms[] = {1, 63, 64, 65, 4096};
    for (int M : Ms) {
        const PoseNmsWs w(BASE, M);
        printf("nms %d %lld %lld %lld %lld %lld\n", M, (long long)w.bytes, (long long)PoseNmsWs(nullptr, M).bytes, OFF(w.mask), OFF(w.area), OFF(w.refused));
    }
    const int MF[][2] = {{1, 1}, {1, 2}, {17, 3}, {300, 22}, {4096, 4096}, {4095, 259}};
    for (auto& c : MF) {
        const ApMatchWs w(BASE, c[0], c[1]);
        printf("match %d %d %lld %lld %lld %lld %lld %lld\n", c[0], c[1], (long long)w.bytes, (long long)ApMatchWs(nullptr, c[0], c[1]).bytes, OFF(w.order),
               OFF(w.ofr), OFF(w.darea), OFF(w.rec_off));
    }
    const int CTA[][3] = {{1, 1, 1}, {7, 2, 1}, {8, 10, 3}, {65536, 10, 3}, {262144, 16, 4}, {4097, 64, 1}};
    for (auto& c : CTA) {
        const ApCurveWs w(BASE, c[0], c[1], c[2]);
        printf("curve %d %d %d %lld %lld %lld %lld %lld %lld %lld\n", c[0], c[1], c[2], (long long)w.bytes,
               (long long)ApCurveWs(nullptr, c[0], c[1], c[2]).bytes, OFF(w.ss), OFF(w.sm), OFF(w.si), OFF(w.tpc), OFF(w.fpc));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_ws")
    (d / "main.cpp").write_text(MAIN)
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-Werror", "-I", os.path.join(ROOT, "uda_poseestimation_amd", "csrc"), str(d / "main.cpp"),
                    "-o", str(d / "main")], check=True)
    out = subprocess.run([str(d / "main")], check=True, capture_output=True, text=True).stdout
    return [(line.split()[0], [int(v) for v in line.split()[1:]]) for line in out.splitlines()]


def _regions_ok(total, regions):
    """regions: (offset, element size, element count) in layout order: aligned, inside [0, total), one after the other."""
    end = 0
    for off, size, count in regions:
        assert off % size == 0 and off >= end, (off, size, end)
        end = off + size * count
    assert end <= total, (end, total)


def test_pose_nms_workspace(rows):
    seen = []
    for kind, (M, total, counted, mask, area, refused) in [r for r in rows if r[0] == "nms"]:
        W = (M + 63) // 64
        assert total == counted == M * W * 8 + M * 4 + M          # the mask, the areas, the refused flags
        assert mask == 0                                          # 8-byte words at the 8-byte aligned base
        _regions_ok(total, [(mask, 8, M * W), (area, 4, M), (refused, 1, M)])
        seen.append(M)
    assert seen == [1, 63, 64, 65, 4096] and 4096 * (64 * 8 + 5) == 4096 * 64 * 8 + 4096 * 4 + 4096


def test_ap_match_workspace(rows):
    cases = [r[1] for r in rows if r[0] == "match"]
    assert len(cases) == 6
    for M, F, total, counted, order, ofr, darea, rec_off in cases:
        assert total == counted == (4 * (3 * M + F) + 7) // 8 * 8  # the order, the ordered frames, the areas, the record offsets, padded to 8
        _regions_ok(total, [(order, 4, M), (ofr, 4, M), (darea, 4, M), (rec_off, 4, F)])


def test_ap_curve_workspace(rows):
    cases = [r[1] for r in rows if r[0] == "curve"]
    assert len(cases) == 6
    for cap, T, A, total, counted, ss, sm, si, tpc, fpc in cases:
        assert total == counted == (4 * cap + 7) // 8 * 8 + 2 * cap * 8 + 2 * T * A * cap * 4
        _regions_ok(total, [(ss, 4, cap), (sm, 8, cap), (si, 8, cap), (tpc, 4, T * A * cap), (fpc, 4, T * A * cap)])
