"""The depth-gather cases (tests/depth_gather_cases.py) on the host, no GPU: every case has the rows it is named for -- how many, the size
of the last one, which are empty, which hold one digit and which many, the ties, the largest bucket against the forced capacity and the
rows it is gathered from -- computed from the fp32 view depths of sc["plan"]; the plan's R against a plain count; and the row geometry
of csrc/depth_sort_plan.hpp, compiled with g++ into a small program that asserts it at the thresholds."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import depth_gather_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(gc.CASES, **gc.FORCED)
_built = {}


def _scene(name):
    if name not in _built:
        _built[name] = gc.build(ALL[name])
    return _built[name]


@pytest.mark.parametrize("name", list(ALL))
def test_case_has_the_rows_it_is_named_for(name):
    case = ALL[name]
    sc = _scene(name)
    pl = sc["plan"]
    f = gc.row_facts(sc)
    P = case["kw"]["P"]
    assert sc["means3D"].shape[0] == P <= gc.MAX_P and f["one_byte"]
    for k, want in case["facts"].items():
        if k == "one_digit_rows":
            assert all(f["digits_per_row"][b] == 1 for b in want), f
        elif k == "spread_rows":
            assert all(f["digits_per_row"][b] >= 48 for b in want), f
        elif k == "ties":
            assert f["ties"] == f["distinct_keys"] == want, f     # every key of the scene is tied across rows and inside one
        else:
            assert f[k] == want, (k, f[k], want)
    # the surfels that left are behind the camera, the ones that stayed kept their binade; the plan's R is a plain count
    d = pl["depth"]
    assert (d[~pl["visible"]] < 0).all() and (d[pl["visible"]] >= 2.0).all() and (d[pl["visible"]] < 4.0).all()
    assert pl["R"] == int(pl["visible"].sum() + (pl["tile2"][pl["visible"]] >= 0).sum())
    if name in gc.FORCED:
        assert (f["largest"] > gc.FORCED_CAP) == name.startswith("f_oversize") and f["largest_rows"] >= 3


def test_moved_surfels_keep_their_pixels():
    """_move slides a surfel along its view ray: the plan's tiles, computed before, still hold (the oracle decides on the GPU side)."""
    from svgir_harness import scenes
    case = gc.CASES["one_digit_row"]
    before = scenes.binning_scene("rgss", **case["kw"])
    after = _scene("one_digit_row")
    eye = np.array(scenes.BINNING_EYE, dtype=np.float64)
    a, b = before["means3D"].astype(np.float64) - eye, after["means3D"].astype(np.float64) - eye
    vis = after["plan"]["visible"]
    ra, rb = a[:, :2] / a[:, 2:3], b[:, :2] / b[:, 2:3]
    assert np.abs(ra - rb)[vis].max() < 1e-6 and np.array_equal(before["plan"]["tile"], after["plan"]["tile"])


def test_table_covers_what_the_rows_add():
    names = set(gc.CASES)
    assert {f"rows_P{p}" for p in (gc.K - 1, gc.K, gc.K + 1, 2 * gc.K + 1)} <= names
    assert gc.CASES[f"rows_P{gc.K + 1}"]["facts"]["last_row"] == 1 and gc.CASES[f"rows_P{gc.K - 1}"]["facts"]["last_row"] == gc.K - 1
    assert gc.CASES["empty_row_between"]["facts"]["empty_rows"] == [1] and gc.CASES["empty_row_between"]["facts"]["rows"] == 3
    assert gc.CASES["last_surfel_only"]["facts"]["visible"] == 1
    assert gc.CASES["max_rows"]["kw"]["P"] == gc.MAX_P and gc.CASES["max_rows"]["facts"]["rows"] == gc.MAX_P // gc.K
    assert {c["facts"]["low"] for n, c in gc.FORCED.items() if n.startswith("f_oversize")} == {"equal", "differ"}
    assert all(c["views"] == 4 for c in ALL.values())


SRC = r'''
#include <cstdio>
#include "depth_sort_plan.hpp"
using namespace svgir;
static int bad = 0;
#define EQ(a, b) do { long long x_ = (long long)(a), y_ = (long long)(b); \
    if (x_ != y_) { std::printf("line %d: %s = %lld, expected %lld\n", __LINE__, #a, x_, y_); bad++; } } while (0)

int main() {
    const int L = (int)DepthSortPlan::kLsd, B = (int)DepthSortPlan::kBuckets;
    EQ(DEPTH_ROW, KROW);
    EQ(DEPTH_ROWS_MAX, (1 << 19) / KROW);
    EQ(depth_rows(1), 1);
    EQ(depth_rows(KROW - 1), 1);
    EQ(depth_rows(KROW), 1);
    EQ(depth_rows(KROW + 1), 2);
    EQ(depth_rows(2 * KROW + 1), 3);
    EQ(depth_rows(DEPTH_BUCKET_MAX_P), DEPTH_ROWS_MAX);
    // one surfel more than the plan's limit: the LSD passes sort, no rows are written
    EQ((int)depth_sort_plan(DEPTH_BUCKET_MAX_P, 0x40, false), B);
    EQ((int)depth_sort_plan(DEPTH_BUCKET_MAX_P + 1, 0x40, false), L);
    if (!bad) std::printf("OK\n");
    return bad ? 1 : 0;
}
'''


def test_row_geometry_of_the_plan():
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.cpp"), "w") as f:
            f.write(SRC)
        exe = os.path.join(d, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-DKROW={gc.K}", "-I", os.path.join(ROOT, "svg-ir_amd", "csrc"),
                        os.path.join(d, "t.cpp"), "-o", exe], check=True, capture_output=True, text=True, timeout=300)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout
