"""The depth-bucket cases (tests/depth_bucket_cases.py) on the host, no GPU: every case has the buckets it is named for -- how many, the
largest one's size against the capacity, equal or differing low 16 key bits, the visible count, one common top byte -- computed from the
fp32 view depths of sc["plan"]; and the plan function of csrc/depth_sort_plan.hpp, compiled with g++ into a small program that asserts
its rules at the threshold."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import depth_bucket_cases as bk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(bk.CASES, **bk.FORCED)


def _within(got, want):
    return want[0] <= got <= want[1] if isinstance(want, tuple) else got == want


@pytest.mark.parametrize("name", list(ALL))
def test_case_has_the_buckets_it_is_named_for(name):
    case = ALL[name]
    kw = case["kw"]
    sc = bk.build(case)
    pl = sc["plan"]
    f = bk.bucket_facts(sc)
    assert sc["means3D"].shape[0] == kw["P"] + kw.get("n_near", 0) <= bk.MAX_P
    assert f["visible"] == case["visible"] == kw["P"] - kw.get("n_culled", 0) + kw.get("n_near", 0)
    assert _within(f["buckets"], case["buckets"]), (f, case["buckets"])
    assert _within(f["largest"], case["largest"]), (f, case["largest"])
    assert f["low"] == case["low"], f
    assert f["one_byte"] == case["one_byte"]
    assert bool(kw.get("n_near")) == (not case["one_byte"])        # whole-grid splats only where the case is about them
    if case["narrow"]:
        # the fp32 view depths of ALL surfels that are in front of the camera share key bits 16..31; the plan's tiles and R still hold
        d = pl["depth"]
        front = d > 0
        assert pl["visible"][~front].sum() == 0 and (np.unique(d[front].view(np.uint32) >> 16) == [0x4040]).all()
        lo, hi = bk.NARROW
        assert lo <= d[pl["visible"]].min() and d[pl["visible"]].max() <= hi
        levels = case["narrow"].get("levels")
        if levels:      # ties: a few long runs of equal keys, each longer than a chunk's share
            k, n = np.unique(bk.visible_keys(sc), return_counts=True)
            assert len(k) == levels and n.min() > f["visible"] // (2 * levels)


def test_tables_cover_every_path_of_the_bucket_kernel():
    def sizes(table, low):
        return {c["largest"] for c in table.values() if c["low"] == low and not isinstance(c["largest"], tuple)}
    for table, cap in ((bk.CASES, bk.CAP), (bk.FORCED, bk.FORCED_CAP)):
        assert {cap - 1, cap, cap + 1} <= sizes(table, "equal")                   # in LDS up to the capacity, above: the order is already there
        assert {cap + 1, 2 * cap + 1} <= sizes(table, "differ")                    # two and three chunks through global memory
        assert any(c["narrow"] and c["narrow"].get("levels") and c["largest"] > 2 * cap for c in table.values())
    assert {bk.CASES[f"size_P{p}"]["kw"]["P"] for p in (1, 63, 64, 65, 1023, 1024, 1025)} == {1, 63, 64, 65, 1023, 1024, 1025}
    assert bk.CASES["one_visible"]["visible"] == 1 and bk.CASES["one_visible"]["kw"]["n_culled"] == 1024
    assert all(c["views"] == 4 for c in ALL.values())
    assert [n for n, c in ALL.items() if not c["one_byte"]] == ["near_breaks_byte"]
    # mixed weights everywhere but the tiny sizes: culled surfels interleaved, right-edge surfels
    assert all(c["kw"].get("n_culled", 0) > 0 and c["kw"].get("edge_frac", 0) > 0 for n, c in ALL.items() if c["kw"]["P"] > 65 and n != "one_visible")


SRC = r'''
#include <cstdio>
#include "depth_sort_plan.hpp"
using namespace svgir;
static int bad = 0;
#define EQ(a, b) do { long long x_ = (long long)(a), y_ = (long long)(b); \
    if (x_ != y_) { std::printf("line %d: %s = %lld, expected %lld\n", __LINE__, #a, x_, y_); bad++; } } while (0)
static int plan(int P, int top, bool lsd = false) { return (int)depth_sort_plan(P, top, lsd); }

int main() {
    const int L = (int)DepthSortPlan::kLsd, B = (int)DepthSortPlan::kBuckets;
    EQ(DEPTH_BUCKET_MAX_P, 1 << 19);
    EQ(DEPTH_BUCKET_CAP, 8192);
    // the threshold, with a speculated byte
    EQ(plan(DEPTH_BUCKET_MAX_P - 1, 0x40), B);
    EQ(plan(DEPTH_BUCKET_MAX_P, 0x40), B);
    EQ(plan(DEPTH_BUCKET_MAX_P + 1, 0x40), L);
    EQ(plan(1, 0), B);                 // (byte 0 is a byte)
    EQ(plan(1, 0xff), B);
    EQ(plan(2000000, 0x40), L);
    // without one: four LSD passes at every size
    EQ(plan(DEPTH_BUCKET_MAX_P - 1, -1), L);
    EQ(plan(DEPTH_BUCKET_MAX_P, -1), L);
    EQ(plan(DEPTH_BUCKET_MAX_P + 1, -1), L);
    EQ(plan(1, -1), L);
    EQ(plan(0, 0x40), L);
    // SVGIR_DEPTH_SORT
    EQ(depth_sort_forced_lsd(nullptr), 0);
    EQ(depth_sort_forced_lsd(""), 0);
    EQ(depth_sort_forced_lsd("buckets"), 0);
    EQ(depth_sort_forced_lsd("lsd"), 1);
    EQ(plan(DEPTH_BUCKET_MAX_P, 0x40, true), L);
    EQ(plan(1000, 0x40, true), L);
    EQ(plan(1000, -1, true), L);
    // SVGIR_DEPTH_BUCKET_CAP only lowers the capacity
    EQ(depth_bucket_cap(nullptr), 8192);
    EQ(depth_bucket_cap(""), 8192);
    EQ(depth_bucket_cap("256"), 256);
    EQ(depth_bucket_cap("8192"), 8192);
    EQ(depth_bucket_cap("8193"), 8192);
    EQ(depth_bucket_cap("100000000"), 8192);
    EQ(depth_bucket_cap("64"), 64);
    EQ(depth_bucket_cap("63"), 64);
    EQ(depth_bucket_cap("0"), 64);
    EQ(depth_bucket_cap("-5"), 64);
    EQ(depth_bucket_cap("x"), 64);
    if (!bad) std::printf("OK\n");
    return bad ? 1 : 0;
}
'''


def test_depth_sort_plan_rules():
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.cpp"), "w") as f:
            f.write(SRC)
        exe = os.path.join(d, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "svg-ir_amd", "csrc"), os.path.join(d, "t.cpp"),
                        "-o", exe], check=True, capture_output=True, text=True, timeout=300)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout
