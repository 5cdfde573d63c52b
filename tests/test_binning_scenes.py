"""The binning scenes of svgir_harness.scenes.binning_scene, on the CPU oracle (no GPU): for every case of tests/binning_cases.py the
oracle's integer state -- instance count, depth-sorted instance list, tile ranges -- must equal what the scene was constructed to
give (plain numpy: lexsort by tile, fp32 depth bits, index; ranges from the run lengths; empty tiles (0, 0)), exactly; and the case
must sit where its name says: surfel count, instance count, tile count and tile bits, number of distinct top bytes of the visible
depth keys, visible span.  tests/test_gpu_binning.py runs the same cases through the HIP binning; DESIGN.md section 5.

The oracle's rasterizer state is not pinned by the reference; for the integer state this is the independent check."""
import numpy as np
import pytest

import binning_cases as bc
from oracle import oracle as orc
from svgir_harness import scenes


def _oracle(sc, variant):
    o = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS)
    o.forward()
    return o


def check_case_on_oracle(name):
    """Builds the case, runs the oracle, asserts the construction and the case's own claims; returns (scene, oracle run)."""
    case = bc.CASES[name]
    ex, kw = case["expect"], case["kw"]
    sc = scenes.binning_scene(case["variant"], **kw)
    plan = sc["plan"]
    o = _oracle(sc, case["variant"])
    R = o.num_rendered
    # -- the oracle against the construction
    exp_list, exp_ranges = scenes.binning_expected(sc)
    vis = np.concatenate([plan["visible"], np.ones(plan["n_near"], dtype=bool)])
    rad = o.get("radii")
    assert R == plan["R"] == len(exp_list), (R, plan["R"])
    assert (rad[:len(plan["tile"])][plan["visible"]] == 3).all() and (rad[~vis] == 0).all()    # the 0.3 px^2 low-pass alone / culled
    dep = o.get("depths").astype(np.float32)
    assert np.array_equal(dep.view(np.uint32)[vis], plan["depth"].view(np.uint32)[vis]), "the oracle's depths are not 4 - z_world"
    assert np.array_equal(o.get("point_list")[:R], exp_list), "instance list differs from lexsort(tile, depth bits, index)"
    rg = o.get("ranges").reshape(-1, 2)
    assert np.array_equal(rg, exp_ranges), "tile ranges differ from the run lengths"
    # -- the case sits where it claims to
    T = plan["T"]
    assert sc["means3D"].shape[0] == ex["P"] and T == ex["T"] == ((sc["W"] + 15) // 16) * ((sc["H"] + 15) // 16)
    if ex["R"] is not None:
        assert R == ex["R"], (R, ex["R"])
    assert int(plan["visible"].sum()) == ex["visible"]
    bits = 1
    while (1 << bits) < T:
        bits += 1
    assert bits == ex["bits"]
    if "passes" in ex:      # (csrc/common.hpp tile_sort_plan with the single counting pass switched off)
        assert (bits + 7) // 8 == ex["passes"]
    top = np.unique(plan["depth"].view(np.uint32)[vis] >> 24)
    assert len(top) == ex["top"], top
    if kw.get("depth") == "same":
        assert np.unique(dep.view(np.uint32)[vis]).size == 1
        if kw.get("layout") == "one":       # one tile, one depth: the list is the indices in order
            assert np.array_equal(exp_list, np.arange(ex["P"], dtype=np.uint32))
    lens = rg[:, 1].astype(np.int64) - rg[:, 0]
    assert lens.max(initial=0) <= bc.MAX_LIST, lens.max()
    if kw.get("layout") == "one":
        assert (lens > 0).sum() == 1 and lens.max() == R
    if kw.get("layout") == "eight":
        assert (lens > 0).sum() == 8 and lens.max() - lens[lens > 0].min() <= 1
    if kw.get("layout") == "skewed":
        assert (lens == 0).mean() > 0.9
    if kw.get("edge_frac"):
        assert R > ex["visible"] + plan["n_near"] * T       # some surfels really are in two tiles
    if plan["n_near"]:
        tt = o.get("tiles_touched")
        assert (tt[-plan["n_near"]:] == T).all() and sc["W"] // 16 == 1023        # rectangles of the full packed width
    return sc, o


@pytest.mark.parametrize("name", list(bc.CASES))
def test_oracle_binning_equals_the_construction(name):
    check_case_on_oracle(name)


def test_case_table_covers_every_threshold():
    """The values the binning code switches on, each named by at least one case (whose test above proves it has that size)."""
    C = bc.CASES.values()
    M = bc.M
    Ps = {c["expect"]["P"] for c in C}
    assert {1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 32767, 32768, 32769, M - 1, M, M + 1} <= Ps
    Ts = {c["expect"]["T"] for c in C}
    assert {1, 255, 256, 257, 3072, 3074, 4095, 4096, 4097, 1023 * 33} <= Ts
    assert {c["expect"]["bits"] for c in C} >= {1, 6, 8, 9, 12, 13, 14, 16}
    rgss = [c for c in C if c["variant"] == "rgss"]
    Rs = lambda pred: {c["expect"]["R"] for c in rgss if c["expect"]["R"] is not None and pred(c["expect"]["T"])}
    assert {2047, 2048} <= Rs(lambda T: T <= 4096) and any(r > 16 * 8 * 2048 for r in Rs(lambda T: T <= 4096))
    assert {2049, M - 1, M + 1} <= Rs(lambda T: T > 256)
    # one two-pass grid whose count is below 2^20 and whose speculative capacity (csrc/api.hip: R + R/8 + 1024, in 4096s) is above
    r = bc.CASES["tiles_T10000_R940000"]["expect"]["R"]
    assert r < M < r + r // 8 + 1024 and bc.CASES["tiles_T10000_R940000"]["views"] == 4
    assert {c["expect"]["visible"] for c in C} >= {63, 64, 65}
    assert all(c["views"] == 4 for c in C if c["expect"]["P"] >= 32767 and c["variant"] == "rgss")
    for depth in ("spread", "binade", "same"):      # the three largest sizes: every depth mode in both layouts
        for layout in ("uniform", "eight"):
            assert {c["expect"]["P"] for c in C if c["kw"].get("depth", "spread") == depth and c["kw"].get("layout", "uniform") == layout} >= {M - 1, M, M + 1}
    assert {bc.CASES[n]["expect"]["T"] for n in bc.FORCED["xcd"]} == {256, 257, 2048, 2049, 3074}
    assert {bc.CASES[n]["expect"]["bits"] for n in bc.FORCED["radix"]} >= {1, 6, 8, 9, 12}


def test_whole_view_culled_scene_is_empty():
    """The middle view of test_gpu_binning's non-empty / empty / non-empty sequence: every surfel culled, no instance, no range."""
    sc = scenes.binning_scene("rgss", P=3000, n_culled=3000, seed=3, **bc.GRID)
    o = _oracle(sc, "rgss")
    assert o.num_rendered == 0 and sc["plan"]["R"] == 0
    assert not o.get("ranges").any() and not o.get("radii").any()
