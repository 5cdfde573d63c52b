"""CPU half of the tile-sort tests on the single-pass plan (the GPU half is tests/test_gpu_tile_bin.py): for every case of
tests/tile_bin_cases.py the oracle's integer state must equal the scene's construction, and the case must have the property it is named
for -- instance count on a key-block boundary, a two-tile surfel across one, key blocks wholly inside one surfel's run, visible span."""
import numpy as np
import pytest

import tile_bin_cases as tb
from oracle import oracle as orc
from svgir_harness import scenes


def depth_ordered_runs(o):
    """(order, offsets, tiles touched): the visible surfels in depth order (fp32 depth bits, then index: the stable depth sort), the first
    instance position of each in the unsorted instance stream, and every surfel's instance count."""
    tt = o.get("tiles_touched").astype(np.int64)
    vis = np.nonzero(tt > 0)[0]
    dbits = o.get("depths").astype(np.float32).view(np.uint32)
    order = vis[np.lexsort((vis, dbits[vis]))]
    offsets = np.concatenate([[0], np.cumsum(tt[order])[:-1]]) if len(order) else np.zeros(0, np.int64)
    return order, offsets, tt


def check_case_on_oracle(name):
    case = tb.CASES[name]
    ex, kw = case["expect"], case["kw"]
    sc = scenes.binning_scene(case["variant"], **kw)
    plan = sc["plan"]
    o = orc.OracleRun(sc, orc.SVGSS if case["variant"] == "svgss" else orc.RGSS)
    R = o.forward()
    # -- the oracle against the construction
    exp_list, exp_ranges = scenes.binning_expected(sc)
    assert R == plan["R"] == len(exp_list)
    assert np.array_equal(o.get("point_list")[:R], exp_list) and np.array_equal(o.get("ranges").reshape(-1, 2), exp_ranges)
    # -- the case sits where it claims to
    T = plan["T"]
    assert T == ex["T"] <= 4096
    if ex["R"] is not None:
        assert R == ex["R"], (R, ex["R"])
    if "R_about" in ex:
        assert abs(R - ex["R_about"]) < 0.02 * ex["R_about"], R
    order, offsets, tt = depth_ordered_runs(o)
    assert len(order) == ex["visible"], len(order)
    if plan["n_near"]:      # the whole-grid splats sort first
        assert (tt[-plan["n_near"]:] == T).all() and set(order[:plan["n_near"]]) == set(range(len(tt) - plan["n_near"], len(tt)))
    if kw.get("edge_frac"):
        assert 0.8 * kw["edge_frac"] < (tt[order] == 2).mean() < 1.2 * kw["edge_frac"]
    if "long_runs" in ex:        # the first instances belong to that many surfels, each with a run per tile
        assert (tt[order[:ex["long_runs"]]] == T).all() and offsets[ex["long_runs"]] == ex["long_runs"] * T > 2 * tb.KEYS
    if ex.get("straddle"):       # a surfel with one instance at 4096 m - 1 and the other at 4096 m
        two = (tt[order] == 2) & ((offsets + 1) % tb.KEYS == 0)
        assert two.any(), "no two-tile surfel straddles a block boundary: move the seed"
    if "whole_blocks" in ex:     # blocks wholly inside one surfel's run
        first = lambda pos: np.searchsorted(offsets, pos, "right") - 1       # the surfel that owns instance position pos
        inside = [b for b in range(R // tb.KEYS) if first(tb.KEYS * b) == first(tb.KEYS * b + tb.KEYS - 1)]
        assert len(inside) >= ex["whole_blocks"], inside


@pytest.mark.parametrize("name", list(tb.CASES))
def test_case_has_the_property_it_is_named_for(name):
    check_case_on_oracle(name)


def test_case_table_covers_every_threshold():
    C = tb.CASES
    assert {c["expect"]["R"] for c in C.values()} >= {2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193}
    assert {c["expect"]["visible"] for c in C.values()} >= {1, 2, 63, 64, 65, 255, 256, 257}
    assert {c["expect"]["T"] for c in C.values()} >= {1, 4096, 3072}
    assert sum(c["backward"] and c["variant"] == "svgss" for c in C.values()) == 1
    a, b = (scenes.binning_scene("rgss", **kw)["plan"] for kw in tb.RERUN)
    assert len(a["tile"]) + a["n_near"] == len(b["tile"]) + b["n_near"]            # equal surfel counts
    cap = (a["R"] + a["R"] // 8 + 1024 + 4095) // 4096 * 4096                        # csrc/api.hip: the speculative capacity
    assert a["R"] < cap < b["R"] and cap % tb.KEYS == 0
