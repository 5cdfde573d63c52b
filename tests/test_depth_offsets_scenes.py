"""The depth-offsets cases (tests/depth_offsets_cases.py) on the host, no GPU: every case has the key count, the visible count and the
instance count it is named for, and its multiset of weights (tile counts per surfel, from sc["plan"]) holds what the case claims --
0 (culled) and 2 (a right edge) present, T present where there are whole-grid splats.  Also: the geometry blob's size through the C
ABI against the layout of csrc/common.hpp geom_layout, at the key counts where the radix scratch grows."""
import numpy as np
import pytest

import depth_offsets_cases as dc
from svgir_harness import scenes


@pytest.mark.parametrize("name", list(dc.CASES))
def test_case_has_the_size_and_the_weights_it_is_named_for(name):
    case = dc.CASES[name]
    kw = case["kw"]
    sc = scenes.binning_scene("rgss", **kw)
    pl = sc["plan"]
    w = dc.weights(sc)
    assert sc["means3D"].shape[0] == case["keys"] == len(w) == kw["P"] + kw.get("n_near", 0)
    assert int(pl["visible"].sum()) == kw["P"] - kw.get("n_culled", 0)
    assert int(w.sum()) == pl["R"]
    if case["R"] is not None:
        assert pl["R"] == case["R"], (pl["R"], case["R"])
    present = set(np.unique(w).tolist())
    if kw.get("n_culled"):
        assert 0 in present
    if kw.get("edge_frac") and kw["P"] - kw.get("n_culled", 0) >= 63:
        assert {1, 2} <= present
    if kw.get("n_near"):
        assert dc.T in present and (w == dc.T).sum() == kw["n_near"]
    # the culled surfels are interleaved with the visible ones by index, not bunched at one end
    if kw.get("n_culled", 0) >= 200 and kw["P"] - kw["n_culled"] >= 200:
        z = np.nonzero(w[:kw["P"]] == 0)[0]
        assert z[0] < kw["P"] // 8 and z[-1] > kw["P"] - kw["P"] // 8 and np.diff(z).max() <= 2 * kw["P"] // kw["n_culled"] + 2
    depth = kw.get("depth", "spread")
    tops = dc.top_bytes(sc)
    if depth == "same":
        assert np.unique(pl["depth"].view(np.uint32)[pl["visible"]]).size == 1      # every visible key in one digit run, in every pass
    if depth == "binade" and not kw.get("n_near"):
        assert len(tops) == 1
    if depth == "spread" and case["keys"] >= 63:
        assert len(tops) > 1


def test_table_covers_the_places_where_the_weighted_pass_changes_behaviour():
    keys = {c["keys"] for c in dc.CASES.values()}
    assert {1, 63, 64, 65, 1023, 1025, 2049, 32769, dc.M + 1} <= keys
    assert [n for n, c in dc.CASES.items() if c["keys"] > dc.M] == ["large"]
    assert all(c["views"] == 4 for c in dc.CASES.values() if c["keys"] >= 32769)
    assert dc.CASES["one_visible"]["R"] == 1
    # no list of the large case beyond 2^20 / 8 (csrc/common.hpp SEG_K_BITS): uniform over 48 tiles
    assert dc.CASES["large"]["R"] / dc.T * 2 < dc.M // 8


def test_special_scenes():
    full = scenes.binning_scene("rgss", **dc.EMPTY_BETWEEN)
    none = scenes.binning_scene("rgss", **dict(dc.EMPTY_BETWEEN, n_culled=dc.EMPTY_BETWEEN["P"]))
    assert none["plan"]["R"] == 0 and not dc.weights(none).any() and full["plan"]["R"] > full["means3D"].shape[0]
    sv = scenes.binning_scene("svgss", **dc.SVGSS)
    assert {0, 1, 2} <= set(np.unique(dc.weights(sv)).tolist())
    a, b = (scenes.binning_scene("rgss", **kw) for kw in dc.BROKEN_SPECULATION)
    assert a["means3D"].shape == b["means3D"].shape and len(dc.top_bytes(a)) == 1 and len(dc.top_bytes(b)) > 1


def _align(x, a=256):
    return (x + a - 1) // a * a


def _geom_bytes(P):
    """csrc/common.hpp geom_layout, array by array (each starts 256-byte aligned)."""
    sort_blocks = (P + 1023) // 1024
    scan_blocks = (P + 2047) // 2048
    gtot = 5 * 256 * (sort_blocks // 32 + 1)                # four passes + the weighted pass's slot
    parts = [P * 24 * 4, P * 6 * 4, P * 4, P * 8,           # rec, cov3D, clamped, tiles
             P * 4, P * 4, P * 4, P * 4, P * 4,             # key[2], idx[2], offsets
             (256 * sort_blocks + gtot) * 4,                # radix_tbl
             256 * sort_blocks * 4,                         # radix_wtbl
             16, (P + 63) // 64 * 4,                        # counters, key_top
             P, P * 4, (scan_blocks + 2) * 4]               # needed, shade_list, shade_work
    return sum(_align(b) for b in parts)


@pytest.mark.parametrize("P", [1, 1024, 1025, (1 << 20) + 1])
def test_geometry_blob_size(P):
    from gaussian_renderer import _native
    assert _native.lib.svgir_geom_bytes(P) == _geom_bytes(P)
