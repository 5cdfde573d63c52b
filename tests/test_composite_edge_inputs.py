"""The table of tests/composite_cases.py holds what it claims, on the CPU oracle (no GPU) -- and the oracle's blend chain is pinned
independently: by chain32, an fp32 emulation in numpy, bit for bit, and by closed_form64 to 1e-12.

  * every axis scene: the oracle's means2D equals the pixel centre exactly;
  * chain32 == the fp32 oracle's n_contrib and opacity plane on the axis pixel, on every view of every case;
  * the switch index of every ladder is the one the table states, and each ladder is monotone with one switch;
  * alpha_off_axis: fp32 and fp64 agree on every decided step, at most 9 of the 65 steps are undecided, in one block around the crossing;
  * closed_form64 == the fp64 oracle's dL_dopacity and dL_dcolors to 1e-12 of the largest entry (measured: 1.4e-15);
  * E32, what the reference's own fp32 arithmetic loses per candidate on the deep lists, is below 2^-19 = 32 eps32 (measured: 11.1, 18.9,
    15.4 eps32 on deep200 / deep1024 / deep700, 5.7 on deep_mixed; dL_dcolors 11.3, 14.4, 12.7, 8.5 eps32 of w_k |g|);
  * every blended candidate's closed-form |dL_dopacity| is at least 1e-3 A_k."""
import functools

import numpy as np
import pytest

import composite_cases as cc

TABLE_IDS = [cc.table_id(t) for t in cc.TABLE]
VALUE_IDS = [cc.table_id(t) for t in cc.VALUE_TABLE]


@functools.lru_cache(maxsize=None)
def _fwd(name, variant, S, VS):
    """The fp32 oracle's forward on every view of a case (computed once, shared, never modified)."""
    out = []
    for v in cc.build(name, variant, S, VS):
        o = cc.oracle_run(v["sc"], variant)
        o.pop("run")
        out.append(o)
    return out


@pytest.mark.parametrize("name,variant,S,VS", cc.TABLE, ids=TABLE_IDS)
def test_chain32_is_the_oracles_chain(name, variant, S, VS):
    for v, o in zip(cc.build(name, variant, S, VS), _fwd(name, variant, S, VS)):
        sc, ch = v["sc"], v["chain"]
        x, y = sc["axis"]
        assert np.array_equal(o["means2D"], np.broadcast_to(np.array([x, y], np.float32), o["means2D"].shape)), v["name"]
        assert o["R"] > 0
        assert int(o["n_contrib"][y, x]) == ch["n_contrib"], (v["name"], int(o["n_contrib"][y, x]), ch["n_contrib"])
        assert o["opacity"][y, x].view(np.uint32) == ch["opacity"].view(np.uint32), (v["name"], o["opacity"][y, x], ch["opacity"])
        assert not (ch["passed"] & ~o["blended"]).any(), v["name"]     # what the axis pixel blends has a weight
        if "n_contrib" in v["claims"]:
            assert ch["n_contrib"] == v["claims"]["n_contrib"], v["name"]


@pytest.mark.parametrize("variant,S,VS", cc.WIDTHS, ids=[cc.wid(*w) for w in cc.WIDTHS])
def test_alpha_ladder_switches_at_index_16(variant, S, VS):
    views, fw = cc.build("alpha_axis", variant, S, VS), _fwd("alpha_axis", variant, S, VS)
    lad = np.array([v["op"][0] for v in views])
    assert len(lad) == 33 and (np.diff(lad.view(np.int32)) == 1).all() and lad[16] == cc.ALPHA_MIN
    for i, (v, o) in enumerate(zip(views, fw)):
        x, y = v["sc"]["axis"]
        assert bool(v["chain"]["passed"][0]) == (i >= 16) == v["claims"]["blends"]
        assert (o["n_contrib"] > 0).sum() == (1 if i >= 16 else 0) and bool(o["blended"][0]) == (i >= 16)   # the axis pixel alone may pass
        one = np.float32(1.0)
        assert o["opacity"][y, x] == (one - (one - lad[i]) if i >= 16 else one - cc.T_CLAMP)     # 1.f - T, T = 1.f - alpha


@pytest.mark.parametrize("variant,S,VS", cc.WIDTHS, ids=[cc.wid(*w) for w in cc.WIDTHS])
def test_packed_alpha_ladder(variant, S, VS):
    v, o = cc.build("alpha_axis_packed", variant, S, VS)[0], _fwd("alpha_axis_packed", variant, S, VS)[0]
    perm = v["claims"]["perm"]
    pos = np.argsort(perm)
    assert sorted(perm) == list(range(33))
    # the steps next to the switch stand in both slots of the forward's candidate pairs
    assert {pos[14] % 2, pos[15] % 2} == {0, 1} and {pos[16] % 2, pos[17] % 2} == {0, 1}
    assert np.array_equal(v["chain"]["passed"], perm >= 16) and np.array_equal(o["blended"], perm >= 16)
    assert (o["n_contrib"] > 0).sum() == 1


@pytest.mark.parametrize("variant,S,VS", cc.WIDTHS, ids=[cc.wid(*w) for w in cc.WIDTHS])
def test_clamp_ladder(variant, S, VS):
    views = cc.build("clamp_axis", variant, S, VS)
    ops = np.array([v["op"][0] for v in views])
    assert len(ops) == 10 and ops[4] == cc.ALPHA_MAX and ops[9] == 1.0 and (np.diff(ops[:9].view(np.int32)) == 1).all()
    for v, o in zip(views, _fwd("clamp_axis", variant, S, VS)):
        x, y = v["sc"]["axis"]
        assert o["opacity"][y, x] == min(cc.ALPHA_MAX, v["op"][0]) == v["claims"]["opacity"] and int(o["n_contrib"][y, x]) == 1


@pytest.mark.parametrize("name,front,switch", [("cutoff_axis", cc.CUTOFF_FRONT, cc.CUTOFF_SWITCH), ("cutoff_mixed", cc.MIXED_FRONT, 16)])
@pytest.mark.parametrize("variant,S,VS", cc.WIDTHS, ids=[cc.wid(*w) for w in cc.WIDTHS])
def test_cutoff_ladders_are_monotone_with_one_switch(variant, S, VS, name, front, switch):
    views, fw = cc.build(name, variant, S, VS), _fwd(name, variant, S, VS)
    lad = np.array([v["op"][front] for v in views])
    assert len(lad) == 33 and (np.diff(lad.view(np.int32)) == 1).all()
    nc = np.array([int(o["n_contrib"][v["sc"]["axis"][1], v["sc"]["axis"][0]]) for v, o in zip(views, fw)])
    assert np.array_equal(nc, np.where(np.arange(33) < switch, front + 1, front)), nc
    if name == "cutoff_axis":
        assert switch == 19 and lad[16] == np.float32(0.1808)       # n_contrib is 14 through index 18
        assert all(v["chain"]["T"][front] == np.float32(2.0 ** -13) for v in views[:switch])
    else:
        # the product's rounding decides: the exact product T (1 - a) of the first step that ends the pixel is NOT below 0.0001f by more than
        # an ulp of it, and the front is not dyadic
        T = np.float64(views[0]["chain"]["T"][front])
        exact = T * (1.0 - np.float64(lad[switch - 1]))
        assert abs(exact - np.float64(cc.T_MIN)) < 2.0 ** -23 * float(cc.T_MIN) * 4
        assert np.frexp(T)[0] != 0.5


@pytest.mark.parametrize("k", cc.CUTOFF_AT)
@pytest.mark.parametrize("variant,S,VS", cc.WIDTHS, ids=[cc.wid(*w) for w in cc.WIDTHS])
def test_cutoff_on_list_position_k(variant, S, VS, k):
    views, fw = cc.build(f"cutoff_at{k}", variant, S, VS), _fwd(f"cutoff_at{k}", variant, S, VS)
    lad = np.array([v["op"][k - 1] for v in views])
    assert (np.diff(lad.view(np.int32)) == 1).all() and cc.ALPHA_MIN < lad[0] and lad[2] < 0.985
    nc = [int(o["n_contrib"][v["sc"]["axis"][1], v["sc"]["axis"][0]]) for v, o in zip(views, fw)]
    assert nc == [k, k - 1, k - 1]
    assert all(v["chain"]["passed"][:k - 1].all() and len(v["op"]) == k + 1 for v in views)     # the whole front blends; one surfel behind


@pytest.mark.parametrize("W,H", cc.RESIDUE_SIZES, ids=[f"{w}x{h}" for w, h in cc.RESIDUE_SIZES])
def test_residues_cover_the_sub_tile(W, H):
    views = cc.build(f"residues_{W}x{H}", "rgss", 5, 0)
    assert [v["chain"]["n_contrib"] for v in views] == [33, 14, 14, 13, 13]
    assert all(v["sc"]["W"] == W and v["sc"]["H"] == H and v["sc"]["axis"] == ((W - 1) // 2, (H - 1) // 2) for v in views)


def test_residues_reach_every_lane_row_column_and_sub_tile():
    px = [(w - 1) // 2 for w, h in cc.RESIDUE_SIZES if w == h]
    assert sorted(p % 8 for p in px) == sorted(list(range(8)) * 2) and {p // 8 for p in px} == {0, 1}
    assert (1, 1) in cc.RESIDUE_SIZES and (31, 3) in cc.RESIDUE_SIZES and max(max(s) for s in cc.RESIDUE_SIZES) <= 31


# ---- off the axis -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def off_axis_host(variant, S, VS):
    """The off-axis ladder: per step the opacity, the fp64 and the fp32 oracle's decision on the pixel under test, and whether it is undecided."""
    sc = cc.off_axis_scene(variant, S, VS, 0.5)
    o = cc.oracle_run(sc, variant, fp64=True)
    power, _ = cc.off_axis_alpha64(o["run"], sc, 0.5)
    cross = np.float32((1.0 / 255.0) / np.exp(power))       # (alpha is linear in the opacity: the bisection's fixed point)
    lad = cc.ladder(cross, 32)
    px, py = cc.off_axis_pixel(sc)
    d64, d32, und = [], [], []
    for a in lad:
        s2 = cc.off_axis_scene(variant, S, VS, a)
        o64, o32 = cc.oracle_run(s2, variant, fp64=True), cc.oracle_run(s2, variant)
        pw, al = cc.off_axis_alpha64(o64["run"], s2, a)
        d64.append(int(o64["n_contrib"][py, px])); d32.append(int(o32["n_contrib"][py, px])); und.append(bool(cc.undecided(pw, al)))
    return lad, np.array(d64), np.array(d32), np.array(und), cross


@pytest.mark.parametrize("variant,S,VS", cc.WIDTHS, ids=[cc.wid(*w) for w in cc.WIDTHS])
def test_alpha_off_axis_ladder(variant, S, VS):
    lad, d64, d32, und, cross = off_axis_host(variant, S, VS)
    assert cross == np.float32(0.0055833375)
    assert np.array_equal(d32[~und], d64[~und])
    assert set(d64) == {0, 1} and (np.diff(d64) >= 0).all() and (np.diff(d32) >= 0).all()     # monotone, one switch each
    assert 1 <= und.sum() <= 9
    iu = np.nonzero(und)[0]
    assert np.array_equal(iu, np.arange(iu[0], iu[-1] + 1))                                   # one block ...
    for d in (d64, d32):
        sw = int(np.argmax(d))
        assert iu[0] <= sw <= iu[-1] + 1 and d[sw] == 1 and (sw == 0 or d[sw - 1] == 0)        # ... around the crossing
    assert np.argmax(d64) == np.argmax(d32)       # (here both switch on the same step; the GPU may fall either way inside the block)


# ---- values -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,variant,S,VS", cc.VALUE_TABLE, ids=VALUE_IDS)
def test_closed_form_is_the_fp64_oracle(name, variant, S, VS):
    v, cf, o32, E32, E32c = cc.value_host(name, variant, S, VS)
    sc, ch = v["sc"], v["chain"]
    x, y = sc["axis"]
    o64 = cc.oracle_run(sc, variant, fp64=True, up=cc.upstream(sc, variant))
    assert int(o64["n_contrib"][y, x]) == ch["n_contrib"]          # fp64 blends the set fp32 blends
    for k, ref in (("dop", cf["dop"]), ("dcolor", cf["dcolor"])):
        d = float(np.abs(o64[k] - ref).max() / np.abs(ref).max())
        print(f"{name}: fp64 oracle vs closed form, {k}: {d:.2e}")
        assert d <= 1e-12
    assert np.abs(o64["color"][:, y, x] - cf["color"]).max() <= 1e-12
    p = ch["passed"]
    assert (o64["dop"][~p] == 0).all() and (o64["dcolor"][~p] == 0).all()
    # every blended candidate's gradient is an observation
    assert (np.abs(cf["dop"])[p] >= 1e-3 * cf["A"][p]).all() and (cf["w"][p] > 0).all()


@pytest.mark.parametrize("name,variant,S,VS", cc.VALUE_TABLE, ids=VALUE_IDS)
def test_the_fp32_reference_loses_less_than_32_eps(name, variant, S, VS):
    v, cf, o32, E32, E32c = cc.value_host(name, variant, S, VS)
    print(f"{name}: E32 = {E32 / cc.EPS32:.1f} eps32 (dL_dopacity / A_k), E32c = {E32c / cc.EPS32:.1f} eps32 (dL_dcolors / w_k |g|)")
    assert E32 < 2.0 ** -19 and E32c < 2.0 ** -19
    p = v["chain"]["passed"]
    assert (o32["dop"][~p] == 0).all() and (o32["dop"][p] != 0).all()


def test_deep_lists_hold_what_they_claim():
    for (n, a), last, all_pixels in zip(cc.DEEP, (200, 1024, 584), (True, True, False)):
        v, cf, o32, _, _ = cc.value_host(f"deep{n}", "rgss", 5, 0)
        assert v["chain"]["n_contrib"] == last and len(v["op"]) == n and (v["op"] == np.float32(a)).all()
        assert o32["blended"].all() or not all_pixels
        if all_pixels:
            assert (o32["n_contrib"] == n).all()      # every candidate blends on every pixel: every sub-tile walks the whole list
    v, cf, o32, _, _ = cc.value_host("deep1024", "rgss", 5, 0)
    assert abs(cf["T_final"] - 3.3e-4) < 1e-5
    v = cc.build("deep_mixed", "rgss", 5, 0)[0]
    assert len(v["op"]) == cc.MIXED_N and not v["chain"]["passed"][list(cc.MIXED_FAINT)].any()
    assert (v["op"][list(cc.MIXED_FAINT)].view(np.int32) == cc.ALPHA_MIN.view(np.int32) - 1).all()
    assert v["chain"]["n_contrib"] > 129 and v["chain"]["passed"][:v["chain"]["n_contrib"]].sum() == v["chain"]["n_contrib"] - 3
