"""The tracer case table (tests/tracer_cases.py) proved on the CPU oracles alone: every case holds what it is named for, exercises both
outcomes, keeps its threshold rays under 1 %, and its recorded tolerance covers what the oracles themselves lose.  Run with -s to see the
occupancy, query-count and threshold-share figures of every case.

Why every loop these inputs reach on the GPU is bounded (csrc/bvh.hip, csrc/pbgi.hip), whatever the floats are:
  * Morton codes: NaN and +-inf go through fminf(fmaxf(x, 0), 1023) -> an integer cell; the radix sort and both hierarchy kernels are
    integer-only (keys made unique by the surfel index / the sorted position), their searches are bounded by P;
  * refit: both walks follow integer parent links for at most 128 steps (`guard`), NaN boxes only flow through fminf / fmaxf;
  * traversal: a push is refused at 64 entries (`sp < BVH_STACK`, `count < PBGI_STACK`) and every iteration pops one entry or descends
    one level of a finite tree; a NaN slab result fails `tmax > 0` / `ex > t_min`, i.e. prunes;
  * pbgi ray loop: at most PBGI_MAX_HITS = 4096 queries per ray (`it < PBGI_MAX_HITS`); a NaN transmittance fails `T > 0.001f`;
  * scheduler: the queue is an integer counter that only grows; a wave stops after it has found all eight parts empty.
coincident / zero_extent / zero_quaternion / zero_scale_axis / far_coordinates / bad_directions only change floats: none of them reaches
a loop whose trip count depends on a float.  deep_stack peaks at 38 (visibility) and 30 + (radiance) of the 64 entries.  Every case runs
through the CPU oracle here before tests/test_gpu_tracer_edges.py gives it to a GPU.
"""
import numpy as np
import pytest

from oracle import bvh_oracle as bo
from oracle import pbgi_oracle as po
from tests import tracer_cases as tc

F32 = np.float32


def _disagree(e):
    return (e["contribute"] != e["contribute64"]) | ((e["visibility"] > 0) != (e["visibility64"] > 0))


# ---- visibility tracer -------------------------------------------------------------------------------------------------------------------
def test_visibility_margin_bound():
    """m = the smallest margin at which the fp32 and the fp64 oracle agree on `contribute` and blocked / open for every ray above it."""
    worst, where = 0.0, None
    for name in tc.VIS:
        if "exact" in tc.VIS[name]():
            continue
        e = tc.vis_expected(name)
        dis = _disagree(e)
        if dis.any() and e["margin"][dis].max() > worst:
            worst, where = float(e["margin"][dis].max()), name
    print(f"measured m = {worst:.3e} ({where}); recorded {tc.VIS_M_MEASURED:.3e}; rule: margin < {tc.VIS_MARGIN:.3e}")
    assert worst <= tc.VIS_M_MEASURED
    assert tc.VIS_M == max(tc.VIS_M_MEASURED, 2.0 ** -23) and tc.VIS_MARGIN == 4 * tc.VIS_M


@pytest.mark.parametrize("name", list(tc.VIS))
def test_visibility_case(name):
    c, e = tc.VIS[name](), tc.vis_expected(name)
    n = e["contribute"].size
    assert c["rays_o"].shape == c["rays_d"].shape == (n, 3)
    share = e["threshold"].mean()
    ok = ~e["threshold"] & np.isfinite(e["visibility"]) & np.isfinite(e["visibility64"])
    diff = float(np.abs(e["visibility"][ok] - e["visibility64"][ok]).max()) if ok.any() else 0.0
    print(f"{name}: {n} rays, threshold share {share:.4f}, fp32-vs-fp64 oracle difference {diff:.2e}, tol {c['tol']:.1e} ({c['tol_source']})")
    assert share <= tc.MAX_THRESHOLD_SHARE
    keep = ~e["threshold"]
    assert np.array_equal(e["contribute"][keep], e["contribute64"][keep])
    assert np.array_equal(e["visibility"][keep] > 0, e["visibility64"][keep] > 0)
    assert np.array_equal(np.isnan(e["visibility"]), np.isnan(e["visibility64"]))
    if c["tol"] == tc.VIS_TOL:
        assert diff <= tc.VIS_TOL                          # the existing tolerance is borne out
    else:
        assert 2 * diff <= c["tol"] <= 10 * tc.VIS_TOL
    if "exact" in c:                                       # decided by exact arithmetic: both precisions give the stated outcome bit for bit
        assert not e["threshold"].any()
        for cnt, vis in ((e["contribute"], e["visibility"]), (e["contribute64"], e["visibility64"])):
            assert np.array_equal(cnt, c["exact"]["contribute"])
            assert np.array_equal(vis, c["exact"]["visibility"])
    if "min_peak" in c:
        peak, leaves = tc.vis_peak_stack(c, c["deep_ray"])
        print(f"{name}: ray {c['deep_ray']} holds up to {peak} pending entries, reaches {leaves} leaves, contribute {e['contribute'][c['deep_ray']]}")
        assert peak >= c["min_peak"] and peak <= 64
        assert e["contribute"][c["deep_ray"]] == (c["opacity"] > 0).sum() == leaves - 2      # every leaf but the two anchors counts
        assert e["visibility"][c["deep_ray"]] == 1.0
    if "nan_box" in c:
        boxes = bo.leaf_boxes(c["means"], c["scales"], c["rots"])
        assert np.isnan(boxes[c["nan_box"]]).all() and np.isfinite(np.delete(boxes, c["nan_box"], axis=0)).all()
    if "bad_rays" in c:
        bad = np.zeros(n, dtype=bool)
        bad[list(c["bad_rays"])] = True
        assert np.isfinite(e["visibility"][~bad]).all() and np.isnan(e["visibility"][list(c["bad_rays"])]).any()
    if "layout" in c:
        code = tc.vis_morton(bo.leaf_boxes(c["means"], c["scales"], c["rots"]))
        if c["layout"] == "low6":
            assert (code >= 64).sum() == 1 and len(np.unique(code)) > 32             # the anchor alone above the low 6 bits
        else:
            # every digit of the 8 + 8 + 8 + 6 plan is busy (1 023 keys cannot fill all 256 bins of a digit: 200 of them)
            assert all(len(np.unique((code >> np.uint64(s)) & np.uint64(0xFF))) > 200 for s in (0, 8, 16)) and len(np.unique(code >> np.uint64(24))) == 64


def test_visibility_groups_exercise_both_outcomes():
    groups = {}
    for name in tc.VIS:
        g = name if name.startswith(("deep", "degenerate", "sort")) else name.split("_")[0]      # exact, wave: one group each
        e = tc.vis_expected(name)
        s = groups.setdefault(g, dict(count=set(), open=set()))
        s["count"] |= set((e["contribute"] > 0).tolist())
        s["open"] |= set((e["visibility"][np.isfinite(e["visibility"])] > 0).tolist())
    for g, s in groups.items():
        if g == "degenerate_zero_extent":                  # zero-volume boxes: nothing can count
            assert s["count"] == {False}
            continue
        assert s["count"] == {False, True}, g
        if g != "deep_stack":                              # (its contributions are negligible on purpose: never cut off)
            assert s["open"] == {False, True}, g


def test_wave_tails_share_their_rays():
    full = tc.VIS["wave_tails_129"]()
    for n in tc.WAVE_TAILS:
        c = tc.VIS[f"wave_tails_{n}"]()
        assert c["rays_d"].shape[0] == n and np.array_equal(c["rays_d"], full["rays_d"][:n]) and np.array_equal(c["rays_o"], full["rays_o"][:n])


def test_caterpillar_codes():
    """Surfel k of the visibility deep_stack has exactly k leading ones in the 30-bit code the KERNEL's fp32 operations give it."""
    c = tc.VIS["deep_stack"]()
    ones = tc.leading_ones30(tc.vis_morton(bo.leaf_boxes(c["means"], c["scales"], c["rots"])))
    assert ones[:30].tolist() == list(range(30)) and (ones[30:30 + tc.DEEP_CLUSTER] == 30).all() and ones[-2:].tolist() == [0, 30]


# ---- radiance tracer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.RAD))
def test_radiance_case(name):
    c, e = tc.RAD[name](), tc.rad_expected(name)
    N, S, P = c["ray_o"].shape[0], c["S"], c["xyz"].shape[0]
    assert c["ray_d"].shape == (N, S, 3)
    hit = e["hit"][..., 0]
    share = e["threshold"].mean()
    print(f"{name}: P {P}, {N} x {S} rays, threshold share {share:.5f}, most queries {e['queries'].max()}, hits {(hit >= 0).mean():.3f}")
    assert share <= tc.MAX_THRESHOLD_SHARE
    assert np.isfinite(e["radiance"]).all() and np.isfinite(e["visibility"]).all()
    if "exact" in c:
        x = c["exact"]
        assert not e["threshold"].any()
        assert hit[x["row"]].tolist() == x["hit"]
        if x["visibility"] is not None:
            assert np.array_equal(e["visibility"][x["row"], :, 0], np.asarray(x["visibility"], dtype=F32))
        if "third_asked" in x:
            assert e["queries"][x["row"], 0] == (3 if x["third_asked"] else 2)
    elif not name.startswith("sample_counts"):
        assert (hit >= 0).any() and (hit < 0).any()        # both outcomes (sample_counts: as a group, see below)
    if "min_peak" in c:
        info, aabb, srt = po.build(c["xyz"], c["scales"])
        r, j = c["deep_ray"]
        pending, fixed = tc.rad_descent_stack(info, aabb, c["ray_o"][r], c["ray_d"][r, j])
        print(f"{name}: ray {j} of row {r} holds {pending} pending entries at its first leaf (fixed: {fixed})")
        assert pending >= c["min_peak"] and pending < 64 and fixed == c["fixed"]
        assert sorted(tc.leading_ones30(srt[:, 0].astype(np.uint32)).tolist()) == sorted(list(range(31)) + [3])   # the anchor shares code 3
    if "fixed" in c:
        assert tc.is_fixed(c["ray_d"]).all() if c["fixed"] else tc.stays_unfixed(c["ray_d"]).all()
    if "long_ray" in c:
        r, j = c["long_ray"]
        others = np.delete(e["queries"][r], j)
        print(f"{name}: the long ray takes {e['queries'][r, j]} queries, the other rays of its chunk at most {others.max()}")
        assert e["queries"][r, j] >= tc.LONG_RAY_MIN_QUERIES and others.max() == 1
        base, moved = tc.rad_reference(c), 0.0
        for ulp in (1, -1):
            sh = tc.rad_reference(c, exp_ulp=ulp)
            assert np.array_equal(sh[2], base[2])
            moved = max(moved, max(float(np.abs(a - b).max()) for a, b in zip((base[0], base[1], base[3]), (sh[0], sh[1], sh[3]))))
        print(f"{name}: a +-1 ulp expf moves the oracle's outputs by at most {moved:.2e}")
        assert 4 * moved <= c["tol"] == tc.RAD_TOL         # the existing tolerance is borne out
    if "sched" in c:
        assert c["sched"] == tc.rad_chunks(N, S)
        assert c["sched"]["nchunks"] * c["sched"]["chunk"] >= N * S > (c["sched"]["nchunks"] - 1) * c["sched"]["chunk"]
    if name == "queue_refill":
        assert c["sched"]["nchunks"] > tc.RESIDENT_SLOTS == 4096 and N * S == 268800
    if name == "more_rows_than_surfels":
        P = c["P"]
        assert N == 2 * P + 3
        own, other = hit[:P, 0], hit[P:2 * P, 0]
        kept = other == np.arange(P)                        # row P + r meets surfel r first and keeps it ...
        assert kept.sum() >= 20 and (own[kept] == -1).all()    # ... the same ray in row r meets its own surfel: rejected, the ray ends
        print(f"{name}: {kept.sum()} of {P} rows r >= P hit surfel r - P; the same rays in rows r < P end at their own surfel")
    if name.startswith("tiny_trees"):
        assert N == 5 and P == int(name[-1]) and not any(np.array_equal(o, x) for o in c["ray_o"] for x in c["xyz"])


def test_sample_counts_cover_few_and_many_chunks():
    n = [tc.SAMPLE_COUNTS[S]["nchunks"] for S in tc.SAMPLE_COUNTS]
    assert min(n) < 8 <= max(n) and set(tc.SAMPLE_COUNTS) == {1, 3, 63, 64, 65, 200}
    assert [tc.SAMPLE_COUNTS[S]["empty_parts"] for S in (1, 3, 63)] == [7, 6, 1]
    hits = np.concatenate([tc.rad_expected(f"sample_counts_S{S}")["hit"].reshape(-1) for S in tc.SAMPLE_COUNTS])
    assert (hits >= 0).any() and (hits < 0).any()


@pytest.mark.parametrize("layout", tc.SORT_LAYOUTS)
def test_sort_tree_inputs(layout):
    for P in tc.SORT_SIZES:
        xyz, scales = tc.sort_tree_inputs(P, layout)
        _, _, srt = po.build(xyz, scales)
        code = srt[:, 0].astype(np.uint32)
        assert (np.diff(code.astype(np.int64)) >= 0).all()
        if layout == "low6":
            assert (code >= 64).sum() == 1 and len(np.unique(code)) > 32
        else:
            assert len(np.unique(code >> 24)) == 64 and all(len(np.unique((code >> s) & 0xFF)) > 200 for s in (0, 8, 16))
