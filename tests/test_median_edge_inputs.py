"""CPU checks of the exact median (csrc/select.hip) and its consumers: the oracle of tests/median_cases.py equals torch.median on every
column case, the table holds what it claims, the consumers' oracles are pinned by the reference's own results (tests/golden/median.npz,
scripts/make_golden_median.py), E32 is measured per albedo case (DESIGN.md quotes it), and the new entry points refuse invalid arguments
before any HIP call.  No GPU work is launched."""
import os
import re

import numpy as np
import pytest
import torch

import median_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "median.npz")
_id = lambda c: c["id"]  # noqa: E731


def _equal_with_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all((a == b) | np.isnan(a)))


# ---- the column table and its oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.COLUMN_CASES, ids=_id)
def test_column_oracle_is_torch_median(case):
    x = mc.column_data(case)
    val, idx, less, greater = mc.column_reference(case)
    n, C = x.shape
    assert val.dtype == np.float32 and val.shape == (C,)
    if n == 0:   # torch raises; the library's decision is NaN, -1, 0, 0
        assert np.isnan(val).all() and (idx == -1).all() and not less.any() and not greater.any()
        return
    view = mc.column_view(case, torch.from_numpy)
    assert tuple(view.shape) == (n, C) and np.array_equal(view.numpy(), x, equal_nan=True)
    tv, ti = torch.median(view, dim=0)
    assert _equal_with_nan(val, tv.numpy()), (val, tv)
    for c in range(C):
        for i in (int(idx[c]), int(ti[c])):   # either index points at a row holding the value
            assert x[i, c] == val[c] or (np.isnan(x[i, c]) and np.isnan(val[c]))
        assert not np.signbit(val[c]) or val[c] != 0            # a zero comes out as +0
        nan = int(np.isnan(x[:, c]).sum())
        if nan:
            assert np.isnan(val[c]) and idx[c] == np.flatnonzero(np.isnan(x[:, c]))[0] and less[c] == n - nan and greater[c] == 0
        else:
            assert less[c] == (x[:, c] < val[c]).sum() and greater[c] == (x[:, c] > val[c]).sum()
            assert less[c] <= (n - 1) // 2 < n - greater[c]
            assert idx[c] == np.flatnonzero(x[:, c] == val[c])[0]


def test_column_table_holds_what_it_claims():
    T = mc.T
    by = {c["id"]: c for c in mc.COLUMN_CASES}
    assert len(by) == len(mc.COLUMN_CASES)
    sizes = {c["n"] for c in mc.COLUMN_CASES if c["kind"] == "generic" and c["layout"] == "rows" and c["C"] == 3}
    assert sizes == {1, 2, 3, 4, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1}
    assert {(c["layout"], c["C"]) for c in mc.COLUMN_CASES} >= {("rows", 3), ("planar", 3), ("rows", 1), ("rows", 4), ("sliced", 3)}
    wide = mc.column_data(by["wide-70001-rows"])
    assert wide.shape[0] > 65535 and (wide == wide[0]).all()
    asc = mc.column_data(by["ascending-257-rows"])
    assert (np.diff(asc[:, 0]) >= 0).all() and (np.diff(asc[:, 1]) <= 0).all()
    for n in (6, 7, 128, 129):        # the rank on either side of the boundary between the two values, in both orders
        x, (val, idx, _, _) = mc.column_data(by[f"ties-{n}-rows"]), mc.column_reference(by[f"ties-{n}-rows"])
        m = n // 2
        assert (x[:m, 0] == 1.5).all() and (x[m:, 0] == 2.5).all() and (x[:m, 1] == 2.5).all()
        assert list(val[:2]) == ([1.5, 1.5] if n % 2 == 0 else [2.5, 1.5]) and list(idx[:2]) == ([0, m] if n % 2 == 0 else [m, m])
    lo, hi = (mc.column_data(by[f"{k}-300-rows"]).view(np.uint32) for k in ("lowdigit", "highdigit"))
    assert len(np.unique(lo & 0x7FFFFF00)) == 1 and len(np.unique(lo[:, 0] & 0xFF)) > 100
    assert len(np.unique(hi & 0x00FFFFFF)) == 1 and len(np.unique(hi[:, 0] >> 24)) > 100 and np.isfinite(hi.view(np.float32)).all()
    assert (mc.column_data(by["negatives-300-rows"]) < 0).all()
    val = mc.column_reference(by["signmix-300-rows"])[0]
    assert val[0] < 0 < val[1]
    den = mc.column_data(by["denormals-300-rows"])
    assert (np.abs(den) < np.finfo(np.float32).tiny).all() and (den != 0).all()
    z, (val, _, _, _) = mc.column_data(by["zeros-300-rows"]), mc.column_reference(by["zeros-300-rows"])
    assert (val == 0).all() and not np.signbit(val).any() and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    assert np.signbit(z[:, 1][z[:, 1] == 0]).all()                       # a column whose every zero is -0 still gives +0
    val = mc.column_reference(by["inf-300-rows"])[0]
    assert val[0] == np.inf and val[1] == -np.inf and np.isfinite(val[2]) and np.isinf(mc.column_data(by["inf-300-rows"])[:, 2]).sum() == 11
    one = mc.column_data(by["nan_one-300-rows"])
    assert np.isnan(one).sum() == 1 and np.isnan(mc.column_reference(by["nan_one-300-rows"])[0]).tolist() == [False, True, False]
    assert np.isnan(mc.column_data(by["nan_all-300-rows"])[:, 0]).all() and mc.column_reference(by["nan_all-300-rows"])[1][1] == 5
    hot = mc.column_data(by["hot_inside-5000-rows"])
    assert ((hot == 10.0).mean(axis=0)[[0, 2]] >= 0.99).all() and (hot[:, 0] < 10).any() and (hot[:, 0] > 10).any()
    assert list(mc.column_reference(by["hot_inside-5000-rows"])[0]) == [10.0, np.float32(1e-6), 10.0]
    for n in (5000, 4999):            # the hot value holds every row short of the rank: the median is its fp32 neighbour
        x, (val, _, less, greater) = mc.column_data(by[f"hot_outside-{n}-rows"]), mc.column_reference(by[f"hot_outside-{n}-rows"])
        k = (n - 1) // 2
        assert val[0] == np.nextafter(np.float32(10), np.float32(11)) and less[0] == k == (x[:, 0] == 10).sum()
        assert val[1] == np.nextafter(np.float32(10), np.float32(9)) and greater[1] == n - k - 1 == (x[:, 1] == 10).sum()
    sl = mc.column_view(by["generic-300-sliced"], torch.from_numpy)
    assert not sl.is_contiguous() and sl.stride() == (5, 1) and torch.isnan(sl._base).sum() == sl._base.numel() - sl.numel()
    pl = mc.column_view(by["generic-300-planar"], torch.from_numpy)
    assert pl.stride() == (1, 300)


def test_rows_per_workgroup_is_the_kernels():
    """metrics.SELECT_ROWS, which the table's sizes are built around, is the constant of csrc/select.hip."""
    from svgir_harness import metrics
    src = open(os.path.join(ROOT, "svg-ir_amd", "csrc", "select.hip")).read()
    per = int(re.search(r"constexpr int SEL_PER_THREAD = (\d+);", src).group(1))
    assert re.search(r"constexpr int SEL_ROWS = BLOCK \* SEL_PER_THREAD;", src)
    block = int(re.search(r"constexpr int BLOCK = (\d+);", open(os.path.join(ROOT, "svg-ir_amd", "csrc", "common.hpp")).read()).group(1))
    assert metrics.SELECT_ROWS == mc.T == block * per


# ---- the consumers' oracles against the reference's own results --------------------------------------------------------------------------
def test_srgb_to_rgb_oracle_is_the_references():
    g = np.load(GOLD)
    k = mc.KNEE
    lad = torch.from_numpy(np.resize(mc.knee_ladder(), 36).reshape(3, 2, 6))
    np.testing.assert_allclose(mc.srgb_to_rgb(lad).numpy(), g["knee_ladder_32"], rtol=2e-7, atol=0)
    np.testing.assert_allclose(mc.srgb_to_rgb(lad.double()).numpy(), g["knee_ladder_64"], rtol=1e-14, atol=0)
    lin = g["knee_ladder_32"].reshape(-1)[:12]
    assert lin[3] == np.nextafter(k, np.float32(0)) / np.float32(12.92) and lin[4] == k / np.float32(12.92)   # the knee itself is linear
    assert lin[5] > lin[4] and lin[1] == 0 and lin[0] < 0


@pytest.mark.parametrize("cid", mc.GOLDEN_ALBEDO)
def test_albedo_oracle_is_the_references(cid):
    g = np.load(GOLD)
    ref = mc.albedo_reference(next(c for c in mc.ALBEDO_CASES if c["id"] == cid))
    assert ref["count"] == int(g[f"albedo.{cid}.count32"]) == int(g[f"albedo.{cid}.count64"])
    s32, s64 = g[f"albedo.{cid}.scale32"], g[f"albedo.{cid}.scale64"]
    assert np.array_equal(np.isnan(ref["scale32"]), np.isnan(s32)) and np.array_equal(np.isnan(ref["scale64"]), np.isnan(s64))
    np.testing.assert_allclose(ref["scale32"], s32, rtol=2e-7, atol=0)     # (pow may differ by an ulp between two builds of torch)
    np.testing.assert_allclose(ref["scale64"], s64, rtol=1e-14, atol=0)


@pytest.mark.parametrize("cid", mc.GOLDEN_LOSS)
def test_loss_oracle_is_the_references(cid):
    g = np.load(GOLD)
    case = next(c for c in mc.LOSS_CASES if c["id"] == cid)
    ref = mc.loss_reference(case)
    l64, g64 = float(g[f"loss.{cid}.loss64"]), g[f"loss.{cid}.grad64"]
    if np.isnan(l64):
        assert np.isnan(ref["loss64"]) and np.isnan(ref["grad"]).all() and np.isnan(g64).all() and np.isnan(float(g[f"loss.{cid}.loss32"]))
        return
    assert abs(ref["loss64"] - l64) <= 1e-13 * l64 and abs(ref["torch64"] - l64) <= 1e-13 * l64
    assert abs(float(g[f"loss.{cid}.loss32"]) - l64) <= max(4 * ref["e32"], 4 * mc.EPS32) * l64
    # torch hands the gradient of `center` to the row its median returned, the oracle to the smallest such row: equal after summing,
    # per column, over the rows that hold the median value; every other element equal as it is
    held, tol = ref["held"], 1e-12 * abs(ref["coef"])
    assert (np.abs(np.where(held, 0.0, ref["grad"] - g64)) <= tol).all()
    assert (np.abs(mc.tie_sum(ref["grad"], held) - mc.tie_sum(g64, held)) <= tol * held.sum(axis=0)).all()
    assert held.sum(axis=0).min() >= 1 and (held.sum(axis=0).max() > 1) == case["ties"]


# ---- the albedo table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.ALBEDO_CASES, ids=_id)
def test_albedo_cases_hold_what_they_claim(case, record_property):
    r, g = mc.build_albedo(case)
    ref = mc.albedo_reference(case)
    H, W = case["H"], case["W"]
    assert r.shape == g.shape == (3, H, W) and r.dtype == g.dtype == np.float32
    # every selected mean is >= 1e-3 in magnitude, every other pixel is exactly zero in all channels (the linear branch gives 0 exactly)
    lin = mc.srgb_to_rgb(torch.from_numpy(r).double()).numpy() if case["srgb"] else r.astype(np.float64)
    mean = lin.mean(axis=0)
    small = np.abs(mean) < 1e-3
    assert (r[:, small] == 0).all() and (mean[small] == 0).all()
    assert np.array_equal(ref["mask32"], ref["mask64"]) and np.array_equal(ref["mask64"], mean > 0) and ref["count"] == int((mean > 0).sum())
    assert {"empty": ref["count"] == 0, "all": ref["count"] == H * W, "partial": 0 < ref["count"] < H * W}[case["sel"]]
    q32 = ref["q32"]
    if case["special"] in (True, "nan"):
        assert (q32 == np.float32(mc.HI)).any() and (q32 == np.float32(mc.LO)).any()
        sel = ref["mask64"].reshape(-1)
        rr, gg = r.reshape(3, -1)[:, sel], g.reshape(3, -1)[:, sel]
        assert ((rr[0] == 0) & (gg[0] > 0)).any() and (rr[1] < 0).any() and (gg[0] < 0).any()          # x / 0, negative ratios
        if not case["srgb"]:
            exact = gg[2].astype(np.float64) / rr[2].astype(np.float64)
            assert (exact == 10.0).any() and (exact == float(np.float32(mc.LO))).any()                   # ratios on hi and on lo exactly
        nan_px = (rr[0] == 0) & (gg[0] == 0)
        assert nan_px.sum() == (1 if case["special"] == "nan" else 0)
        assert np.isnan(ref["scale64"]).tolist() == [case["special"] == "nan", False, False] == np.isnan(ref["scale32"]).tolist()
    elif case["special"] == "knee":
        k = np.float32(0.04045)
        for v in (np.nextafter(k, np.float32(0)), k, np.nextafter(k, np.float32(1))):
            assert ((r == v).all(axis=0) & ref["mask64"]).any()
    elif ref["count"]:
        assert not np.isnan(ref["scale64"]).any()
    # E32: what the reference's fp32 lines lose against fp64 on the selected ratios
    record_property("E32", ref["e32"])
    assert ref["e32"] <= (1e-6 if case["srgb"] else mc.EPS32 / 2 + 1e-12)
    ok = ~np.isnan(ref["scale64"])
    assert (np.abs(ref["scale32"][ok] - ref["scale64"][ok]) <= max(ref["e32"], 1e-30) * np.abs(ref["scale64"][ok])).all()   # monotone


def test_loss_table_holds_what_it_claims():
    assert {c["P"] for c in mc.LOSS_CASES} == {1, 2, 3, 257, 70001}
    for case in mc.LOSS_CASES:
        x, ref = mc.build_loss(case), mc.loss_reference(case)
        assert x.shape == (case["P"], 3)
        if case["shape"] in ("cloud", "nan"):
            assert all(len(np.unique(x[:, c][~np.isnan(x[:, c])])) == (~np.isnan(x[:, c])).sum() for c in range(3))
        if case["shape"] == "equal" or case["P"] == 1:
            assert ref["loss64"] == 1.0 and ref["sum32"] == 0.0
        if case["shape"] == "nan":
            assert np.isnan(x).sum() == 1 and np.isnan(ref["loss64"]) and np.isnan(ref["grad"]).all()
        if case["shape"] == "cube":
            assert (np.abs(x - 1e6) <= 1).all() and ref["held"].sum(axis=0).min() > 1
        if case["ties"] and case["P"] > 3:
            assert ref["held"].sum(axis=0).max() > 1
        if not np.isnan(ref["loss64"]):   # the fp32 subtraction the kernel makes costs less than the tolerance
            assert abs(np.exp(-ref["sum32"] / (3 * case["P"])) - ref["loss64"]) <= mc.EPS32 * ref["loss64"]
            assert ref["e32"] <= 1e-6


# ---- arguments and exports -----------------------------------------------------------------------------------------------------------------
NEW = ("svgir_column_median_scratch_bytes", "svgir_column_median", "svgir_albedo_scale_median_scratch_bytes", "svgir_albedo_scale_median",
       "svgir_surface_center_loss_partials", "svgir_surface_center_loss_forward", "svgir_surface_center_loss_backward")


def test_new_symbols_are_declared_and_exported(built):
    from gaussian_renderer import _native as N
    hdr = open(os.path.join(ROOT, "include", "svgir_raster.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr) and name in N.EXPORTS and hasattr(N.lib, name), name
    assert N.lib.svgir_abi_version() == 14


def test_invalid_arguments_are_refused_before_any_launch(built):
    from gaussian_renderer import _native as N
    lib, bad = N.lib, 16   # (a non-NULL pointer that is never dereferenced: every call below returns before its first HIP call)
    words = lib.svgir_column_median_scratch_bytes(1000, 3)
    assert words > 0 and words == lib.svgir_column_median_scratch_bytes(2 ** 31 - 1, 1) == lib.svgir_albedo_scale_median_scratch_bytes(800, 800)
    assert lib.svgir_column_median_scratch_bytes(-1, 3) == 0 and lib.svgir_column_median_scratch_bytes(2 ** 31, 3) == 0
    assert lib.svgir_column_median_scratch_bytes(10, 0) == 0 and lib.svgir_column_median_scratch_bytes(10, 5) == 0
    for C in (0, 5, -1):
        assert lib.svgir_column_median(bad, 10, C, 3, 1, bad, bad, bad, bad, bad, None) == -1 and "columns per call" in N.last_error()
    for n in (-1, 2 ** 31, 2 ** 40):
        assert lib.svgir_column_median(bad, n, 3, 3, 1, bad, bad, bad, bad, bad, None) == -1 and "outside" in N.last_error()
    for args in ((None, 10, 3, 3, 1, bad, bad, bad), (bad, 10, 3, 3, 1, None, bad, bad), (bad, 10, 3, 3, 1, bad, None, bad),
                 (bad, 10, 3, 3, 1, bad, bad, None)):
        assert lib.svgir_column_median(*args, None, None, None) == -1 and "must be provided" in N.last_error()
    for W, H in ((0, 3), (3, 0), (-4, 4)):
        assert lib.svgir_albedo_scale_median(W, H, bad, bad, 1, 1e-6, 10.0, bad, bad, bad, None) == -1 and "bad image size" in N.last_error()
    assert lib.svgir_albedo_scale_median(65536, 32768, bad, bad, 1, 1e-6, 10.0, bad, bad, bad, None) == -1 and "exceeds" in N.last_error()
    assert lib.svgir_albedo_scale_median_scratch_bytes(65536, 32768) == 0 and lib.svgir_albedo_scale_median_scratch_bytes(0, 4) == 0
    for lo, hi in ((10.0, 1e-6), (float("nan"), 1.0), (0.0, float("nan"))):
        assert lib.svgir_albedo_scale_median(4, 3, bad, bad, 1, lo, hi, bad, bad, bad, None) == -1 and "lo <= hi" in N.last_error()
    for k in range(5):
        ptrs = [bad] * 5
        ptrs[k] = None
        assert lib.svgir_albedo_scale_median(4, 3, ptrs[0], ptrs[1], 0, 1e-6, 10.0, ptrs[2], ptrs[3], ptrs[4], None) == -1
        assert "must be provided" in N.last_error()
    assert lib.svgir_surface_center_loss_partials(-1) == 0 and lib.svgir_surface_center_loss_partials(2 ** 31) == 0
    base = lib.svgir_surface_center_loss_partials(0)
    assert base * 8 == words and lib.svgir_surface_center_loss_partials(mc.T) == base + 1 and lib.svgir_surface_center_loss_partials(mc.T + 1) == base + 2
    for P in (-1, 2 ** 31):
        assert lib.svgir_surface_center_loss_forward(P, bad, bad, bad, bad, None) == -1 and "outside" in N.last_error()
        assert lib.svgir_surface_center_loss_backward(P, bad, bad, bad, bad, None) == -1 and "outside" in N.last_error()
    for args in ((None, bad, bad, bad), (bad, None, bad, bad), (bad, bad, None, bad), (bad, bad, bad, None)):
        assert lib.svgir_surface_center_loss_forward(10, *args, None) == -1 and "must be provided" in N.last_error()
        assert lib.svgir_surface_center_loss_backward(10, *args, None) == -1 and "must be provided" in N.last_error()


def test_python_surface_refuses_what_the_kernels_do_not_take(built):
    from svgir_harness import losses, metrics
    x = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.column_median(x)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        metrics.albedo_scale_median(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        losses.surface_center_loss(x)
    assert callable(losses.surface_loss) and callable(metrics.albedo_scale)   # the existing names keep their meaning
