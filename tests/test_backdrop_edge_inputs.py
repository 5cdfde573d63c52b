"""CPU half of the environment-backdrop tests (csrc/backdrop.hip; the GPU half is tests/test_gpu_backdrop.py): pins the oracle of
tests/backdrop_cases.py against what the reference's own eval `render_view` recorded, proves that the table contains what it claims
(unsaturated backdrops, the pole and seam pixels where intended and nowhere else), measures the reference's own fp32 error E32, and
checks the C ABI of svgir_env_backdrop without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import backdrop_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = bc.cases()


# ---- the oracle is pinned ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(bc.fixture_cases())), ids=[c["name"] for c, _ in bc.fixture_cases()])
def test_oracle_matches_the_reference_recordings(idx):
    """The fp64 composition against the reference's render_env, pbr_env and env_only (svgss.py:255-260) at the bounds of
    test_view_fixtures.py; render_view.npz's pbr_env is compared nowhere else."""
    case, exp = bc.fixture_cases()[idx]
    got = bc.oracle64(case)
    for k in bc.OUTPUTS:
        np.testing.assert_allclose(got[k], exp[k], rtol=2e-4, atol=2e-5, err_msg=k)
    # and the fp32 restatement of the reference's operation order agrees with the recording far inside those bounds
    r32 = bc.reference32(case)
    for k in bc.OUTPUTS:
        np.testing.assert_allclose(r32[k], exp[k], rtol=0, atol=2e-6, err_msg=k)


def test_backdrop_fixture_is_not_saturated():
    """render_view.npz's env_only is 1.0 in every pixel (softplus(.) * 2 >= 1): a wrong lookup cannot show there.  backdrop.npz's maps
    keep the backdrop inside (0, 1)."""
    for case, exp in bc.fixture_cases():
        inside = np.mean((exp["env_only"] > 0) & (exp["env_only"] < 1))
        if case["saturates"]:
            assert inside == 0.0
        else:
            assert inside >= 0.8, (case["name"], inside)
            assert np.ptp(exp["env_only"]) > 0.3


# ---- the table holds what it claims ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=bc.case_ids())
def test_table_is_unsaturated_and_its_threshold_pixels_are_where_intended(case):
    o64 = bc.oracle64(case)
    e = o64["env_only"]
    if not case["saturates"]:
        assert np.mean((e > 0) & (e < 1)) >= 0.5
    m = bc.condition_masks(case)
    pole = np.zeros((case["H"], case["W"]), bool)
    if case["pole"]:
        pole[case["pole"]] = True
    assert np.array_equal(m["pole"], pole)
    seam = np.zeros_like(pole)
    if case["seam_row"]:
        row, n = case["seam_row"]
        seam[row, :n] = True
    assert np.array_equal(m["seam"], seam) and seam.sum() <= max(case["H"], case["W"])
    if not case["inf"]:
        assert not m["inf"].any() and np.isfinite(bc.env64(case)[0]).all()
    # the arrays are read-only: a test cannot change what the next one sees
    for k in ("K", "R", "tex", "image", "opacity", "vfeature"):
        assert not case[k].flags.writeable


def test_table_covers_the_listed_shapes_and_inputs():
    shapes = {(c["H"], c["W"]) for c in CASES}
    assert {(1, 1), (1, 53), (37, 1), (37, 53), (40, 56)} <= shapes
    maps = {bc.env64(c)[0].shape[:2] for c in CASES}
    assert {(1, 2), (2, 4), (8, 16), (32, 64), (256, 512)} <= maps
    assert any(c["kind"] == "el" and c["tex"].shape[:2] == (48, 96) for c in CASES) and any(c["T"] is not None for c in CASES)
    by = {c["name"]: c for c in CASES}
    op = by["opacity_and_knee_edges"]["opacity"].reshape(-1)
    for v in (0.0, 1e-6, 1.0 - 1e-6, 1.0):
        assert (op == np.float32(v)).sum() > 50
    assert np.isnan(op).sum() > 50 and np.float32(1e-6) < np.float32(1e-5)
    o64 = bc.oracle64(by["opacity_and_knee_edges"])
    lin = by["opacity_and_knee_edges"]["vfeature"].astype(np.float64)   # (pbr * o, before the backdrop's share is added)
    assert (lin < 0.0031308).mean() > 0.1 and (lin > 1).mean() > 0.05 and ((lin > 0.0031308) & (lin < 1)).mean() > 0.3
    assert (np.isnan(o64["pbr_env"]) == np.isnan(np.broadcast_to(by["opacity_and_knee_edges"]["opacity"], (3, 37, 53)))).all()
    assert not np.isnan(o64["env_only"]).any()
    # the flat map gives one value everywhere; the +inf texel is reached by the view, and a pole sits on the padded row
    assert np.ptp(bc.oracle64(by["flat_env"])["env_only"]) < 1e-12
    tex, softplus, scale = bc.env64(by["inf_texel"])
    assert np.isinf(tex).sum() == 1
    inf_env = bc.oracle64(by["inf_texel"])["env_only"][1]
    assert (inf_env == 1.0).sum() > 20 and (inf_env < 1.0).sum() > 1000
    K = by["principal_point_outside"]["K"]
    assert K[0, 2] < 0 and K[1, 2] > 37
    K = by["principal_point_off_centre_fx_ne_fy"]["K"]
    assert K[0, 0] != K[1, 1]


@pytest.mark.parametrize("name", ["pole_plus_z_2x4", "pole_minus_z_8x16"])
def test_pole_pixel_lies_in_its_rows_range(name):
    """The oracle's own value at the pole obeys the range the GPU test holds the kernel to; at +z one of the two rows is padding."""
    case = next(c for c in CASES if c["name"] == name)
    py, px = case["pole"]
    rng_ = bc.pole_range(case)
    o64 = bc.oracle64(case)
    for k in bc.OUTPUTS:
        lo, hi = rng_[k]
        assert (o64[k][:, py, px] >= lo - 1e-12).all() and (o64[k][:, py, px] <= hi + 1e-12).all(), k
    _, y = bc.tap_coords64(case)
    assert (y[py, px] < 0) == (name == "pole_plus_z_2x4")


# ---- E32: the reference's own fp32 error -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=bc.case_ids())
def test_reference_fp32_error_is_measured_and_reproducible(case):
    o64, r32, e32, bound = bc.shared_oracle(case)
    again = bc.reference32(case)
    meas = bc.measured_mask(case)
    # no direction of the reference's own arithmetic leaves [-1, 1] (where its arccos would be NaN): the clamp changes nothing here
    assert float(bc.lookup_dirs32(case)[:, 2].abs().max()) <= 1.0
    for k in bc.OUTPUTS:
        assert np.array_equal(again[k], r32[k], equal_nan=True)
        a, b = o64[k], r32[k].astype(np.float64)
        ok = meas[None] & np.ones_like(a, bool)
        assert np.array_equal(np.isnan(a)[ok], np.isnan(b)[ok]), k
        fin = np.isfinite(a) & np.isfinite(b) & ok
        assert e32[k] == float(np.abs(a - b)[fin].max())
        scale = max(1.0, float(np.abs(a[np.isfinite(a)]).max()))
        # well-conditioned: a grid coordinate carries ~We eps32 texels of error, times the texel contrast (<= ~1.4 after f)
        assert e32[k] <= 2e-4 * scale, (k, e32[k])
        assert bound[k] == 4.0 * e32[k] + 16.0 * bc.EPS32 * scale
        print(f"{case['name']:40s} {k:10s} E32 = {e32[k]:.3e}  bound = {bound[k]:.3e}")


# ---- the C ABI, without a GPU --------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point(built):
    from gaussian_renderer import _native as N
    hdr = open(os.path.join(ROOT, "include", "svgir_raster.h")).read()
    assert re.search(r"\bint\s+svgir_env_backdrop\s*\(", hdr)
    assert "svgir_env_backdrop" in N.EXPORTS
    lib = C.CDLL(N.LIB_PATH)
    assert hasattr(lib, "svgir_env_backdrop")
    assert lib.svgir_abi_version() == 14 and int(re.search(r"#define SVGIR_ABI_VERSION (\d+)", hdr).group(1)) == 14


def test_invalid_arguments_are_rejected_before_any_hip_call(built):
    from gaussian_renderer import _native as N
    intr = (C.c_float * 4)(50.0, 50.0, 8.0, 8.0)
    rot = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    buf = (C.c_float * 64)()                       # host memory: never dereferenced, every call below fails its checks first
    p = C.cast(buf, C.c_void_p)

    def call(W=16, H=16, intr=intr, rot=rot, env=p, eh=2, ew=4, work=p, image=p, opacity=p, vf=p, out=p):
        return N.lib.svgir_env_backdrop(W, H, intr, rot, None, env, eh, ew, 1, 2.0, work, image, opacity, vf, out, None)

    for kw, msg in ((dict(W=0), "image size"), (dict(H=-3), "image size"), (dict(eh=0), "environment map size"),
                    (dict(ew=-1), "environment map size"), (dict(intr=None), "intrinsics"), (dict(rot=None), "rotation"),
                    (dict(env=None), "environment map"), (dict(work=None), "environment map"), (dict(image=None), "must be provided"),
                    (dict(opacity=None), "must be provided"), (dict(vf=None), "must be provided"), (dict(out=None), "must be provided"),
                    (dict(intr=(C.c_float * 4)(0.0, 50.0, 8.0, 8.0)), "focal"), (dict(intr=(C.c_float * 4)(50.0, float("inf"), 8.0, 8.0)), "focal"),
                    (dict(intr=(C.c_float * 4)(float("nan"), 50.0, 8.0, 8.0)), "focal"),
                    (dict(work=C.c_void_p(p.value + 4)), "16-byte aligned")):
        assert call(**kw) == -1, kw
        assert msg in N.last_error(), (kw, N.last_error())
    with pytest.raises(RuntimeError, match="env_backdrop"):
        N.check(call(W=0), "env_backdrop")


def test_cpu_tensors_fail_loudly_no_fallback(built):
    from svgir_harness import render_view
    case = CASES[0]
    t = lambda k: torch.from_numpy(np.array(case[k]))  # noqa: E731
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        render_view.environment_backdrop(bc.light_of(case), t("K"), t("R"), t("image"), t("opacity"), t("vfeature"))
    el = next(c for c in CASES if c["kind"] == "el")
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        render_view.environment_backdrop(bc.light_of(el), t("K"), t("R"), t("image"), t("opacity"), t("vfeature"))


def test_camera_of_follows_the_reference_formulas(built):
    """scene/cameras.py:116-130 and c2w = inverse of the view matrix, against the reference Camera's own intrinsics / c2w recorded in
    render_view.npz for the same fields of view and view matrix."""
    from svgir_harness import render_view
    g = np.load(os.path.join(bc.GOLD, "render_view.npz"))
    H, W = [int(v) for v in g["cam_hw"]]
    fovx, fovy = g["cam_fov"]
    sc = dict(W=W, H=H, tanfovx=np.tan(fovx * 0.5), tanfovy=np.tan(fovy * 0.5), viewmatrix=torch.from_numpy(g["eval_settings_viewmatrix"]))
    cam = render_view.camera_of(sc)
    np.testing.assert_allclose(cam["intrinsics"].numpy(), g["cam_intrinsics"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(cam["c2w"].numpy(), g["cam_c2w"], rtol=0, atol=2e-6)
