"""The environment backdrop kernel (csrc/backdrop.hip, svgir_harness.render_view.environment_backdrop) on the GPU against the table of
tests/backdrop_cases.py: every element written, values within 4 E32 + 16 eps32 max(1, max |oracle|) of the fp64 oracle (E32 = the error
the reference's own fp32 arithmetic makes on the case), bit-identical on a second run, the reference's recorded arrays at the
fixture bounds, and the wiring into render_svgss_view.  Threshold pixels (seam, pole, taps next to the +inf texel) are held to
conditions instead of values: see backdrop_cases."""
import numpy as np
import pytest
import torch

import backdrop_cases as bc
from svgir_harness import render_view, runner, scenes, shade_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(case):
    dev = torch.device(DEV)
    t = lambda k: torch.from_numpy(np.array(case[k])).to(dev)  # noqa: E731
    res = render_view.environment_backdrop(bc.light_of(case, dev), torch.from_numpy(np.array(case["K"])), torch.from_numpy(np.array(case["R"])),
                                           t("image"), t("opacity"), t("vfeature"))
    assert set(res) == set(bc.OUTPUTS)
    base = res["env_only"].untyped_storage().data_ptr()
    for k in bc.OUTPUTS:   # [3,H,W] views of one buffer, no gradient
        assert res[k].shape == (3, case["H"], case["W"]) and not res[k].requires_grad and res[k].untyped_storage().data_ptr() == base
    return {k: res[k].cpu().numpy() for k in bc.OUTPUTS}


@pytest.mark.parametrize("case", bc.cases(), ids=bc.case_ids())
def test_backdrop_matches_the_oracle(built, case):
    from gaussian_renderer import _native as N
    assert N.POISON   # (conftest: every output buffer is NaN-filled before the call, so an element the kernel skips stays NaN)
    o64, _, e32, bound = bc.shared_oracle(case)
    got = _run(case)
    again = _run(case)
    m = bc.condition_masks(case)
    meas = bc.measured_mask(case)[None]
    alt = {s: bc.oracle64(case, seam=s) for s in (+1, -1)} if m["seam"].any() else None
    for k in bc.OUTPUTS:
        g, ref = got[k].astype(np.float64), o64[k]
        assert np.array_equal(got[k], again[k], equal_nan=True), f"{k}: the second run differs"
        # every element written and non-finite exactly where the oracle is (a NaN opacity; 0 * inf), outside the threshold pixels
        sel = np.broadcast_to(meas, ref.shape)
        assert np.array_equal(np.isnan(g)[sel], np.isnan(ref)[sel]), f"{k}: NaN pattern differs ({np.isnan(g)[sel].sum()} vs {np.isnan(ref)[sel].sum()})"
        fin = sel & np.isfinite(ref)
        err = float(np.abs(g - ref)[fin].max())
        print(f"{case['name']:40s} {k:10s} max err = {err:.3e}  E32 = {e32[k]:.3e}  bound = {bound[k]:.3e}")
        assert err <= bound[k], (k, err, bound[k])
        if m["seam"].any():   # theta = +pi or -pi: either alternative, pixel by pixel
            s = np.broadcast_to(m["seam"][None], ref.shape)
            e = np.minimum(np.abs(g - alt[+1][k]), np.abs(g - alt[-1][k]))[s]
            assert np.isfinite(e).all() and e.max() <= bound[k], (k, "seam", float(e.max()), bound[k])
        if m["pole"].any():   # azimuth undetermined: finite and inside the range of the env rows at that pole
            py, px = case["pole"]
            lo, hi = bc.pole_range(case)[k]
            v = g[:, py, px]
            assert np.isfinite(v).all() and (v >= lo - bound[k]).all() and (v <= hi + bound[k]).all(), (k, "pole", v, lo, hi)
        if m["inf"].any():    # a zero weight may or may not meet the inf texel: finite or not, but written
            s = np.broadcast_to(m["inf"][None], ref.shape) & np.isfinite(g) & np.isfinite(ref)
            assert (np.abs(g - ref)[s] <= bound[k]).all()


@pytest.mark.parametrize("idx", range(len(bc.fixture_cases())), ids=[c["name"] for c, _ in bc.fixture_cases()])
def test_backdrop_matches_the_reference_recordings(built, idx):
    """What the reference's own eval render_view produced (golden/backdrop.npz, golden/render_view.npz), at the fixture bounds."""
    case, exp = bc.fixture_cases()[idx]
    got = _run(case)
    for k in bc.OUTPUTS:
        np.testing.assert_allclose(got[k], exp[k], rtol=2e-4, atol=2e-5, err_msg=k)


def test_render_svgss_view_gains_the_backdrop_with_a_camera(built):
    dev = torch.device(DEV)
    sc = scenes.surface_scene(P=600, W=53, H=37, seed=3, sh_degree=1, variant="svgss", S=7, VS=64, scale_lo=0.03, scale_hi=0.09)
    d = shade_inputs.make(sc["means3D"].shape[0], 8, seed=2)
    sct = runner.to_torch(sc, dev)
    mat = {k: v.to(dev) for k, v in d.items() if k != "env"}
    light = shade_inputs.Light((d["env"] - 4.0).to(dev))
    cam = render_view.camera_of(sct)
    with torch.no_grad():
        plain, _ = render_view.render_svgss_view(sct, mat, light, False)
        res, _ = render_view.render_svgss_view(sct, mat, light, False, camera=cam)
    assert not (set(bc.OUTPUTS) & set(plain)) and set(res) == set(plain) | set(bc.OUTPUTS)
    # the stand-alone call on the rasterizer's raw planes gives the same bits
    out, _ = runner.render(dict(sct, **dict(zip(("features", "vfeatures"), _packed(sct, mat, light)))), "svgss")
    assert torch.equal(out["color"], res["render"]) and torch.equal(out["opacity"], res["opacity"])   # (the rasterizer is deterministic)
    alone = render_view.environment_backdrop(light, cam["intrinsics"], cam["c2w"], out["color"], out["opacity"], out["vfeature"])
    for k in bc.OUTPUTS:
        assert torch.equal(alone[k], res[k]), k
        assert torch.isfinite(res[k]).all() and not res[k].requires_grad
    e = res["env_only"]
    assert float(((e > 0) & (e < 1)).float().mean()) > 0.5 and float(e.max() - e.min()) > 0.05
    # the fused path carries it too
    with torch.no_grad():
        fused, _ = render_view.render_svgss_view(sct, mat, light, False, fused=True, camera=cam)
    assert torch.equal(fused["env_only"], res["env_only"])


def _packed(sct, mat, light):
    from gaussian_renderer import shading
    with torch.no_grad():
        feats, vfeats, _ = shading.shade_and_pack(mat["base_color"], mat["roughness"], mat["normals"], mat["viewdirs"], mat["radiance"], light,
                                                  mat["visibility"], mat["dirs"], mat["areas"], sct["viewmatrix"], False)
    return feats, vfeats


def test_training_view_ignores_the_camera(built):
    dev = torch.device(DEV)
    sc = scenes.surface_scene(P=300, W=40, H=24, seed=4, sh_degree=1, variant="svgss", S=4, VS=52, scale_lo=0.03, scale_hi=0.09)
    d = shade_inputs.make(sc["means3D"].shape[0], 8, seed=2)
    sct = runner.to_torch(sc, dev)
    mat = {k: v.to(dev) for k, v in d.items() if k != "env"}
    with torch.no_grad():
        res, _ = render_view.render_svgss_view(sct, mat, shade_inputs.Light(d["env"].to(dev)), True, camera=render_view.camera_of(sct))
    assert not (set(bc.OUTPUTS) & set(res))
