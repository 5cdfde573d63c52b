"""GPU parity tests: the HIP path (through the C ABI and the drop-in bindings) against the CPU oracle.

Tolerance: north_star asks for 1e-4 relative fp32 agreement.  Integer outputs (num_rendered, radii, n_contrib, the
depth-sorted instance list, the tile ranges) must match EXACTLY.  Float images / gradients are compared two ways
(tests/parity_util.py): normalised, |a-b| <= 1e-4 (max|b| + |b|), and element-wise relative on the entries that carry
signal.  The composite kernels evaluate alpha in exactly the operation order of the reference's source with a ~1 ulp
exp, so the alpha >= 1/255 and T < 1e-4 decisions agree with the oracle's; the measured flip share is 0 on every
BASELINE config (profiles/parity_r02.json), and the tests allow at most FLIP_FRAC isolated outliers, each bounded.
"""
import os
import numpy as np
import pytest
import torch

import parity_util as pu
from oracle import oracle as orc
from svgir_harness import runner, scenes

pytestmark = pytest.mark.gpu

TOL = 1e-4          # normalised tolerance (north_star)
# Budgets 2-10x what profiles/parity_r03.json measures (REL_TOL / REL_FRAC: 2x its p99.99 = 1.1e-3 and share 1.6e-4) on cfg1-cfg5 (0 threshold flips anywhere, worst normalised error 5.2e-5,
# worst share beyond REL_TOL 1.6e-4): a regression that introduces real flips fails.
FLIP_FRAC = 5e-6    # share of forward entries that may exceed TOL (threshold flips), each bounded by FLIP_BOUND * max|ref|
GRAD_FLIP_FRAC = 2e-5
FLIP_BOUND = 0.05
REL_TOL = 2e-3      # element-wise relative tolerance on entries > 1e-3 max|ref| ...
REL_FRAC = 3e-4     # ... for all but this share (differences of nearly cancelling sums)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _cmp(name, a, b, tol=TOL, flip_frac=FLIP_FRAC, flip_bound=FLIP_BOUND, rel=True, rel_frac=REL_FRAC):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    st = pu.stats(a, b, tol=tol, rel_tol=REL_TOL)
    if st["n"] == 0:
        return st
    assert st["finite"], name
    assert st["flip_frac"] <= flip_frac, f"{name}: {st['flip_frac']:.2e} of the entries beyond {tol:g} (max {st['max_norm']:.2e} of scale {st['scale']:.3e})"
    assert st["max_abs"] <= max(flip_bound, tol * 2) * st["scale"], f"{name}: outlier {st['max_abs']:.3e} exceeds the flip bound"
    if rel:
        assert st["rel_frac"] <= rel_frac, f"{name}: {st['rel_frac']:.2e} of the signal-carrying entries beyond {REL_TOL:g} relative (budget {rel_frac:.2e})"
    return st


def _run_both(sc, variant, grads=None):
    dev = _dev()
    var_id = orc.SVGSS if variant == "svgss" else orc.RGSS
    out, leaves = runner.render(runner.to_torch(sc, dev), variant, requires_grad=grads is not None)
    if grads is not None:
        runner.backward(out, grads, variant)
    torch.cuda.synchronize()
    o = orc.OracleRun(sc, var_id)
    R = o.forward()
    if grads is not None:
        o.backward(grads["color"], grads["normal"], grads["depth"], grads["opacity"], grads["feature"], grads.get("vfeature"))
    return out, leaves, o, R


def _check_binning(sc, variant, o, R):
    """Integer state compared directly with the oracle: instance list (a5), tile ranges (a6), last contributors (a7)."""
    _check_binning_raw(runner.forward_raw(runner.to_torch(sc, _dev()), variant), o, R)


def _check_binning_raw(raw, o, R):
    """The same on a forward the caller has run (runner.forward_raw), so that one view can be checked for its images as well."""
    assert raw["num_rendered"] == R
    assert np.array_equal(raw["point_list"], o.get("point_list")[:R]), "depth-sorted instance list differs from the oracle's"
    assert np.array_equal(raw["ranges"].reshape(-1), o.get("ranges").reshape(-1)), "tile ranges differ"
    nc = o.get("n_contrib").reshape(raw["n_contrib"].shape)
    assert (raw["n_contrib"] != nc).mean() <= FLIP_FRAC, "n_contrib differs"


def _check_forward(out, o, R, variant):
    im = o.images()
    assert out["num_rendered"] == R
    assert np.array_equal(out["radii"].cpu().numpy(), im["radii"])
    for k in ["color", "normal", "depth", "opacity", "feature"] + (["vfeature"] if variant == "svgss" else []):
        assert tuple(out[k].shape) == im[k].shape, k
        _cmp(k, out[k], im[k])
    _cmp("weights", out["weights"], im["weights"])
    return im


GRAD_PAIRS = [("means3D", "means3D"), ("scales", "scales"), ("rotations", "rotations"), ("opacities", "opacity"), ("shs", "sh"),
              ("features", "features"), ("means2D", "means2D"), ("cov3D_precomp", "cov3D"), ("colors_precomp", "colors")]
ANCHOR_FLOOR = 1e-4   # north_star's tolerance: what the product may be from the exact gradient where the fp32 oracle is (nearly) exact


def _check_backward(leaves, o, variant, exact=None):
    """`exact`: gradients of the fp64 oracle.  Where given, NO flat element-wise tolerance is used: per tensor, the distribution of
    the product's relative error against the exact gradient (its tail quantile over the signal-carrying entries -- p99.99 from 100 000
    entries on, p99.9 from 10 000, else p99: parity_util.tail_quantile -- and the share beyond REL_TOL) must be within 1.5 x that of the
    reference's own fp32 arithmetic (the fp32 oracle) + north_star's 1e-4.  Sums of tens of
    thousands of nearly cancelling (pixel, splat) terms per Gaussian differ between ANY two fp32 summation orders; the product must
    be as close to the exact gradient as the reference arithmetic is, not equal to one particular order."""
    gr = o.grads()
    pairs = [pr for pr in GRAD_PAIRS if pr[0] in leaves]
    if variant == "svgss" and "vfeatures" in leaves:
        pairs.append(("vfeatures", "vfeatures"))
    for lk, ok in pairs:
        g = leaves[lk].grad
        if g is None:
            assert gr[ok].size == 0 or np.abs(gr[ok]).max() == 0, lk
            continue
        budget = REL_FRAC
        if exact is not None:
            ref = pu.stats(gr[ok], exact[ok], tol=TOL, rel_tol=REL_TOL)
            own = pu.stats(g.detach().cpu().numpy(), exact[ok], tol=TOL, rel_tol=REL_TOL)
            assert own["tail_rel"] <= 1.5 * ref["tail_rel"] + ANCHOR_FLOOR, \
                f"grad_{lk}: p{100 * own['tail_q']:g} relative error vs the exact gradient {own['tail_rel']:.2e}, the fp32 oracle's {ref['tail_rel']:.2e}"
            assert own["tail_norm"] <= 1.5 * ref["tail_norm"] + ANCHOR_FLOOR, \
                f"grad_{lk}: tail normalised error vs the exact gradient {own['tail_norm']:.2e}, the fp32 oracle's {ref['tail_norm']:.2e}"
            few = 3.0 / max(own["n_signal"], 1)   # (small tensors: three entries -- a few thousand signal-carrying entries make ONE nearly cancelling sum 4e-4 of them)
            assert own["rel_frac"] <= 1.5 * ref["rel_frac"] + REL_FRAC + few, f"grad_{lk}: {own['rel_frac']:.2e} of the entries beyond {REL_TOL:g} of the exact gradient, the fp32 oracle {ref['rel_frac']:.2e}"
            budget = max(REL_FRAC, 2.5 * ref["rel_frac"] + REL_FRAC) + few   # (two fp32 evaluations, each that far from the exact one)
        _cmp("grad_" + lk, g, gr[ok], flip_frac=GRAD_FLIP_FRAC, rel_frac=budget)


def _exact_grads(sc, variant, grads, R):
    """Gradients of the fp64 oracle on the same inputs (the anchor of _check_backward)."""
    o64 = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS, fp64=True)
    assert abs(o64.forward() - R) <= max(2, 1e-5 * R)   # (a handful of radius roundings differ between fp32 and fp64)
    o64.backward(grads["color"], grads["normal"], grads["depth"], grads["opacity"], grads["feature"], grads.get("vfeature"))
    return o64.grads()


CASES = [
    # name, generator kwargs
    ("svgss_S3_VS8", dict(P=6000, W=208, H=144, seed=21, sh_degree=3, variant="svgss", S=3, VS=8, scale_lo=0.01, scale_hi=0.06)),
    ("svgss_S1_VS4_deg1", dict(P=3000, W=100, H=75, seed=22, sh_degree=1, variant="svgss", S=1, VS=4, scale_lo=0.02, scale_hi=0.1)),
    ("svgss_nofeat", dict(P=4000, W=128, H=128, seed=23, sh_degree=0, variant="svgss", S=0, VS=0, scale_lo=0.02, scale_hi=0.08)),
    ("rgss_S5", dict(P=6000, W=208, H=144, seed=24, sh_degree=3, variant="rgss", S=5, VS=0, scale_lo=0.01, scale_hi=0.06)),
    ("rgss_S3_deg2", dict(P=3000, W=97, H=61, seed=25, sh_degree=2, variant="rgss", S=3, VS=0, scale_lo=0.02, scale_hi=0.1)),
    ("rgss_nofeat", dict(P=2000, W=64, H=64, seed=26, sh_degree=0, variant="rgss", S=0, VS=0, scale_lo=0.03, scale_hi=0.1)),
]


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_forward_backward_parity_small(built, name, kw):
    sc = scenes.surface_scene(**kw)
    variant = kw["variant"]
    grads = scenes.upstream_grads(sc, variant, seed=77)
    out, leaves, o, R = _run_both(sc, variant, grads)
    assert R > 0
    im = _check_forward(out, o, R, variant)
    _check_binning(sc, variant, o, R)
    _check_backward(leaves, o, variant, exact=_exact_grads(sc, variant, grads, R))


@pytest.mark.parametrize("cfg,variant", [("cfg1", "svgss"), ("cfg2", "rgss"), ("cfg3_train", "svgss"), ("cfg3_eval", "svgss"),
                                         ("cfg4", "svgss")])
def test_baseline_configs_full_size(built, cfg, variant):
    """BASELINE.json configs 0-3 at full size (the oracle finishes them in seconds).  cfg4 = one of the eight armadillo
    views at the eval widths (the other seven only differ in the camera: test_cfg4_all_eight_views)."""
    sc = scenes.make(cfg)
    train = cfg != "cfg3_eval"
    grads = scenes.upstream_grads(sc, variant) if train else None
    out, leaves, o, R = _run_both(sc, variant, grads)
    _check_forward(out, o, R, variant)
    _check_binning(sc, variant, o, R)
    if train:   # every gradient tensor anchored on the fp64 oracle: as close to the exact gradient as the reference's fp32 arithmetic is
        _check_backward(leaves, o, variant, exact=_exact_grads(sc, variant, grads, R))


def test_cfg4_all_eight_views(built):
    """BASELINE configs[3]: the eight test views (azimuth k * 45 degrees, elevation 30 degrees) that the view-parallel
    driver shards over 8 GPUs, each forward against the oracle on this one GPU."""
    from svgir_harness import cameras
    base = scenes.make("cfg4")
    for k in range(8):
        sc = dict(base)
        sc.update(cameras.make_camera(sc["W"], sc["H"], cameras.orbit_eye(4.0, 45.0 * k, 30.0)))
        out, leaves, o, R = _run_both(sc, "svgss", None)
        _check_forward(out, o, R, "svgss")


def test_cfg5_stress_full_size(built):
    """BASELINE configs[4]: 2 M surfels, 1600x1600, eval widths -- forward and backward against the oracle at full size,
    plus the size-independent properties (idempotence, linearity in the feature channels)."""
    sc = scenes.make("cfg5")
    grads = scenes.upstream_grads(sc, "svgss")
    out, leaves, o, R = _run_both(sc, "svgss", grads)
    assert R > 3_000_000
    _check_forward(out, o, R, "svgss")
    _check_binning(sc, "svgss", o, R)
    _check_backward(leaves, o, "svgss", exact=_exact_grads(sc, "svgss", grads, R))
    del o
    sct = runner.to_torch(sc, _dev())
    out2, _ = runner.render(sct, "svgss")
    for k in ("color", "normal", "depth", "opacity", "feature", "vfeature"):
        assert torch.equal(out[k].detach(), out2[k]), k
    sct["features"] = sct["features"] * 2.0
    out3, _ = runner.render(sct, "svgss")
    torch.testing.assert_close(out3["feature"], out2["feature"] * 2.0, rtol=1e-5, atol=1e-6)


def test_cfg5_dense_full_size(built):
    """The stress scene at the generator's default surfel scales: R = 18.3 M instances (the order SURVEY 8(a) a1 budgets the state
    blobs for: R ~ 20 M; ~40 GB of blobs + backward scratch), forward and backward against the oracle at full size."""
    sc = scenes.make("cfg5_dense")
    grads = scenes.upstream_grads(sc, "svgss")
    out, leaves, o, R = _run_both(sc, "svgss", grads)
    assert R >= 18_000_000, R
    _check_forward(out, o, R, "svgss")
    _check_binning(sc, "svgss", o, R)
    _check_backward(leaves, o, "svgss", exact=_exact_grads(sc, "svgss", grads, R))


@pytest.mark.parametrize("variant,S,VS", [("rgss", 5, 0), ("svgss", 3, 8)])
def test_deep_translucent_stack_many_backward_segments(built, variant, S, VS):
    """Hundreds of faint surfels over every pixel: no early termination, sub-tile candidate lists several times longer
    than one backward segment (common.hpp SEG = 128), so most backward waves start from a dumped forward state."""
    sc = scenes.surface_scene(P=5000, W=72, H=56, seed=41, sh_degree=1, variant=variant, S=S, VS=VS, scale_lo=0.08,
                              scale_hi=0.25)
    sc["opacities"] = (sc["opacities"] * 0.04).astype(np.float32)
    grads = scenes.upstream_grads(sc, variant, seed=9)
    out, leaves, o, R = _run_both(sc, variant, grads)
    T = ((72 + 15) // 16) * ((56 + 15) // 16)
    assert R / T > 500, "scene not deep enough to exercise the segmented backward"
    _check_forward(out, o, R, variant)
    _check_backward(leaves, o, variant, exact=_exact_grads(sc, variant, grads, R))


def test_config_flags_and_quirks(built):
    """normalize_depth off, per-pixel depth off, surface off (svgss config tensor), scale modifier, Q1."""
    base = scenes.surface_scene(P=3000, W=112, H=80, seed=31, sh_degree=2, variant="svgss", S=3, VS=8, scale_lo=0.02, scale_hi=0.08)
    for cfgv, smod in (([1, 0, 1], 1.0), ([1, 1, 0], 1.0), ([0, 1, 0], 0.7), ([1, 1, 1], 1.4)):
        sc = dict(base)
        sc["config"] = np.array(cfgv, dtype=np.float32)
        sc["scale_modifier"] = smod
        grads = scenes.upstream_grads(sc, "svgss", seed=5)
        out, leaves, o, R = _run_both(sc, "svgss", grads)
        _check_forward(out, o, R, "svgss")
        _check_backward(leaves, o, "svgss", exact=_exact_grads(sc, "svgss", grads, R))
    # Q7: 4-entry config with config[3] > 0 switches the camera gradients on
    sc = dict(base)
    sc["config"] = np.array([1, 1, 1, 1], dtype=np.float32)
    dev = _dev()
    sct = runner.to_torch(sc, dev)
    vm = sct["viewmatrix"].clone().requires_grad_(True)
    pm = sct["projmatrix"].clone().requires_grad_(True)
    cp = sct["campos"].clone().requires_grad_(True)
    sct.update(viewmatrix=vm, projmatrix=pm, campos=cp)
    grads = scenes.upstream_grads(sc, "svgss", seed=5)
    out, leaves = runner.render(sct, "svgss", requires_grad=True)
    runner.backward(out, grads, "svgss")
    o = orc.OracleRun(sc, orc.SVGSS)
    o.forward()
    o.backward(grads["color"], grads["normal"], grads["depth"], grads["opacity"], grads["feature"], grads["vfeature"])
    gr = o.grads()
    _cmp("viewmat", vm.grad, gr["viewmat"], tol=5e-4, flip_frac=0.0, rel=False)
    _cmp("projmat", pm.grad, gr["projmat"], tol=5e-4, flip_frac=0.0, rel=False)
    _cmp("campos", cp.grad, gr["campos"], tol=5e-4, flip_frac=0.0, rel=False)


def test_rgss_pseudo_normal_ncontrib_view_and_backward_geometry(built):
    sc = scenes.surface_scene(P=5000, W=160, H=120, seed=41, sh_degree=1, variant="rgss", S=5, VS=0, scale_lo=0.02, scale_hi=0.08)
    sc["computer_pseudo_normal"] = True
    sc["backward_geometry"] = False
    grads = scenes.upstream_grads(sc, "rgss", seed=3)
    out, leaves, o, R = _run_both(sc, "rgss", grads)
    im = _check_forward(out, o, R, "rgss")
    _cmp("surface_xyz", out["surface_xyz"], im["surface_xyz"])
    # the stencil normal divides differences of neighbouring depths by their (possibly tiny) norm: it is compared on every pixel
    # whose 3x3 neighbourhood of depth AND opacity agrees with the oracle's to 1e-6 -- there ALL normals must agree to 1e-4 --
    # and those pixels must be nearly all of the image
    pn, pr = out["pseudo_normal"].detach().cpu().numpy(), im["pseudo_normal"]
    dd = np.maximum(np.abs(out["depth"].detach().cpu().numpy() - im["depth"])[0], np.abs(out["opacity"].detach().cpu().numpy() - im["opacity"])[0])
    pad = np.pad(dd, 1, mode="edge")
    nb = np.max([pad[1 + dy:1 + dy + dd.shape[0], 1 + dx:1 + dx + dd.shape[1]] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    agree = nb <= 1e-6
    assert agree.mean() > 0.98, agree.mean()
    assert np.abs(pn - pr).max(0)[agree].max() < 1e-4, np.abs(pn - pr).max(0)[agree].max()
    assert out["n_contrib"].dtype == torch.int32 and tuple(out["n_contrib"].shape) == (120, 160)
    _check_backward(leaves, o, "rgss")


def test_edge_cases(built):
    dev = _dev()
    # P == 0: zero outputs, num_rendered 0 (rasterize_points.cu:100)
    sc = scenes.random_cloud(P=1, W=40, H=24, variant="svgss", S=0, VS=0)
    sct = runner.to_torch(sc, dev)
    for k in ("means3D", "scales", "rotations", "opacities", "shs", "features", "vfeatures"):
        sct[k] = sct[k][:0]
    out, _ = runner.render(sct, "svgss")
    assert out["num_rendered"] == 0 and float(out["color"].abs().max()) == 0 and out["radii"].numel() == 0
    # everything culled: colour = T*bg everywhere, no instances
    sc = scenes.surface_scene(P=500, W=50, H=37, seed=2, sh_degree=1, variant="svgss", S=1, VS=4, bg=0.25, scale_lo=0.05, scale_hi=0.2)
    sc2 = dict(sc)
    sc2["means3D"] = sc["means3D"] + np.array([100.0, 100.0, 100.0], dtype=np.float32) * np.sign(sc["campos"])
    grads = scenes.upstream_grads(sc2, "svgss")
    out, leaves, o, R = _run_both(sc2, "svgss", grads)
    assert R == 0 and out["num_rendered"] == 0
    _check_forward(out, o, R, "svgss")
    assert float(leaves["means3D"].grad.abs().max()) == 0
    # ragged image size + single huge splat list in one tile
    out, leaves, o, R = _run_both(sc, "svgss", scenes.upstream_grads(sc, "svgss"))
    _check_forward(out, o, R, "svgss")
    _check_backward(leaves, o, "svgss")


def test_mark_visible(built):
    dev = _dev()
    from gaussian_renderer import rgss_rasterization, svgss_rasterization
    sc = scenes.random_cloud(P=1000, W=64, H=64, variant="rgss")
    sct = runner.to_torch(sc, dev)
    vis = rgss_rasterization.GaussianRasterizer(runner.settings(sct, "rgss")).markVisible(sct["means3D"])
    o = orc.OracleRun(sc, orc.RGSS)
    assert np.array_equal(vis.cpu().numpy(), o.mark_visible())
    sct = runner.to_torch(scenes.random_cloud(P=1000, W=64, H=64, variant="svgss"), dev)
    vis = svgss_rasterization.GaussianRasterizer(runner.settings(sct, "svgss")).markVisible(sct["means3D"])
    assert not bool(vis.any())  # Q14


def _precomp_case(variant, which):
    """A scene whose colours / 3D covariances enter PRECOMPUTED (forward.cu:326-328, :370-376; rasterize_points.cu:111-119): the
    covariances are the ones the oracle derives from scales + rotations of the same scene, the colours are random.  With cov3D_precomp
    the bindings pass no rotations (exactly one of the two may be given, svgss_rasterization.py:373-375): the surfel frame is then the
    identity quaternion, i.e. every normal is the world z axis -- the camera sits above the scene so that they face it."""
    from svgir_harness import cameras
    kw = dict(P=5000, W=144, H=112, seed=53, sh_degree=2, variant=variant, scale_lo=0.02, scale_hi=0.08)
    kw.update(dict(S=3, VS=8) if variant == "svgss" else dict(S=5, VS=0))
    sc = scenes.surface_scene(**kw)
    sc.update(cameras.make_camera(sc["W"], sc["H"], cameras.orbit_eye(4.0, 35.0, 55.0)))
    var_id = orc.SVGSS if variant == "svgss" else orc.RGSS
    if which == "cov3D":
        o0 = orc.OracleRun(sc, var_id)
        o0.forward()
        sc["cov3D_precomp"] = o0.get("cov3D").reshape(-1, 6).astype(np.float32).copy()
        del sc["scales"], sc["rotations"]
    else:
        sc["colors_precomp"] = np.random.default_rng(3).uniform(0, 1, size=(kw["P"], 3)).astype(np.float32)
        del sc["shs"]
    return sc, var_id


@pytest.mark.parametrize("variant", ["svgss", "rgss"])
@pytest.mark.parametrize("which", ["cov3D", "colors"])
def test_precomputed_inputs_forward_and_backward(built, variant, which):
    """cov3D_precomp (incl. dL_dcov3D; no dL_dscales / dL_drotations: backward.cu:520-524) and colors_precomp (incl. dL_dcolors; no
    dL_dsh: rasterize_points.cu:199-264) through the bindings, forward and every gradient against the oracle, fp64-anchored."""
    dev = _dev()
    sc, var_id = _precomp_case(variant, which)
    grads = scenes.upstream_grads(sc, variant, seed=12)
    if variant == "svgss":
        from gaussian_renderer.svgss_rasterization import GaussianRasterizer
    else:
        from gaussian_renderer.rgss_rasterization import GaussianRasterizer
    sct = runner.to_torch(sc, dev)
    names = [k for k in ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp", "features") if k in sct]
    if variant == "svgss":
        names.append("vfeatures")
    leaves = {k: sct[k].detach().clone().requires_grad_(True) for k in names}
    leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=True)
    res = GaussianRasterizer(runner.settings(sct, variant))(**leaves)
    if variant == "svgss":
        (R, color, normal, opacity, depth, feature, vfeature, weights, radii) = res
        out = dict(num_rendered=R, color=color, normal=normal, opacity=opacity, depth=depth, feature=feature, vfeature=vfeature, weights=weights, radii=radii)
    else:
        (R, n_contrib, color, normal, opacity, depth, feature, pseudo_normal, surface_xyz, weights, radii) = res
        out = dict(num_rendered=R, color=color, normal=normal, opacity=opacity, depth=depth, feature=feature, weights=weights, radii=radii)
    runner.backward(out, grads, variant)
    torch.cuda.synchronize()
    o = orc.OracleRun(sc, var_id)
    assert o.forward() == R and R > 2000, R
    o.backward(grads["color"], grads["normal"], grads["depth"], grads["opacity"], grads["feature"], grads.get("vfeature"))
    _check_forward(out, o, R, variant)
    _check_backward(leaves, o, variant, exact=_exact_grads(sc, variant, grads, R))
    # the gradient of the precomputed input exists and carries signal; the inputs it replaces have none
    g = leaves["cov3D_precomp" if which == "cov3D" else "colors_precomp"].grad
    assert g is not None and float(g.abs().max()) > 0
    gr = o.grads()
    if which == "cov3D":
        assert gr["scales"].size == 0 or float(np.abs(gr["scales"]).max()) == 0.0
    else:
        assert gr["sh"].size == 0 or float(np.abs(gr["sh"]).max()) == 0.0


def test_full_size_properties_cfg3_eval(built):
    """Size-independent properties at BASELINE's 800x800 eval widths: linearity in the feature channels,
    idempotence (bitwise-identical images run to run except atomically accumulated weights), opacity bounds."""
    dev = _dev()
    sc = scenes.make("cfg3_eval")
    sct = runner.to_torch(sc, dev)
    out1, _ = runner.render(sct, "svgss")
    out2, _ = runner.render(sct, "svgss")
    for k in ("color", "normal", "depth", "opacity", "feature", "vfeature"):
        assert torch.equal(out1[k], out2[k]), k
    assert out1["num_rendered"] == out2["num_rendered"]
    assert float(out1["opacity"].min()) >= 0.0 and float(out1["opacity"].max()) <= 1.0
    sct2 = dict(sct)
    sct2["features"] = sct["features"] * 2.0
    sct2["vfeatures"] = sct["vfeatures"] * -0.5
    out3, _ = runner.render(sct2, "svgss")
    torch.testing.assert_close(out3["feature"], out1["feature"] * 2.0, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out3["vfeature"], out1["vfeature"] * -0.5, rtol=1e-5, atol=1e-6)
    assert torch.equal(out3["color"], out1["color"])
    # sum of blending weights per pixel == opacity  =>  sum over Gaussians of weights == sum of opacity
    torch.testing.assert_close(out1["weights"].sum(), out1["opacity"].sum() - 1e-6 * 0, rtol=2e-3, atol=1.0)


@pytest.mark.parametrize("variant,S,VS", [("svgss", 9, 72), ("svgss", 2, 0), ("svgss", 0, 12), ("rgss", 7, 0), ("rgss", 2, 0),
                                          ("svgss", 50, 80), ("rgss", 33, 0)])
def test_channel_widths_without_specialised_kernel(built, variant, S, VS):
    """Widths outside the instantiated (S, VS) set run through the run-time-width kernels of csrc/render_generic.hip
    (the bare C ABI accepts every width the reference does: S <= 50 / 33, VS/4 <= 20); results and gradients must still
    match the oracle."""
    sc = scenes.surface_scene(P=2500, W=96, H=80, seed=51, sh_degree=2, variant=variant, S=S, VS=VS, scale_lo=0.02,
                              scale_hi=0.08)
    grads = scenes.upstream_grads(sc, variant, seed=13)
    out, leaves, o, R = _run_both(sc, variant, grads)
    _check_forward(out, o, R, variant)
    _check_backward(leaves, o, variant)


def test_svgss_gradients_bit_reproducible(built):
    """The svgss backward accumulates the composite gradients without atomics (gradient rows summed per Gaussian in a
    fixed order, csrc/grad_reduce.hip): two runs give bit-identical gradients."""
    sc = scenes.surface_scene(P=6000, W=160, H=128, seed=71, sh_degree=2, variant="svgss", S=4, VS=52, scale_lo=0.02,
                              scale_hi=0.08)
    grads = scenes.upstream_grads(sc, "svgss", seed=3)
    sct = runner.to_torch(sc, _dev())
    runs = []
    for _ in range(2):
        out, leaves = runner.render(sct, "svgss", requires_grad=True)
        runner.backward(out, grads, "svgss")
        torch.cuda.synchronize()
        runs.append({k: v.grad.clone() for k, v in leaves.items() if v.grad is not None})
    assert set(runs[0]) == set(runs[1]) and len(runs[0]) >= 6
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_svgss_backward_scratch_is_sized_by_the_views_pair_count(built, monkeypatch):
    """svgir_backward_scratch_bytes_for(): one gradient row per (sub-tile, instance) pair that survived THIS view's cull (the forward
    reads the count back behind its cull) instead of four per instance -- well under half the worst case on a surface scene -- and
    the gradients are bit-identical to a run with the worst-case scratch (same rows, same summation order)."""
    from gaussian_renderer import _native as N
    sc = scenes.surface_scene(P=20000, W=320, H=256, seed=72, sh_degree=2, variant="svgss", S=4, VS=52, scale_lo=0.01, scale_hi=0.05)
    grads = scenes.upstream_grads(sc, "svgss", seed=4)
    sct = runner.to_torch(sc, _dev())
    sizes = []
    real = N.lib.svgir_backward_scratch_bytes_for

    def spy(variant, P, nbin, iblob, W, H, S, VS):
        n = real(variant, P, nbin, iblob, W, H, S, VS)
        sizes.append((int(n), int(N.lib.svgir_backward_scratch_bytes(variant, P, nbin, W, H, S, VS))))
        return n

    class _Lib:   # (ctypes function pointers cannot be monkeypatched on the CDLL: wrap the library object)
        def __getattr__(self, k):
            return spy if k == "svgir_backward_scratch_bytes_for" else getattr(N_lib, k)

    N_lib = N.lib
    monkeypatch.setattr(N, "lib", _Lib())
    out, leaves = runner.render(sct, "svgss", requires_grad=True)
    runner.backward(out, grads, "svgss")
    torch.cuda.synchronize()
    compact = {k: v.grad.clone() for k, v in leaves.items() if v.grad is not None}
    assert sizes and sizes[-1][0] < 0.55 * sizes[-1][1], sizes

    class _LibWorst:
        def __getattr__(self, k):
            if k == "svgir_backward_scratch_bytes_for":
                return lambda variant, P, nbin, iblob, W, H, S, VS: N_lib.svgir_backward_scratch_bytes(variant, P, nbin, W, H, S, VS)
            return getattr(N_lib, k)

    monkeypatch.setattr(N, "lib", _LibWorst())
    out, leaves = runner.render(sct, "svgss", requires_grad=True)
    runner.backward(out, grads, "svgss")
    torch.cuda.synchronize()
    for k, v in leaves.items():
        if v.grad is not None:
            assert torch.equal(v.grad, compact[k]), k


def test_speculative_capacity_small_large_small(built):
    """The count-dependent forward stages are launched speculatively for a capacity guessed from the previous call's
    instance count (csrc/api.hip): a much larger scene after a small one must take the re-run path, a small one after
    a large one runs inside an over-sized blob -- all three must match the oracle, forward and backward."""
    small = scenes.surface_scene(P=1500, W=80, H=64, seed=81, sh_degree=1, variant="rgss", S=5, VS=0, scale_lo=0.02,
                                 scale_hi=0.06)
    large = scenes.surface_scene(P=30000, W=256, H=192, seed=82, sh_degree=1, variant="rgss", S=5, VS=0, scale_lo=0.02,
                                 scale_hi=0.08)
    last_R = None
    for sc in (small, large, small):
        grads = scenes.upstream_grads(sc, "rgss", seed=17)
        out, leaves, o, R = _run_both(sc, "rgss", grads)
        _check_forward(out, o, R, "rgss")
        _check_backward(leaves, o, "rgss")
        if last_R is not None:
            assert R > 3 * last_R or last_R > 3 * R, "the scenes should differ a lot in instance count"
        last_R = R


def test_state_slot_capacity_guess_too_small_reruns(built):
    """The composite forward dumps its blend state every 64 candidates of a sub-tile; the slots it may use are allocated from the
    pair statistics of the workload's recent views (csrc/api.hip).  A view whose lists are suddenly much longer -- the same surfels,
    the same instance count, but all of them on top of each other -- exceeds that guess: the forward (which does not wait for the cull)
    drops the dumps that do not fit, and the view's backward replays the composite forward for the states alone; before and after it,
    views with short lists run inside their (tiny / over-sized) allocations.  All three match the oracle, forward and backward."""
    spread = scenes.surface_scene(P=20000, W=512, H=512, seed=91, sh_degree=1, variant="svgss", S=4, VS=52, scale_lo=0.004, scale_hi=0.006)   # short lists: few state slots
    stacked = dict(spread)
    rng = np.random.default_rng(92)
    stacked["means3D"] = (0.004 * rng.normal(size=spread["means3D"].shape)).astype(np.float32)
    stacked["opacities"] = (spread["opacities"] * 0.02).astype(np.float32)   # translucent: the lists are consumed to the end
    # (fewer instances than the spread views, so that the instance capacity holds: every second surfel goes behind the camera)
    campos = np.asarray(spread["campos"], dtype=np.float64)
    behind = campos + 2.0 * (campos - 0.0) / np.linalg.norm(campos)
    stacked["means3D"][1::2] = (behind + 0.01 * rng.normal(size=stacked["means3D"][1::2].shape)).astype(np.float32)
    from gaussian_renderer import _native
    before = _native.speculation_stats()
    Rs = []
    for sc in (spread, spread, stacked, spread):
        grads = scenes.upstream_grads(sc, "svgss", seed=5)
        out, leaves, o, R = _run_both(sc, "svgss", grads)
        _check_forward(out, o, R, "svgss")
        _check_backward(leaves, o, "svgss")
        Rs.append(R)
    after = _native.speculation_stats()
    assert after["rerun_capacity"] == before["rerun_capacity"]      # (it is the slot guess that fails, not the instance capacity)
    assert after["rerun_slots"] == before["rerun_slots"] + 1        # the stacked view's states were dumped again by its backward


def _native_lib():
    from gaussian_renderer import _native
    return _native.lib


def test_forward_only_loops_learn_their_slot_capacity(built):
    """Without a backward (evaluation renders) nobody reads a view's state-slot total on its behalf: the workload's NEXT forward looks at
    it (no wait) before it sizes its own blob.  Every view's binning blob is compact (an odd multiple of 128 bytes, csrc/common.hpp
    bin_layout): the first one is sized from its own cull (a sizing pass into a temporary, round 5 -- never the worst case over the
    cull), later ones from the history (+12 %), and the images stay equal to the first view's."""
    dev = _dev()
    sc = scenes.surface_scene(P=12000, W=192, H=160, seed=23, sh_degree=1, variant="svgss", S=4, VS=52, scale_lo=0.01, scale_hi=0.03)
    sct = runner.to_torch(sc, dev)
    sizes, first = [], None
    for it in range(5):
        raw = runner.forward_raw(sct, "svgss")
        torch.cuda.synchronize()
        sizes.append(int(raw["blobs"][1].numel()))
        color, R_last = raw["color"], raw["num_rendered"]
        if first is None:
            first = color.clone()
        else:
            assert torch.equal(color, first)
        del raw
    worst = int(_native_lib().svgir_binning_bytes(int(R_last), 192, 160, 4, 52))
    assert all(b % 256 == 128 for b in sizes), sizes             # compact from the first view on
    assert max(sizes) < 0.8 * worst and sizes[0] <= min(sizes[2:]), (sizes, worst)


def test_depth_key_byte_speculation_reruns_when_a_view_breaks_it(built):
    """The depth sort drops its fourth 8-bit pass once three consecutive views of a workload had all visible depth keys in one top byte
    (depths in [2, 8) here: 0x40), csrc/api.hip.  A view of the same workload whose surfels straddle two bytes (half of them pushed
    beyond depth 8) must be detected and re-run with four passes; `point_list` (exact) and the images pin the order either way."""
    from gaussian_renderer import _native
    near = scenes.surface_scene(P=6000, W=160, H=128, seed=17, sh_degree=2, variant="rgss", S=3, VS=0, scale_lo=0.01, scale_hi=0.03)
    far = dict(near)
    V = np.asarray(near["viewmatrix"], dtype=np.float64).reshape(4, 4)   # row-vector convention: p_view = [p, 1] @ V
    m = np.asarray(near["means3D"], dtype=np.float64)
    z = (np.c_[m, np.ones(len(m))] @ V)[:, 2]
    assert z.min() > 2.0 and z.max() < 8.0
    campos = np.asarray(near["campos"], dtype=np.float64)
    push = (np.arange(len(m)) % 2 == 0)[:, None]
    far["means3D"] = np.where(push, campos + (m - campos) * 2.6, m).astype(np.float32)   # every second surfel 2.6x as far away (same pixel)
    z2 = (np.c_[far["means3D"].astype(np.float64), np.ones(len(m))] @ V)[:, 2]
    assert (z2 > 8.0).sum() > 1000 and (z2 < 8.0).sum() > 1000
    before = _native.speculation_stats()
    for sc in (near, near, near, near, near, far, near, near, near, near):
        grads = scenes.upstream_grads(sc, "rgss", seed=6)
        out, leaves, o, R = _run_both(sc, "rgss", grads)
        _check_forward(out, o, R, "rgss")
        _check_backward(leaves, o, "rgss")
    after = _native.speculation_stats()
    if os.environ.get("SVGIR_NO_KEY_SPEC") is None:
        assert after["three_pass"] - before["three_pass"] >= 3      # views 4-5 and the last one(s) ran the short sort ...
        assert after["rerun_depth_key"] - before["rerun_depth_key"] == 1   # ... and exactly the straddling view was re-run


def test_prefiltered_flag_reports_culled_points(built):
    """`prefiltered=True` asserts that the caller has already removed every point the frustum / back-face tests would
    cull; the reference traps the device when one is culled anyway (auxiliary.h:163-167, 195-199).  Here the forward
    returns an error through the C ABI (RuntimeError in the binding) -- and runs normally when nothing is culled."""
    from gaussian_renderer.svgss_rasterization import GaussianRasterizer
    dev = _dev()
    sc = scenes.surface_scene(P=800, W=64, H=48, seed=91, sh_degree=0, variant="svgss", S=0, VS=0, scale_lo=0.03, scale_hi=0.1)
    sct = runner.to_torch(sc, dev)
    st = runner.settings(sct, "svgss")._replace(prefiltered=True)
    kw = dict(means3D=sct["means3D"], means2D=torch.zeros_like(sct["means3D"]), opacities=sct["opacities"], shs=sct["shs"],
              scales=sct["scales"], rotations=sct["rotations"], features=sct["features"], vfeatures=sct["vfeatures"])
    with pytest.raises(RuntimeError, match="filtered although prefiltered"):
        GaussianRasterizer(st)(**kw)   # half of the surfels face away from the camera
    # keep only what survives the culls: the same call now succeeds and matches the unfiltered render
    out_all, _ = runner.render(sct, "svgss")
    keep = out_all["radii"] > 0
    kw2 = {k: (v[keep] if v.shape[0] == keep.shape[0] else v) for k, v in kw.items()}
    res = GaussianRasterizer(st)(**kw2)
    assert res[0] == out_all["num_rendered"]
    assert torch.equal(res[1], out_all["color"])


@pytest.mark.parametrize("variant,S,VS", [("rgss", 5, 0), ("svgss", 3, 8)])
def test_outputs_need_no_clearing_by_the_caller(built, variant, S, VS, monkeypatch):
    """ABI 5: the library writes / clears every output itself.  The suite runs with SVGIR_POISON=1 (conftest.py: the
    bindings NaN-fill every output and gradient buffer before the call); here additionally WITHOUT the clear_base hint, so
    that svgir_backward clears the gradient tensors one by one on its side stream -- and twice in a row, so that the second
    call runs while buffers of the first are being recycled by the allocator."""
    from gaussian_renderer import _native
    assert _native.POISON, "tests are expected to run with poisoned output buffers"
    monkeypatch.setattr(_native, "CLEAR_HINT", False)
    sc = scenes.surface_scene(P=5000, W=160, H=112, seed=93, sh_degree=2, variant=variant, S=S, VS=VS, scale_lo=0.01, scale_hi=0.07)
    grads = scenes.upstream_grads(sc, variant, seed=5)
    for _ in range(2):
        out, leaves, o, R = _run_both(sc, variant, grads)
        _check_forward(out, o, R, variant)
        _check_backward(leaves, o, variant)
    for k, v in out.items():
        if torch.is_tensor(v) and v.is_floating_point():
            assert torch.isfinite(v).all(), k
