"""The geometry-loss case table (tests/geom_loss_cases.py) on the host: its fp64 oracle reproduces the reference's recorded results
(tests/golden/geom_losses.npz: the reference's own cos_loss / depth2normal with autograd and the literal pooled-mask and entropy lines,
scripts/make_golden_geom_loss.py), the table covers what it promises, few pixels sit on the selection threshold or are degenerate, and
E32 -- what the reference's own fp32 arithmetic loses per case -- is measured (DESIGN.md section 5 holds the figures)."""
import os

import numpy as np
import pytest
import torch

import geom_loss_cases as gc
import image_cases as ic

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geom_losses.npz")
_id = lambda r: r["id"] if isinstance(r, dict) else str(r)   # noqa: E731


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("k", range(4))
def test_oracle_reproduces_the_reference(gold, k):
    g = lambda name: gold[f"{k}.{name}"]   # noqa: E731
    prcp = tuple(float(v) for v in g("prcppoint"))
    fovx, fovy = float(g("fovx")), float(g("fovy"))
    for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        t = {n: torch.from_numpy(g(n)).to(dt) for n in ("normal", "depth", "mask", "target", "opacity")}
        normal, depth, op = t["normal"].requires_grad_(True), t["depth"].requires_grad_(True), t["opacity"].requires_grad_(True)
        ls, ns, _, _ = gc.surface_torch(normal, depth, t["mask"], prcp, fovx=fovx, fovy=fovy)
        lt, nt, _ = gc.cos_loss_torch(normal, t["target"], t["mask"])
        lm = gc.mask_torch(op, t["mask"])
        # (the recorded fp64 run clamps with the double bounds 1e-6 / 1 - 1e-6, the fp32 one with their fp32 roundings)
        le = gc.entropy_torch(op, t["mask"], *((1e-6, 1 - 1e-6) if dt == torch.float64 else (gc.ENT_LO, gc.ENT_HI)))
        got = np.array([float(ls.detach()), float(lt.detach()), float(lm.detach()), float(le.detach())])
        if dt == torch.float64:
            np.testing.assert_allclose(got[1:], g("f64.losses")[1:], rtol=0, atol=1e-12)
            # the reference's depth2normal keeps its pixel grid and intrinsics in fp32 whatever the depth's dtype, so its fp64 run is mixed
            # precision: cos_loss is held to 1e-12 on the pseudo normal that run returned, the whole surface term to fp32 rounding
            lr, nr, _ = gc.cos_loss_torch(normal, torch.from_numpy(g("f64.d2n")))
            assert abs(float(lr.detach()) - g("f64.losses")[0]) <= 1e-12 and [nr, nt] == list(g("f64.counts"))
            np.testing.assert_allclose(torch.autograd.grad(lr, normal)[0].numpy(), g("f64.d_normal_surface"), rtol=0, atol=1e-12)
            assert abs(got[0] - g("f64.losses")[0]) <= 1e-8 and ns == nr
            gn, gd = torch.autograd.grad(ls, (normal, depth))
            np.testing.assert_allclose(gn.numpy(), g("f64.d_normal_surface"), rtol=0, atol=1e-8)
            np.testing.assert_allclose(gd.numpy(), g("f64.d_depth"), rtol=0, atol=1e-5 * np.abs(g("f64.d_depth")).max())
            np.testing.assert_allclose(torch.autograd.grad(lt, normal)[0].numpy(), g("f64.d_normal_mono"), rtol=0, atol=1e-12)
            np.testing.assert_allclose(torch.autograd.grad(lm, op)[0].numpy(), g("f64.d_opacity_mask"), rtol=0, atol=1e-15)
            np.testing.assert_allclose(torch.autograd.grad(le, op)[0].numpy(), g("f64.d_opacity_entropy"), rtol=0, atol=1e-12 * 1e6)
        else:
            assert nt == int(g("f32.counts")[1])        # the target form: a pure function of the inputs, bit for bit
            assert abs(ns - int(g("f32.counts")[0])) <= int(gc.threshold_pixels(gold_cos64(gold, k)).sum())
            np.testing.assert_allclose(got, g("f32.losses"), rtol=2e-6, atol=1e-7)
    assert 0 < g("f64.counts")[0] < g("mask").size and 0 < g("f64.counts")[1] < g("mask").size      # both sides of the selection are present


def gold_cos64(gold, k):
    g = lambda name: torch.from_numpy(gold[f"{k}.{name}"]).double()   # noqa: E731
    prcp = tuple(float(v) for v in gold[f"{k}.prcppoint"])
    _, _, _, d2n = gc.surface_torch(g("normal"), g("depth"), g("mask"), prcp, fovx=float(gold[f"{k}.fovx"]), fovy=float(gold[f"{k}.fovy"]))
    return gc.cos_map(g("normal"), d2n).numpy()


def test_fixture_is_small_data():
    assert os.path.getsize(GOLD) < 400 * 1024
    with np.load(GOLD) as z:
        assert all(z[k].dtype.kind in "fiu" for k in z.files)


def test_table_covers_the_sizes_masks_and_edges():
    sizes = {(r["H"], r["W"]) for r in gc.RUNS}
    assert sizes == set(gc.SIZES) and {(1, 1), (1, 19), (23, 1), (5, 7), (16, 16), (17, 33), (37, 29), (150, 161)} == sizes
    assert {r["mask"] for r in gc.RUNS if (r["H"], r["W"]) == (37, 29)} >= set(ic.MASKS)
    assert {r["depth"] for r in gc.RUNS} >= {"holes", "plane1e-3", "plane1e4"}
    assert {r["opacity"] for r in gc.RUNS} == {"rand", "ends", "nan"}
    assert sum(r["normal"] == "equal" for r in gc.RUNS) == 1
    assert len(gc.FUSED_RUNS) == 4
    th, tw = gc.TILE
    assert (150 + th - 1) // th * ((161 + tw - 1) // tw) > 64         # more tile records than one wave of the reduce kernel reads at once
    for r in gc.RUNS:
        if r["mask"] != "tile_edges":
            continue
        m = gc.build_mask(r)[1][0] != 0
        H, W = m.shape
        edge = np.zeros_like(m)                                        # pixels whose mask differs from a 4-neighbour's
        edge[1:] |= m[1:] != m[:-1]; edge[:-1] |= m[1:] != m[:-1]; edge[:, 1:] |= m[:, 1:] != m[:, :-1]; edge[:, :-1] |= m[:, 1:] != m[:, :-1]
        ys, xs = np.nonzero(edge)
        assert (np.minimum(ys, H - 1 - ys) < 4).any() and (np.minimum(xs, W - 1 - xs) < 4).any()      # ... within 4 pixels of the border
        if H > th:
            assert (np.minimum(ys % th, th - 1 - ys % th) < 4).any()
        if W > tw:
            assert ((np.minimum(xs % tw, tw - 1 - xs % tw) < 4) & (xs >= tw - 4)).any()               # ... and of a column-tile edge


@pytest.mark.parametrize("run", gc.RUNS, ids=_id)
def test_caps_and_e32(run):
    r64, r32 = gc.reference(run), gc.reference(run, torch.float32)
    d = gc.build(run)
    n = run["H"] * run["W"]
    thr = gc.threshold_pixels(r64["cos"])
    if run["normal"] == "equal":
        assert n // 4 < r32["count"] < n - n // 4          # ill-conditioned on purpose: about half the pixels on either side in fp32
        assert np.isfinite(r32["surface"])
    else:
        assert thr.sum() <= gc.MAX_THRESHOLD_SHARE * n, (int(thr.sum()), n)
        sure = int((r64["sel"] & ~thr).sum())
        assert sure <= r32["count"] <= sure + int(thr.sum())
    if run["grad"] and min(run["H"], run["W"]) > 1 and run["mask"] != "zeros":
        excl = ic.d2n_excluded(r64["d2n"], d["mask"])[1]
        assert excl.sum() <= gc.MAX_DEGENERATE_SHARE * n, (int(excl.sum()), n)
    if run["opacity"] == "nan":
        assert np.isnan(r64["mask"]) and np.isnan(r64["entropy"]) and np.isfinite(r64["surface"])
        assert r64["d_opacity_entropy"][0, run["H"] // 2, run["W"] // 3] == 0      # torch.clamp's backward: no gradient for a NaN
    else:
        e32 = {k: abs(r32[k] - r64[k]) for k in ("surface", "mask", "entropy")}
        print(f"{run['id']}: losses " + ", ".join(f"{k} {r64[k]:.6g} (E32 {e32[k]:.2e})" for k in e32) + f"; count {r64['count']}, threshold {int(thr.sum())}")
        for k, v in e32.items():
            if run["normal"] == "equal" and k == "surface":
                continue
            assert np.isfinite(v) and v <= 2e-5 * max(abs(r64[k]), 1e-3), (k, v)       # the fp32 restatement is the same function
    if run["opacity"] == "ends":
        op = d["opacity"][0]
        assert (op == gc.F32(gc.ENT_LO)).any() and (op == gc.F32(gc.ENT_HI)).any() and (op < gc.F32(gc.ENT_LO)).any() and (op > gc.F32(gc.ENT_HI)).any() \
            or op.size < 27
        g = r64["d_opacity_entropy"][0]
        inside = (op >= gc.F32(gc.ENT_LO)) & (op <= gc.F32(gc.ENT_HI))
        assert not g[~inside].any() and (g[inside] != 0).all()      # the gradient passes on the bounds, not beyond them


@pytest.mark.parametrize("name", gc.TARGET_RUNS)
def test_target_cases_hold_what_they_are_named_for(name):
    d = gc.build_target(name)
    r64, r32 = gc.target_reference(name), gc.target_reference(name, torch.float32)
    n = d["output"][0].size
    assert r64["count"] == r32["count"] and np.array_equal(r64["sel"], r32["sel"])      # no case sits on the threshold in the target form
    if name == "unit_z":
        assert not r64["sel"][37 // 2:].any() and r64["sel"][:37 // 2].all() and not r64["d_output"][:, 37 // 2:].any()
    elif name == "zeros":
        assert r64["count"] == n and r64["loss"] == 1.0 and r32["loss"] == 1.0
    elif name == "nan_pixel":
        assert r64["count"] == n - 2 and not r64["sel"][3, 5] and not r64["sel"][-1, -1]
        assert np.isfinite(r64["loss"]) and not r64["d_output"][:, 3, 5].any() and not r64["d_output"][:, -1, -1].any()
    elif name == "empty":
        assert r64["count"] == 0 and np.isnan(r64["loss"]) and not r64["d_output"].any()
    else:
        assert 0 < r64["count"] <= n and np.isfinite(r64["loss"])
        if name == "weight_fractions":
            assert r64["count"] < n
        if name == "weights01":
            assert set(np.unique(d["weight"])) == {0.0, 1.0}


def test_cpu_tensors_and_bad_arguments_are_refused(built):
    """No CPU path behind the geometry losses, and the C entry points validate before any launch (no GPU is touched here)."""
    from gaussian_renderer import _native as N
    from svgir_harness import losses
    z3, z1 = torch.zeros(3, 4, 4), torch.ones(1, 4, 4)
    for call in (lambda: losses.cos_loss(z3, z3), lambda: losses.surface_loss(z3, z1, z1, 0.9, 0.6), lambda: losses.mask_loss(z1, z1),
                 lambda: losses.mask_entropy_loss(z1, z1), lambda: losses.geometry_losses(normal=z3, target=z3, opacity=z1, mask=z1)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()
    with pytest.raises(NotImplementedError):
        losses.cos_loss(z3, z3, thrsh=0.1)
    with pytest.raises(ValueError, match="without its planes"):
        losses.geometry_losses(normal=z3, terms=("surface",))
    with pytest.raises(ValueError, match="no term"):
        losses.geometry_losses()
    assert N.lib.svgir_geometry_loss_partials(161, 150) == 19 * 6 and N.lib.svgir_geometry_loss_partials(1, 1) == 1
    none6 = [None] * 6
    assert N.lib.svgir_geometry_loss_forward(0, 4, 1, *none6, 0.9, 0.6, 0.5, 0.5, None, None, None, None) == -1 and "bad image size" in N.last_error()
    assert N.lib.svgir_geometry_loss_forward(4, 4, 0, *none6, 0.9, 0.6, 0.5, 0.5, None, None, None, None) == -1 and "no term requested" in N.last_error()
    assert N.lib.svgir_geometry_loss_forward(4, 4, 8, *none6, 0.9, 0.6, 0.5, 0.5, None, None, None, None) == -1 and "need the opacity" in N.last_error()
    assert N.lib.svgir_geometry_loss_backward(4, 4, 1, *none6, 0.9, 0.6, 0.5, 0.5, None, None, None, None, None, None) == -1 \
        and "surface term needs" in N.last_error()
