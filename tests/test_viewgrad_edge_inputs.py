"""The view-direction gradient on the host: the oracle's d_viewdirs pinned by the reference's own autograd (tests/golden/
shading_viewgrad.npz, scripts/make_golden_viewgrad.py) and by central differences, the case table of tests/viewgrad_cases.py proved
(threshold share, what `view_alignment` is named for, finiteness, E32 per run), and the public surface of the feature."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import shading_cases as sc
import viewgrad_cases as vc
from oracle import shading_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _gold(tag):
    g, v = np.load(os.path.join(GOLD, "shading.npz")), np.load(os.path.join(GOLD, "shading_viewgrad.npz"))
    pre = "shade_" + tag + "_"
    d = {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}
    d.update({k[len(pre):]: torch.from_numpy(v[k]) for k in v.files if k.startswith(pre)})
    return d


def _oracle_grad(d, dtype):
    cv = lambda t: t.to(dtype)  # noqa: E731
    v = cv(d["viewdirs"]).clone().requires_grad_(True)
    out = so.shade(cv(d["base"]), cv(d["rough"]), cv(d["normals"]), v, cv(d["radiance"]), cv(d["vis"]), cv(d["dirs"]), cv(d["areas"]),
                   cv(d["env"]))
    loss = (out["pbr"] * cv(d["w_pbr"])).sum() + sum((out[k] * cv(d["w_" + k])).sum() for k in ("diffuse_light", "specular", "direct", "indirect"))
    loss = loss + (out["mean_incident"] * cv(d["w_inc"])).sum() + (out["mean_global"] * cv(d["w_glob"])).sum()
    loss.backward()
    return v.grad


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_oracle_view_gradient_matches_reference_autograd(tag):
    """fp64: the tolerance tests/test_shading_oracle.py applies to the other gradients; the fp32 keys against the oracle run in fp32,
    likewise relative to the gradient's size at fp32 resolution (the two fp32 programs order their sums differently)."""
    d = _gold(tag)
    assert d["g_viewdirs"].dtype == torch.float64 and d["f32_g_viewdirs"].dtype == torch.float32
    assert float(d["g_viewdirs"].abs().max()) > 1.0
    torch.testing.assert_close(_oracle_grad(d, torch.float64), d["g_viewdirs"], rtol=1e-8, atol=1e-11)
    g32 = _oracle_grad(d, torch.float32)
    assert g32.dtype == torch.float32
    e = sc.row_err(g32, d["f32_g_viewdirs"].double())
    e64 = sc.row_err(d["f32_g_viewdirs"], d["g_viewdirs"])
    print(f"set {tag}: fp32 oracle vs fp32 reference {float(e.max()):.2e}; fp32 reference vs fp64 reference {float(e64.max()):.2e}")
    # two fp32 evaluations of the same formula differ by no more than either differs from fp64 (plus fp32 resolution)
    assert float(e.max()) <= 2.0 * float(e64.max()) + 1e-5


def _row_loss(d, opt, w, viewdirs):
    out = so.shade(d["base_color"], d["roughness"], d["normals"], viewdirs, torch.nan_to_num(d["radiance"], nan=0.0) *
                   (1.0 if opt["radiance_ratio"] is None else opt["radiance_ratio"]), d["visibility"], d["dirs"], d["areas"], d["env"],
                   softplus=opt["softplus"], scale=opt["scale"], transform=opt["transform"])
    return sum((out[k] * w[k]).sum(-1) for k in w)


_TABLE = {}


def _table(run):
    """(inputs, labels, options, probe, threshold rows, weights, fp64 gradients, E32) of a run, computed once."""
    if run["id"] not in _TABLE:
        d, lab, opt = vc.build(run)
        clean = {k: torch.nan_to_num(v, nan=0.0) for k, v in d.items()}
        p = sc.probe(clean, opt)
        thr = vc.threshold_rows(p)
        w = sc.weights(d, thr, seed=11)
        _, g64, E = vc.e32(clean, opt, w, thr)
        _TABLE[run["id"]] = (d, lab, opt, p, thr, w, g64, E)
    return _TABLE[run["id"]]


@pytest.mark.parametrize("run", vc.CPU_RUNS, ids=lambda r: r["id"])
def test_table_thresholds_finiteness_and_central_differences(run):
    d, lab, opt, p, thr, w, g64, E = _table(run)
    share = float(thr.double().mean())
    print(f"{run['id']}: threshold share {share:.4f}, E32 d_viewdirs {E['d_viewdirs']:.2e}, max |d_viewdirs| {float(g64['viewdirs'].abs().max()):.3g}")
    assert share <= vc.MAX_THRESHOLD_SHARE
    assert float(g64["viewdirs"].abs().max()) > 0
    # weights on every row: still finite, in both precisions (e32 asserts it)
    clean = {k: torch.nan_to_num(v, nan=0.0) for k, v in d.items()}
    vc.e32(clean, opt, sc.weights(d, None, seed=12), thr)
    # exactly-zero rows (a zero view direction; every sample at H = 0 behind the surface), in both precisions
    z = vc.exact_zero_rows(lab)
    if bool(z.any()):
        _, g32 = vc.oracle_run(clean, opt, sc.weights(d, None, seed=12), torch.float32)
        _, g64a = vc.oracle_run(clean, opt, sc.weights(d, None, seed=12), torch.float64)
        assert bool((g32["viewdirs"][z] == 0).all()) and bool((g64a["viewdirs"][z] == 0).all())
    # central differences, fp64, on the rows that are differentiable: no threshold, no exact zero of a norm or of the sign's argument
    # (there the function jumps: a zero vector becomes a unit vector under any perturbation)
    rows = lambda m: m.reshape(m.shape[0], -1).any(1)  # noqa: E731
    ok = ~thr & ~rows(p["norm_h"] == 0) & ~rows(p["norm_v"] == 0) & ~rows(p["sgn_arg"] == 0) & ~rows(p["norm_n"] == 0)
    ok &= ~rows(p["norm_h"] < 1e-6) & ~rows(p["sgn_arg"].abs() < 1e-5)
    if run["Ns"] * thr.numel() > 40000 or not bool(ok.any()):
        return
    h = 1e-7
    fd = torch.zeros_like(g64["viewdirs"])
    for j in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[j] = h
        fd[:, j] = (_row_loss(clean, opt, w, clean["viewdirs"] + e) - _row_loss(clean, opt, w, clean["viewdirs"] - e)) / (2 * h)
    # bound per row: 1e-4 of the row's size (the O(h^2) term and the distance to the nearest kink), plus the cancellation of the
    # difference itself: a few hundred roundings of the row's loss terms, divided by h
    g = g64["viewdirs"]
    size = torch.maximum(g.abs().max(1).values, 1e-6 * g.abs().max())
    out = so.shade(clean["base_color"], clean["roughness"], clean["normals"], clean["viewdirs"], clean["radiance"] *
                   (1.0 if opt["radiance_ratio"] is None else opt["radiance_ratio"]), clean["visibility"], clean["dirs"], clean["areas"],
                   clean["env"], softplus=opt["softplus"], scale=opt["scale"], transform=opt["transform"])
    mag = sum((out[k] * w[k]).abs().sum(-1) for k in w)
    err = ((g - fd).abs().max(1).values / (1e-4 * size + 256 * 2.2e-16 * mag / h))[ok]
    print(f"  central differences on {int(ok.sum())} rows: max error / bound {float(err.max()):.2e}")
    assert float(err.max()) <= 1.0


def test_view_alignment_holds_what_it_is_named_for():
    run = next(r for r in vc.RUNS if r["case"] == "view_alignment")
    d, lab, opt, p, thr, w, g64, E = _table(run)
    assert run["Ns"] == 65 and lab.shape[0] == 197
    f = {k: d[k].float() for k in ("dirs", "viewdirs")}   # the kernels' inputs
    al, zv, ah = (torch.from_numpy(lab == k) for k in ("aligned", "zero_view", "all_h0"))
    assert int(al.sum()) >= 3 and int(zv.sum()) >= 3 and int(ah.sum()) >= 3 and int((lab == "ordinary").sum()) > 150
    assert bool((f["dirs"][al] == f["viewdirs"][al][:, None]).all(-1).any(1).all())            # dirs == viewdirs, bit for bit
    assert bool((f["dirs"][~zv] == -f["viewdirs"][~zv][:, None]).all(-1).any(1).all())         # dirs == -viewdirs, bit for bit
    assert bool((p["VoH"][al] >= 1 - 1e-12).any(1).all()) and bool(thr[al].all())               # V.H = 1: thresholds by construction
    assert bool((p["norm_h"][~zv] == 0).any(1).all()) and bool((p["norm_h"][ah] == 0).all())    # H = 0 exactly
    assert bool((p["norm_v"][zv] == 0).all()) and bool((p["norm_v"][~zv] > 0.5).all())          # V = 0
    assert bool((p["ndl"][ah] < 0).all())                                                        # every sample behind the surface
    assert not bool(thr[zv].any()) and not bool(thr[ah].any())                                   # exact zeros are not thresholds
    assert float(g64["viewdirs"][torch.from_numpy(lab == "ordinary")].abs().max()) > 0


def test_runs_cover_both_sides_of_the_chunk_and_a_second_batch():
    ns = {r["Ns"] for r in vc.RUNS}
    assert 1 in ns and 65 in ns
    big = [r for r in vc.RUNS if r.get("n", 0) > 256 * 12 * 4]
    assert len(big) == 1 and big[0]["Ns"] == 8
    ids = {r["id"] for r in vc.RUNS}
    assert {r["id"] for r in sc.RUNS} <= ids and len(ids) == len(vc.RUNS)
    assert any(r["lattice"] for r in vc.RUNS) and any(r["ratio"] == 0.0 for r in vc.RUNS)


def test_public_surface_of_the_view_gradient(built):
    from gaussian_renderer import _native, shading
    from svgir_harness import workloads
    for fn in (shading.rendering_equation4, shading.shade_and_pack, shading.render_shaded, workloads.TrainStep.__init__):
        prm = inspect.signature(fn).parameters
        assert "view_gradient" in prm, fn
        assert prm["view_gradient"].default is False, fn
        assert prm["view_gradient"].kind is inspect.Parameter.KEYWORD_ONLY, fn
    hdr = open(os.path.join(ROOT, "include", "svgir_raster.h")).read()
    assert re.search(r"\bint svgir_shade_backward_view\s*\(", hdr) and "svgir_shade_backward_view" in _native.EXPORTS
    assert hasattr(_native.lib, "svgir_shade_backward_view")
    body = re.search(r"typedef struct svgir_grads \{(.*?)\} svgir_grads;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [s for s in body.split(";") if s.strip()][-1].split("*")[-1].strip() == "dL_dviewdirs"
    assert _native.Grads._fields_[-1][0] == "dL_dviewdirs"
    assert re.search(r"#define SVGIR_ABI_VERSION (\d+)", hdr).group(1) == "14" and _native.lib.svgir_abi_version() == 14
    # the C entry point validates before any HIP call
    assert _native.lib.svgir_shade_backward_view(None, *([None] * 12)) == -1
