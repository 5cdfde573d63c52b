"""The shading edge-input cases on the fp64 oracle alone (no GPU): every case of tests/shading_cases.py holds what it is named for,
at most 5 % of its rows sit on a threshold, the reference arithmetic stays finite on all of it in fp64 and in fp32, and what the
reference's own fp32 arithmetic loses on it (E32, the yardstick of tests/test_gpu_shading_edges.py) is computed and printed.

Shares are floors of a few per cent of the case, counted on the probe of tests/shading_cases.py (an instrumented restatement of
oracle/shading_oracle.py, tied to the oracle by test_probe_restates_the_oracle).

E32 measured (largest per-row error of the fp32 oracle against the fp64 oracle over non-threshold rows; run with -s for the table):
see DESIGN.md section 5, "Shading edge inputs"."""
import math

import numpy as np
import pytest
import torch

import shading_cases as sc
from oracle import shading_oracle as so

HOST_RUNS = [r for r in sc.RUNS if not r["lattice"]]     # (lattice mode takes its directions from the kernels: GPU test)


def _first(case, **kw):
    return next(r for r in sc.RUNS if r["case"] == case and not r["lattice"] and all(r[k] == v for k, v in kw.items()))


def _probe(run):
    d, lab, opt = sc.build(run)
    return d, lab, opt, sc.probe({k: torch.nan_to_num(v, nan=0.0) for k, v in d.items()}, opt)


def _share(mask):
    return float(mask.double().mean())


@pytest.mark.parametrize("case", list(sc.CASES))
def test_rows_are_labelled_and_partial(case):
    n = sc.CASES[case]["n"]
    assert n <= 512 and n % 16 != 0
    d, lab, opt = sc.build(_first(case))
    assert lab.shape == (n,) and all(d[k].dtype == torch.float64 and d[k].shape[0] in (1, n) for k in sc.INPUTS)
    small = [r["Ns"] for r in sc.RUNS if r["Ns"] < 128]
    big = [r["Ns"] for r in sc.RUNS if r["Ns"] >= 128]
    assert any(s % 4 for s in small) and 130 in big
    assert {r["Ns"] < 128 for r in sc.RUNS if r["case"] == case} == {True, False}, "both forward layouts"
    # unit directions never exceed length 1 (the reference's arccos of the raw z is NaN beyond)
    assert float(d["dirs"].norm(dim=-1).max()) <= 1 + 1e-12


@pytest.mark.parametrize("run", [_first("mirror_lobe", Ns=61), _first("mirror_lobe", Ns=130)], ids=lambda r: r["id"])
def test_mirror_lobe_sits_inside_and_on_the_edge_of_the_denominator_clamp(run):
    d, lab, opt, p = _probe(run)
    assert float(d["roughness"].min()) == pytest.approx(0.09) and _share(torch.from_numpy(lab == "mirror_0.09")) >= 0.7
    some = d["roughness"][torch.from_numpy(lab == "mirror_0.09_0.15")]
    assert some.numel() and float(some.min()) >= 0.09 and float(some.max()) <= 0.15
    clamped, releasing = _share(p["nom"] < 1e-6), _share((p["nom"] > 1e-6) & (p["nom"] < 1e-4))
    print(f"{run['id']}: pairs with nom < 1e-6: {clamped:.3f}, in (1e-6, 1e-4): {releasing:.3f}")
    assert clamped >= 0.05 and releasing >= 0.03
    # the clamp is active over the peak: the pairs aimed at (within 1e-3 rad of the reflection about their corner's normal)
    rows = torch.from_numpy(lab == "mirror_0.09")
    s = torch.arange(0, run["Ns"], 3)
    aimed = p["nom"][rows][:, s, (s // 3) % 4]
    assert float(aimed.max()) < 1e-6 and float(p["NoH"][rows][:, s, (s // 3) % 4].min()) > 1 - 2e-6


def test_grazing_view_has_both_signs_sign_zero_and_the_two_magnitudes():
    d, lab, opt, p = _probe(_first("grazing_view"))
    sg = p["sgn_arg"]
    for mag in (1e-2, 1e-4):
        at = ((sg.abs() - mag).abs() <= 1e-9)
        assert _share(at.all(1)) >= 0.15 and _share(at & (sg > 0)) >= 0.05 and _share(at & (sg < 0)) >= 0.05, mag
    assert _share((sg == 0).all(1)) >= 0.10, "rows with sign 0 at every corner"
    assert _share((sg > 0).any(1) & (sg < 0).any(1)) >= 0.10, "corners of one surfel on both sides of the sign"
    # ... and the sign-0 rows stay exact zeros in fp32
    f32 = sc.probe({k: v.float() for k, v in d.items()}, opt)
    assert torch.equal(f32["sgn_arg"] == 0, sg == 0)
    assert float(p["NoV"][(sg.abs() - 1e-4).abs() <= 1e-9].min()) > 5e-5      # (N flipped to the viewer: N.V = +1e-4, above its clamp)


def test_backfacing_and_opposed_has_what_it_says():
    d, lab, opt, p = _probe(_first("backfacing_and_opposed"))
    assert _share(p["ndl"] <= 0) >= 0.15, "samples behind the raw normal"
    assert _share(p["norm_h"] == 0) >= 0.10, "L = -V exactly: H = 0"
    assert _share(p["norm_v"] == 0) >= 0.05, "zero view directions"
    f32 = sc.probe({k: v.float() for k, v in d.items()}, opt)
    assert torch.equal(f32["norm_h"] == 0, p["norm_h"] == 0)


@pytest.mark.parametrize("run", [r for r in HOST_RUNS if r["case"] == "env_poles_and_seam" and r["Ns"] < 128], ids=lambda r: r["id"])
def test_env_poles_and_seam_reach_the_padding(run):
    d, lab, opt, p = _probe(run)
    He, We = p["He"], p["We"]
    assert (He, We) == (run["He"], run["We"])
    row_out, col_out = (p["y0"] < 0) | (p["y0"] + 1 >= He), (p["x0"] < 0) | (p["x0"] + 1 >= We)
    print(f"{run['id']}: samples with an out-of-range tap row {_share(row_out):.3f}, column {_share(col_out):.3f}")
    assert _share(p["y0"] == -1) >= 0.02, "north pole: row -1"
    if not run["transform"]:   # (theta = -pi needs y = -0.0, which no sum of products returns: the rotated lookups meet the seam at +pi)
        assert _share(p["x0"] + 1 == We) >= 0.02, "seam: column We"
    assert _share(p["y0"] == He - 2) >= 0.02 and _share(p["x0"] == 0) >= 0.02      # south pole, the seam's other side
    assert _share((p["y0"] == 1) | (p["y0"] == 0)) >= 0.02 and _share(p["x0"] == We - 2) >= 0.02   # one texel off
    if run["transform"]:   # a direction that is not special itself lands on the pole
        z = d["dirs"][..., 2]
        assert _share((p["y0"] == -1) & (z.abs() < 0.5)) >= 0.01


@pytest.mark.parametrize("run", [r for r in HOST_RUNS if r["case"] == "env_clamp" and r["Ns"] < 128], ids=lambda r: r["id"])
def test_env_clamp_has_every_channel_on_each_side(run):
    d, lab, opt, p = _probe(run)
    assert opt["softplus"] != run["hdr"]
    if not run["hdr"]:
        assert float(d["env"].abs().max()) <= 40.0 and float(d["env"].max()) > 32 and float(d["env"].min()) < -32
    for ch in range(3):
        e = p["env_pre"][..., ch]
        assert _share(e > 64) >= 0.10 and _share((e >= 0) & (e <= 64)) >= 0.10, ch
        if run["hdr"]:
            assert _share(e < 0) >= 0.05, ch
        tex = p["sp"][..., ch] * opt["scale"]
        assert _share(tex > 64) >= 0.10 and _share(tex <= 64) >= 0.10


def test_vector_scales_cross_the_norm_clamp():
    d, lab, opt, p = _probe(_first("vector_scales"))
    nn = p["norm_n"]
    assert _share(((nn > 0) & (nn < 1e-12)).all(1)) >= 0.08, "rows under the 1e-12 norm clamp"
    for sc_, tol in ((1e-5, 1e-6), (7.0, 0.1), (1e3, 10.0)):
        assert _share(((nn - sc_).abs() <= tol).all(1)) >= 0.08, sc_
    assert _share((nn == 0).any(1)) >= 0.05, "a corner normal exactly zero"
    assert _share((p["norm_v"] - 3).abs() < 1e-9) >= 0.10 and _share(((p["norm_l"] - 0.5).abs() < 1e-9).all(1)) >= 0.10
    assert float(p["norm_l"].max()) <= 1 + 1e-12


def test_material_ends_labels():
    d, lab, opt = sc.build(_first("material_ends", ratio=0.83))
    n = lab.size
    for label in ("rough_0", "rough_0.001", "rough_1", "base_0", "base_1", "vis_0.37", "vis_0", "area_0", "area_varying", "radiance_0",
                  "radiance_1e4"):
        assert (lab == label).sum() >= 0.04 * n, label
    r = torch.from_numpy
    assert float(d["roughness"][r(lab == "rough_0")].abs().max()) == 0 and float(d["roughness"][r(lab == "rough_1")].min()) == 1
    assert float(d["visibility"][r(lab == "vis_0.37")].min()) == 0.37 and float(d["areas"][r(lab == "area_0")].abs().max()) == 0
    assert float(d["areas"][r(lab == "area_varying")].std()) > 1 and float(d["radiance"][r(lab == "radiance_1e4")].max()) > 5e3
    assert int(torch.isnan(d["radiance"]).sum()) >= 3 and opt["radiance_ratio"] == 0.83


@pytest.mark.parametrize("run", [_first(c) for c in sc.CASES] + [_first("env_clamp", hdr=True), _first("env_poles_and_seam", transform=True)],
                         ids=lambda r: r["id"])
def test_probe_restates_the_oracle(run):
    d, lab, opt, p = _probe(run)
    d = {k: torch.nan_to_num(v, nan=0.0) for k, v in d.items()}
    fs = so.ggx(d["normals"], d["viewdirs"], d["dirs"], d["roughness"])
    assert torch.equal(p["fs"], fs) or float((p["fs"] - fs).abs().max()) <= 1e-12 * float(fs.abs().max())
    ld = d["dirs"] if opt["transform"] is None else d["dirs"] @ opt["transform"].T
    look = so.env_lookup(d["env"], ld, opt["softplus"], opt["scale"])
    assert float((p["env_pre"] - look).abs().max()) <= 1e-12 * float(look.abs().max())
    ref = so.shade(*(d[k] for k in sc.INPUTS), softplus=opt["softplus"], scale=opt["scale"], transform=opt["transform"])
    glob = p["env_pre"].clamp(0, 64) * d["visibility"]
    assert float((glob.mean(1) - ref["mean_global"]).abs().max()) <= 1e-12 * float(ref["mean_global"].abs().max())
    geo = d["areas"] * p["ndl"].clamp(min=0)
    spec = (p["fs"][:, :, None, :] * (d["radiance"] + glob)[:, :, :, None] * geo[:, :, None, :]).mean(1).reshape(-1, 12)
    assert float((spec - ref["specular"]).abs().max()) <= 1e-12 * max(float(ref["specular"].abs().max()), 1e-300)


@pytest.mark.parametrize("run", HOST_RUNS, ids=lambda r: r["id"])
def test_threshold_rows_are_few_and_the_reference_is_finite(run):
    """The cap (at most 5 % threshold rows, from the fp64 oracle alone), finiteness of the reference arithmetic in fp64 and fp32 --
    under weights that vanish on the threshold rows and under weights that do not --, and E32 per tensor."""
    d, lab, opt, p = _probe(run)
    thr = sc.threshold_rows(p)
    share = _share(thr)
    assert share <= sc.MAX_THRESHOLD_SHARE, f"{share:.3f} of the rows sit on a threshold"
    _, _, E = sc.e32(d, opt, sc.weights(d, thr, seed=3), thr)
    view = sc.view3x3()
    for training in (True, False):
        _, _, Ep = sc.e32(d, opt, sc.weights(d, thr, seed=4, training=training), thr, view, training)
        for k in ("features", "vfeatures"):
            E[f"{k}[{'train' if training else 'eval'}]"] = Ep[k]
        for k in Ep:
            if k.startswith("d_"):
                E[k] = max(E[k], Ep[k])
    sc.e32(d, opt, sc.weights(d, None, seed=5), torch.zeros_like(thr))     # finiteness with weight on every row
    print(f"E32 {run['id']}: threshold rows {share:.3f}; " + ", ".join(f"{k} {v:.1e}" for k, v in E.items()))
    assert all(np.isfinite(v) for v in E.values())
