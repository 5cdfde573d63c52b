"""The oracle and the case table of the spherical-Gaussian direct light (tests/sg_light_cases.py), on the CPU:
  * the oracle is pinned by tests/golden/sg_light.npz -- the reference's own render_envmap_sg / compute_envmap / rendering_equation4 and its
    autograd gradients (scripts/make_golden_sg.py): in fp64 the two agree to rounding, and the reference's fp32 results lie within the
    fixture's own fp32 error (reference fp32 against reference fp64, printed) of the fp64 oracle;
  * the gradient formulas of include/svgir_raster.h equal autograd of the fp64 forward, and central differences on three lobes;
  * the table holds what the GPU test relies on: no sample's light within 1e-3 relative of the clamp at 64, every special case shows what
    it is named for, few rows on a threshold of the existing arithmetic;
  * E32 / G32 per case, printed.
"""
import os

import numpy as np
import pytest
import torch

import sg_light_cases as sg
import shading_cases as sc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sg_light.npz")


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_oracle_reproduces_the_reference_light():
    g = np.load(GOLD)
    lobes, dirs = torch.from_numpy(g["eval_lgtSGs"]), torch.from_numpy(g["eval_dirs"])
    L = sg.sg_light(lobes, dirs)
    own32 = _rel(g["eval_light_f32"], g["eval_light"])
    print(f"  render_envmap_sg: oracle fp64 vs reference fp64 {_rel(L, g['eval_light']):.2e}; reference fp32 vs fp64 {own32:.2e}, "
          f"vs oracle {_rel(g['eval_light_f32'], L):.2e}")
    assert _rel(L, g["eval_light"]) < 1e-12
    assert _rel(g["eval_light_f32"], L) <= 2 * own32 + 1e-12
    assert float(L[:32].max()) > 0.05     # (the directions into the lobes see them)
    # compute_envmap's grid (scene/direct_light_sg.py:66-80), restated
    phi, theta = torch.meshgrid([torch.linspace(0., np.pi, 8), torch.linspace(1.0 * np.pi, -1.0 * np.pi, 16)], indexing="ij")
    grid = torch.stack([torch.cos(theta) * torch.sin(phi), torch.sin(theta) * torch.sin(phi), torch.cos(phi)], dim=-1)
    env = sg.sg_light(lobes, grid.double())
    assert env.shape == (8, 16, 3)
    assert _rel(env, g["envmap_8x16"]) < 1e-12


@pytest.mark.parametrize("tag", ["a", "b"])
def test_oracle_reproduces_the_reference_shading_and_gradients(tag):
    g = np.load(GOLD)
    pre = "shade_" + tag + "_"
    t = lambda k: torch.from_numpy(g[pre + k])  # noqa: E731
    L = sg.sg_light(t("lgtSGs"), t("dirs"))
    assert bool(((L - 64).abs() > 64e-3).all())     # no sample at the clamp
    names = {"pbr": "pbr", "inc": "mean_incident", "glob": "mean_global", "diffuse_light": "diffuse_light", "specular": "specular",
             "direct": "direct", "indirect": "indirect"}
    leaves = {"lgtSGs": "lgtSGs", "base": "base", "rough": "rough", "normals": "normals"}
    for loss_tag in ("gs", "gw"):
        lv = {k: t(k).clone().requires_grad_(True) for k in leaves}
        out = sg.shade(lv["base"], lv["rough"], lv["normals"], t("viewdirs"), t("radiance"), t("vis"), t("dirs"), t("areas"), lv["lgtSGs"])
        if loss_tag == "gs":
            for k, ok in names.items():
                own32 = _rel(g[pre + "out_" + k + "_f32"], g[pre + "out_" + k])
                e64, e32 = _rel(out[ok], g[pre + "out_" + k]), _rel(g[pre + "out_" + k + "_f32"], out[ok])
                print(f"  {tag} {k}: oracle vs reference fp64 {e64:.2e}; reference fp32 vs fp64 {own32:.2e}, vs oracle {e32:.2e}")
                assert e64 < 1e-11 and e32 <= 2 * own32 + 1e-12, k
            loss = out["pbr"].sum()
        else:
            loss = sum((out[ok] * t("w_" + k)).sum() for k, ok in names.items())
        grads = torch.autograd.grad(loss, [lv[k] for k in leaves])
        for k, gv in zip(leaves, grads):
            ref, ref32 = g[pre + loss_tag + "_" + k], g[pre + loss_tag + "_" + k + "_f32"]
            own32 = _rel(ref32, ref)
            print(f"  {tag} {loss_tag} d_{k}: oracle vs reference fp64 {_rel(gv, ref):.2e}; reference fp32 vs fp64 {own32:.2e}, "
                  f"vs oracle {_rel(ref32, gv):.2e}")
            assert _rel(gv, ref) < 1e-10 and _rel(ref32, gv) <= 2 * own32 + 1e-12, (loss_tag, k)
    assert float(torch.from_numpy(g[pre + "gs_lgtSGs"]).abs().max()) > 0


def test_gradient_formulas_match_autograd_and_central_differences():
    for cid in ("P65-Ns128-M32-ratio", "signs-and-zeros", "unnormalised-dirs", "sharp-on-axis"):
        d = sg.build(sg.BY_ID[cid])
        lobes = d["lobes"].clone().requires_grad_(True)
        gen = torch.Generator().manual_seed(5)
        gl = torch.randn(d["dirs"].shape, generator=gen, dtype=torch.float64)
        (sg.sg_light(lobes, d["dirs"]) * gl).sum().backward()
        closed = sg.sg_grad(d["lobes"], d["dirs"], gl)
        err = sc.row_err(closed, lobes.grad)
        print(f"  {cid}: closed form vs autograd, worst lobe {float(err.max()):.2e}")
        assert float(err.max()) < 1e-11
        if cid == "signs-and-zeros":    # sign(0) = 0: no gradient where the raw value is 0
            assert float(closed[1, 3]) == 0.0 and float(closed[2, 5]) == 0.0 and not bool(closed[3, 4:].any()) and float(closed[4, 4]) == 0.0
            assert float(closed[0, 3].abs()) > 0 and bool((closed[0, 4:] != 0).all())
    # central differences on three lobes of the reference-scale case
    d = sg.build(sg.BY_ID["P65-Ns128-M32-ratio"])
    gl = torch.randn(d["dirs"].shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    closed = sg.sg_grad(d["lobes"], d["dirs"], gl)
    f = lambda lb: float((sg.sg_light(lb, d["dirs"]) * gl).sum())  # noqa: E731
    for m in (0, 1, 7):    # sharpness x20, x20, x20 / x100 rows of the table
        for j in range(7):
            h = 1e-6 * max(1.0, abs(float(d["lobes"][m, j])))
            lp, lm = d["lobes"].clone(), d["lobes"].clone()
            lp[m, j] += h
            lm[m, j] -= h
            num = (f(lp) - f(lm)) / (2 * h)
            scale = max(float(closed[m].abs().max()), 1e-12)
            assert abs(num - float(closed[m, j])) <= 1e-5 * scale + 1e-9, (m, j, num, float(closed[m, j]))


def test_table_conditions():
    seen = dict(P=set(), Ns=set(), M=set())
    for case in sg.CASES:
        d = sg.build(case)
        for k in seen:
            seen[k].add(case[k])
        for k, v in d.items():
            assert torch.equal(v, v.float().double()), (case["id"], k)    # fp32-representable
        L = sg.light64(d)
        if case["special"] == "zero_norm":
            assert bool(torch.isnan(L).all())        # NaN * 0 = NaN: every sample, as in torch
            continue
        assert bool(torch.isfinite(L).all()) and bool((L >= 0).all())
        near = (L - 64).abs() <= 1e-3 * 64
        assert not bool(near.any()), (case["id"], int(near.sum()))
        thr = sg.threshold_rows(d)
        share = float(thr.double().mean())
        print(f"  {case['id']}: max L {float(L.max()):.3g}, samples over 64: {int((L > 64).any(-1).sum())}, threshold rows {int(thr.sum())} "
              f"of {thr.numel()} ({share:.1%})")
        assert share <= sc.MAX_THRESHOLD_SHARE or thr.numel() < 20 and int(thr.sum()) <= 1, case["id"]
        sp = case["special"]
        if sp == "clamp":
            over = (L > 64).any(-1)
            assert 0.05 < float(over.double().mean()) < 0.95            # part of the samples clamp
        elif sp == "sharp":
            e_on = torch.exp(d["lobes"][0, 3].abs() * ((d["dirs"][0, 0] * torch.tensor([0., 0., 1.], dtype=torch.float64)).sum() - 1))
            e_off = torch.exp(d["lobes"][0, 3].abs() * ((d["dirs"][0, 1] * torch.tensor([0., 0., 1.], dtype=torch.float64)).sum() - 1))
            assert float(e_on) == 1.0 and float(e_off) == 0.0 and float(d["lobes"][0, 3]) == 1000.0 and float(d["lobes"][1, 3]) == -1000.0
            assert float(torch.exp(torch.tensor(-2000.0, dtype=torch.float32))) == 0.0
        elif sp == "occluded":
            assert not bool(d["visibility"].any())
        elif sp == "unnormalised":
            nrm = d["dirs"].norm(dim=-1)
            assert float(nrm.min()) < 0.6 and float(nrm.max()) > 1.4
        elif sp == "signs":
            lb = d["lobes"]
            assert float(lb[0, 3]) < 0 and bool((lb[0, 4:] < 0).all()) and float(lb[1, 3]) == 0 and float(lb[2, 5]) == 0 and not bool(lb[3, 4:].any())
        else:
            assert not bool((L > 64).any())
    assert seen["P"] >= {1, 15, 16, 17, 65, 257} and seen["Ns"] >= {1, 7, 64, 65, 128, 129, 384} and seen["M"] >= {1, 3, 4, 5, 32, 33, 128}
    assert {c["mode"] for c in sg.CASES} == {None, True, False} and any(c["lattice"] for c in sg.CASES)
    assert any(c["ratio"] is not None for c in sg.CASES) and any(c["view"] for c in sg.CASES)


@pytest.mark.parametrize("case", [c for c in sg.CASES if c["grads"]], ids=lambda c: c["id"])
def test_fp32_loss_of_the_oracle(case):
    d = sg.build(case)
    thr = sg.threshold_rows(d)
    w = sg.weights(case, d, thr)
    o64, g64, E = sg.e32(case, d, w, thr)
    print("  " + case["id"] + ": " + ", ".join(f"{k} {v:.1e}" for k, v in E.items()))
    assert all(np.isfinite(v) for v in E.values())
    assert float(g64["lobes"].abs().max()) > 0 or case["special"] == "occluded"
