"""The HIP shading kernels (csrc/shade.hip: both forward layouts and the backward) at their clamps, poles and degenerate vectors:
every run of tests/shading_cases.py against the fp64 oracle, through rendering_equation4 (forward + backward) and through
shade_and_pack in training and evaluation packing.

Budget.  For every non-threshold row and every tensor -- the eight reduced outputs, features / vfeatures, d base, d rough, d normals,
d radiance, d env (and d radiance_ratio) -- the per-row error of HIP against the fp64 oracle is at most 1.5 x E32 + 1e-4, where E32
is the largest per-row error of the reference arithmetic in fp32 against itself in fp64 on the same inputs (computed here, per run
and tensor; tests/shading_cases.py defines the per-row error, the threshold rows and why they are held to finiteness only).  The
upstream weights vanish on the threshold rows; a second call with weights on every row must return finite outputs and gradients
everywhere.  Everything runs with NaN-poisoned buffers (conftest.py).

The light.  Softplus maps (DirectLightMap) go through the public entry points with a `.env` light.  The EnvLight mode (no softplus,
scale 1, optional lookup rotation) exists in the reference only behind a 32x64 down-sample without a gradient to the map; to reach
every env size and d env in that mode the test hands the light's four properties to the entry points directly (`_env_of` replaced
for a light that carries them), and test_envlight_class_equals_the_explicit_light shows on the rotated pole case that the
reference's class arrives at the same bits.

With NaN entries in the radiance cache (material_ends with a ratio) `mean_local` stays out of the loss of the rendering_equation4
call: there the entry point returns the cleaned product formed by torch, whose autograd adds 0 x NaN to the ratio's gradient; the
packed calls, where the kernels form that mean, keep the weight."""
import numpy as np
import pytest
import torch

import shading_cases as sc
from svgir_harness import shade_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _ExplicitLight:
    def __init__(self, env, softplus, scale, transform):
        self.spec = (env, softplus, scale, transform)


def _light(monkeypatch, shading, env, opt, dev):
    if opt["softplus"] and opt["transform"] is None and opt["scale"] == 2.0:
        return shade_inputs.Light(env)
    monkeypatch.setattr(shading, "_env_of", lambda light: light.spec)
    tr = None if opt["transform"] is None else opt["transform"].float().to(dev)
    return _ExplicitLight(env, opt["softplus"], opt["scale"], tr)


def _inputs(run, dev):
    """(inputs fp64, labels, options, lattice or None): lattice runs take the directions the kernels generate."""
    from gaussian_renderer import shading
    if not run["lattice"]:
        return (*sc.build(run), None)
    d, _, _ = sc.build(run)
    geo = torch.nn.functional.normalize(d["geo_normals"].float(), dim=-1).to(dev)
    offs = torch.rand(geo.shape[0], generator=torch.Generator().manual_seed(2)).to(dev) * 6.2831855
    lat = shading.FibonacciLattice(geo, run["Ns"], offs)
    return (*sc.build(run, dirs=lat.dirs()), lat)


def _hip(monkeypatch, d, opt, lat, w, api, view, dev):
    """One forward + backward through the HIP kernels under the upstream weights w: (outputs, gradients) named like the oracle's."""
    from gaussian_renderer import shading
    f32 = lambda t: t.float().to(dev)  # noqa: E731
    names = [k for k in sc.LEAVES if not (k == "radiance" and opt["radiance_ratio"] is not None)]
    lv = {k: f32(d[k]).requires_grad_(True) for k in names}
    kw = {}
    rad = lv.get("radiance")
    if opt["radiance_ratio"] is not None:
        lv["radiance_ratio"] = torch.tensor(opt["radiance_ratio"], dtype=torch.float32, device=dev, requires_grad=True)
        rad, kw = f32(d["radiance"]), dict(radiance_ratio=lv["radiance_ratio"])
    dirs, areas = (lat, None) if lat is not None else (f32(d["dirs"]), f32(d["areas"]))
    light = _light(monkeypatch, shading, lv["env"], opt, dev)
    if api == "rendering_equation4":
        pbr, ex = shading.rendering_equation4(lv["base_color"], lv["roughness"], lv["normals"], f32(d["viewdirs"]), rad, light,
                                              visibility_precompute=f32(d["visibility"]), incident_dirs_precompute=dirs,
                                              incident_areas_precompute=areas, **kw)
        out = dict(pbr=pbr, mean_incident=ex["incident_lights"].mean(-2), mean_local=ex["local_incident_lights"].mean(-2),
                   mean_global=ex["global_incident_lights"].mean(-2), **{k: ex[k] for k in ("diffuse_light", "specular", "direct", "indirect")})
    else:
        vm = torch.eye(4, dtype=torch.float64)
        vm[:3, :3] = view
        f, vf, red = shading.shade_and_pack(lv["base_color"], lv["roughness"], lv["normals"], f32(d["viewdirs"]), rad, light,
                                            f32(d["visibility"]), dirs, areas, f32(vm), api == "pack_train", **kw)
        out = dict(features=f, vfeatures=vf, pbr=red[:, 0:12])
    sum((out[k] * f32(w[k])).sum() for k in w).backward()
    torch.cuda.synchronize()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in lv.items()}
    return {k: v.detach() for k, v in out.items()}, grads


def _budget(tag, got, ref, E, thr, lab, bad):
    for k, r in ref.items():
        if k not in got:
            continue
        whole = r.dim() == 0 or k == "env"
        key = ("d_" + k) if tag.endswith("grad") else k
        e = sc.row_err(got[k].reshape(1, -1), r.reshape(1, -1), whole=True) if whole else sc.row_err(got[k], r)
        if not whole:
            e = torch.where(thr, torch.zeros_like(e), e)
        lim = 1.5 * E[key] + 1e-4
        worst = int(e.argmax())
        print(f"    {tag} {key}: HIP {float(e.max()):.2e} (row {worst} {'' if whole else lab[worst]}), E32 {E[key]:.2e}, budget {lim:.2e}")
        if not bool(torch.isfinite(e).all()) or float(e.max()) > lim:
            rows = [] if whole else [f"{i}:{lab[i]}:{float(e[i]):.1e}" for i in torch.nonzero(~(e <= lim)).flatten().tolist()[:8]]
            bad.append(f"{tag} {key}: HIP err {float(e.max()):.3e} > 1.5 x E32 {E[key]:.3e} + 1e-4 {rows}")


@pytest.mark.parametrize("run", sc.RUNS, ids=lambda r: r["id"])
def test_edge_inputs_within_the_reference_fp32_budget(built, monkeypatch, run):
    dev = torch.device(DEV)
    d, lab, opt, lat = _inputs(run, dev)
    clean = {k: torch.nan_to_num(v, nan=0.0) for k, v in d.items()}
    thr = sc.threshold_rows(sc.probe(clean, opt))
    assert float(thr.double().mean()) <= sc.MAX_THRESHOLD_SHARE
    view = sc.view3x3()
    nan_cache = bool(torch.isnan(d["radiance"]).any())
    bad = []
    for api in ("rendering_equation4", "pack_train", "pack_eval"):
        training = None if api == "rendering_equation4" else api == "pack_train"
        for every_row in (False, True):
            w = sc.weights(d, None if every_row else thr, seed=3 + len(api), training=training)
            if nan_cache and api == "rendering_equation4":
                del w["mean_local"]      # (module docstring; a zero weight would still send 0 x NaN through torch's product)
            out, grads = _hip(monkeypatch, d, opt, lat, w, api, view, dev)
            for k, v in {**out, **{"d_" + k: g for k, g in grads.items()}}.items():
                assert bool(torch.isfinite(v).all()), f"{api} {k}: {int((~torch.isfinite(v)).sum())} non-finite entries" + \
                    (" (weights on every row)" if every_row else "")
            if every_row:
                continue
            o64, g64, E = sc.e32(d, opt, w, thr, view, training)
            print(f"  {run['id']} {api}: {int(thr.sum())} threshold rows of {thr.numel()}")
            _budget(api, out, o64, E, thr, lab, bad)
            _budget(api + " grad", grads, g64, E, thr, lab, bad)
    assert not bad, "\n".join([run["id"]] + bad)


def test_envlight_class_equals_the_explicit_light(built, monkeypatch):
    """scene/envmap.py EnvLight with `.envmap` (32x64: its down-sample is the identity) and `.transform`: bit-identical to the explicit
    (env, no softplus, scale 1, transform) light of the runs above, on the rotated pole case."""
    from gaussian_renderer import shading
    dev = torch.device(DEV)
    run = next(r for r in sc.RUNS if r["case"] == "env_poles_and_seam" and r["transform"] and (r["He"], r["We"]) == (32, 64))
    d, lab, opt = sc.build(run)
    f32 = lambda t: t.float().to(dev)  # noqa: E731

    class EnvLight:
        def __init__(self, envmap, transform):
            self.envmap, self.transform = envmap, transform

    res = []
    for light in (EnvLight(f32(d["env"])[0], f32(opt["transform"])), None):
        if light is None:
            light = _light(monkeypatch, shading, f32(d["env"]), opt, dev)
        with torch.no_grad():
            pbr, ex = shading.rendering_equation4(f32(d["base_color"]), f32(d["roughness"]), f32(d["normals"]), f32(d["viewdirs"]),
                                                  f32(d["radiance"]), light, visibility_precompute=f32(d["visibility"]),
                                                  incident_dirs_precompute=f32(d["dirs"]), incident_areas_precompute=f32(d["areas"]))
        res.append((pbr, ex["direct"], ex["global_incident_lights"]))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", sc.FUSED_CASES)
def test_fused_view_with_edge_materials_is_bit_identical(built, case):
    """The small surface scene of test_fused_view_is_bit_identical_small with the edge rows as the surfels' materials (row i mod n):
    render_shaded stays bit-identical to shade-then-rasterize, and every gradient it returns is finite."""
    import test_gpu_fused_shade as fs
    from svgir_harness import runner, scenes
    dev = torch.device(DEV)
    sc_ = scenes.surface_scene(P=6000, W=176, H=144, seed=41, sh_degree=2, variant="svgss", S=4, VS=52, scale_lo=0.01, scale_hi=0.06)
    sct = runner.to_torch(sc_, dev)
    st = runner.settings(sct, "svgss")
    e, lab, opt = shade_inputs.edge_case(case, sc.CASES[case]["n"], 64)
    assert opt["softplus"] and opt["transform"] is None
    rows = torch.arange(6000) % e["base_color"].shape[0]
    d = {k: e[k][rows].float().contiguous().to(dev) for k in sc.INPUTS if k != "env"}
    d["env"] = e["env"].float().to(dev)
    la, lb = fs._leaves(sct, d), fs._leaves(sct, d)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in scenes.upstream_grads(sc_, "svgss", seed=6).items()}
    for _ in range(3):   # (the third view of a workload runs the speculative launch sequence)
        fs._compare(sct, st, d, scenes.upstream_grads(sc_, "svgss", seed=6), True)
    oa, m2a, _ = fs._unfused(sct, st, d, la, True)
    fs._loss(oa, gt).backward()
    ob, m2b, _ = fs._fused(sct, st, d, lb, True)
    fs._loss(ob, gt).backward()
    torch.cuda.synchronize()
    blended = ob[7][:, 0] > 0
    assert int(blended.sum()) > 500
    for k in lb:
        assert bool(torch.isfinite(lb[k].grad).all()) and bool(torch.isfinite(la[k].grad).all()), k
    for k in ("base_color", "roughness", "normals", "radiance"):
        assert torch.equal(la[k].grad, lb[k].grad), k
        assert float(lb[k].grad[blended].abs().max()) > 0, k
