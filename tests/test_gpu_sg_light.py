"""The spherical-Gaussian direct light on the GPU (csrc/shade.hip LIGHT_SG instantiations, csrc/sg_light.hpp): every case of
tests/sg_light_cases.py against the fp64 oracle, and the surface around it.

Budget (the rule of tests/test_gpu_shading_edges.py): for every row that is not on a threshold of the existing arithmetic and every tensor --
svgir_sg_eval's light, the reduced columns, features / vfeatures, d base, d rough, d normals, d radiance / d ratio, d viewdirs and d lobes
(a row = a lobe) -- the per-row error of HIP against the fp64 oracle is at most 1.5 x E32 + 1e-4 (1.5 x G32 + 1e-4 for gradients), E32 / G32
the largest per-row error of the same arithmetic in torch fp32 against fp64 on the same inputs, computed here per case and tensor.
Everything runs with NaN-poisoned output buffers (conftest.py: SVGIR_POISON): an element the kernels forget fails the finiteness checks.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sg_light_cases as sg
import shading_cases as sc
from svgir_harness import shade_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sg_light.npz")


def _f32(t, dev=DEV):
    return t.float().to(dev)


def _check(tag, key, got, ref, E, thr, bad, rows_are_lobes=False):
    whole = ref.dim() == 0
    e = sc.row_err(got.reshape(1, -1), ref.reshape(1, -1), whole=True) if whole else sc.row_err(got, ref)
    if not whole and not rows_are_lobes:
        e = torch.where(thr, torch.zeros_like(e), e)
    lim = 1.5 * E[key] + 1e-4
    print(f"    {tag} {key}: HIP {float(e.max()):.2e} (row {int(e.argmax())}), E32 {E[key]:.2e}, budget {lim:.2e}")
    if not bool(torch.isfinite(e).all()) or float(e.max()) > lim:
        bad.append(f"{tag} {key}: HIP err {float(e.max()):.3e} > 1.5 x E32 {E[key]:.3e} + 1e-4")


def test_sg_eval_and_compute_envmap(built):
    from gaussian_renderer import shading
    g = np.load(GOLD)
    lobes, dirs = torch.from_numpy(g["eval_lgtSGs"]), torch.from_numpy(g["eval_dirs"])
    L64 = sg.sg_light(lobes, dirs)
    E = {"light": float(sc.row_err(sg.sg_light(lobes.float(), dirs.float()), L64).max()),
         "envmap": float(sc.row_err(torch.from_numpy(g["envmap_8x16_f32"]).reshape(-1, 3), torch.from_numpy(g["envmap_8x16"]).reshape(-1, 3)).max())}
    bad = []
    got = shading.sg_direct_light(_f32(lobes), _f32(dirs))
    assert got.shape == dirs.shape and bool(torch.isfinite(got).all())
    _check("sg_eval", "light", got, L64, E, None, bad, rows_are_lobes=True)
    # any leading shape; more than one block
    big = torch.cat([dirs] * 5)[:1200].reshape(4, 100, 3, 3)
    got4 = shading.sg_direct_light(_f32(lobes), _f32(big))
    assert got4.shape == big.shape and torch.equal(got4.reshape(-1, 3)[:257], got)
    assert shading.sg_direct_light(_f32(lobes), torch.empty(0, 3, device=DEV)).shape == (0, 3)
    env = shading.compute_envmap(_f32(lobes), 8, 16)
    assert env.shape == (8, 16, 3)
    _check("compute_envmap", "envmap", env.reshape(-1, 3), torch.from_numpy(g["envmap_8x16"]).reshape(-1, 3), E, None, bad, rows_are_lobes=True)
    # the reference's default lobe count, and one lobe
    for M in (1, 128):
        lb = shade_inputs.sg_lobes(M, seed=M).double()
        ref = sg.sg_light(lb, dirs)
        E["M"] = float(sc.row_err(sg.sg_light(lb.float(), dirs.float()), ref).max())
        _check(f"sg_eval M={M}", "M", shading.sg_direct_light(_f32(lb), _f32(dirs)), ref, E, None, bad, rows_are_lobes=True)
    assert not bad, "\n".join(bad)


def _inputs(case, dev):
    from gaussian_renderer import shading
    if not case["lattice"]:
        return sg.build(case), None
    d = sg.build(case)
    geo = torch.nn.functional.normalize(d["geo"].float(), dim=-1).to(dev)
    offs = torch.rand(geo.shape[0], generator=torch.Generator().manual_seed(2)).to(dev) * 6.2831855
    lat = shading.FibonacciLattice(geo, case["Ns"], offs)
    return sg.build(case, dirs=lat.dirs()), lat


def _hip(case, d, lat, w, dev):
    """One forward (+ backward) through the HIP kernels under the upstream weights w: (outputs, gradients) named like the oracle's."""
    from gaussian_renderer import shading
    names = [k for k in sg.LEAVES if not (k == "radiance" and case["ratio"] is not None)]
    lv = {k: _f32(d[k], dev).requires_grad_(True) for k in names}
    kw = {}
    rad = lv.get("radiance")
    if case["ratio"] is not None:
        lv["radiance_ratio"] = torch.tensor(case["ratio"], dtype=torch.float32, device=dev, requires_grad=True)
        rad, kw = _f32(d["radiance"], dev), dict(radiance_ratio=lv["radiance_ratio"])
    vd = _f32(d["viewdirs"], dev)
    if case["view"]:
        lv["viewdirs"] = vd = vd.requires_grad_(True)
        kw["view_gradient"] = True
    dirs, areas = (lat, None) if lat is not None else (_f32(d["dirs"], dev), _f32(d["areas"], dev))
    light = shade_inputs.SGLight(lv["lobes"])
    if case["mode"] is None:
        pbr, ex = shading.rendering_equation4(lv["base_color"], lv["roughness"], lv["normals"], vd, rad, light,
                                              visibility_precompute=_f32(d["visibility"], dev), incident_dirs_precompute=dirs,
                                              incident_areas_precompute=areas, **kw)
        out = dict(pbr=pbr, mean_incident=ex["incident_lights"].mean(-2), mean_local=ex["local_incident_lights"].mean(-2),
                   mean_global=ex["global_incident_lights"].mean(-2), **{k: ex[k] for k in ("diffuse_light", "specular", "direct", "indirect")})
    else:
        vm = torch.eye(4, dtype=torch.float64)
        vm[:3, :3] = sc.view3x3()
        f, vf, red = shading.shade_and_pack(lv["base_color"], lv["roughness"], lv["normals"], vd, rad, light, _f32(d["visibility"], dev), dirs,
                                            areas, _f32(vm, dev), case["mode"], **kw)
        out = dict(features=f, vfeatures=vf, pbr=red[:, 0:12])
    grads = {}
    if case["grads"]:
        sum((out[k] * _f32(w[k], dev)).sum() for k in w).backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in lv.items()}
    torch.cuda.synchronize()
    return {k: v.detach() for k, v in out.items()}, grads


@pytest.mark.parametrize("case", [c for c in sg.CASES if c["grads"]], ids=lambda c: c["id"])
def test_cases_within_the_fp32_budget(built, case):
    dev = torch.device(DEV)
    d, lat = _inputs(case, dev)
    thr = sg.threshold_rows(d)
    w = sg.weights(case, d, thr)
    o64, g64, E = sg.e32(case, d, w, thr)
    out, grads = _hip(case, d, lat, w, dev)
    bad = []
    for k, v in {**out, **{"d_" + k: g for k, g in grads.items()}}.items():
        assert bool(torch.isfinite(v).all()), f"{k}: {int((~torch.isfinite(v)).sum())} non-finite (or never written) entries"
    assert set(grads) == set(g64)
    for k, r in o64.items():
        if k in out:
            _check(case["id"], k, out[k], r, E, thr, bad)
    for k, r in g64.items():
        _check(case["id"], "d_" + k, grads[k], r, E, thr, bad, rows_are_lobes=(k == "lobes"))
    assert not bad, "\n".join(bad)
    # weights on every row (threshold rows included): everything stays finite
    out, grads = _hip(case, d, lat, sg.weights(case, d, None), dev)
    for k, v in {**out, **{"d_" + k: g for k, g in grads.items()}}.items():
        assert bool(torch.isfinite(v).all()), f"{k} (weights on every row)"


def test_zero_norm_lobe_gives_nan_and_no_fault(built):
    from gaussian_renderer import shading
    case = sg.BY_ID["zero-norm-lobe"]
    d, lat = _inputs(case, torch.device(DEV))
    out, _ = _hip(case, d, lat, {}, torch.device(DEV))
    for k in ("mean_global", "mean_incident", "direct", "pbr", "diffuse_light"):
        assert bool(torch.isnan(out[k]).all()), k        # NaN * 0 = NaN: every sample, visible or not
    assert bool(torch.isfinite(out["mean_local"]).all())
    L = shading.sg_direct_light(_f32(d["lobes"]), _f32(d["dirs"]))
    assert bool(torch.isnan(L).all())
    # the kernels are still in order afterwards
    ok = sg.BY_ID["P15-Ns7-M3"]
    d2, _ = _inputs(ok, torch.device(DEV))
    out2, _ = _hip(dict(ok, grads=False), d2, None, {}, torch.device(DEV))
    assert bool(torch.isfinite(out2["pbr"]).all())


def test_render_shaded_with_an_sg_light_is_the_unfused_sequence(built):
    from gaussian_renderer import shading
    from gaussian_renderer.svgss_rasterization import GaussianRasterizer
    from svgir_harness import runner, scenes
    dev = torch.device(DEV)
    scn = scenes.surface_scene(P=64, W=32, H=32, seed=13, sh_degree=2, variant="svgss", S=4, VS=52, scale_lo=0.05, scale_hi=0.2)
    sct = runner.to_torch(scn, dev)
    st = runner.settings(sct, "svgss")
    d = shade_inputs.make(64, 24, seed=4, device=dev)
    lobes = shade_inputs.sg_lobes(32, seed=8, device=dev)
    lobes[:, 3] *= 0.05
    res = []
    for fused in (False, True):
        lv = {k: d[k].clone().requires_grad_(True) for k in ("base_color", "roughness", "normals", "radiance")}
        lv["lobes"] = lobes.clone().requires_grad_(True)
        lv["means3D"] = sct["means3D"].clone().requires_grad_(True)
        light = shade_inputs.SGLight(lv["lobes"])
        means2D = torch.zeros_like(lv["means3D"], requires_grad=True)
        if fused:
            out, red = shading.render_shaded(st, lv["means3D"], means2D, sct["opacities"], sct["shs"], sct["scales"], sct["rotations"],
                                             lv["base_color"], lv["roughness"], lv["normals"], d["viewdirs"], lv["radiance"], light,
                                             d["visibility"], d["dirs"], d["areas"], True, want_reduced=True)
            assert red.shape == (64, 70)
        else:
            f, vf, _ = shading.shade_and_pack(lv["base_color"], lv["roughness"], lv["normals"], d["viewdirs"], lv["radiance"], light,
                                              d["visibility"], d["dirs"], d["areas"], st.viewmatrix, True)
            out = GaussianRasterizer(st)(means3D=lv["means3D"], means2D=means2D, opacities=sct["opacities"], shs=sct["shs"],
                                         scales=sct["scales"], rotations=sct["rotations"], features=f, vfeatures=vf)
        (out[1].sum() + (out[5] * 0.3).sum() + (out[6] * 0.7).sum()).backward()
        torch.cuda.synchronize()
        res.append((out, {k: v.grad for k, v in lv.items()}))
    (oa, ga), (ob, gb) = res
    assert oa[0] == ob[0] and int((oa[7] > 0).sum()) > 8
    for i in (1, 2, 3, 4, 5, 6, 8):
        assert torch.equal(oa[i], ob[i]), i
    for k in ("base_color", "roughness", "normals", "radiance", "means3D"):
        assert torch.equal(ga[k], gb[k]), k
    assert torch.allclose(ga["lobes"], gb["lobes"], rtol=2e-5, atol=2e-6 * float(ga["lobes"].abs().max()))   # float atomics
    assert float(ga["lobes"].abs().max()) > 0


def test_invalid_arguments_are_rejected_before_any_launch(built):
    from gaussian_renderer import _native as N
    dev = torch.device(DEV)
    lobes = shade_inputs.sg_lobes(4, device=dev)
    work = torch.empty(8 * 4 + 4, dtype=torch.float32, device=dev)
    dirs, out = torch.zeros(5, 3, device=dev), torch.zeros(5, 3, device=dev)

    def light(count=4, lb=lobes.data_ptr(), wk=work.data_ptr()):
        lt = N.SgLight()
        lt.count, lt.lobes, lt.work = count, lb, wk
        return lt

    def ev(lt):
        return N.lib.svgir_sg_eval(lt, 5, dirs.data_ptr(), out.data_ptr(), None)

    for lt, word in ((light(count=0), "count"), (light(count=129), "count"), (light(lb=None), "NULL"), (light(wk=None), "NULL"),
                     (light(wk=work.data_ptr() + 4), "aligned")):
        assert ev(lt) == -1 and word in N.last_error(), (word, N.last_error())
    assert ev(light()) == 0
    torch.cuda.synchronize()
    # the shading entry points: the same light checks, and no subset
    d = shade_inputs.make(8, 6, seed=1, device=dev)
    from gaussian_renderer import shading
    p, keep, *_ = shading._params(d["base_color"], d["roughness"], d["normals"], d["viewdirs"], d["radiance"], d["visibility"], d["dirs"], d["areas"],
                                  None, False, 1.0)
    red = torch.empty(8, 70, device=dev)
    assert N.lib.svgir_shade_forward_sg(p, light(count=200), red.data_ptr(), None, None, None) == -1 and "count" in N.last_error()
    assert N.lib.svgir_shade_forward_sg(p, light(wk=work.data_ptr() + 4), red.data_ptr(), None, None, None) == -1 and "aligned" in N.last_error()
    sub = torch.arange(8, dtype=torch.int32, device=dev)
    cnt = torch.tensor([4], dtype=torch.int32, device=dev)
    p.subset, p.subset_count = sub.data_ptr(), cnt.data_ptr()
    assert N.lib.svgir_shade_forward_sg(p, light(), red.data_ptr(), None, None, None) == -1 and "subset" in N.last_error()
    g = [torch.empty_like(d[k]) for k in ("base_color", "roughness", "normals", "radiance")]
    gl, gw = torch.empty(4, 7, device=dev), torch.empty(N.lib.svgir_sg_grad_work_bytes(4) // 4, device=dev)
    args = (red.data_ptr(), None, None, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), gl.data_ptr(), gw.data_ptr(), None, None,
            None)
    assert N.lib.svgir_shade_backward_sg(p, light(), *args) == -1 and "subset" in N.last_error()
    p.subset, p.subset_count = None, None
    assert N.lib.svgir_shade_backward_sg(p, light(count=-3), *args) == -1 and "count" in N.last_error()
    assert N.lib.svgir_sg_grad_work_bytes(32) == (8 * 32 + 256) * 4 and N.lib.svgir_sg_grad_work_bytes(0) == 0
    with pytest.raises(RuntimeError, match="lgtSGs must be"):
        shading.sg_direct_light(torch.zeros(129, 7, device=dev), dirs)


def test_paths_without_an_sg_light_raise_type_error(built):
    from gaussian_renderer import shading
    from svgir_harness import losses, render_view
    dev = torch.device(DEV)
    light = shade_inputs.SGLight(shade_inputs.sg_lobes(4, device=dev))
    d = shade_inputs.make(8, 6, seed=1, device=dev)
    with pytest.raises(TypeError, match="lgtSGs"):
        shading.fused_shade(d["base_color"], d["roughness"], d["normals"], d["viewdirs"], d["radiance"], light, d["visibility"], d["dirs"],
                            d["areas"], torch.eye(4, device=dev), True)
    with pytest.raises(TypeError, match="lgtSGs"):
        render_view.environment_backdrop(light, None, None, None, None, None)
    with pytest.raises(TypeError, match="lgtSGs"):
        losses.fused_radiance_loss(None, None, None, None, None, None, None, light, None, None, None, None, None)
    with pytest.raises(TypeError, match="lgtSGs"):
        shading.rendering_equation4(d["base_color"], d["roughness"], d["normals"], d["viewdirs"], d["radiance"], object(),
                                    visibility_precompute=d["visibility"], incident_dirs_precompute=d["dirs"],
                                    incident_areas_precompute=d["areas"])


def test_texture_light_bits_are_unchanged_around_sg_calls(built):
    """A texture-light forward + backward before and after SG calls in the same process: identical bits (shared tables and LDS are not
    left dirty); d env, summed with float atomics, to rounding."""
    from gaussian_renderer import shading
    dev = torch.device(DEV)
    d = shade_inputs.make(300, 70, seed=6, device=dev)

    def texture():
        lv = {k: d[k].clone().requires_grad_(True) for k in ("base_color", "roughness", "normals", "radiance", "env")}
        pbr, ex = shading.rendering_equation4(lv["base_color"], lv["roughness"], lv["normals"], d["viewdirs"], lv["radiance"],
                                              shade_inputs.Light(lv["env"]), visibility_precompute=d["visibility"],
                                              incident_dirs_precompute=d["dirs"], incident_areas_precompute=d["areas"])
        (pbr.sum() + ex["diffuse_light"].sum() + ex["global_incident_lights"].sum()).backward()
        torch.cuda.synchronize()
        return [pbr.detach(), ex["direct"].detach()] + [lv[k].grad for k in ("base_color", "roughness", "normals", "radiance")], lv["env"].grad

    before, env_before = texture()
    for cid in ("P65-Ns64-M128-train-lattice-ratio", "P17-Ns384-M128-eval", "clamp64"):
        case = sg.BY_ID[cid]
        dd, lat = _inputs(case, dev)
        _hip(case, dd, lat, sg.weights(case, dd, None), dev)
    after, env_after = texture()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert torch.allclose(env_before, env_after, rtol=2e-5, atol=2e-6 * float(env_before.abs().max()))


def test_train_step_with_an_sg_light(built):
    from svgir_harness import scenes, workloads
    dev = torch.device(DEV)
    scn = scenes.surface_scene(P=2000, W=96, H=80, seed=71, sh_degree=3, variant="svgss", S=4, VS=52, scale_lo=0.02, scale_hi=0.07)
    ts = workloads.TrainStep(dev, seed=9, Ns=32, fused=False, scene=scn, sg_lobes=32)
    assert ts.params["env"].shape == (32, 7) and not ts.fused
    assert [g["name"] for g in ts.optimizer.param_groups if g["params"][0] is ts.params["env"]] == ["env"]
    before = {k: v.detach().clone() for k, v in ts.params.items()}
    R, pbr, loss = ts.step(keep_grads=True)
    torch.cuda.synchronize()
    assert R > 0 and bool(torch.isfinite(loss))
    g = ts.params["env"].grad
    assert g is not None and g.shape == (32, 7) and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    for k in ("env", "base_color", "roughness"):
        assert not torch.equal(before[k], ts.params[k].detach()), k
    assert bool(torch.isfinite(ts.params["env"]).all())
