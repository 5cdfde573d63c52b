"""The view-direction gradient of the HIP shading backward (csrc/shade.hip: the VIEW instantiations of shade_bwd_kernel, through
svgir_shade_backward_view and svgir_grads.dL_dviewdirs) on the runs of tests/viewgrad_cases.py:

  1. budget: d_viewdirs against the fp64 oracle within 1.5 x E32 + 1e-4 per non-threshold row (E32: the oracle in fp32 against itself
     in fp64, per run), through rendering_equation4 and shade_and_pack in both packings; finite everywhere with weights on every
     row; exactly zero on the zero-view and all-H = 0 rows;
  2. nothing else moves: outputs and every other gradient keep the bits of a view_gradient=False call (d_env: its budget);
  3. write contract: two runs give the same bits; a subset launch leaves the rows outside exactly zero, the rows inside as an all-P call;
  4. fused path: render_shaded(view_gradient=True) against the unfused sequence and against view_gradient=False;
  5. TrainStep(raw_params=True, view_gradient=True): the gradient reaches act["viewdirs"] and, through svgir_activate_backward, xyz.

Everything runs with NaN-poisoned buffers (conftest.py)."""
import numpy as np
import pytest
import torch

import shading_cases as sc
import viewgrad_cases as vc
from svgir_harness import shade_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
APIS = ("rendering_equation4", "pack_train", "pack_eval")


def _inputs(run, dev):
    """(inputs fp64, labels, options, lattice or None): lattice runs take the directions the kernels generate."""
    from gaussian_renderer import shading
    if not run["lattice"]:
        return (*vc.build(run), None)
    d, _, _ = vc.build(run)
    geo = torch.nn.functional.normalize(d["geo_normals"].float(), dim=-1).to(dev)
    offs = torch.rand(geo.shape[0], generator=torch.Generator().manual_seed(2)).to(dev) * 6.2831855
    lat = shading.FibonacciLattice(geo, run["Ns"], offs)
    return (*vc.build(run, dirs=lat.dirs()), lat)


def _hip(monkeypatch, d, opt, lat, w, api, view, dev, view_gradient=True):
    """One forward + backward through the HIP kernels under the upstream weights w, `viewdirs` a leaf: (outputs, gradients) named
    like the oracle's (no "viewdirs" entry when the kernels return none)."""
    import test_gpu_shading_edges as ge
    from gaussian_renderer import shading
    f32 = lambda t: t.float().to(dev)  # noqa: E731
    names = [k for k in vc.LEAVES if not (k == "radiance" and opt["radiance_ratio"] is not None)]
    lv = {k: f32(d[k]).requires_grad_(True) for k in names}
    kw = dict(view_gradient=True) if view_gradient else {}
    rad = lv.get("radiance")
    if opt["radiance_ratio"] is not None:
        lv["radiance_ratio"] = torch.tensor(opt["radiance_ratio"], dtype=torch.float32, device=dev, requires_grad=True)
        rad, kw = f32(d["radiance"]), dict(kw, radiance_ratio=lv["radiance_ratio"])
    dirs, areas = (lat, None) if lat is not None else (f32(d["dirs"]), f32(d["areas"]))
    light = ge._light(monkeypatch, shading, lv["env"], opt, dev)
    if api == "rendering_equation4":
        pbr, ex = shading.rendering_equation4(lv["base_color"], lv["roughness"], lv["normals"], lv["viewdirs"], rad, light,
                                              visibility_precompute=f32(d["visibility"]), incident_dirs_precompute=dirs,
                                              incident_areas_precompute=areas, **kw)
        out = dict(pbr=pbr, mean_incident=ex["incident_lights"].mean(-2), mean_local=ex["local_incident_lights"].mean(-2),
                   mean_global=ex["global_incident_lights"].mean(-2), **{k: ex[k] for k in ("diffuse_light", "specular", "direct", "indirect")})
    else:
        vm = torch.eye(4, dtype=torch.float64)
        vm[:3, :3] = view
        f, vf, red = shading.shade_and_pack(lv["base_color"], lv["roughness"], lv["normals"], lv["viewdirs"], rad, light,
                                            f32(d["visibility"]), dirs, areas, f32(vm), api == "pack_train", **kw)
        out = dict(features=f, vfeatures=vf, pbr=red[:, 0:12])
    sum((out[k] * f32(w[k])).sum() for k in w).backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in lv.items() if v.grad is not None}
    return {k: v.detach() for k, v in out.items()}, grads


def _weights(d, thr, api, every_row):
    training = None if api == "rendering_equation4" else api == "pack_train"
    w = sc.weights(d, None if every_row else thr, seed=3 + len(api), training=training)
    if bool(torch.isnan(d["radiance"]).any()) and api == "rendering_equation4":
        del w["mean_local"]      # (tests/test_gpu_shading_edges.py: torch's own product would add 0 x NaN to the ratio's gradient)
    return w, training


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", vc.RUNS, ids=lambda r: r["id"])
def test_view_gradient_within_the_reference_fp32_budget(built, monkeypatch, run):
    dev = torch.device(DEV)
    d, lab, opt, lat = _inputs(run, dev)
    clean = {k: torch.nan_to_num(v, nan=0.0) for k, v in d.items()}
    thr = vc.threshold_rows(sc.probe(clean, opt))
    assert float(thr.double().mean()) <= vc.MAX_THRESHOLD_SHARE
    zero = vc.exact_zero_rows(lab)
    view = sc.view3x3()
    bad = []
    for api in APIS:
        for every_row in (False, True):
            w, training = _weights(d, thr, api, every_row)
            out, grads = _hip(monkeypatch, d, opt, lat, w, api, view, dev)
            assert "viewdirs" in grads, "no gradient reached viewdirs"
            for k, v in {**out, **{"d_" + k: g for k, g in grads.items()}}.items():
                assert bool(torch.isfinite(v).all()), f"{api} {k}: {int((~torch.isfinite(v)).sum())} non-finite entries" + \
                    (" (weights on every row)" if every_row else "")
            gv = grads["viewdirs"].cpu()
            assert bool((gv[zero] == 0).all()), f"{api}: zero-view / all-H=0 rows are not exactly zero"
            if every_row:
                continue
            _, g64, E = vc.e32(d, opt, w, thr, view, training)
            e = torch.where(thr, torch.zeros(thr.numel(), dtype=torch.float64), sc.row_err(gv, g64["viewdirs"]))
            lim = 1.5 * E["d_viewdirs"] + 1e-4
            worst = int(e.argmax())
            print(f"  {run['id']} {api}: d_viewdirs HIP {float(e.max()):.2e} (row {worst} {lab[worst]}), E32 {E['d_viewdirs']:.2e}, "
                  f"budget {lim:.2e}; {int(thr.sum())} threshold rows of {thr.numel()}; max |d_viewdirs| {float(g64['viewdirs'].abs().max()):.3g}")
            if not bool(torch.isfinite(e).all()) or float(e.max()) > lim:
                rows = [f"{i}:{lab[i]}:{float(e[i]):.1e}" for i in torch.nonzero(~(e <= lim)).flatten().tolist()[:8]]
                bad.append(f"{api} d_viewdirs: HIP err {float(e.max()):.3e} > 1.5 x E32 {E['d_viewdirs']:.3e} + 1e-4 {rows}")
    assert not bad, "\n".join([run["id"]] + bad)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
_STILL = [r for r in vc.RUNS if r["ratio"] is not None or r["case"] == "view_alignment" or (r["lattice"] and r["case"] == "env_clamp")]


@pytest.mark.parametrize("run", _STILL, ids=lambda r: r["id"])
def test_nothing_else_moves(built, monkeypatch, run):
    import test_gpu_shading_edges as ge
    dev = torch.device(DEV)
    d, lab, opt, lat = _inputs(run, dev)
    clean = {k: torch.nan_to_num(v, nan=0.0) for k, v in d.items()}
    thr = vc.threshold_rows(sc.probe(clean, opt))
    view = sc.view3x3()
    bad = []
    for api in APIS:
        w, training = _weights(d, thr, api, False)
        o0, g0 = _hip(monkeypatch, d, opt, lat, w, api, view, dev, view_gradient=False)
        o1, g1 = _hip(monkeypatch, d, opt, lat, w, api, view, dev, view_gradient=True)
        assert "viewdirs" not in g0 and "viewdirs" in g1
        assert set(g1) - {"viewdirs"} == set(g0) and ("radiance_ratio" in g0) == (opt["radiance_ratio"] is not None)
        for k in o0:
            assert torch.equal(o0[k], o1[k]), (api, k)
        for k in g0:
            if k != "env":
                assert torch.equal(g0[k], g1[k]), (api, "d_" + k)
        _, g64, E = vc.e32(d, opt, w, thr, view, training)
        ge._budget(api + " grad", {"env": g1["env"].cpu()}, {"env": g64["env"]}, E, thr, lab, bad)
    assert not bad, "\n".join([run["id"]] + bad)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ns,ratio", [(65, False), (24, True)])
def test_write_contract_repeatability_and_subset(built, Ns, ratio):
    import test_gpu_fused_shade as fs
    from gaussian_renderer import _native as N
    from gaussian_renderer import shading
    dev = torch.device(DEV)
    P = 3001
    d = shade_inputs.make(P, Ns, seed=11, device=dev)
    vm = torch.eye(4, device=dev) + 0.1 * torch.randn(4, 4, device=dev, generator=torch.Generator(dev).manual_seed(1))
    mask = torch.rand(P, device=dev, generator=torch.Generator(dev).manual_seed(2)) < 0.37
    lst, cnt = fs._partition(mask)
    rt = torch.tensor(0.83, device=dev) if ratio else None
    g = torch.Generator(dev).manual_seed(5)
    gf, gvf = torch.randn(P, 4, device=dev, generator=g), torch.randn(P, 52, device=dev, generator=g)

    def run(subset):
        sp, keep, *_ = shading._params(d["base_color"], d["roughness"], d["normals"], d["viewdirs"], d["radiance"], d["visibility"],
                                       d["dirs"], d["areas"], d["env"], True, 2.0, viewmatrix=vm, training=True, ratio=rt)
        if subset:
            sp.subset, sp.subset_count = lst.data_ptr(), cnt.data_ptr()
        outs = [N.out_tensor(t.shape, torch.float32, dev) for t in (d["base_color"], d["roughness"], d["normals"], d["radiance"], d["env"])]
        d_ratio = N.out_tensor((1,), torch.float32, dev) if ratio else None
        d_view = N.out_tensor((P, 3), torch.float32, dev)
        gwork = torch.empty(d["env"].numel() + shading.RATIO_WORK, device=dev)
        N.check(N.lib.svgir_shade_backward_view(sp, None, gf.data_ptr(), gvf.data_ptr(), *[t.data_ptr() for t in outs], gwork.data_ptr(),
                                                N.ptr(d_ratio), d_view.data_ptr(), N.stream_ptr(dev)), "shade_backward_view")
        torch.cuda.synchronize()
        return outs[:4] + [d_view] + ([d_ratio] if ratio else [])

    full, again, sub = run(False), run(False), run(True)
    assert bool(torch.isfinite(full[4]).all()) and float(full[4].abs().max()) > 0
    for i, (a, b) in enumerate(zip(full, again)):
        assert torch.equal(a, b), i                       # no atomics outside d_env: the same bits
    for i, (a, b) in enumerate(zip(full[:5], sub[:5])):
        assert torch.equal(a[mask], b[mask]), i
        assert not torch.isnan(b).any() and float(b[~mask].abs().max()) == 0.0, i
    # the plain entry point writes the bits it always wrote, the ratio's gradient included
    sp, keep, *_ = shading._params(d["base_color"], d["roughness"], d["normals"], d["viewdirs"], d["radiance"], d["visibility"],
                                   d["dirs"], d["areas"], d["env"], True, 2.0, viewmatrix=vm, training=True, ratio=rt)
    outs = [N.out_tensor(t.shape, torch.float32, dev) for t in (d["base_color"], d["roughness"], d["normals"], d["radiance"], d["env"])]
    d_ratio = N.out_tensor((1,), torch.float32, dev) if ratio else None
    gwork = torch.empty(d["env"].numel() + shading.RATIO_WORK, device=dev)
    N.check(N.lib.svgir_shade_backward(sp, None, gf.data_ptr(), gvf.data_ptr(), *[t.data_ptr() for t in outs], gwork.data_ptr(),
                                       N.ptr(d_ratio), N.stream_ptr(dev)), "shade_backward")
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(full[:4] + full[5:], outs[:4] + ([d_ratio] if ratio else []))):
        assert torch.equal(a, b), i
    # required output
    assert N.lib.svgir_shade_backward_view(sp, None, gf.data_ptr(), gvf.data_ptr(), *[t.data_ptr() for t in outs], gwork.data_ptr(),
                                           N.ptr(d_ratio), None, N.stream_ptr(dev)) == -1


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.FUSED_CASES[:2])
def test_fused_view_gradient_is_bit_identical(built, case):
    """The small surface scene of tests/test_gpu_shading_edges.py's fused test, edge rows as the surfels' materials."""
    import test_gpu_fused_shade as fs
    from gaussian_renderer import shading
    from gaussian_renderer.svgss_rasterization import GaussianRasterizer
    from svgir_harness import runner, scenes
    dev = torch.device(DEV)
    sc_ = scenes.surface_scene(P=6000, W=176, H=144, seed=41, sh_degree=2, variant="svgss", S=4, VS=52, scale_lo=0.01, scale_hi=0.06)
    sct = runner.to_torch(sc_, dev)
    st = runner.settings(sct, "svgss")
    e, lab, opt = shade_inputs.edge_case(case, sc.CASES[case]["n"], 64)
    rows = torch.arange(6000) % e["base_color"].shape[0]
    d = {k: e[k][rows].float().contiguous().to(dev) for k in sc.INPUTS if k != "env"}
    d["env"] = e["env"].float().to(dev)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in scenes.upstream_grads(sc_, "svgss", seed=6).items()}

    def unfused(lv, dv):
        f, vf, _ = shading.shade_and_pack(lv["base_color"], lv["roughness"], lv["normals"], dv["viewdirs"], lv["radiance"],
                                          shade_inputs.Light(lv["env"]), dv["visibility"], dv["dirs"], dv["areas"], st.viewmatrix, True,
                                          view_gradient=True)
        means2D = torch.zeros_like(lv["means3D"], requires_grad=True)
        return GaussianRasterizer(st)(means3D=lv["means3D"], means2D=means2D, opacities=lv["opacities"], shs=lv["shs"],
                                      scales=lv["scales"], rotations=lv["rotations"], features=f, vfeatures=vf)

    for _ in range(3):   # (the third view of a workload runs the speculative launch sequence)
        la, lb, lc = fs._leaves(sct, d), fs._leaves(sct, d), fs._leaves(sct, d)
        da, db = (dict(d, viewdirs=d["viewdirs"].clone().requires_grad_(True)) for _ in range(2))
        oa = unfused(la, da)
        fs._loss(oa, gt).backward()
        ob, _, _ = fs._fused(sct, st, db, lb, True, view_gradient=True)
        fs._loss(ob, gt).backward()
        oc, _, _ = fs._fused(sct, st, d, lc, True)
        fs._loss(oc, gt).backward()
        torch.cuda.synchronize()
    ga, gb = da["viewdirs"].grad, db["viewdirs"].grad
    assert ga is not None and gb is not None
    blended = ob[7][:, 0] > 0
    assert int(blended.sum()) > 500 and int((~blended).sum()) > 500
    assert bool(torch.isfinite(gb).all()) and torch.equal(ga, gb)
    assert float(gb[~blended].abs().max()) == 0.0 and float(gb[blended].abs().max()) > 0
    names = ("color", "normal", "opacity", "depth", "feature", "vfeature", "weights", "radii")
    for n, a, b in zip(names, ob[1:], oc[1:]):             # the image and every other output: the bits of view_gradient=False
        if n == "weights":   # (float atomics across sub-tiles, in any two calls: tests/test_gpu_fused_shade.py)
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), n
        else:
            assert torch.equal(a, b), n
    for k in lb:
        if k == "env":
            assert torch.allclose(lb[k].grad, lc[k].grad, rtol=2e-5, atol=2e-6 * float(lc[k].grad.abs().max())), k
        else:
            assert torch.equal(lb[k].grad, lc[k].grad), k


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
class _Tap(torch.autograd.Function):
    """Identity on xyz in front of the activation stage; records the gradient that stage returns for it."""

    @staticmethod
    def forward(ctx, x, store):
        ctx.store = store
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.store.append(g.detach().clone())
        return g, None


def test_train_step_sends_the_view_gradient_into_xyz(built):
    """xyz is also the rasterizer's means3D, and torch adds the two gradients in fp32: `xyz.grad` of the view step minus the default
    step's carries the rounding of that sum (half an ulp of a rasterizer gradient 40 x the view term here: measured 358 x the bound
    when the difference is taken literally).  So the statement is split where the sum is formed: the gradient the activation stage
    returns for xyz (tapped in front of it) equals the oracle's adjoint within activation_cases.grad_bound, and the view step's
    xyz.grad has exactly the bits of fp32(default step's xyz.grad + that gradient)."""
    import activation_cases as ac
    from svgir_harness import activations, scenes, workloads
    dev = torch.device(DEV)
    sc_ = scenes.surface_scene(P=4000, W=160, H=128, seed=71, sh_degree=3, variant="svgss", S=4, VS=52, scale_lo=0.02, scale_hi=0.07)
    offs = None
    res = {}
    for vg in (False, True):
        tap = []
        act_fn = lambda raw, *a, _t=tap, **k: activations.activate(dict(raw, xyz=_Tap.apply(raw["xyz"], _t)), *a, **k)  # noqa: E731
        ts = workloads.TrainStep(dev, seed=9, Ns=32, scene=sc_, raw_params=True, activate=act_fn, view_gradient=vg)
        raw0 = {k: ts.params[k].detach().cpu().clone() for k in workloads.TrainStep.RAW}
        if offs is None:
            offs = torch.rand(ts.P, device=dev, generator=torch.Generator(DEV).manual_seed(5)) * (2 * np.pi)
        R, pbr, loss = ts.step(offsets=offs, keep_grads=True)
        torch.cuda.synchronize()
        res[vg] = dict(R=R, pbr=pbr.detach().clone(), loss=loss.detach().clone(), xyz=ts.params["xyz"].grad.detach().clone(),
                       up=ts.last_activated["viewdirs"].grad, campos=ts.st.campos.detach().cpu(), raw0=raw0, tap=tap)
    a, b = res[False], res[True]
    assert a["up"] is None
    assert b["up"] is not None, "no gradient reached act['viewdirs']"
    assert a["R"] == b["R"] and torch.equal(a["pbr"], b["pbr"]) and torch.equal(a["loss"].reshape(1), b["loss"].reshape(1))
    up = {k: None for k in workloads.TrainStep.ACTIVATED}
    up["viewdirs"] = b["up"].detach().cpu()
    assert bool(torch.isfinite(up["viewdirs"]).all()) and float(up["viewdirs"].abs().max()) > 0
    o = ac.oracle(b["raw0"], b["campos"], None, up, workloads.TrainStep.ACTIVATED, False)
    assert len(b["tap"]) == 1 and all(not bool(t.any()) for t in a["tap"])        # (the default step's activation stage returns zeros)
    g_act = b["tap"][0]
    bound = ac.grad_bound("xyz", o["aabs"]["xyz"])
    err = (g_act.double().cpu() - o["grads"]["xyz"]).abs()
    print(f"d xyz through viewdirs: max |adjoint| {float(o['grads']['xyz'].abs().max()):.3g}, max |err| / bound = {float((err / bound).max()):.3g}, "
          f"max |xyz.grad| of the default step {float(a['xyz'].abs().max()):.3g}")
    n, _ = ac.mismatches(g_act, o["grads"]["xyz"], bound)
    assert n == 0, n
    assert float(o["grads"]["xyz"].abs().max()) > 0
    assert torch.equal(b["xyz"], a["xyz"] + g_act)
