"""The three paths of the spherical-Gaussian light around the shading on the GPU, against the tables of tests/sg_paths_cases.py:
A  svgir_sg_eval_backward behind shading.sg_direct_light / compute_envmap (csrc/sg_light.hip): d_lobes per lobe and d_dirs per direction
   within 1.5 x G32 + 1e-4 (shading_cases.row_err; G32 = the same arithmetic in torch fp32 against fp64, per case and tensor);
B  svgir_env_backdrop_sg behind render_view.sg_environment_backdrop / render_svgss_view (csrc/backdrop.hip): 4 E32 + 16 eps32 max(1, max
   |oracle|), threshold pixels of the sRGB knee / clip held to finiteness;
C  svgir_radiance_loss_forward_sg / _backward_sg behind losses.fused_radiance_loss_sg (csrc/irradiance.hip): the bounds of
   tests/test_gpu_radiance_loss.py with E_SG, d_lobes per lobe within 1.5 x G32 + 1e-4, and the equivalence with the composed path
   radiance_loss(sg_direct_light(lgtSGs, dirs) * areas), lgtSGs.grad included.
Every output buffer is NaN-filled before the call (conftest.py: SVGIR_POISON): an element the kernels forget fails the finiteness checks."""
import numpy as np
import pytest
import torch

import backdrop_cases as bc
import sg_light_cases as sg
import sg_paths_cases as sp
import shading_cases as sc
from svgir_harness import render_view, runner, scenes, shade_inputs
from tests import radiance_loss_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _f32(t, dev=DEV):
    return t.float().to(dev)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def _budget(tag, got, ref, G, bad):
    assert bool(torch.isfinite(got).all()), f"{tag}: {int((~torch.isfinite(got)).sum())} non-finite (or never written) entries"
    e = sc.row_err(got, ref)
    lim = 1.5 * G + 1e-4
    print(f"    {tag}: HIP {float(e.max()):.2e} (row {int(e.argmax())}), G32 {G:.2e}, budget {lim:.2e}")
    if float(e.max()) > lim:
        bad.append(f"{tag}: HIP err {float(e.max()):.3e} > 1.5 x G32 {G:.3e} + 1e-4")


# ---- A: the eval backward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sp.EVAL_CASES, ids=lambda c: c["id"])
def test_eval_backward_within_the_fp32_budget(built, case):
    from gaussian_renderer import _native as N, shading
    assert N.POISON
    lobes, dirs, up = sp.eval_build(case["id"])
    l64, d64, G = sp.eval_g32(case["id"])
    bad = []
    for want_l, want_d in ((True, True), (True, False), (False, True)):
        lb, d = _f32(lobes).requires_grad_(want_l), _f32(dirs).requires_grad_(want_d)
        L = shading.sg_direct_light(lb, d)
        (L * _f32(up)).sum().backward()
        torch.cuda.synchronize()
        tag = f"{case['id']} lobes={want_l} dirs={want_d}"
        if want_l:
            assert lb.grad.shape == lb.shape
            _budget(tag + " d_lobes", lb.grad, l64, G["d_lobes"], bad)
        else:
            assert lb.grad is None
        if want_d:
            assert d.grad.shape == d.shape
            _budget(tag + " d_dirs", d.grad, d64, G["d_dirs"], bad)
        else:
            assert d.grad is None
    assert not bad, "\n".join(bad)
    if case["special"] == "signs":      # sign(0) = 0, exactly
        lb = _f32(lobes).requires_grad_(True)
        (shading.sg_direct_light(lb, _f32(dirs)) * _f32(up)).sum().backward()
        g = lb.grad.cpu()
        assert g[1, 3] == 0 and g[2, 5] == 0 and bool((g[3, 4:] == 0).all()) and g[4, 4] == 0
    if case["special"] == "zero_up":
        lb, d = _f32(lobes).requires_grad_(True), _f32(dirs).requires_grad_(True)
        (shading.sg_direct_light(lb, d) * _f32(up)).sum().backward()
        assert float(lb.grad.abs().max()) == 0.0 and float(d.grad.abs().max()) == 0.0


def test_forward_bits_direct_call_leading_shapes_and_compute_envmap(built):
    from gaussian_renderer import _native as N, shading
    lobes, dirs, up = sp.eval_build("n1200-M32")
    lb, d = _f32(lobes), _f32(dirs)
    # the forward of sg_direct_light is svgir_sg_eval, bit for bit, with and without a graph
    lt, keep = shading._sg_light(lb, torch.device(DEV))
    direct = torch.full((1200, 3), float("nan"), device=DEV)
    N.check(N.lib.svgir_sg_eval(lt, 1200, d.data_ptr(), direct.data_ptr(), N.stream_ptr(torch.device(DEV))), "sg_eval")
    plain = shading.sg_direct_light(lb, d)
    graph = shading.sg_direct_light(lb.clone().requires_grad_(True), d.clone().requires_grad_(True))
    assert not plain.requires_grad and graph.requires_grad
    assert torch.equal(plain, direct) and torch.equal(graph.detach(), direct)
    # any leading shape, both gradients reshaped like their inputs; d_dirs has the same bits on a second run
    d4 = d.reshape(4, 100, 3, 3).clone().requires_grad_(True)
    l4 = lb.clone().requires_grad_(True)
    (shading.sg_direct_light(l4, d4) * _f32(up).reshape(4, 100, 3, 3)).sum().backward()
    l64, d64, G = sp.eval_g32("n1200-M32")
    bad = []
    _budget("leading shape d_dirs", d4.grad.reshape(-1, 3), d64, G["d_dirs"], bad)
    _budget("leading shape d_lobes", l4.grad, l64, G["d_lobes"], bad)
    assert not bad, "\n".join(bad)
    d5 = d.clone().requires_grad_(True)
    (shading.sg_direct_light(lb, d5) * _f32(up)).sum().backward()
    assert torch.equal(d5.grad.reshape(-1), d4.grad.reshape(-1))
    # no direction: zeros for the lobes
    l0 = lb.clone().requires_grad_(True)
    shading.sg_direct_light(l0, torch.empty(0, 3, device=DEV)).sum().backward()
    assert l0.grad.shape == l0.shape and float(l0.grad.abs().max()) == 0.0
    # compute_envmap inherits the gradient: against the fp64 oracle on the same grid
    le = lb.clone().requires_grad_(True)
    env = shading.compute_envmap(le, 8, 16)
    env.sum().backward()
    phi, theta = torch.meshgrid([torch.linspace(0., torch.pi, 8), torch.linspace(1.0 * torch.pi, -1.0 * torch.pi, 16)], indexing="ij")
    vd = torch.stack([torch.cos(theta) * torch.sin(phi), torch.sin(theta) * torch.sin(phi), torch.cos(phi)], dim=-1).double()
    ref = sg.sg_grad(lobes, vd, torch.ones_like(vd))
    G = float(sc.row_err(sg.sg_grad(lobes.float(), vd.float(), torch.ones_like(vd).float()), ref).max())
    assert le.grad is not None and float(le.grad.abs().max()) > 0
    _budget("compute_envmap d_lobes", le.grad, ref, G, bad)
    assert not bad, "\n".join(bad)


def test_eval_backward_zero_directions_through_the_abi(built):
    from gaussian_renderer import _native as N, shading
    dev = torch.device(DEV)
    lt, keep = shading._sg_light(shade_inputs.sg_lobes(5, device=dev), dev)
    out = torch.full((5, 7), float("nan"), device=dev)
    gw = torch.empty(N.lib.svgir_sg_grad_work_bytes(5) // 4, device=dev)
    assert N.lib.svgir_sg_eval_backward(lt, 0, None, None, out.data_ptr(), None, gw.data_ptr(), N.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


# ---- B: the backdrop ---------------------------------------------------------------------------------------------------------
def _backdrop(case):
    dev = torch.device(DEV)
    t = lambda k: torch.from_numpy(np.array(case[k])).to(dev)  # noqa: E731
    light = shade_inputs.SGLight(torch.from_numpy(np.array(case["lobes"])).float().to(dev))
    res = render_view.sg_environment_backdrop(light, torch.from_numpy(np.array(case["K"])), torch.from_numpy(np.array(case["R"])), t("image"),
                                              t("opacity"), t("vfeature"))
    assert set(res) == set(bc.OUTPUTS)
    base = res["env_only"].untyped_storage().data_ptr()
    for k in bc.OUTPUTS:
        assert res[k].shape == (3, case["H"], case["W"]) and not res[k].requires_grad and res[k].untyped_storage().data_ptr() == base
    return {k: res[k].cpu().numpy() for k in bc.OUTPUTS}


@pytest.mark.parametrize("case", sp.views(), ids=sp.view_ids())
def test_sg_backdrop_matches_the_oracle(built, case):
    from gaussian_renderer import _native as N
    assert N.POISON
    o64, _, e32, bound, thr = sp.view_tables(case["name"])
    got, again = _backdrop(case), _backdrop(case)
    for k in bc.OUTPUTS:
        g, ref = got[k].astype(np.float64), o64[k]
        assert np.array_equal(got[k], again[k], equal_nan=True), f"{k}: the second run differs"
        assert np.array_equal(np.isnan(g), np.isnan(ref)), f"{k}: NaN pattern differs ({np.isnan(g).sum()} vs {np.isnan(ref).sum()})"
        assert np.isfinite(g[thr[k] & np.isfinite(ref)]).all()
        fin = np.isfinite(ref) & ~thr[k]
        err = float(np.abs(g - ref)[fin].max())
        print(f"{case['name']:40s} {k:10s} max err = {err:.3e}  E32 = {e32[k]:.3e}  bound = {bound[k]:.3e}")
        assert err <= bound[k], (k, err, bound[k])


def test_sg_backdrop_matches_the_reference_recording(built):
    g = np.load(sp.bc.GOLD + "/sg_paths.npz")
    dev = torch.device(DEV)
    light = shade_inputs.SGLight(torch.from_numpy(g["view_lgtSGs"]).float().to(dev))
    t = lambda k: torch.from_numpy(g[k]).float().to(dev)  # noqa: E731
    res = render_view.sg_environment_backdrop(light, t("view_intrinsics").cpu(), t("view_c2w").cpu(), t("view_image"), t("view_opacity"),
                                              t("view_vfeature"))
    for k in bc.OUTPUTS:
        np.testing.assert_allclose(res[k].cpu().numpy(), g["view_" + k], rtol=2e-4, atol=2e-5, err_msg=k)


def test_render_svgss_view_with_an_sg_light_gains_the_backdrop(built):
    dev = torch.device(DEV)
    scn = scenes.surface_scene(P=600, W=53, H=37, seed=3, sh_degree=1, variant="svgss", S=7, VS=64, scale_lo=0.03, scale_hi=0.09)
    d = shade_inputs.make(scn["means3D"].shape[0], 8, seed=2)
    sct = runner.to_torch(scn, dev)
    mat = {k: v.to(dev) for k, v in d.items() if k != "env"}
    lobes = shade_inputs.sg_lobes(32, seed=8, device=dev)
    lobes[:, 3] *= 0.05
    lobes[:, 4:] *= 0.1
    light = shade_inputs.SGLight(lobes)
    cam = render_view.camera_of(sct)
    with torch.no_grad():
        plain, _ = render_view.render_svgss_view(sct, mat, light, False)
        res, _ = render_view.render_svgss_view(sct, mat, light, False, camera=cam)
        train, _ = render_view.render_svgss_view(sct, mat, light, True, camera=cam)
    assert not (set(bc.OUTPUTS) & set(plain)) and set(res) == set(plain) | set(bc.OUTPUTS) and not (set(bc.OUTPUTS) & set(train))
    for k in bc.OUTPUTS:
        assert res[k].shape == (3, 37, 53) and bool(torch.isfinite(res[k]).all()) and not res[k].requires_grad
    e = res["env_only"]
    assert float(((e > 0) & (e < 1)).float().mean()) > 0.5 and float(e.max() - e.min()) > 0.05
    # the texture binding still refuses the light, and the SG binding a texture
    with pytest.raises(TypeError, match="lgtSGs"):
        render_view.environment_backdrop(light, cam["intrinsics"], cam["c2w"], res["render"], res["opacity"], res["render"])
    with pytest.raises(TypeError, match="lgtSGs"):
        render_view.sg_environment_backdrop(shade_inputs.Light(d["env"].to(dev)), cam["intrinsics"], cam["c2w"], res["render"], res["opacity"],
                                            res["render"])
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        render_view.sg_environment_backdrop(light, cam["intrinsics"], cam["c2w"], res["render"].cpu(), res["opacity"], res["render"])
    with pytest.raises(RuntimeError, match="expected image"):
        render_view.sg_environment_backdrop(light, cam["intrinsics"], cam["c2w"], res["render"], res["opacity"][:, :5], res["render"])


# ---- C: the fused loss -------------------------------------------------------------------------------------------------------
def _renderer(c):
    from pbgi.renderer import Renderer
    r = Renderer()
    r.hemi_index_buffers = _t(c["hit"]).reshape(c["N"], c["S"], 1)
    r.uv_buffers = _t(c["uvs"])
    return r


def _leaves(c, lobes_grad=True):
    return [_t(c["lobes"]).requires_grad_(lobes_grad), _t(c["albedos"]).requires_grad_(True), _t(c["roughnesses"]).requires_grad_(True),
            _t(c["radiance_ratio"]).requires_grad_(c.get("ratio_grad", True))]   # (ratio_grad False: the backward gets no d_radiance_ratio)


def _run(r, c, leaves, with_sum=True):
    lobes, alb, rough, ratio = leaves
    return r.radiance_consistency_sg(_t(c["xyz"]), _t(c["camera_center"]), _t(c["geo_normal"]), _t(c["ray_d"]), _t(c["areas"]), _t(c["visibility"]),
                                     lobes, _t(c["normals"]), alb, rough, _t(c["radiances"]), ratio, with_sum=with_sum)


def _close(kind, got, want, cnt, mag, what, finite_only=None):
    got = got.detach().cpu().numpy().astype(np.float64).reshape(want.shape)
    assert np.isfinite(got).all(), f"{what}: {np.count_nonzero(~np.isfinite(got))} non-finite elements (an element the kernel did not write is NaN)"
    err, tol = np.abs(got - want), sp.bound(kind, cnt, mag)
    ratio = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
    print(f"{what}: worst error / bound = {ratio:.3g}")
    bad = err > tol
    if finite_only is not None:
        bad &= ~finite_only
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} elements off, first {np.argwhere(bad)[0]}: {got[bad][0]} vs {want[bad][0]} (bound {tol[bad][0]})"


def _texture_selection(c):
    """sample_indices of the texture kernel on the same geometry (any map: the selection does not see the light)"""
    r = _renderer(c)
    env = torch.zeros(1, 2, 4, 3, device=DEV)
    _, idx, _ = r.radiance_consistency(_t(c["xyz"]), _t(c["camera_center"]), _t(c["geo_normal"]), _t(c["ray_d"]), _t(c["areas"]),
                                       _t(c["visibility"]), env, True, 2.0, None, _t(c["normals"]), _t(c["albedos"]), _t(c["roughnesses"]),
                                       _t(c["radiances"]), _t(c["radiance_ratio"]))
    return idx


@pytest.mark.parametrize("name", sp.RL_NAMES)
def test_fused_sg_loss_forward_and_backward(built, name):
    c, o = sp.rl_case(name), sp.rl_oracle(name)
    N, S = c["N"], c["S"]
    r = _renderer(c)
    leaves = _leaves(c)
    loss, idx, R, total = _run(r, c, leaves)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    assert idx.dtype == torch.int32 and idx.shape == (N,) and R.shape == (N, 3) and not idx.requires_grad and not R.requires_grad
    assert torch.equal(idx, _texture_selection(c)), "the selection must not see the light"
    # the selection against the oracle; everything else at the kernel's own indices
    ix = idx.cpu().numpy().astype(np.int64)
    thr = o["threshold"]
    assert ((ix >= 0) & (ix < S)).all() and (ix[~thr] == o["sel"][~thr]).all()
    rows = np.arange(N)
    assert (o["score"][rows, o["sel"]][thr] - o["score"][rows, ix][thr] <= 4 * lc.E_SEL).all()
    if not (ix == o["sel"]).all():
        o = sp.rl_oracle_at(c, ix)
    excluded = float((thr | o["unsafe"]).mean())
    assert excluded <= sp.MAX_EXCLUDED and float(o["unsafe_lobes"].mean()) <= sp.MAX_EXCLUDED
    # forward
    Rn = R.detach().cpu().numpy().astype(np.float64)
    fin = np.isfinite(o["out"])
    assert not np.isfinite(Rn[~fin]).any()
    _close("out", torch.from_numpy(np.where(fin, Rn, 0.0)), np.where(fin, o["out"], 0.0), float(S), np.where(fin, o["out_abs"], 0.0), name + " R")
    if o["bad"].any():
        assert np.isnan(float(loss)) and not np.isfinite(float(total))
    else:
        print(f"{name}: sum {float(total)} fp64 {o['loss_sum']} bound {o['loss_sum_bound']}")
        assert abs(float(total) - o["loss_sum"]) <= o["loss_sum_bound"]
        assert np.float32(float(loss)) == np.float32(float(total) / (3 * N))
    loss2, idx2, R2, total2 = _run(r, c, _leaves(c))
    assert torch.equal(idx, idx2) and torch.equal(R.view(torch.int32), R2.view(torch.int32))
    assert torch.equal(total.view(torch.int64), total2.view(torch.int64)) and torch.equal(loss.detach().view(torch.int32), loss2.detach().view(torch.int32))
    # backward
    loss.backward()
    lobes, alb, rough, ratio = leaves
    k = o["kernel"]
    for leaf, kind in ((alb, "d_albedos"), (rough, "d_roughnesses")):
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape and leaf.grad.dtype == torch.float32
        only = np.zeros(k[kind].shape, bool)
        only[o["unsafe"]] = True
        if kind == "d_roughnesses":
            only[:, 0] |= k["thr"]
        _close(kind, leaf.grad, k[kind], k[kind + "_cnt"], k[kind + "_abs"], f"{name} {kind}", only)
    tol = (3 * N + 4) * 2.0 ** -24 * o["d_ratio_abs"] + 2 * o["unsafe_ratio_abs"]
    if c["ratio_grad"]:
        assert ratio.grad is not None and abs(float(ratio.grad) - o["d_ratio"]) <= tol, (float(ratio.grad), o["d_ratio"], tol)
    else:
        assert ratio.grad is None
    assert lobes.grad is not None and lobes.grad.shape == lobes.shape and bool(torch.isfinite(lobes.grad).all())
    e = sc.row_err(lobes.grad, torch.from_numpy(o["d_lobes"]))
    e = torch.where(torch.from_numpy(o["unsafe_lobes"]), torch.zeros_like(e), e)
    lim = 1.5 * o["G32"] + 1e-4
    print(f"{name} d_lobes: HIP {float(e.max()):.2e} (lobe {int(e.argmax())}), G32 {o['G32']:.2e}, budget {lim:.2e}")
    assert float(e.max()) <= lim
    if name.startswith("all_primaries_miss"):
        assert float(lobes.grad.abs().max()) == 0.0 and float(alb.grad.abs().max()) == 0.0


def test_fused_sg_loss_agrees_with_the_composed_path(built):
    """losses.fused_radiance_loss_sg against the path it replaces: radiance_loss fed envmap = sg_direct_light(lgtSGs, dirs) * areas, whose
    light gradient now comes through svgir_sg_eval_backward.  Both lie within their own bound of the fp64 value."""
    from gaussian_renderer import shading
    from svgir_harness.losses import fused_radiance_loss, fused_radiance_loss_sg, radiance_loss
    name = "physical-M32"
    c, o = sp.rl_case(name), sp.rl_oracle(name)
    N, S = c["N"], c["S"]
    k = o["kernel"]
    r = _renderer(c)
    args = lambda: (_t(c["xyz"]), _t(c["camera_center"]), _t(c["geo_normal"]), _t(c["ray_d"]))  # noqa: E731
    fused = _leaves(c)
    loss, idx, R = fused_radiance_loss_sg(r, *args(), _t(c["areas"])[..., None], _t(c["visibility"])[..., None], shade_inputs.SGLight(fused[0]),
                                          _t(c["normals"]), fused[1], fused[2], _t(c["radiances"]), fused[3], with_rows=True)
    assert (idx.cpu().numpy() == o["sel"])[~o["threshold"]].all()
    (2.0 * loss).backward()             # (an upstream scalar other than 1)
    lobes, alb, rough, ratio = old = _leaves(c)
    envmap = shading.sg_direct_light(lobes, _t(c["ray_d"])) * _t(c["areas"])[..., None]
    loss_old = radiance_loss(r, *args(), _t(c["visibility"]), envmap, _t(c["normals"]), alb, rough, _t(c["radiances"]), ratio)
    (2.0 * loss_old).backward()
    tol = (o["loss_sum_bound"] + (3 * N + 4) * 2.0 ** -24 * (np.abs(o["out"]).sum() + np.abs(o["target"]).sum())) / (3 * N)
    print("fused", float(loss), "composed", float(loss_old), "fp64", o["loss"], "tol", 2 * tol)
    assert abs(float(loss) - o["loss"]) <= tol and abs(float(loss) - float(loss_old)) <= 2 * tol
    for a, b, kind in ((fused[1], alb, "d_albedos"), (fused[2], rough, "d_roughnesses")):
        diff = (a.grad - b.grad).detach().cpu().numpy().astype(np.float64) / 2.0
        bad = np.abs(diff) > 2 * sp.bound(kind, k[kind + "_cnt"], k[kind + "_abs"])
        skip = np.repeat(o["unsafe"][:, None], diff.shape[1], 1)
        if kind == "d_roughnesses":
            skip[:, 0] |= k["thr"]
        assert np.isfinite(diff).all() and not (bad & ~skip).any(), (kind, int((bad & ~skip).sum()))
    assert abs(float(fused[3].grad) - float(ratio.grad)) / 2.0 <= 2 * ((3 * N + 4) * 2.0 ** -24 * o["d_ratio_abs"] + 2 * o["unsafe_ratio_abs"])
    ref = torch.from_numpy(o["d_lobes"])
    assert lobes.grad is not None and float(lobes.grad.abs().max()) > 0
    lim = 1.5 * o["G32"] + 1e-4
    for tag, g in (("fused", fused[0].grad), ("composed", lobes.grad)):
        e = sc.row_err(g / 2.0, ref)
        print(f"{tag} d_lobes: {float(e.max()):.2e}, budget {lim:.2e}")
        assert float(e.max()) <= lim, tag
    # the texture binding still refuses the light, the SG binding a texture; a light that does not require grad gets none
    with pytest.raises(TypeError, match="lgtSGs"):
        fused_radiance_loss(r, *args(), None, None, shade_inputs.SGLight(fused[0]), None, None, None, None, None)
    with pytest.raises(TypeError, match="lgtSGs"):
        fused_radiance_loss_sg(r, *args(), None, None, shade_inputs.Light(torch.zeros(1, 2, 4, 3, device=DEV)), None, None, None, None, None)
    plain = _leaves(c, lobes_grad=False)
    _run(r, c, plain)[0].backward()
    assert plain[0].grad is None and plain[1].grad is not None
    assert torch.allclose(plain[1].grad, fused[1].grad / 2.0, rtol=1e-4, atol=1e-7 * float(plain[1].grad.abs().max()))


def test_fused_sg_loss_without_rows(built):
    from pbgi.renderer import Renderer
    S = 8
    empty = Renderer()
    empty.hemi_index_buffers, empty.uv_buffers = torch.zeros(0, S, 1, dtype=torch.int32, device=DEV), torch.zeros(0, S, 2, device=DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    lobes = shade_inputs.sg_lobes(4, device=torch.device(DEV)).requires_grad_(True)
    loss, idx, R = empty.radiance_consistency_sg(z(0, 3), z(3), z(0, 3), z(0, S, 3), z(0, S), z(0, S), lobes, z(0, 12), z(0, 12), z(0, 4), z(0, S, 3),
                                                 torch.ones((), device=DEV))
    assert torch.isnan(loss) and idx.shape == (0,) and R.shape == (0, 3)
    loss.backward()
    assert lobes.grad is not None and float(lobes.grad.abs().sum()) == 0.0
