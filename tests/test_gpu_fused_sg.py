"""The fused shading under a spherical-Gaussian light (svgir_forward_sg / svgir_backward_sg; include/svgir_raster.h).

The arbiter is the unfused sequence -- shade_and_pack over all P surfels (svgir_shade_forward_sg / _backward_sg), then the rasterizer:
images and every gradient must be BIT-IDENTICAL, no row and no case excluded, except
  * `weights`: float atomics across sub-tiles in both runs (rtol 1e-5, atol 1e-6, as tests/test_gpu_fused_shade.py);
  * the lobes' gradient: fp64 LDS sums per workgroup, then one float atomic per workgroup and sum -- the fused backward walks another
    list of surfels, so the workgroups' shares and the order of their adds differ (rtol 2e-5, atol 2e-6 max|g|: the project's bound for
    this sum, tests/test_gpu_sg_light.py);
  * the radiance ratio's gradient: one fp32 partial sum per workgroup added in a fixed tree -- reproducible per call, but the partial sums
    belong to other surfels in the fused call (2e-5 |g| + 1e-6: the project's bound for this sum, tests/test_gpu_shading.py).
The suite poisons every output (SVGIR_POISON): an element the kernels forget is a NaN."""
import numpy as np
import pytest
import torch

import fused_sg_cases as fc
from gaussian_renderer import _native as N
from gaussian_renderer import shading
from gaussian_renderer.svgss_rasterization import GaussianRasterizer
from svgir_harness import runner, scenes, shade_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAT = ("base_color", "roughness", "normals", "radiance")
GEO = ("means3D", "shs", "opacities", "scales", "rotations")
NAMES = ("num_rendered", "color", "normal", "opacity", "depth", "feature", "vfeature", "weights", "radii")


def _leaves(sct, d, lobes, ratio, view):
    lv = {k: sct[k].detach().clone().requires_grad_(True) for k in GEO}
    lv.update({k: d[k].detach().clone().requires_grad_(True) for k in MAT})
    lv["lobes"] = lobes.detach().clone().requires_grad_(True)
    lv["viewdirs"] = d["viewdirs"].detach().clone().requires_grad_(view)
    if ratio:
        lv["ratio"] = torch.tensor(0.83, device=lobes.device, requires_grad=True)
    return lv


def _unfused(st, d, lv, training, view):
    f, vf, red = shading.shade_and_pack(lv["base_color"], lv["roughness"], lv["normals"], lv["viewdirs"], lv["radiance"],
                                        shade_inputs.SGLight(lv["lobes"]), d["visibility"], d["dirs"], d["areas"], st.viewmatrix, training,
                                        lv.get("ratio"), view_gradient=view)
    m2 = torch.zeros_like(lv["means3D"], requires_grad=True)
    out = GaussianRasterizer(st)(means3D=lv["means3D"], means2D=m2, opacities=lv["opacities"], shs=lv["shs"], scales=lv["scales"],
                                 rotations=lv["rotations"], features=f, vfeatures=vf)
    return out, m2, red


def _fused(st, d, lv, training, view, **kw):
    m2 = torch.zeros_like(lv["means3D"], requires_grad=True)
    out, red = shading.render_shaded(st, lv["means3D"], m2, lv["opacities"], lv["shs"], lv["scales"], lv["rotations"], lv["base_color"],
                                     lv["roughness"], lv["normals"], lv["viewdirs"], lv["radiance"], shade_inputs.SGLight(lv["lobes"]),
                                     d["visibility"], d["dirs"], d["areas"], training, radiance_ratio=lv.get("ratio"), view_gradient=view, **kw)
    return out, m2, red


def _loss(out, gt):
    (R, color, normal, opacity, depth, feature, vfeature, weights, radii) = out
    return ((color * gt["color"]).sum() + (normal * gt["normal"]).sum() + (depth * gt["depth"]).sum() + (opacity * gt["opacity"]).sum() +
            (feature * gt["feature"]).sum() + (vfeature * gt["vfeature"]).sum())


def _same_lobes(ga, gb, what="lobes"):
    print(f"{what}: max|g| {float(ga.abs().max()):.4e}  max|diff| {float((ga - gb).abs().max()):.4e}")
    assert torch.allclose(ga, gb, rtol=2e-5, atol=2e-6 * float(ga.abs().max())), (what, float((ga - gb).abs().max()))
    assert float(ga.abs().max()) > 0


def _same_grads(la, lb, m2a, m2b):
    assert torch.equal(m2a.grad, m2b.grad)
    for k in la:
        ga, gb = la[k].grad, lb[k].grad
        if ga is None:
            assert gb is None and not la[k].requires_grad, k
            continue
        assert gb is not None and not torch.isnan(gb).any(), k
        if k == "lobes":
            _same_lobes(ga, gb)
        elif k == "ratio":
            print(f"ratio: {float(ga):.6e} fused {float(gb):.6e}")
            assert abs(float(ga) - float(gb)) <= 2e-5 * abs(float(ga)) + 1e-6, (float(ga), float(gb))
        else:
            assert torch.equal(ga, gb), k


def _same_images(oa, ob):
    assert oa[0] == ob[0]
    for n, a, b in zip(NAMES[1:], oa[1:], ob[1:]):
        if n == "weights":
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), n
        else:
            assert torch.equal(a, b), n


def _compare(sc, training, lattice, Ns, M, ratio, view, mat_seed=4):
    dev = torch.device(DEV)
    sct = runner.to_torch(sc, dev)
    st = runner.settings(sct, "svgss")
    P = sct["means3D"].shape[0]
    d = fc.materials(sct, st.campos, Ns, training, mat_seed, lattice)
    lobes = fc.lobes(M, device=dev)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in scenes.upstream_grads(sc, "svgss", seed=6).items()}
    la, lb = _leaves(sct, d, lobes, ratio, view), _leaves(sct, d, lobes, ratio, view)
    oa, m2a, _ = _unfused(st, d, la, training, view)
    _loss(oa, gt).backward()
    ob, m2b, _ = _fused(st, d, lb, training, view)
    _loss(ob, gt).backward()
    torch.cuda.synchronize()
    # the subset must be a proper one, or the comparison shows nothing
    blended, culled = int((oa[7] > 0).sum()), int((oa[8] == 0).sum())
    assert 0 < blended < P and culled > 0, (blended, culled)
    _same_images(oa, ob)
    _same_grads(la, lb, m2a, m2b)
    return oa


@pytest.mark.parametrize("case", fc.SMALL, ids=fc.case_id)
def test_fused_view_equals_the_unfused_sequence_small(built, case):
    training, lattice, Ns, M, ratio, view = case
    _compare(fc.small_scene(training), training, lattice, Ns, M, ratio, view)


@pytest.mark.parametrize("P,Ns,training", fc.CHUNK_EDGES)
def test_fused_view_equals_the_unfused_sequence_at_the_chunk_edges(built, P, Ns, training):
    assert N.POISON
    _compare(fc.chunk_scene(P, training), training, True, Ns, 32, False, False, mat_seed=3)


def test_a_view_that_renders_nothing_writes_zero_gradients(built):
    """All surfels behind the camera: nothing is blended, the backward's list is empty (P = one chunk and one more) -- every gradient
    tensor, dL_dlobes and dL_dradiance_ratio are written and exactly zero over NaN-poisoned outputs and scratch."""
    assert N.POISON
    dev = torch.device(DEV)
    sc = fc.chunk_scene(2049, True)
    sct = runner.to_torch(sc, dev)
    st = runner.settings(sct, "svgss")
    axis = st.viewmatrix[:3, 2]   # view depth = means3D @ axis + viewmatrix[3, 2]
    depth = sct["means3D"] @ axis + st.viewmatrix[3, 2]
    sct["means3D"] = (sct["means3D"] - (depth.max() + 5.0) * axis / (axis @ axis)).contiguous()
    d = fc.materials(sct, st.campos, 64, True, 3, True)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in scenes.upstream_grads(sc, "svgss", seed=6).items()}
    lv = _leaves(sct, d, fc.lobes(32, device=dev), True, True)
    out, m2, _ = _fused(st, d, lv, True, True)
    assert out[0] == 0 and int((out[8] != 0).sum()) == 0
    _loss(out, gt).backward()
    torch.cuda.synchronize()
    for k, g in [(k, v.grad) for k, v in lv.items()] + [("means2D", m2.grad)]:
        assert g is not None and g.shape == (m2.shape if k == "means2D" else lv[k].shape), k
        assert not torch.isnan(g).any() and float(g.abs().max()) == 0.0, k


def test_all_surfels_and_a_loss_on_reduced(built):
    """all_surfels=True, want_reduced=True with a loss on `reduced` (the lambda_light form, svgss.py:359-364): every row of `reduced` is
    written and equals the unfused one, the gradients are those of the unfused path; without all_surfels such a loss raises."""
    assert N.POISON
    dev = torch.device(DEV)
    sc = fc.small_scene(True)
    sct = runner.to_torch(sc, dev)
    st = runner.settings(sct, "svgss")
    d = fc.materials(sct, st.campos, 24, True, 4, True)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in scenes.upstream_grads(sc, "svgss", seed=8).items()}
    wr = torch.randn(64, 70, device=dev, generator=torch.Generator(dev).manual_seed(3))
    lobes = fc.lobes(32, device=dev)
    la, lb = _leaves(sct, d, lobes, True, False), _leaves(sct, d, lobes, True, False)
    oa, m2a, red_a = _unfused(st, d, la, True, False)
    (_loss(oa, gt) + (red_a * wr).sum()).backward()
    ob, m2b, red_b = _fused(st, d, lb, True, False, all_surfels=True, want_reduced=True)
    (_loss(ob, gt) + (red_b * wr).sum()).backward()
    torch.cuda.synchronize()
    assert red_b.shape == (64, 70) and not torch.isnan(red_b).any() and torch.equal(red_a, red_b)
    assert int((red_b.abs().sum(1) > 0).sum()) == 64 > int((oa[7] > 0).sum())   # the rows of unblended surfels too
    _same_images(oa, ob)
    _same_grads(la, lb, m2a, m2b)
    with pytest.raises(RuntimeError, match="all_surfels"):
        lc = _leaves(sct, d, lobes, True, False)
        oc, _, red_c = _fused(st, d, lc, True, False, want_reduced=True)
        (_loss(oc, gt) + (red_c * wr).sum()).backward()


def test_write_contract_and_repeatability(built):
    """The binding-level form over poisoned buffers: rows of features / vfeatures / reduced outside the working set and gradient rows of
    unblended surfels are exactly zero, nothing is NaN, and a second run returns identical bits in everything but dL_dlobes."""
    assert N.POISON
    from gaussian_renderer.svgss_rasterization import _C
    dev = torch.device(DEV)
    sc = fc.small_scene(True)
    sct = runner.to_torch(sc, dev)
    st = runner.settings(sct, "svgss")
    P, Ns, M = 64, 24, 33
    d = fc.materials(sct, st.campos, Ns, True, 4, False)
    light = shade_inputs.SGLight(fc.lobes(M, device=dev))
    ratio = torch.tensor(0.83, device=dev)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in scenes.upstream_grads(sc, "svgss", seed=6).items()}
    empty = torch.empty(0, device=dev)
    nan = float("nan")

    def run():
        red = torch.full((P, 70), nan, device=dev)
        f, vf = torch.full((P, 4), nan, device=dev), torch.full((P, 52), nan, device=dev)
        fs, lt, keep = shading.fused_shade_sg(d["base_color"], d["roughness"], d["normals"], d["viewdirs"], d["radiance"], light,
                                              d["visibility"], d["dirs"], d["areas"], st.viewmatrix, True, reduced=red, radiance_ratio=ratio)
        out = _C.rasterize_gaussians(st.bg, sct["means3D"], f, vf, empty, sct["opacities"], sct["scales"], sct["rotations"], st.scale_modifier,
                                     empty, st.viewmatrix, st.projmatrix, st.prcppoint, st.patch_bbox, st.tanfovx, st.tanfovy,
                                     st.image_height, st.image_width, sct["shs"], st.sh_degree, st.campos, False, False, st.config,
                                     shade=fs, sg_light=lt)
        (R, color, normal, depth, opacity, feature, vfeature, weights, radii, gb, bb, ib) = out
        d_lobes = torch.full((M, 7), nan, device=dev)
        gwork = torch.full((N.lib.svgir_sg_grad_work_bytes(M) // 4,), nan, device=dev)
        d_ratio = torch.full((1,), nan, device=dev)
        sg = dict(dL_denv=d_lobes, env_grad_work=gwork, out_weights=weights, dL_dradiance_ratio=d_ratio,
                  _shapes=dict(dL_dbase_color=(P, 12), dL_droughness=(P, 4), dL_dshade_normals=(P, 4, 3), dL_dradiance=(P, Ns, 3),
                               dL_dviewdirs=(P, 3)))
        res = _C.rasterize_gaussians_backward(st.bg, sct["means3D"], f, vf, radii, empty, sct["scales"], sct["rotations"], st.scale_modifier,
                                              empty, st.viewmatrix, st.projmatrix, st.prcppoint, st.patch_bbox, st.tanfovx, st.tanfovy,
                                              gt["color"], gt["normal"], gt["depth"], gt["opacity"], gt["feature"], gt["vfeature"], sct["shs"],
                                              st.sh_degree, st.campos, gb, R, bb, ib, False, st.config, shade=fs, shade_grads=sg,
                                              out_weights=weights, sg_light=lt)
        torch.cuda.synchronize()
        per_surfel = [sg[k] for k in ("dL_dbase_color", "dL_droughness", "dL_dshade_normals", "dL_dradiance", "dL_dviewdirs")]
        return dict(rows=[red, f, vf], weights=weights, radii=radii, images=[color, normal, depth, opacity, feature, vfeature],
                    per_surfel=per_surfel, geo=list(res), d_lobes=d_lobes, d_ratio=d_ratio)

    a, b = run(), run()
    w = a["weights"][:, 0]
    shaded = a["rows"][2].abs().sum(1) > 0
    assert 0 < int(shaded.sum()) < P and bool((shaded | (w == 0)).all()) and bool((a["radii"][shaded] > 0).all())
    for t in a["rows"]:
        assert not torch.isnan(t).any() and float(t[~shaded].abs().max()) == 0.0
    assert 0 < int((w > 0).sum()) < P
    for t in a["per_surfel"]:
        assert not torch.isnan(t).any() and float(t[w == 0].abs().max()) == 0.0 and float(t[w > 0].abs().max()) > 0
    for t in a["geo"] + [a["d_lobes"], a["d_ratio"]]:
        assert not torch.isnan(t).any()
    assert float(a["d_lobes"].abs().max()) > 0 and float(a["d_ratio"].abs()) > 0
    for k in ("rows", "images", "per_surfel", "geo"):
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x, y), k
    assert torch.equal(a["d_ratio"], b["d_ratio"]) and torch.equal(a["radii"], b["radii"])
    _same_lobes(a["d_lobes"], b["d_lobes"], "lobes, second run")


def _texture_run(sc, sct, st, d, gt):
    lv = {k: sct[k].detach().clone().requires_grad_(True) for k in GEO}
    lv.update({k: d[k].detach().clone().requires_grad_(True) for k in MAT + ("env",)})
    m2 = torch.zeros_like(lv["means3D"], requires_grad=True)
    out, _ = shading.render_shaded(st, lv["means3D"], m2, lv["opacities"], lv["shs"], lv["scales"], lv["rotations"], lv["base_color"],
                                   lv["roughness"], lv["normals"], d["viewdirs"], lv["radiance"], shade_inputs.Light(lv["env"]),
                                   d["visibility"], d["dirs"], d["areas"], True)
    _loss(out, gt).backward()
    torch.cuda.synchronize()
    return out, {**{k: v.grad for k, v in lv.items()}, "means2D": m2.grad}


def test_texture_path_bits_are_unchanged_by_fused_sg_calls(built):
    """A texture render_shaded forward + backward before and after fused SG calls in one process: identical bits (d_env: float atomics, to
    rounding).  The SG calls leave nothing behind -- no table, no history entry -- that the texture path would read."""
    dev = torch.device(DEV)
    sc = fc.small_scene(True)
    sct = runner.to_torch(sc, dev)
    st = runner.settings(sct, "svgss")
    d = fc.materials(sct, st.campos, 24, True, 4, True)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in scenes.upstream_grads(sc, "svgss", seed=6).items()}
    oa, ga = _texture_run(sc, sct, st, d, gt)
    for M in (3, 128):
        lv = _leaves(sct, d, fc.lobes(M, device=dev), False, False)
        out, m2, _ = _fused(st, d, lv, True, False)
        _loss(out, gt).backward()
    ob, gb = _texture_run(sc, sct, st, d, gt)
    _same_images(oa, ob)
    for k in ga:
        if k == "env":
            assert torch.allclose(ga[k], gb[k], rtol=2e-5, atol=2e-6 * float(ga[k].abs().max()))
        else:
            assert torch.equal(ga[k], gb[k]), k


def test_a_non_finite_lobe_gives_nan_and_no_fault(built):
    """A zero-norm axis in the fused call: the light of every sample is NaN (torch: 0 / 0), so the light-dependent planes of the view are
    NaN where something was blended; the process goes on, and a following good call is finite."""
    dev = torch.device(DEV)
    sc = fc.small_scene(True)
    sct = runner.to_torch(sc, dev)
    st = runner.settings(sct, "svgss")
    d = fc.materials(sct, st.campos, 24, True, 4, True)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in scenes.upstream_grads(sc, "svgss", seed=6).items()}
    good = fc.lobes(3, device=dev)
    bad = good.clone()
    bad[1, :3] = 0.0
    lv = _leaves(sct, d, bad, False, False)
    out, m2, _ = _fused(st, d, lv, True, False)
    _loss(out, gt).backward()
    torch.cuda.synchronize()
    covered = out[3][0] > 0.5
    assert int(covered.sum()) > 0
    vfeature = out[6]   # training widths: planes 0..2 = pbr, 10..12 = diffuse light (both read the global light)
    assert bool(torch.isnan(vfeature[0:3][:, covered]).all()) and bool(torch.isnan(vfeature[10:13][:, covered]).all())
    assert bool(torch.isfinite(out[1]).all()) and bool(torch.isfinite(out[4]).all())   # colour and depth do not read the light
    lv = _leaves(sct, d, good, False, False)
    out, m2, _ = _fused(st, d, lv, True, False)
    _loss(out, gt).backward()
    torch.cuda.synchronize()
    for t in list(out[1:7]) + [v.grad for v in lv.values() if v.grad is not None]:
        assert bool(torch.isfinite(t).all())


def test_train_step_runs_the_fused_path_under_an_sg_light(built):
    """TrainStep(sg_lobes=32) honours `fused`: after one step with the same lattice offsets every parameter except `env` (the lobes) equals
    the fused=False step's bit for bit, and the lobes' gradients agree to the bound of that sum."""
    from svgir_harness import workloads
    dev = torch.device(DEV)
    offs = (torch.rand(2000, generator=torch.Generator().manual_seed(5)) * 6.2831855).to(dev)
    steps = {}
    for fused in (True, False):
        ts = workloads.TrainStep(dev, seed=9, Ns=32, scene=fc.train_scene(), sg_lobes=32, **({} if fused else {"fused": False}))
        assert ts.fused is fused and ts.params["env"].shape == (32, 7)
        R, pbr, loss = ts.step(offsets=offs, keep_grads=True)
        torch.cuda.synchronize()
        assert R > 0 and bool(torch.isfinite(loss))
        steps[fused] = (R, pbr.detach().clone(), float(loss.detach()), {k: (v.detach().clone(), None if v.grad is None else v.grad.clone())
                                                               for k, v in ts.params.items()})
    (Ra, pa, la, A), (Rb, pb, lb, B) = steps[True], steps[False]
    assert Ra == Rb and torch.equal(pa, pb) and la == lb
    for k in A:
        (va, ga), (vb, gb) = A[k], B[k]
        assert (ga is None) == (gb is None), k
        if k == "env":
            _same_lobes(gb, ga, "env (lobes)")
            continue
        assert torch.equal(va, vb), k   # (the updated value: every parameter but the lobes, bit for bit)
        if k == "radiance_ratio":       # (its gradient: per-workgroup partial sums of other surfels, see the module's docstring)
            assert abs(float(ga) - float(gb)) <= 2e-5 * abs(float(gb)) + 1e-6
        else:
            assert ga is None or torch.equal(ga, gb), k
