"""The fused shading under a spherical-Gaussian light, without a GPU: the two entry points svgir_forward_sg / svgir_backward_sg exist in
the header, the library and the ctypes layer, the ABI is still 14, the binding-level form `shading.fused_shade_sg` exists next to a
`fused_shade` that still refuses an SG light, and every argument check the header lists is made before any launch -- host memory stands
in for device memory, a rejected call dereferences none of it.  The case table the GPU suite runs (tests/fused_sg_cases.py) is checked
to hold what it is built for."""
import ctypes as C
import os
import re

import pytest
import torch

import fused_sg_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svgir_forward_sg", "svgir_backward_sg")


def test_header_library_and_ctypes_agree_and_the_abi_stays_14(built):
    from gaussian_renderer import _native as N
    hdr = open(os.path.join(ROOT, "include", "svgir_raster.h")).read()
    lib = C.CDLL(N.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in N.EXPORTS, name
        fn = getattr(N.lib, name)
        assert fn.restype is C.c_int and fn.argtypes[0] == C.POINTER(N.Params) and fn.argtypes[1] == C.POINTER(N.SgLight), name
    assert N.lib.svgir_forward_sg.argtypes[2] == C.POINTER(N.Outputs) and len(N.lib.svgir_forward_sg.argtypes) == 10
    assert N.lib.svgir_backward_sg.argtypes[2] == C.POINTER(N.Grads) and len(N.lib.svgir_backward_sg.argtypes) == 12
    assert re.search(r"#define\s+SVGIR_ABI_VERSION\s+14\b", hdr)
    assert lib.svgir_abi_version() == N.ABI_VERSION == 14
    # the struct the entry points share with the texture path did not grow
    assert C.sizeof(N.FusedShade) == C.sizeof(N.ShadeParams) + 16 and not hasattr(N.FusedShade, "light")
    assert "svgir_view_call has no room" in hdr   # (svgir_forward_batch with an SG light: stated as not provided)


def test_binding_forms(built):
    from gaussian_renderer import shading
    from svgir_harness import shade_inputs
    assert callable(shading.fused_shade_sg)
    d = shade_inputs.make(4, 3, seed=1)
    args = (d["base_color"], d["roughness"], d["normals"], d["viewdirs"], d["radiance"])
    rest = (d["visibility"], d["dirs"], d["areas"], torch.eye(4), True)
    with pytest.raises(TypeError, match="lgtSGs"):      # the texture binding keeps refusing an SG light
        shading.fused_shade(*args, shade_inputs.SGLight(shade_inputs.sg_lobes(4)), *rest)
    with pytest.raises(TypeError, match="lgtSGs"):      # and the SG binding a texture
        shading.fused_shade_sg(*args, shade_inputs.Light(d["env"]), *rest)
    with pytest.raises(RuntimeError, match="lgtSGs must be"):
        shading.fused_shade_sg(*args, shade_inputs.SGLight(torch.zeros(129, 7)), *rest)
    with pytest.raises(RuntimeError, match="GPU"):      # valid arguments on the CPU: no CPU path
        shading.fused_shade_sg(*args, shade_inputs.SGLight(shade_inputs.sg_lobes(4)), *rest)
    from gaussian_renderer.svgss_rasterization import _C
    with pytest.raises(ValueError, match="sg_light"):   # a light without the fused shading it belongs to
        _C.rasterize_gaussians(*([None] * 24), sg_light=object())


def _host_call():
    """A complete svgir_forward_sg / svgir_backward_sg argument set over host memory (never launched: every use below breaks one thing)."""
    from gaussian_renderer import _native as N
    buf = (C.c_float * 8192)()
    base = C.addressof(buf)
    base += -base % 16
    a = base
    fs = N.FusedShade()
    sp = fs.sp
    sp.P, sp.Ns, sp.training = 8, 6, 1
    for k in ("base_color", "roughness", "normals", "viewdirs", "radiance", "visibility", "incident_dirs", "incident_areas", "viewmatrix"):
        setattr(sp, k, a)
    p = N.Params()
    p.variant, p.P, p.S, p.VS, p.D, p.M, p.W, p.H = N.SVGSS, 8, 4, 52, 0, 1, 32, 32
    for k in ("background", "means3D", "shs", "features", "vfeatures", "opacities", "scales", "rotations", "viewmatrix", "projmatrix",
              "cam_pos", "patchbbox"):
        setattr(p, k, a)
    p.scale_modifier, p.tan_fovx, p.tan_fovy = 1.0, 0.5, 0.5
    p.shade = C.addressof(fs)
    lt = N.SgLight()
    lt.count, lt.lobes, lt.work = 4, a, a + 1024
    o = N.Outputs()
    g = N.Grads()
    for k in ("dL_dout_color", "dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dfeatures", "dL_dvfeatures", "dL_dnormal", "dL_ddepth",
              "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dbase_color", "dL_droughness", "dL_dshade_normals",
              "dL_dradiance", "dL_denv", "env_grad_work", "out_weights"):
        setattr(g, k, a)
    return N, dict(p=p, lt=lt, o=o, g=g, fs=fs, buf=buf, a=a)


def _alloc_must_not_run(nbytes, ctx):
    raise AssertionError("an allocator ran: the call was not rejected up front")


def test_invalid_arguments_are_rejected_before_any_launch(built):
    N, h = _host_call()
    cb = N.ALLOC_FN(_alloc_must_not_run)
    a = h["a"]

    def fwd(p=h["p"], lt=h["lt"]):
        return N.lib.svgir_forward_sg(p, lt, h["o"], cb, None, cb, None, cb, None, None)

    def bwd(p=h["p"], lt=h["lt"], g=h["g"]):
        return N.lib.svgir_backward_sg(p, lt, g, 1, a, a, a, 4096, a, a, 4096, None)

    def light(count=4, lobes=a, work=a + 1024):
        lt = N.SgLight()
        lt.count, lt.lobes, lt.work = count, lobes, work
        return lt

    def params(**kw):
        q = N.Params()
        C.memmove(C.addressof(q), C.addressof(h["p"]), C.sizeof(q))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def fused(**kw):
        fs = N.FusedShade()
        C.memmove(C.addressof(fs), C.addressof(h["fs"]), C.sizeof(fs))
        for k, v in kw.items():
            setattr(fs.sp if hasattr(fs.sp, k) else fs, k, v)
        return fs

    def grads(**kw):
        g = N.Grads()
        C.memmove(C.addressof(g), C.addressof(h["g"]), C.sizeof(g))
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    for call in (fwd, bwd):
        # the light
        assert call(lt=None) == -1 and "light is NULL" in N.last_error(), N.last_error()
        for lt, word in ((light(count=0), "count"), (light(count=129), "count"), (light(count=-3), "count"), (light(lobes=None), "NULL"),
                         (light(work=None), "NULL"), (light(work=a + 1024 + 4), "aligned")):
            assert call(lt=lt) == -1 and word in N.last_error(), (word, N.last_error())
        assert call(p=None) == -1 and "params" in N.last_error()
        # the call must be a fused-shading call of the svgss variant at the widths `training` packs
        assert call(p=params(shade=None)) == -1 and "shade" in N.last_error(), N.last_error()
        assert call(p=params(variant=N.RGSS, VS=0)) == -1 and "svgss" in N.last_error(), N.last_error()
        assert call(p=params(S=7, VS=64)) == -1 and "packs" in N.last_error(), N.last_error()
        keep = fused(training=0)
        assert call(p=params(shade=C.addressof(keep))) == -1 and "packs" in N.last_error(), N.last_error()
        keep = fused(P=9)
        assert call(p=params(shade=C.addressof(keep))) == -1 and "sp.P" in N.last_error(), N.last_error()
        keep = fused(viewmatrix=None)
        assert call(p=params(shade=C.addressof(keep))) == -1 and "viewmatrix" in N.last_error(), N.last_error()
    # the backward's outputs, checked before its first launch
    for field in ("dL_denv", "env_grad_work", "dL_dbase_color", "dL_droughness", "dL_dshade_normals", "dL_dradiance"):
        assert bwd(g=grads(**{field: None})) == -1 and "gradient outputs" in N.last_error(), (field, N.last_error())
    assert bwd(g=grads(out_weights=None)) == -1 and "out_weights" in N.last_error()
    assert bwd(g=grads(dL_dreduced=a)) == -1 and "all_surfels" in N.last_error()
    assert bwd(g=None) == -1
    with pytest.raises(RuntimeError, match=r"forward_sg failed \(-1\).*count"):
        N.check(fwd(lt=light(count=0)), "forward_sg")


def test_the_case_table_holds_what_it_is_built_for():
    lobe_counts = {c[3] for c in fc.SMALL}
    assert lobe_counts == {1, 3, 32, 33, 128}
    for quad in (True, False):   # 128 lobes once per forward kernel
        assert sum(1 for c in fc.SMALL if c[3] == 128 and (c[2] < 128) == quad) == 1
    assert {c[2] for c in fc.SMALL} == {7, 24, 200}
    for col in (0, 1, 4, 5):     # widths, lattice, radiance_ratio, view_gradient: both values
        assert {c[col] for c in fc.SMALL} == {True, False}, col
    for tr in (True, False):     # both widths with both direction kinds and both kernels
        assert {(c[1], c[2] >= 128) for c in fc.SMALL if c[0] == tr} == {(True, True), (True, False), (False, True), (False, False)}
    assert len({fc.case_id(c) for c in fc.SMALL}) == len(fc.SMALL)
    assert {c[0] for c in fc.CHUNK_EDGES} == {2047, 2048, 2049, 4097} and len(fc.CHUNK_EDGES) == 8
    lb = fc.lobes(33)
    assert lb.shape == (33, 7) and torch.equal(lb, fc.lobes(33)) and float(lb[:, :3].norm(dim=-1).min()) > 0
    sc = fc.small_scene(True)
    assert sc["means3D"].shape == (64, 3) and (sc["W"], sc["H"]) == (32, 32)


def test_the_small_view_culls_some_surfels_and_blends_some(built):
    """On the CPU oracle: the working set of the small view and of a chunk-edge view is a proper, non-empty subset."""
    import numpy as np
    from oracle import oracle as orc
    for sc in (fc.small_scene(True), fc.chunk_scene(2049, True)):
        o = orc.OracleRun(sc, orc.SVGSS)
        o.forward()
        im = o.images()
        P = sc["means3D"].shape[0]
        blended = int((np.asarray(im["weights"]).reshape(-1) > 0).sum())
        assert 0 < blended < P and int((im["radii"] == 0).sum()) > 0
