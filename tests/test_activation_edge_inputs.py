"""CPU checks of the activation cases (tests/activation_cases.py): the fp64 oracle is pinned against the reference's own getters
(tests/golden/activations.npz, scripts/make_golden_activations.py), against central differences and against the zero-gradient decision;
every case of the table holds what it claims; and E32 / G32 -- what the reference's fp32 arithmetic loses -- are measured and compared
with the constants the GPU test's tolerances are built from.  The entry points' argument checks run here too (no kernel is launched)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import activation_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "activations.npz")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("tag", ["ones", "scaled"])
def test_oracle_matches_the_reference_getters(tag):
    """The reference's getters and autograd (fp32, CPU) against the oracle, to the bounds the kernels are held to; where the reference's
    gradient is NaN the oracle has either the decision's exact zero or a propagated NaN."""
    g = np.load(GOLD)
    raw = {k: _t(g[f"{tag}/raw_{k}"]) for k in ac.RAW}
    want = tuple(k for k in ac.OUTPUTS if k != "shading_normal12")
    up = {k: _t(g[f"{tag}/up_{k}"]) for k in want}
    bcs = _t(g[f"{tag}/base_color_scale"])
    o = ac.oracle(raw, _t(g[f"{tag}/campos"]), bcs, up, want, True, float(g[f"{tag}/g_reg"]))
    thr = ac.threshold_mask(raw["scaling"])
    assert not bool(thr.any())
    for k in want:
        n, bad = ac.mismatches(_t(g[f"{tag}/out_{k}"]), o["values"][k], ac.value_bound(k, o["values"][k]))
        assert n == 0, (k, n, g[f"{tag}/labels"][np.nonzero(bad.reshape(bad.shape[0], -1).any(1).numpy())[0]])
    reg, oreg = float(g[f"{tag}/out_normal_reg"]), float(o["values"]["normal_reg"])
    assert np.isnan(reg) and np.isnan(oreg) if tag == "ones" else abs(reg - oreg) <= 4 * ac.E32["normal_reg"] * oreg
    n_dec = 0
    for k in ac.RAW:
        ref, mine, dec = _t(g[f"{tag}/grad_{k}"]).double(), o["grads"][k], o["decision"][k]
        nan = torch.isnan(ref)
        assert bool((nan[dec]).all()), k                                   # torch yields NaN wherever the decision applies ...
        assert bool((mine[dec] == 0).all()), k                             # ... and the oracle an exact zero
        assert bool((torch.isnan(mine) == (nan & ~dec)).all()), k          # every other NaN is a propagated one, in both
        n_dec += int(dec.sum())
        fin = ~nan
        err = (ref - mine).abs()[fin]
        assert bool((err <= ac.grad_bound(k, o["aabs"][k])[fin]).all()), (k, float(err.max()))
    assert n_dec >= 6 + 12 + 1      # scaling: NaN x 4, +100, +inf; three rotation rows; one roughness element


def test_oracle_matches_central_differences():
    g = torch.Generator().manual_seed(3)
    raw = ac._random_rows(12, g)
    campos, bcs = torch.tensor(ac.CAMPOS), torch.tensor([1.0, 0.5, 2.0])
    up = {k: torch.randn(12, *s, generator=g) for k, s in (("scales", (3,)), ("rotations", (4,)), ("opacities", (1,)), ("geo_normal", (3,)),
          ("shading_normal", (4, 3)), ("shading_normal12", (12,)), ("base_color", (12,)), ("roughness", (4,)), ("viewdirs", (3,)))}
    o = ac.oracle(raw, campos, bcs, up, ac.OUTPUTS, True, 0.37)

    def loss(lv):
        out = ac.oracle_outputs(lv, campos.double(), bcs.double(), ac.OUTPUTS, True)
        return float(sum((out[k] * up[k].double().reshape(out[k].shape)).sum() for k in ac.OUTPUTS) + 0.37 * out["normal_reg"])
    base = {k: v.double() for k, v in raw.items()}
    for k in ac.RAW:
        num = torch.zeros_like(base[k])
        flat = num.view(-1)
        for i in range(flat.numel()):
            h = 1e-6 * max(1.0, abs(float(base[k].view(-1)[i])))
            lo, hi = {r: v.clone() for r, v in base.items()}, {r: v.clone() for r, v in base.items()}
            lo[k].view(-1)[i] -= h
            hi[k].view(-1)[i] += h
            flat[i] = (loss(hi) - loss(lo)) / (2 * h)
        scale = o["aabs"][k].clamp_min(1e-12)
        assert float(((num - o["grads"][k]).abs() / scale).max()) < 1e-6, k


def test_every_case_holds_what_it_claims():
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    for name in ac.CASES:
        c = ac.case(name)
        thr = ac.threshold_mask(c["raw"]["scaling"])
        assert bool(thr.any()) == (name == "threshold"), name              # exactly one case holds threshold elements
    assert int(ac.threshold_mask(ac.case("threshold")["raw"]["scaling"]).sum()) == 5
    c, o, r32 = ac.case("edges"), ac.case_oracle("edges"), ac.case_ref32("edges")
    row = lambda lab: int(np.nonzero(c["labels"] == lab)[0][0])  # noqa: E731
    v, v32, gr, dec = o["values"], r32["values"], o["grads"], o["decision"]
    # replaced values: the oracle holds the constant, ref32 the fp32 constant exactly
    assert float(v["scales"][row("scaling_nan"), 1]) == 1e-6 and float(v32["scales"][row("scaling_nan"), 1]) == f32(1e-6)
    assert bool((v32["scales"][row("scaling_all_nan")] == f32(1e-6)).all())
    for lab, col in (("scaling_+100", 0), ("scaling_+inf", 1)):
        assert float(v["scales"][row(lab), col]) == ac.FLT_MAX == float(v32["scales"][row(lab), col]) and bool(dec["scaling"][row(lab), col])
    assert 0 < float(v["scales"][row("scaling_-100"), 2]) < ac.FLT_MIN and not bool(dec["scaling"][row("scaling_-100")].any())
    assert float(v["scales"][row("scaling_-inf"), 0]) == 0.0 and float(gr["scaling"][row("scaling_-inf"), 0]) == 0.0
    # the clamp of normalize: zero and 1e-20 below it, 1e-6 above it, none inside
    q = c["raw"]["rotation"].double()
    n = q.norm(dim=-1)
    assert float(n[row("quat_zero")]) == 0 and float(n[row("quat_1e-20")]) < 1e-15 and float(n[row("quat_1e-6")]) > 1e-9
    fin = torch.isfinite(n)
    assert not bool(((n[fin] > 1e-13) & (n[fin] < 1e-11)).any())
    assert bool((v["rotations"][row("quat_zero")] == 0).all())
    gz = gr["rotation"][row("quat_zero")]
    assert bool(torch.isfinite(gz).all()) and float(gz.abs().max()) > 1e9      # g / 1e-12: finite
    assert abs(float(v["rotations"][row("quat_1e-20")].norm()) - float(n[row("quat_1e-20")]) / 1e-12) < 1e-20
    assert abs(float(v["rotations"][row("quat_1e-6")].norm()) - 1) < 1e-12
    for lab in ("quat_nan", "quat_inf", "quat_-inf"):
        assert bool(dec["rotation"][row(lab)].all()) and bool((gr["rotation"][row(lab)] == 0).all())
    assert bool((v32["rotations"][row("quat_nan")] == f32(1e-6)).all())
    qi = v["rotations"][row("quat_inf")]
    assert float(qi[1]) == 1e-6 and bool((qi[[0, 2, 3]] == 0).all())
    assert abs(float(n[row("quat_unit")]) - 1) == 0 and bool((v["geo_normal"][row("quat_unit")] == torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)).all())
    # saturations and NaNs of the sigmoids
    assert float(v32["opacities"][row("opacity_+100")]) == 1.0 and 0 < float(v["opacities"][row("opacity_-100")]) < ac.FLT_MIN
    assert bool(torch.isnan(v["opacities"][row("opacity_nan")]).all()) and bool(torch.isnan(gr["opacity"][row("opacity_nan")]).all())
    bs = v32["base_color"][row("base_color_sat")]
    assert bool((bs[0::2] == f32(f32(0.77) + f32(0.03))).all()) and bool(((bs[1::2] - f32(0.03)).abs() < 1e-8).all())
    assert bool(torch.isnan(v["base_color"][row("base_color_nan"), 5])) and int(torch.isnan(v["base_color"]).sum()) == 1
    rs = v32["roughness"][row("roughness_sat")]
    assert bool(((rs[0::2] - 0.99).abs() < 1e-7).all()) and bool(((rs[1::2] - 0.09).abs() < 1e-7).all())
    assert float(v["roughness"][row("roughness_nan"), 2]) == 1e-8 and float(v32["roughness"][row("roughness_nan"), 2]) == f32(1e-8)
    assert bool(dec["roughness"][row("roughness_nan"), 2]) and int(dec["roughness"].sum()) == 1
    # the shading normals' own edges
    assert bool((c["raw"]["normal"][row("offsets_zero")] == 0).all())
    assert bool((v["shading_normal"][row("offset_cancels_geo"), 2] == 0).all()) and bool((v["shading_normal"][row("offset_cancels_geo_x"), 1] == 0).all())
    assert bool(torch.isfinite(gr["normal"][row("offset_cancels_geo")]).all()) and float(gr["normal"][row("offset_cancels_geo")].abs().max()) > 1e9
    assert float(c["raw"]["normal"][row("offsets_1e3")].abs().max()) > 1e3
    assert bool((v["shading_normal12"].reshape(-1, 3, 4).transpose(1, 2) == v["shading_normal"]).masked_fill(torch.isnan(v["shading_normal"]), True).all())
    assert bool((v["viewdirs"][row("xyz_at_campos")] == 0).all()) and bool(torch.isfinite(gr["xyz"][row("xyz_at_campos")]).all())
    # an upstream NaN passes through, into its own element only
    assert bool(torch.isnan(gr["opacity"][0]).all()) and bool(torch.isnan(gr["base_color"][0, 3])) and int(torch.isnan(gr["base_color"][0]).sum()) == 1
    # the sizes: 1, one below / on / one above / twice the workgroup, several workgroups
    assert [ac.case(n)["raw"]["xyz"].shape[0] for n in ac.CASES if n.startswith("p")] == [1, ac.WG - 1, ac.WG, ac.WG + 1, 2 * ac.WG, 5000]
    assert {ac.case(n)["bcs"] is None for n in ac.CASES} == {True, False}


def test_e32_g32_tables():
    """What the reference's own operation order loses in fp32, per output (E32) and per raw gradient (G32, relative to Aabs), over the whole
    table.  The constants of activation_cases.py must not be smaller than the measurement."""
    e32 = {k: 0.0 for k in ac.OUTPUTS + ("normal_reg",)}
    g32 = {k: 0.0 for k in ac.RAW}
    for name in ac.CASES:
        c, o, r = ac.case(name), ac.case_oracle(name), ac.case_ref32(name)
        thr = ac.threshold_mask(c["raw"]["scaling"])
        for k in e32:
            ref, got = o["values"][k], r["values"][k].double().reshape(o["values"][k].shape)
            assert bool((torch.isnan(ref) == torch.isnan(got)).all()), (name, k)
            ok = ~torch.isnan(ref)
            if k == "scales":
                ok &= ~thr
            if bool(ok.any()):
                e32[k] = max(e32[k], float(((got - ref).abs() / ref.abs().clamp_min(ac.FLT_MIN))[ok].max()))
        for k in ac.RAW:
            ref, got, dec = o["grads"][k], r["grads"][k].double(), o["decision"][k]
            assert bool((ref[dec] == 0).all()) and bool(torch.isnan(got[dec]).all()), (name, k)     # the decision: exactly 0 where torch has NaN
            ok = ~dec & ~torch.isnan(ref)
            assert bool((torch.isnan(got) == (torch.isnan(ref) | dec)).all()), (name, k)
            if k == "scaling":
                ok &= ~thr
                assert bool(torch.isfinite(ref[thr]).all())
            over = ((got - ref).abs() - ac.FLT_MIN).clamp_min(0.0)[ok]
            a = o["aabs"][k][ok]
            assert bool((over[a == 0] == 0).all()), (name, k)
            if bool((a > 0).any()):
                g32[k] = max(g32[k], float((over[a > 0] / a[a > 0]).max()))
    print("E32 (measured | constant):")
    for k, v in e32.items():
        print(f"  {k:18s} {v:.3e} | {ac.E32[k]:.1e}")
    print("G32 (measured | constant):")
    for k, v in g32.items():
        print(f"  {k:18s} {v:.3e} | {ac.G32[k]:.1e}")
    for k, v in e32.items():
        assert v <= ac.E32[k], (k, v)
    for k, v in g32.items():
        assert v <= ac.G32[k], (k, v)


def test_entry_points_validate_their_arguments(built):
    """A requested output whose input is missing: -1 and a message; P == 0: success; nothing is launched in either case."""
    from gaussian_renderer import _native as N
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16          # a 16-byte aligned host address: never dereferenced
    a = N.Activation()
    a.P, a.scales = 4, p
    assert N.lib.svgir_activate_forward(C.byref(a), None) == -1 and "scaling" in N.last_error()
    a = N.Activation()
    a.P, a.viewdirs, a.xyz = 4, p, p
    assert N.lib.svgir_activate_forward(C.byref(a), None) == -1 and "campos" in N.last_error()
    a = N.Activation()
    a.P, a.shading_normal, a.rotation = 4, p, p
    assert N.lib.svgir_activate_forward(C.byref(a), None) == -1 and "normal" in N.last_error()
    a = N.Activation()
    a.P, a.rotations, a.rotation = 4, p, p + 4
    assert N.lib.svgir_activate_forward(C.byref(a), None) == -1 and "aligned" in N.last_error()
    a = N.Activation()
    a.P, a.normal_reg, a.normal = 4, p, p
    assert N.lib.svgir_activate_forward(C.byref(a), None) == -1 and "partial" in N.last_error()
    a = N.Activation()
    a.P, a.rotation = 4, p
    assert N.lib.svgir_activate_forward(C.byref(a), None) == -1 and "no output" in N.last_error()
    a.P = -1
    assert N.lib.svgir_activate_forward(C.byref(a), None) == -1 and "bad P" in N.last_error()
    a = N.Activation()
    a.P, a.scales, a.scaling = 0, p, p
    assert N.lib.svgir_activate_forward(C.byref(a), None) == 0
    g = N.ActivationGrads()
    assert N.lib.svgir_activate_backward(C.byref(a), C.byref(g), None) == -1 and "no gradient" in N.last_error()
    g.dL_dscaling = p
    assert N.lib.svgir_activate_backward(C.byref(a), C.byref(g), None) == 0          # P == 0
    a.P, a.scaling = 4, None
    assert N.lib.svgir_activate_backward(C.byref(a), C.byref(g), None) == -1 and "scaling" in N.last_error()
    g = N.ActivationGrads()
    a = N.Activation()
    a.P, a.normal, g.dL_dnormal, g.dL_dshading_normal = 4, p, p, p
    assert N.lib.svgir_activate_backward(C.byref(a), C.byref(g), None) == -1 and "rotation" in N.last_error()
    assert N.lib.svgir_activate_partials(0) == 0 and N.lib.svgir_activate_partials(1) == 1
    assert N.lib.svgir_activate_partials(ac.WG) == 1 and N.lib.svgir_activate_partials(ac.WG + 1) == 2


def test_struct_mirrors_match_the_header(built):
    import re
    from gaussian_renderer import _native as N
    hdr = open(os.path.join(ROOT, "include", "svgir_raster.h")).read()
    for struct, mirror in (("svgir_activation", N.Activation), ("svgir_activation_grads", N.ActivationGrads)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") if decl.strip()
                 for n in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).replace("*", " ").replace(",", " ").split()]
        assert names == [f[0] for f in mirror._fields_], struct


def test_python_surface_rejects_cpu_tensors_and_missing_inputs(built):
    from svgir_harness import activations
    c = ac.case("p1")
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        activations.activate(c["raw"], c["campos"])
    with pytest.raises(RuntimeError, match="needs the raw parameter 'normal'"):
        activations.activate({k: c["raw"][k] for k in ("xyz", "scaling", "rotation", "opacity")}, c["campos"])
    with pytest.raises(RuntimeError, match="needs campos"):
        activations.activate(c["raw"], None)
    with pytest.raises(ValueError, match="unknown output"):
        activations.activate(c["raw"], c["campos"], want=("scale",))
    assert activations.OUTPUTS == ac.OUTPUTS and activations.RAW == ac.RAW
