"""The fused activation getters (csrc/activate.hip, svgir_harness/activations.py) on the GPU against the fp64 oracle of
tests/activation_cases.py: values and raw gradients to the bounds stated there, the replaced values and the decision's zeros exactly, the
write and launch contract of the C ABI on NaN-poisoned / sentinel-filled buffers, and TrainStep(raw_params=True)."""
import ctypes as C

import numpy as np
import pytest
import torch

import activation_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0
OUT_FIELD = {"base_color": "out_base_color", "roughness": "out_roughness"}
OUT_WIDTH = {"scales": 3, "rotations": 4, "opacities": 1, "geo_normal": 3, "shading_normal": 12, "shading_normal12": 12, "base_color": 12,
             "roughness": 4, "viewdirs": 3}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _gpu(c):
    raw = {k: v.to(DEV) for k, v in c["raw"].items()}
    return raw, c["campos"].to(DEV), None if c["bcs"] is None else c["bcs"].to(DEV)


def _run(c, want=ac.OUTPUTS, normal_reg=True, fn=None):
    """activate (or `fn`) forward + backward on the case's inputs and upstream gradients: (outputs, raw gradients)."""
    from svgir_harness import activations
    raw, campos, bcs = _gpu(c)
    lv = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    out = (fn or activations.activate)(lv, campos, bcs, want, normal_reg)
    loss = sum((out[k] * c["upstream"][k].to(DEV).reshape(out[k].shape)).sum() for k in want)
    if normal_reg:
        loss = loss + out["normal_reg"] * np.float32(c["g_reg"])
    gr = torch.autograd.grad(loss, [lv[k] for k in ac.RAW], allow_unused=True)
    torch.cuda.synchronize()
    return {k: v.detach() for k, v in out.items()}, dict(zip(ac.RAW, gr))


@pytest.mark.parametrize("name", ac.CASES)
def test_values_and_gradients_match_the_oracle(built, name):
    c, o = ac.case(name), ac.case_oracle(name)
    out, gr = _run(c)
    thr = ac.threshold_mask(c["raw"]["scaling"])
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    for k in ac.OUTPUTS:
        ref = o["values"][k]
        n, bad = ac.mismatches(out[k], ref, ac.value_bound(k, ref), exclude=thr if k == "scales" else None)
        err = (out[k].double().cpu().reshape(ref.shape) - ref).abs()
        print(f"{name} {k}: max |err| / bound = {float(torch.nan_to_num(err / ac.value_bound(k, ref), nan=0.0).max()):.3g}")
        assert n == 0, (name, k, n, c["labels"][np.nonzero(bad.reshape(bad.shape[0], -1).any(1).numpy())[0]])
    # threshold elements: the clamped or the unclamped oracle value
    if bool(thr.any()):
        got = out["scales"].double().cpu()[thr]
        un = torch.exp(c["raw"]["scaling"].double())[thr]
        assert bool(((got == ac.FLT_MAX) | ((got - un).abs() <= ac.value_bound("scales", un))).all()), (got, un)
        assert bool(torch.isfinite(gr["scaling"].cpu()[thr]).all())
    # replaced values are the fp32 constants, exactly
    e = torch.exp(c["raw"]["scaling"].double())
    sc = out["scales"].cpu()
    assert bool((sc[torch.isnan(e)] == f32(1e-6)).all()) and bool((sc[torch.isinf(e.float()) & ~torch.isnan(e) & ~thr] == ac.FLT_MAX).all())
    rot_ref = o["values"]["rotations"]
    assert bool((out["rotations"].cpu()[rot_ref == 1e-6] == f32(1e-6)).all())
    assert bool((out["roughness"].cpu()[torch.isnan(c["raw"]["roughness"])] == f32(1e-8)).all())
    # normal_reg: the double sum to the order of summation, its fp32 rounding
    ref = float(o["values"]["normal_reg"])
    if np.isnan(ref):
        assert bool(torch.isnan(out["normal_reg"])) and bool(torch.isnan(out["normal_reg_sum"]))
    else:
        nel = c["raw"]["normal"].numel()
        assert abs(float(out["normal_reg_sum"]) / nel - ref) <= nel * 2.0 ** -53 * ref
        assert abs(float(out["normal_reg"]) - ref) <= 4 * max(ac.E32["normal_reg"], ac.EPS32) * ref + ac.FLT_MIN
        assert float(out["normal_reg"]) == f32(float(out["normal_reg_sum"]) / nel)
    for k in ac.RAW:
        ref, dec = o["grads"][k], o["decision"][k]
        n, bad = ac.mismatches(gr[k], ref, ac.grad_bound(k, o["aabs"][k]), exclude=thr if k == "scaling" else None)
        err = (gr[k].double().cpu() - ref).abs()
        print(f"{name} d{k}: max |err| / bound = {float(torch.nan_to_num(err / ac.grad_bound(k, o['aabs'][k]), nan=0.0).max()):.3g}")
        assert n == 0, (name, k, n, c["labels"][np.nonzero(bad.reshape(bad.shape[0], -1).any(1).numpy())[0]])
        assert bool((_bits(gr[k].cpu())[dec] == 0).all()), (name, k)          # the decision: +0.0 exactly
    # the same numbers in both layouts, bit for bit
    assert _same_bits(out["shading_normal12"].reshape(-1, 3, 4).transpose(1, 2), out["shading_normal"])
    # a second run gives identical bits, normal_reg included
    out2, gr2 = _run(c)
    for k in out:
        assert _same_bits(out[k], out2[k]) if out[k].dtype == torch.float32 else torch.equal(out[k].view(torch.int64), out2[k].view(torch.int64)), k
    for k in ac.RAW:
        assert _same_bits(gr[k], gr2[k]), k


@pytest.mark.parametrize("name", ["edges", "p5000"])
def test_values_carry_one_fp32_rounding(built, name):
    """Beyond the issue's bound (which for geo_normal and the shading normals is as loose as the reference's fp32 cancellation): the
    kernel evaluates in double and rounds once, so a value is within ONE fp32 rounding of the oracle -- eps32 |oracle| covers it twice
    over -- plus FLT_MIN (denormal flushing) and 1e-15 (the two fp64 evaluations sum the norms in different orders; terms are O(1))."""
    c, o = ac.case(name), ac.case_oracle(name)
    out, _ = _run(c)
    thr = ac.threshold_mask(c["raw"]["scaling"])
    for k in ac.OUTPUTS:
        ref = o["values"][k]
        scale = 1e3 if k in ("geo_normal", "shading_normal", "shading_normal12") else 1.0     # (offsets of 1e3 enter these sums)
        n, bad = ac.mismatches(out[k], ref, ac.EPS32 * ref.abs() + ac.FLT_MIN + 1e-15 * scale, exclude=thr if k == "scales" else None)
        assert n == 0, (name, k, n, c["labels"][np.nonzero(bad.reshape(bad.shape[0], -1).any(1).numpy())[0]])


@pytest.mark.parametrize("name", ["edges_scaled", "p257", "p5000"])
def test_activate_matches_eager_on_the_gpu(built, name):
    """The reference's lines as eager torch fp32 on the same GPU: the same tolerance, except where the decision replaces torch's NaN."""
    c, o = ac.case(name), ac.case_oracle(name)
    out, gr = _run(c)
    eout, egr = _run(c, fn=ac.eager_activate)
    for k in ac.OUTPUTS:
        n, _ = ac.mismatches(out[k], eout[k].double().cpu(), ac.value_bound(k, o["values"][k]))
        assert n == 0, (name, k, n)
    for k in ac.RAW:
        dec = o["decision"][k]
        assert bool(torch.isnan(egr[k].cpu()[dec]).all())
        n, _ = ac.mismatches(gr[k], egr[k].double().cpu(), ac.grad_bound(k, o["aabs"][k]), exclude=dec)
        assert n == 0, (name, k, n)


# ---- the C ABI's write and launch contract -----------------------------------------------------------------------------------------
def _launch_forward(c, want, normal_reg=False, raws=ac.RAW):
    """svgir_activate_forward on sentinel-filled buffers for ALL outputs, pointers passed for `want` only."""
    from gaussian_renderer import _native as N
    raw, campos, bcs = _gpu(c)
    P = raw["xyz"].shape[0]
    bufs = {k: torch.full((P, OUT_WIDTH[k]), SENTINEL, device=DEV) for k in ac.OUTPUTS}
    for k in want:
        bufs[k].fill_(float("nan"))
    a = N.Activation()
    a.P = P
    for k in raws:
        setattr(a, k, raw[k].data_ptr())
    a.campos, a.base_color_scale = campos.data_ptr(), N.ptr(bcs)
    for k in want:
        setattr(a, OUT_FIELD.get(k, k), bufs[k].data_ptr())
    reg = torch.full((3,), SENTINEL, device=DEV)
    reg_sum = torch.full((1,), SENTINEL, device=DEV, dtype=torch.float64)
    partial = torch.zeros(N.lib.svgir_activate_partials(P), device=DEV, dtype=torch.float64)
    if normal_reg:
        a.partial, a.normal_reg_sum, a.normal_reg = partial.data_ptr(), reg_sum.data_ptr(), reg.data_ptr()
    N.guarded(torch.device(DEV), "activate forward", N.lib.svgir_activate_forward, C.byref(a), N.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return bufs, reg, reg_sum


def test_single_output_launches_write_their_buffer_and_nothing_else(built):
    c = ac.case("p257")
    full, reg, reg_sum = _launch_forward(c, ac.OUTPUTS, True)
    assert float(reg[1]) == SENTINEL and float(reg[2]) == SENTINEL and bool(torch.isnan(reg[0]))     # (p257 holds the NaN offset)
    o = ac.case_oracle("p257")
    for k in ac.OUTPUTS:   # every element written: a NaN only where the oracle has one
        assert bool((torch.isnan(full[k]).cpu().reshape(o["values"][k].shape) == torch.isnan(o["values"][k])).all()), k
    for k in ac.OUTPUTS:
        one, reg1, _ = _launch_forward(c, (k,), False, raws=ac.READS[k])
        assert _same_bits(one[k], full[k]), k
        for j in ac.OUTPUTS:
            if j != k:
                assert bool((one[j] == SENTINEL).all()), (k, j)
        assert bool((reg1 == SENTINEL).all())
    s1, _, _ = _launch_forward(c, ac.STAGE1, False, raws=("xyz", "scaling", "rotation", "opacity"))   # stage 1: no material pointers
    for k in ac.OUTPUTS:
        assert _same_bits(s1[k], full[k]) if k in ac.STAGE1 else bool((s1[k] == SENTINEL).all()), k
    only_reg, reg2, reg_sum2 = _launch_forward(c, (), True, raws=("normal",))
    assert _same_bits(reg2[:1], reg[:1]) and torch.equal(reg_sum2.view(torch.int64), reg_sum.view(torch.int64))
    assert all(bool((v == SENTINEL).all()) for v in only_reg.values())


def _launch_backward(c, results, ups=ac.OUTPUTS, g_reg=True):
    from gaussian_renderer import _native as N
    raw, campos, bcs = _gpu(c)
    P = raw["xyz"].shape[0]
    a = N.Activation()
    a.P = P
    for k in ac.RAW:
        setattr(a, k, raw[k].data_ptr())
    a.campos, a.base_color_scale = campos.data_ptr(), N.ptr(bcs)
    g = N.ActivationGrads()
    keep = [c["upstream"][k].to(DEV).contiguous() for k in ups]
    for k, t in zip(ups, keep):
        setattr(g, "dL_d" + OUT_FIELD.get(k, k), t.data_ptr())
    gr = torch.tensor([c["g_reg"]], device=DEV)
    if g_reg:
        g.dL_dnormal_reg = gr.data_ptr()
    bufs = {k: torch.full((P, ac.WIDTH[k]), SENTINEL, device=DEV) for k in ac.RAW}
    for k in results:
        bufs[k].fill_(float("nan"))
        setattr(g, "dL_d" + k, bufs[k].data_ptr())
    N.guarded(torch.device(DEV), "activate backward", N.lib.svgir_activate_backward, C.byref(a), C.byref(g), N.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return bufs


def test_single_result_backward_launches_write_their_buffer_and_nothing_else(built):
    c, o = ac.case("p257"), ac.case_oracle("p257")
    full = _launch_backward(c, ac.RAW)
    for k in ac.RAW:     # written completely, and what the autograd wrapper returns
        assert bool((torch.isnan(full[k]).cpu() == torch.isnan(o["grads"][k])).all()), k
    _, gr = _run(c)
    for k in ac.RAW:
        assert _same_bits(full[k], gr[k]), k
    for k in ac.RAW:
        one = _launch_backward(c, (k,))
        assert _same_bits(one[k], full[k]), k
        for j in ac.RAW:
            if j != k:
                assert bool((one[j] == SENTINEL).all()), (k, j)
    # no upstream gradient at all: every requested result is written, with zeros
    z = _launch_backward(c, ac.RAW, ups=(), g_reg=False)
    for k in ac.RAW:
        assert bool((_bits(z[k]) == 0).all()), k


def test_python_surface_p0_missing_inputs_and_cpu_tensors(built):
    from svgir_harness import activations
    c = ac.case("p1")
    raw, campos, _ = _gpu(c)
    empty = {k: v[:0].clone().requires_grad_(True) for k, v in raw.items()}
    out = activations.activate(empty, campos, None, ac.OUTPUTS, True)
    assert all(out[k].shape[0] == 0 for k in ac.OUTPUTS) and bool(torch.isnan(out["normal_reg"]))
    sum(v.sum() for k, v in out.items() if k in ac.OUTPUTS).backward()
    assert all(empty[k].grad is None or empty[k].grad.shape == empty[k].shape for k in ac.RAW)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        activations.activate(c["raw"], c["campos"])
    with pytest.raises(RuntimeError, match="needs the raw parameter"):
        activations.activate({"xyz": raw["xyz"]}, campos, want=("viewdirs", "scales"))
    s1 = activations.activate({k: raw[k] for k in ("xyz", "scaling", "rotation", "opacity")}, campos, want=ac.STAGE1)
    full = activations.activate(raw, campos)
    assert all(_same_bits(s1[k], full[k]) for k in ac.STAGE1)
    m = activations.ModelActivations({k: torch.nn.Parameter(v.clone()) for k, v in raw.items()})
    m.refresh(campos)
    for getter, k in (("get_scaling", "scales"), ("get_rotation", "rotations"), ("get_opacity", "opacities"), ("get_geo_normal", "geo_normal"),
                      ("get_shading_normal", "shading_normal"), ("get_base_color", "base_color"), ("get_albedo", "base_color"),
                      ("get_roughness", "roughness")):
        assert _same_bits(getattr(m, getter), full[k]), getter
    assert m.get_normals is m.raw["normal"] and m.get_scaling.requires_grad
    base = m.get_scaling.untyped_storage().data_ptr()
    assert all(getattr(m, gname).untyped_storage().data_ptr() == base for gname in ("get_rotation", "get_roughness", "viewdirs"))   # one allocation


# ---- TrainStep(raw_params=True) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["kernel", "eager"])
def test_train_step_on_raw_parameters(built, which):
    from svgir_harness import scenes, workloads
    dev = torch.device(DEV)
    sc = scenes.surface_scene(P=4000, W=160, H=128, seed=71, sh_degree=3, variant="svgss", S=4, VS=52, scale_lo=0.02, scale_hi=0.07)
    ts = workloads.TrainStep(dev, seed=9, Ns=32, scene=sc, raw_params=True, activate=ac.eager_activate if which == "eager" else None)
    raw0 = {k: ts.params[k].detach().cpu().clone() for k in workloads.TrainStep.RAW}
    offs = torch.rand(ts.P, device=dev, generator=torch.Generator(DEV).manual_seed(5)) * (2 * np.pi)
    R, pbr, loss = ts.step(offsets=offs, keep_grads=True)
    torch.cuda.synchronize()
    act = ts.last_activated
    assert set(act) == set(workloads.TrainStep.ACTIVATED) and act["viewdirs"].requires_grad
    # the image of a default TrainStep whose parameters are the activated outputs (and which shades with the same view directions)
    ref = workloads.TrainStep(dev, seed=9, Ns=32, scene=sc)
    with torch.no_grad():
        for k, a in (("scaling", "scales"), ("rotation", "rotations"), ("opacity", "opacities"), ("normal", "shading_normal"),
                     ("base_color", "base_color"), ("roughness", "roughness")):
            ref.params[k].copy_(act[a].detach().reshape(ref.params[k].shape))
    R2, pbr2, loss2 = ref.step(offsets=offs, keep_grads=True, viewdirs=act["viewdirs"].detach())
    torch.cuda.synchronize()
    assert R == R2 and _same_bits(pbr, pbr2) and _same_bits(loss.reshape(1), loss2.reshape(1))
    # the raw gradients = the oracle's adjoint of the activation stage applied to the gradients that reached its outputs
    up = {k: (None if v.grad is None else v.grad.detach().cpu()) for k, v in act.items()}
    assert up["viewdirs"] is None       # (the shading kernels return no gradient for the view directions)
    assert all(up[k] is not None for k in workloads.TrainStep.ACTIVATED if k != "viewdirs")
    campos = ts.st.campos.detach().cpu()
    o = ac.oracle(raw0, campos, None, up, workloads.TrainStep.ACTIVATED, False)
    for k in workloads.TrainStep.RAW:
        if k == "xyz":   # (xyz is also the rasterizer's means3D: its gradient is the rasterizer's alone here, the default step's)
            assert bool((o["grads"]["xyz"] == 0).all()) and bool(torch.isfinite(ts.params["xyz"].grad).all())
            continue
        n, _ = ac.mismatches(ts.params[k].grad, o["grads"][k], ac.grad_bound(k, o["aabs"][k]))
        err = (ts.params[k].grad.double().cpu() - o["grads"][k]).abs()
        print(f"{which} d{k}: max |err| / bound = {float((err / ac.grad_bound(k, o['aabs'][k])).max()):.3g}")
        assert n == 0, (which, k, n)
