"""GPU tests of the pbgi irradiance kernels (csrc/irradiance.hip) through `pbgi.Renderer.render_irradiance_sample` (forward and
backward), `Renderer.render_irradiance` and `svgir_harness.losses.radiance_loss`, on every case of tests/radiance_cases.py.

Tolerances (tests/radiance_cases.py `bound`): per element |gpu - fp64| <= (n * 2^-24 + 4 * E_TERM[kind]) * sum |t|, n = S for the forward and
the number of contributions for a gradient element.  The first term bounds a sum taken in any order (the order is free), E_TERM[kind] is
the measured deviation of one fp32 term of that kind (out, d_envmap, d_albedos, d_roughnesses; the full form's out) from fp64 and the factor 4 allows the device's exp2, divide and square root a few ulp each.  An
element without any contribution has sum |t| = 0 and must be exactly zero -- every buffer is NaN-filled before the call
(tests/conftest.py), so that also proves the element was written.  Elements of d_roughnesses that receive a threshold term (a
denominator within 1e-4 relative of the 1e-6 clamp) are compared for finiteness only.  The forward is bitwise equal on a second call."""
import numpy as np
import pytest
import torch

from tests import radiance_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = sorted(rc.CASES)
FULL_NAMES = [n for n in NAMES if rc.has_full(n)]


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).to(DEV)


def _renderer(c):
    from pbgi.renderer import Renderer
    r = Renderer()
    r.hemi_index_buffers = _t(c["hit"]).reshape(c["N"], c["S"], 1)
    r.uv_buffers = _t(c["uvs"])
    return r


def _sample(r, c, leaves=None, sample=None):
    env, alb, rough = leaves if leaves is not None else (_t(c["envmap"]), _t(c["albedos"]), _t(c["roughnesses"]))
    idx = _t(c["sample"] if sample is None else sample).reshape(-1, 1)
    return r.render_irradiance_sample(c["N"], c["S"], idx, env, _t(c["ray_d"]), None, None, None, _t(c["normals"]), alb, rough, None, None, None)


def _close(kind, got, want, cnt, mag, what, finite_only=None):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: {np.count_nonzero(~np.isfinite(got))} non-finite elements (an element the kernel did not write is NaN)"
    err, tol = np.abs(got - want), rc.bound(kind, cnt, mag)
    ratio = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
    print(f"{what}: worst error / bound = {ratio:.3g}")
    bad = err > tol
    if finite_only is not None:
        bad &= ~finite_only
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} elements off, first {np.argwhere(bad)[0]}: {got[bad][0]} vs {want[bad][0]} (bound {tol[bad][0]})"


@pytest.mark.parametrize("name", NAMES)
def test_sample_form_forward_and_backward(built, name):
    c, o = rc.case(name), rc.oracle(name)
    N, S = c["N"], c["S"]
    r = _renderer(c)
    leaves = [_t(c[k]).requires_grad_(True) for k in ("envmap", "albedos", "roughnesses")]
    out = _sample(r, c, leaves)
    assert out.shape == (N, 3) and out.dtype == torch.float32 and out.requires_grad
    _close("out", out, o["out"], o["out_cnt"], o["out_abs"], name + " out")
    again = _sample(r, c)
    assert torch.equal(out.detach().view(torch.int32), again.view(torch.int32)) and not again.requires_grad
    out.backward(_t(c["grad_out"]))
    for leaf, k in zip(leaves, ("d_envmap", "d_albedos", "d_roughnesses")):
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape and leaf.grad.dtype == torch.float32
        only = None
        if k == "d_roughnesses":
            only = np.zeros((N, 4), bool)
            only[:, 0] = o["thr"]
        _close(k, leaf.grad, o[k], o[k + "_cnt"], o[k + "_abs"], name + " " + k, only)


@pytest.mark.parametrize("name", FULL_NAMES)
def test_full_form_forward(built, name):
    c, o = rc.case(name), rc.oracle_full(name)
    N, S = c["N"], c["S"]
    r = _renderer(c)
    args = lambda: (N, S, _t(c["envmap"]).requires_grad_(True), _t(c["ray_d"]), None, None, None, _t(c["normals"]), _t(c["albedos"]).requires_grad_(True),
                    _t(c["roughnesses"]), None, None, None)
    out = r.render_irradiance(*args())
    assert out.shape == (N, S, 3) and out.dtype == torch.float32 and not out.requires_grad and out.grad_fn is None
    _close("full", out, o["out"], float(S), o["out_abs"], name + " full out")
    assert torch.equal(out.view(torch.int32), r.render_irradiance(*args()).view(torch.int32))


def test_none_gradients_dtypes_and_strided_inputs(built):
    """every argument other than envmap, albedos and roughnesses gets no gradient; fp64 / strided / [N] or [N,1] int64 inputs are taken
    as their contiguous fp32 / int32 copies"""
    name = "random_65x65"
    c, o = rc.case(name), rc.oracle(name)
    N, S = c["N"], c["S"]
    r = _renderer(c)
    r.hemi_index_buffers = r.hemi_index_buffers.long()
    ray_d, normals = _t(c["ray_d"]).requires_grad_(True), _t(c["normals"]).requires_grad_(True)
    wide = torch.zeros(N, S, 5, dtype=torch.float64, device=DEV)
    wide[..., 1:4] = _t(c["envmap"]).double()
    env = wide[..., 1:4].requires_grad_(True)
    alb, rough = _t(c["albedos"]).requires_grad_(True), _t(c["roughnesses"]).requires_grad_(True)
    assert not env.is_contiguous()
    out = r.render_irradiance_sample(N, S, _t(c["sample"]).long(), env, ray_d, None, None, None, normals, alb, rough, None, None, None)
    _close("out", out, o["out"], o["out_cnt"], o["out_abs"], name + " out (strided)")
    out.backward(_t(c["grad_out"]))
    assert ray_d.grad is None and normals.grad is None
    assert env.grad.shape == env.shape and alb.grad.shape == alb.shape and rough.grad.shape == rough.shape
    _close("d_envmap", env.grad, o["d_envmap"], o["d_envmap_cnt"], o["d_envmap_abs"], name + " d_envmap (strided)")


def test_unset_buffers_mismatched_rows_and_cpu_tensors_raise(built):
    from pbgi.renderer import Renderer
    c = rc.case("random_65x3")
    N, S = c["N"], c["S"]
    call = lambda r, n=N, f=_t: r.render_irradiance_sample(n, S, f(c["sample"][:n]), f(c["envmap"][:n]), f(c["ray_d"][:n]), None, None, None,
                                                           f(c["normals"][:n]), f(c["albedos"][:n]), f(c["roughnesses"][:n]), None, None, None)
    with pytest.raises(RuntimeError, match="are not set"):
        call(Renderer())
    r = _renderer(c)
    with pytest.raises(ValueError, match="do not hold N"):
        call(r, N - 1)
    with pytest.raises(ValueError, match="do not hold N"):
        r.render_irradiance(N - 1, S, _t(c["envmap"][:N - 1]), _t(c["ray_d"][:N - 1]), None, None, None, _t(c["normals"][:N - 1]),
                            _t(c["albedos"][:N - 1]), _t(c["roughnesses"][:N - 1]), None, None, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(r, N, lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()))
    empty = Renderer()
    empty.hemi_index_buffers, empty.uv_buffers = torch.zeros(0, S, 1, dtype=torch.int32, device=DEV), torch.zeros(0, S, 2, device=DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    out = empty.render_irradiance_sample(0, S, torch.zeros(0, 1, dtype=torch.int32, device=DEV), z(0, S, 3), z(0, S, 3), None, None, None, z(0, 12),
                                         z(0, 12), z(0, 4), None, None, None)
    assert out.shape == (0, 3) and empty.render_irradiance(0, S, z(0, S, 3), z(0, S, 3), None, None, None, z(0, 12), z(0, 12), z(0, 4), None, None,
                                                           None).shape == (0, S, 3)


def test_side_stream_without_synchronisation(built):
    name = "random_300x64"
    c, o = rc.case(name), rc.oracle(name)
    r = _renderer(c)
    leaves = [_t(c[k]).requires_grad_(True) for k in ("envmap", "albedos", "roughnesses")]
    g = _t(c["grad_out"])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        out = _sample(r, c, leaves)
        out.backward(g)
        copies = [out.detach().clone()] + [l.grad.clone() for l in leaves]
    side.synchronize()
    for got, k in zip(copies, ("out", "d_envmap", "d_albedos", "d_roughnesses")):
        only = None
        if k == "d_roughnesses":
            only = np.zeros((c["N"], 4), bool)
            only[:, 0] = o["thr"]
        _close(k, got, o[k], o[k + "_cnt"], o[k + "_abs"], name + " side stream " + k, only)


def test_radiance_loss_on_the_physical_case(built):
    """value and all four gradients (envmap, albedos, roughnesses, radiance_ratio) against the fp64 restatement"""
    from svgir_harness.losses import radiance_loss
    c, lo = rc.case("physical"), rc.loss_oracle()
    N, S = c["N"], c["S"]
    k = lo["kernel"]
    r = _renderer(c)
    env, alb, rough = (_t(c[x]).requires_grad_(True) for x in ("envmap", "albedos", "roughnesses"))
    ratio = _t(c["radiance_ratio"]).requires_grad_(True)
    radiances = _t(c["radiances"]).requires_grad_(True)
    loss = radiance_loss(r, _t(c["xyz"]), _t(c["camera_center"]), _t(c["geo_normal"]), _t(c["ray_d"]), _t(c["visibility"]), env, _t(c["normals"]),
                         alb, rough, radiances, ratio)
    assert loss.shape == () and loss.dtype == torch.float32
    # the mean of 3N absolute differences, each off by at most the kernel's bound and the rounding of the target and of the mean
    tol = rc.bound("out", S, k["out_abs"]).mean() + (3 * N + 4) * 2.0 ** -24 * (np.abs(k["out"]).mean() + np.abs(lo["target"]).mean())
    print("loss", float(loss), "fp64", lo["loss"], "tol", tol)
    assert abs(float(loss) - lo["loss"]) <= tol
    loss.backward()
    assert radiances.grad is None                      # (the cached radiances are detached, as in get_radiances)
    unsafe = lo["unsafe"]
    for leaf, name in ((env, "d_envmap"), (alb, "d_albedos"), (rough, "d_roughnesses")):
        only = np.zeros(k[name].shape, bool)
        only[unsafe] = True
        if name == "d_roughnesses":
            only[:, 0] |= k["thr"]
        _close(name, leaf.grad, k[name], k[name + "_cnt"], k[name + "_abs"], "radiance_loss " + name, only)
    tol = (3 * N + 4) * 2.0 ** -24 * lo["d_ratio_abs"] + 2 * lo["unsafe_ratio_abs"]
    assert abs(float(ratio.grad) - lo["d_ratio"]) <= tol, (float(ratio.grad), lo["d_ratio"], tol)
