"""GPU tests of the fused radiance-consistency loss (csrc/irradiance.hip: svgir_radiance_loss_forward / _backward) through
`svgir_harness.losses.fused_radiance_loss` and `pbgi.Renderer.radiance_consistency`, on every case of tests/radiance_loss_cases.py.

Selection: sample_indices equals the fp64 selection on every row that is no threshold row (best minus runner-up below 4 E_SEL without
being an exact tie); on a threshold row the chosen sample's fp64 score lies within 4 E_SEL of the best.  Everything else is compared with
the oracle evaluated AT THE KERNEL'S OWN INDICES.
Tolerances (radiance_loss_cases.bound): per element |gpu - fp64| <= (n * 2^-24 + 4 (E_TERM[kind] + E_ENV)) * sum |t| -- the bound of
tests/test_gpu_radiance.py with the measured relative deviation of one looked-up light value added to that of one brdf term; n = S for a
row of R and the number of contributions for a gradient element (d_env: `cnt` taps).  An element without a contribution must be exactly
zero -- every output is NaN-filled before the call (tests/conftest.py), so that also proves it was written.  The double sum is held to
the summed row bounds plus the two fp32 roundings of each |R - T|; the fp32 loss is the rounding of sum / 3N, bit for bit.  Gradient
elements fed by rows whose |R - T| lies within 10 bounds of zero are held to finiteness only (the sign of the L1 depends on rounding there),
as are elements of d_roughnesses that receive a threshold term of radiance_cases.  The forward is bitwise equal on a second call."""
import types

import numpy as np
import pytest
import torch

from tests import radiance_cases as rc
from tests import radiance_loss_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = sorted(lc.CASES)


def _t(a, dtype=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.copy() if dtype is None else a.astype(dtype)).to(DEV)


def _renderer(c):
    from pbgi.renderer import Renderer
    r = Renderer()
    r.hemi_index_buffers = _t(c["hit"]).reshape(c["N"], c["S"], 1)
    r.uv_buffers = _t(c["uvs"])
    return r


def _light(c, env):
    """the reference's two light classes, as far as shading._env_of reads them"""
    if c["softplus"]:
        return types.SimpleNamespace(env=env)
    return types.SimpleNamespace(envmap=env, transform=None if c["transform"] is None else _t(c["transform"]))


def _leaves(c, env_grad=True):
    env = _t(c["env"])[None] if c["softplus"] else _t(c["env"])          # DirectLightMap.env is [1,He,We,3]
    return [env.requires_grad_(env_grad), _t(c["albedos"]).requires_grad_(True), _t(c["roughnesses"]).requires_grad_(True),
            _t(c["radiance_ratio"]).requires_grad_(c.get("ratio_grad", True))]   # (ratio_grad False: the backward gets no d_radiance_ratio)


def _run(r, c, leaves, with_sum=True, conv=_t):
    from gaussian_renderer import shading
    env, alb, rough, ratio = leaves
    e, softplus, scale, transform = shading._env_of(_light(c, env))
    if not c["softplus"]:   # EnvLight's map is no parameter; its 32 x 64 resample stands in as the leaf, so that d_env with f = identity is checked
        leaves[0] = e = e.detach().requires_grad_(env.requires_grad)
    return r.radiance_consistency(conv(c["xyz"]), conv(c["camera_center"]), conv(c["geo_normal"]), conv(c["ray_d"]), conv(c["areas"]),
                                  conv(c["visibility"]), e, softplus, scale, transform, conv(c["normals"]), alb, rough, conv(c["radiances"]), ratio,
                                  with_sum=with_sum)


def _fused(r, c, leaves, **kw):
    from svgir_harness.losses import fused_radiance_loss
    env, alb, rough, ratio = leaves
    return fused_radiance_loss(r, _t(c["xyz"]), _t(c["camera_center"]), _t(c["geo_normal"]), _t(c["ray_d"]), _t(c["areas"])[..., None],
                               _t(c["visibility"])[..., None], _light(c, env), _t(c["normals"]), alb, rough, _t(c["radiances"]), ratio, **kw)


def _close(kind, got, want, cnt, mag, what, finite_only=None):
    got = got.detach().cpu().numpy().astype(np.float64).reshape(want.shape)
    assert np.isfinite(got).all(), f"{what}: {np.count_nonzero(~np.isfinite(got))} non-finite elements (an element the kernel did not write is NaN)"
    err, tol = np.abs(got - want), lc.bound(kind, cnt, mag)
    ratio = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
    print(f"{what}: worst error / bound = {ratio:.3g}")
    bad = err > tol
    if finite_only is not None:
        bad &= ~finite_only
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} elements off, first {np.argwhere(bad)[0]}: {got[bad][0]} vs {want[bad][0]} (bound {tol[bad][0]})"


def _oracle_for(name, idx):
    """the oracle at the kernel's indices, after the selection itself is checked"""
    c, o = lc.case(name), lc.oracle(name)
    idx = idx.cpu().numpy().astype(np.int64)
    thr = o["threshold"]
    assert idx.shape == o["sel"].shape and ((idx >= 0) & (idx < c["S"])).all()
    assert (idx[~thr] == o["sel"][~thr]).all(), (name, np.flatnonzero((idx != o["sel"]) & ~thr)[:5], idx[:8], o["sel"][:8])
    rows = np.arange(c["N"])
    assert (o["score"][rows, o["sel"]][thr] - o["score"][rows, idx][thr] <= 4 * lc.E_SEL).all()
    return o if (idx == o["sel"]).all() else lc.oracle_at(c, idx)


def _check_forward(name, c, o, loss, R, total):
    N, S = c["N"], c["S"]
    good = ~o["bad"]
    Rn = R.detach().cpu().numpy().astype(np.float64)
    assert not np.isfinite(Rn[~np.isfinite(o["out"])]).any()
    fin = np.isfinite(o["out"])
    _close("out", torch.from_numpy(np.where(fin, Rn, 0.0)), np.where(fin, o["out"], 0.0), float(S), np.where(fin, o["out_abs"], 0.0), name + " R")
    total, loss = float(total), float(loss)
    if o["bad"].any():
        assert np.isnan(loss) and not np.isfinite(total), (loss, total)
    else:
        print(f"{name}: sum {total} fp64 {o['loss_sum']} bound {o['loss_sum_bound']}")
        assert abs(total - o["loss_sum"]) <= o["loss_sum_bound"], (total, o["loss_sum"], o["loss_sum_bound"])
        assert np.float32(loss) == np.float32(total / (3 * N)), (loss, total / (3 * N))
    return good


def _check_gradients(name, c, o, leaves, env_grad=True):
    env, alb, rough, ratio = leaves
    k = o["kernel"]
    for leaf, kind in ((alb, "d_albedos"), (rough, "d_roughnesses")):
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape and leaf.grad.dtype == torch.float32
        only = np.zeros(k[kind].shape, bool)
        only[o["unsafe"]] = True
        if kind == "d_roughnesses":
            only[:, 0] |= k["thr"]
        _close(kind, leaf.grad, k[kind], k[kind + "_cnt"], k[kind + "_abs"], f"{name} {kind}", only)
    if env_grad:
        assert env.grad is not None and env.grad.shape == env.shape and env.grad.dtype == torch.float32
        _close("d_envmap", env.grad, o["d_env"], o["d_env_cnt"], o["d_env_abs"], f"{name} d_env", o["unsafe_env"])
    else:
        assert env.grad is None
    N = c["N"]
    tol = (3 * N + 4) * 2.0 ** -24 * o["d_ratio_abs"] + 2 * o["unsafe_ratio_abs"]
    if not c.get("ratio_grad", True):
        assert ratio.grad is None
        return
    assert ratio.grad is not None and ratio.grad.shape == ratio.shape
    assert abs(float(ratio.grad) - o["d_ratio"]) <= tol, (float(ratio.grad), o["d_ratio"], tol)


@pytest.mark.parametrize("name", NAMES)
def test_forward_and_backward(built, name):
    """selection, R, the double sum, the fp32 loss and all four gradients; the forward twice (same bits).  `non_finite` (whole rows) and
    `non_finite_channels` (single elements: a NaN and an inf texel in one channel, a target that is inf in one channel): the loss is NaN and
    every gradient is finite and equals the oracle without the non-finite elements."""
    c = lc.case(name)
    r = _renderer(c)
    leaves = _leaves(c)
    loss, idx, R, total = _run(r, c, leaves)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    assert idx.dtype == torch.int32 and idx.shape == (c["N"],) and R.shape == (c["N"], 3) and not idx.requires_grad and not R.requires_grad
    assert total.dtype == torch.float64 and not total.requires_grad
    o = _oracle_for(name, idx)
    _check_forward(name, c, o, loss, R, total)
    loss2, idx2, R2, total2 = _run(r, c, _leaves(c))
    assert torch.equal(idx, idx2) and torch.equal(R.view(torch.int32), R2.view(torch.int32))
    assert torch.equal(total.view(torch.int64), total2.view(torch.int64)) and torch.equal(loss.detach().view(torch.int32), loss2.detach().view(torch.int32))
    loss.backward()
    _check_gradients(name, c, o, leaves)


@pytest.mark.parametrize("name", ["map_lds_last", "map_lds_first_global"])
def test_both_accumulation_paths_around_the_threshold(built, name):
    """the largest map whose double table fits the LDS rule and the first that does not: both agree with the oracle (and the case table
    proves on the CPU which branch each takes)"""
    c = lc.case(name)
    He, We = c["env"].shape[:2]
    assert (He * We <= lc.LDS_TEXELS) == (name == "map_lds_last")
    r = _renderer(c)
    leaves = _leaves(c)
    loss, idx, R = _fused(r, c, leaves, with_rows=True)
    o = _oracle_for(name, idx)
    (3.0 * loss).backward()           # (an upstream scalar other than 1)
    env = leaves[0]
    _close("d_envmap", env.grad / 3.0, o["d_env"], o["d_env_cnt"], o["d_env_abs"], f"{name} d_env (upstream 3)", o["unsafe_env"])


def test_plain_env_strided_and_fp64_inputs_and_side_stream(built):
    """a light whose env does not require grad gets None; fp64 and strided inputs are taken as their contiguous fp32 copies; the calls
    run on a side stream without synchronisation"""
    name = "random_70x64"
    c = lc.case(name)
    r = _renderer(c)
    r.hemi_index_buffers = r.hemi_index_buffers.long()

    def wide(a):
        a = np.asarray(a)
        if a.ndim == 0:
            return _t(a).double()
        w = torch.zeros(a.shape + (2,), dtype=torch.float64, device=DEV)
        w[..., 1] = _t(a).double()
        return w[..., 1]
    leaves = _leaves(c, env_grad=False)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        loss, idx, R, total = _run(r, c, leaves, conv=wide)
        loss.backward()
        got = [t.detach().clone() for t in (loss, R, total)]
    side.synchronize()
    o = _oracle_for(name, idx)
    _check_forward(name, c, o, got[0], got[1], got[2])
    _check_gradients(name, c, o, leaves, env_grad=False)


def test_unset_buffers_mismatched_rows_cpu_tensors_and_no_rows(built):
    from pbgi.renderer import Renderer
    c = lc.case("random_5x65")
    N, S = c["N"], c["S"]
    with pytest.raises(RuntimeError, match="are not set"):
        _run(Renderer(), c, _leaves(c))
    r = _renderer(c)
    r.hemi_index_buffers = r.hemi_index_buffers[:N - 1]
    with pytest.raises(ValueError, match="do not hold N"):
        _run(r, c, _leaves(c))
    r = _renderer(c)
    with pytest.raises(ValueError, match="does not hold"):
        _run(r, dict(c, areas=c["areas"][:N - 1]), _leaves(c))
    with pytest.raises(RuntimeError, match="no CPU path"):
        _run(r, c, _leaves(c), conv=lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()))
    two = _leaves(c)
    two[0] = torch.cat([two[0].detach(), two[0].detach()])          # two maps: not silently the first
    with pytest.raises(ValueError, match="ONE"):
        _run(r, c, two)
    empty = Renderer()
    empty.hemi_index_buffers, empty.uv_buffers = torch.zeros(0, S, 1, dtype=torch.int32, device=DEV), torch.zeros(0, S, 2, device=DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    env = _t(c["env"])[None].requires_grad_(True)
    loss, idx, R = empty.radiance_consistency(z(0, 3), z(3), z(0, 3), z(0, S, 3), z(0, S), z(0, S), env, True, 2.0, None, z(0, 12), z(0, 12), z(0, 4),
                                              z(0, S, 3), torch.ones((), device=DEV))
    assert torch.isnan(loss) and idx.shape == (0,) and R.shape == (0, 3)     # torch's mean of an empty tensor
    loss.backward()
    assert env.grad is not None and float(env.grad.abs().sum()) == 0.0


def test_agrees_with_radiance_loss_on_the_physical_case(built):
    """fused_radiance_loss against the path it replaces: svgir_harness.losses.radiance_loss fed envmap = direct_light(dirs) * areas composed
    in torch (the reference's lines: shading_oracle.env_lookup on the device).  Both lie within their own bound of the fp64 value, so they
    agree within the sum of the two: the loss, d_albedos, d_roughnesses, d_env and d_ratio.  The composed path's d_env goes back through
    torch's fp32 lookup, whose tap weights are off by the grid coordinates' absolute fp32 error whatever the weight
    (radiance_loss_cases.composed_adjoint_slack, measured from the reference's fp32 lines): its bound carries that term on top."""
    from oracle import shading_oracle as so
    from svgir_harness.losses import radiance_loss
    name = "physical"
    c, o = lc.case(name), lc.oracle(name)
    N, S = c["N"], c["S"]
    k = o["kernel"]
    r = _renderer(c)
    fused = _leaves(c)
    loss = _fused(r, c, fused)
    loss.backward()
    env, alb, rough, ratio = old = _leaves(c)
    envmap = so.env_lookup(env.cpu(), _t(c["ray_d"]).cpu(), softplus=True, scale=2.0).to(DEV) * _t(c["areas"])[..., None]
    loss_old = radiance_loss(r, _t(c["xyz"]), _t(c["camera_center"]), _t(c["geo_normal"]), _t(c["ray_d"]), _t(c["visibility"]), envmap,
                             _t(c["normals"]), alb, rough, _t(c["radiances"]), ratio)
    loss_old.backward()
    tol = (o["loss_sum_bound"] + (3 * N + 4) * 2.0 ** -24 * (np.abs(o["out"]).sum() + np.abs(o["target"]).sum())) / (3 * N)
    print("fused", float(loss), "composed", float(loss_old), "fp64", o["loss"], "tol", 2 * tol)
    assert abs(float(loss) - o["loss"]) <= tol and abs(float(loss) - float(loss_old)) <= 2 * tol
    slack, e_w = lc.composed_adjoint_slack(c, k["d_envmap_abs"] * c["areas"].astype(np.float64)[..., None])
    print("E_W", e_w, "largest slack / bound", float((slack / np.maximum(lc.bound("d_envmap", o["d_env_cnt"], o["d_env_abs"]), 1e-300)).max()))
    for a, b, kind, cnt, mag, only in ((fused[1], alb, "d_albedos", k["d_albedos_cnt"], k["d_albedos_abs"], None),
                                       (fused[2], rough, "d_roughnesses", k["d_roughnesses_cnt"], k["d_roughnesses_abs"], k["thr"]),
                                       (fused[0], env, "d_envmap", o["d_env_cnt"], o["d_env_abs"], None)):
        diff = (a.grad - b.grad).detach().cpu().numpy().astype(np.float64).reshape(mag.shape)
        bad = np.abs(diff) > 2 * lc.bound(kind, cnt, mag) + (slack if kind == "d_envmap" else 0.0)
        skip = o["unsafe_env"] if kind == "d_envmap" else np.repeat(o["unsafe"][:, None], mag.shape[1], 1)
        if only is not None:
            skip = skip.copy()
            skip[:, 0] |= only
        assert np.isfinite(diff).all() and not (bad & ~skip).any(), (kind, int((bad & ~skip).sum()))
    tol = 2 * ((3 * N + 4) * 2.0 ** -24 * o["d_ratio_abs"] + 2 * o["unsafe_ratio_abs"])
    assert abs(float(fused[3].grad) - float(ratio.grad)) <= tol
