"""The fused geometry losses (csrc/geom_loss.hip through svgir_harness.losses) on the cases of tests/geom_loss_cases.py against the fp64 oracle.

Losses: within 4 x E32 of the case (E32 = |the oracle in fp32 - the oracle in fp64|: what the reference's own arithmetic loses).  The bound
is held on the kernels' own sum / count, which `stats` returns in double; the fp32 scalar a loss function returns must then be exactly
float32(sum / count), the one rounding an fp32 result cannot avoid (half an fp32 spacing of the value is more than 4 x E32 in several
cases, 3.7e-9 against 1.4e-9 for the mask term at 150 x 161).  Counts: the target form equals the oracle's; the surface form lies in
[sure, sure + threshold].  The oracle is evaluated with the kernel's own count, for the surface value as for the gradients (1 / count is not
charged to threshold pixels).  Gradients are compared as the depth2normal edge test compares, max |difference| <= 2e-4 max |oracle| over the
compared pixels: dL_ddepth without the degenerate pixels, the threshold pixels and their 4-neighbours, dL_dnormal without the threshold
pixels (held to finiteness).  Every output buffer is NaN-filled first (tests/conftest.py sets SVGIR_POISON; the direct-ABI test fills its
own)."""
import numpy as np
import pytest
import torch

import geom_loss_cases as gc
import image_cases as ic

pytestmark = pytest.mark.gpu
_id = lambda r: r["id"] if isinstance(r, dict) else str(r)   # noqa: E731
GRAD_TOL = 2 * ic.REL                      # tests/test_gpu_image_edges.py::test_depth2normal_on_edge_inputs
UPSTREAM = {"surface": -1.7, "target": 0.0, "mask": 0.6, "entropy": 2.0}   # a negative one, and a zero for one term


def _dev():
    return torch.device("cuda:0")


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _close(name, scalar, stats, k, ref, e32):
    """The kernels' sum / count of term k (doubles) within 4 x E32 of the oracle; the returned fp32 scalar is its rounding, exactly."""
    got = float(stats[k, 0]) / float(stats[k, 1]) if stats[k, 1] else float("nan")
    tol = 4 * e32
    print(f"{name}: kernel {got!r}, oracle {ref!r}, |difference| {abs(got - ref):.3e}, E32 {e32:.3e}, bound {tol:.3e}")
    if np.isnan(ref):
        assert np.isnan(got) and np.isnan(scalar), name
    else:
        assert abs(got - ref) <= tol, (name, got, ref, e32)
        assert np.float32(scalar) == np.float32(got), (name, scalar, got)


def _grad(name, got, ref, keep=None):
    got = got.detach().double().cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all(), name       # complete writes: no NaN of the poison is left, anywhere
    if keep is not None:
        got, ref = got[..., keep], ref[..., keep]
    if ref.size == 0:
        return
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f"{name}: max |difference| {err:.3e}, max |oracle| {scale:.3e}, ratio {err / max(scale, 1e-300):.2e}")
    assert err <= GRAD_TOL * scale, (name, err, scale)


@pytest.fixture(scope="module")
def refs():
    """The oracle of every run, computed once: (fp64, fp32)."""
    cache = {}

    def get(run):
        if run["id"] not in cache:
            cache[run["id"]] = (gc.reference(run), gc.reference(run, torch.float32))
        return cache[run["id"]]
    return get


def _leaves(run, dev):
    d = gc.build(run)
    t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    for k in ("normal", "depth", "opacity"):
        t[k].requires_grad_(True)
    return d, t


@pytest.mark.parametrize("run", gc.RUNS, ids=_id)
def test_surface_mask_entropy_on_edge_inputs(built, refs, run):
    from svgir_harness import losses
    dev = _dev()
    r64, r32 = refs(run)
    d, t = _leaves(run, dev)
    H, W = run["H"], run["W"]
    res = losses.geometry_losses(normal=t["normal"], depth=t["depth"], mask=t["mask"], opacity=t["opacity"], fovx=ic.FOVX, fovy=ic.FOVY,
                                 prcppoint=run["prcp"], terms=("surface", "mask", "entropy"), with_stats=True)
    stats = res["stats"].cpu().numpy()
    count = int(stats[0, 1])
    thr = gc.threshold_pixels(r64["cos"])
    sure = int((r64["sel"] & ~thr).sum())
    print(f"{run['id']}: count {count}, sure {sure}, threshold {int(thr.sum())}, fp64 count {r64['count']}, fp32 count {r32['count']}")
    assert sure <= count <= sure + int(thr.sum())
    assert stats[2, 1] == H * W and stats[3, 1] == H * W and not stats[1].any()
    # (the oracle with the kernel's own count, for the value as for the gradients: a threshold pixel that falls on the other side adds
    # next to nothing to the sum, and the count bounds above hold the count)
    ref = gc.reference(run, count=count) if count != r64["count"] else r64
    if run["normal"] == "equal":
        assert np.isfinite(float(res["surface"].detach()))
    else:
        _close("surface", float(res["surface"].detach()), stats, 0, ref["surface"], abs(r32["surface"] - r64["surface"]))
    for k in ("mask", "entropy"):
        _close(k, float(res[k].detach()), stats, gc_terms().index(k), r64[k], abs(r32[k] - r64[k]))
    # backward: the upstream scalars are device tensors (a negative one among them)
    up = {k: torch.tensor(UPSTREAM[k], device=dev) for k in ("surface", "mask", "entropy")}
    sum(up[k] * res[k] for k in up).backward()
    g_n, g_d, g_o = t["normal"].grad, t["depth"].grad, t["opacity"].grad
    for g in (g_n, g_d, g_o):
        assert torch.isfinite(g).all()                                 # every element written, threshold pixels included
    if run["grad"]:
        _grad("dL_dnormal", g_n, UPSTREAM["surface"] * ref["d_normal"], ~thr)
        excl = ic.d2n_excluded(r64["d2n"], d["mask"])[1] | gc.grow(thr)
        if H * W == 1 or run["mask"] == "zeros":                       # nothing to differentiate: the depth gradient is exactly zero
            assert not g_d.cpu().numpy().any()
        elif min(H, W) > 1:                                            # (one row / column: every pixel is degenerate, finiteness only)
            _grad("dL_ddepth", g_d, UPSTREAM["surface"] * ref["d_depth"], ~excl)
    ref_o = UPSTREAM["mask"] * r64["d_opacity_mask"] + UPSTREAM["entropy"] * r64["d_opacity_entropy"]
    np.testing.assert_allclose(g_o.cpu().numpy(), ref_o, rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize("name", gc.TARGET_RUNS)
def test_target_form(built, name):
    from svgir_harness import losses
    dev = _dev()
    d = gc.build_target(name)
    r64, r32 = gc.target_reference(name), gc.target_reference(name, torch.float32)
    out = torch.from_numpy(d["output"]).to(dev).requires_grad_(True)
    gt = torch.from_numpy(d["gt"]).to(dev)
    w = None if d["weight"] is None else torch.from_numpy(d["weight"]).to(dev)
    res = losses.geometry_losses(normal=out, target=gt, weight=w, with_stats=True)
    assert set(res) == {"target", "stats"}
    assert int(res["stats"][1, 1]) == r64["count"] == r32["count"]     # the selection is a pure function of the inputs: bit for bit
    _close("target", float(res["target"].detach()), res["stats"].cpu().numpy(), 1, r64["loss"], abs(r32["loss"] - r64["loss"]))
    loss = losses.cos_loss(out, gt) if w is None else losses.cos_loss(out, gt, weight=w)
    assert torch.equal(loss.detach(), res["target"].detach()) or (name == "empty" and torch.isnan(loss))
    (torch.tensor(-2.5, device=dev) * loss).backward()
    g = out.grad.cpu().numpy()
    assert np.isfinite(g).all() and not g[:, ~r64["sel"]].any()        # unselected pixels (NaN ones included): exactly zero
    _grad("dL_doutput", out.grad, -2.5 * r64["d_output"])


def _raw_call(N, dev, t, terms, prcp, H, W):
    """One forward + backward through the C ABI with every output NaN-filled; returns the buffers."""
    nblk = N.lib.svgir_geometry_loss_partials(W, H)
    partial, stats, lo = _nan((nblk, 8), dev, torch.float64), _nan((4, 2), dev, torch.float64), _nan((4,), dev)
    ptr = lambda k: t[k].data_ptr() if k in t else None   # noqa: E731
    planes = [ptr(k) for k in ("normal", "depth", "mask", "opacity", "target", "weight")]
    N.check(N.lib.svgir_geometry_loss_forward(W, H, terms, *planes, ic.FOVX, ic.FOVY, prcp[0], prcp[1], partial.data_ptr(), stats.data_ptr(),
                                              lo.data_ptr(), N.stream_ptr(dev)), "forward")
    g = torch.tensor([UPSTREAM[k] for k in gc_terms()], device=dev)
    dn, dd, do = _nan((3, H, W), dev), _nan((1, H, W), dev), _nan((1, H, W), dev)
    N.check(N.lib.svgir_geometry_loss_backward(W, H, terms, *planes, ic.FOVX, ic.FOVY, prcp[0], prcp[1], stats.data_ptr(), g.data_ptr(),
                                               dn.data_ptr(), dd.data_ptr(), do.data_ptr(), N.stream_ptr(dev)), "backward")
    return partial, stats, lo, dn, dd, do


def gc_terms():
    from svgir_harness import losses
    return losses.GEOMETRY_TERMS


@pytest.mark.parametrize("run", gc.FUSED_RUNS, ids=_id)
def test_every_element_is_written_and_two_runs_give_the_same_bits(built, run):
    from gaussian_renderer import _native as N
    dev = _dev()
    d = gc.build(run)
    H, W = run["H"], run["W"]
    t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    rng = ic._rng("fused-" + run["id"])
    v = rng.standard_normal((3, H, W))
    t["target"] = torch.from_numpy((v / np.linalg.norm(v, axis=0, keepdims=True)).astype(np.float32)).to(dev)
    t["weight"] = t["mask"]
    for terms in (15, 1, 2, 12):
        a = _raw_call(N, dev, t, terms, run["prcp"], H, W)
        b = _raw_call(N, dev, t, terms, run["prcp"], H, W)
        for name, x, y in zip(("partial", "stats", "losses", "dL_dnormal", "dL_ddepth", "dL_dopacity"), a, b):
            assert not torch.isnan(x).any(), (terms, name)                         # (no case here has a NaN of its own)
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (terms, name)
        if not terms & 1:
            assert not a[4].any()                                                   # no surface term: the depth gradient is written as zeros


@pytest.mark.parametrize("run", gc.FUSED_RUNS, ids=_id)
def test_fused_launch_equals_the_four_single_calls(built, run):
    from svgir_harness import losses
    dev = _dev()
    H, W = run["H"], run["W"]
    rng = ic._rng("fused-" + run["id"])
    v = rng.standard_normal((3, H, W))
    target = torch.from_numpy((v / np.linalg.norm(v, axis=0, keepdims=True)).astype(np.float32)).to(dev)
    up = {k: torch.tensor(val, device=dev) for k, val in UPSTREAM.items()}

    _, t = _leaves(run, dev)
    cam = dict(fovx=ic.FOVX, fovy=ic.FOVY, prcppoint=run["prcp"])
    fused = losses.geometry_losses(normal=t["normal"], depth=t["depth"], mask=t["mask"], opacity=t["opacity"], target=target, weight=t["mask"], **cam)
    assert set(fused) == set(losses.GEOMETRY_TERMS)
    sum(up[k] * fused[k] for k in up).backward()

    _, s = _leaves(run, dev)
    single = dict(surface=losses.surface_loss(s["normal"], s["depth"], s["mask"], ic.FOVX, ic.FOVY, run["prcp"]),
                  target=losses.cos_loss(s["normal"], target, weight=s["mask"]),
                  mask=losses.mask_loss(s["opacity"], s["mask"]), entropy=losses.mask_entropy_loss(s["opacity"], s["mask"]))
    for k in losses.GEOMETRY_TERMS:
        assert torch.equal(fused[k].detach().view(torch.int32), single[k].detach().view(torch.int32)), k
    grads = {k: torch.autograd.grad(up[k] * single[k], [s[n] for n in names], allow_unused=True)
             for k, names in (("surface", ("normal", "depth")), ("target", ("normal",)), ("mask", ("opacity",)), ("entropy", ("opacity",)))}
    assert torch.equal(t["normal"].grad, grads["surface"][0] + grads["target"][0])
    assert torch.equal(t["depth"].grad, grads["surface"][1])
    assert torch.equal(t["opacity"].grad, grads["mask"][0] + grads["entropy"][0])
    assert not grads["target"][0].any()                                # the zero upstream, read on the device


def test_errors(built):
    from gaussian_renderer import _native as N
    from svgir_harness import losses
    dev = _dev()
    z3, z1 = torch.zeros(3, 4, 4, device=dev), torch.ones(1, 4, 4, device=dev)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        losses.cos_loss(z3.cpu(), z3.cpu())
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        losses.surface_loss(z3, z1.cpu(), z1, 0.9, 0.6)
    with pytest.raises(NotImplementedError):
        losses.cos_loss(z3, z3, thrsh=0.1)
    with pytest.raises(RuntimeError, match="differentiable"):
        losses.cos_loss(z3, z3.clone().requires_grad_(True))
    buf = torch.zeros(64, dtype=torch.float64, device=dev)
    args = lambda Wd, Ht, terms, normal, depth, mask, op: (Wd, Ht, terms, normal, depth, mask, op, None, None, 0.9, 0.6, 0.5, 0.5,   # noqa: E731
                                                           buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None)
    p3, p1 = z3.data_ptr(), z1.data_ptr()
    for a, msg in ((args(0, 4, 1, p3, p1, p1, None), "bad image size"), (args(4, -1, 1, p3, p1, p1, None), "bad image size"),
                   (args(4, 4, 0, p3, p1, p1, p1), "no term requested"), (args(4, 4, 1, p3, None, p1, None), "surface term needs"),
                   (args(4, 4, 2, p3, None, None, None), "target term needs"), (args(4, 4, 4, None, None, p1, None), "need the opacity")):
        assert N.lib.svgir_geometry_loss_forward(*a) == -1 and msg in N.last_error(), (msg, N.last_error())
    with pytest.raises(RuntimeError, match="geometry_loss"):
        N.check(N.lib.svgir_geometry_loss_backward(4, 4, 4, None, None, p1, p1, None, None, 0.9, 0.6, 0.5, 0.5, buf.data_ptr(), buf.data_ptr(), None, None,
                                                   None, None), "geometry_loss backward")
    assert "no gradient requested" in N.last_error()
