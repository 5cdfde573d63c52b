"""The image-space kernels (csrc/epilogue.hip: svgss / rgss unpack, depth2normal; csrc/loss.hip: L1 + SSIM) on the edge cases of
tests/image_cases.py against the fp64 oracle (oracle/epilogue_oracle.py): the opacity clamp and its tie, the sRGB knee and clips,
non-finite inputs, one-pixel / one-row / one-column images, partial workgroups and tiles, flat and saturated SSIM windows, more tile
partials than the reduce kernel has threads -- and that every element of every output buffer is written.

Tolerances are the ones of tests/test_gpu_render_view.py; the SSIM cases get max(that, 4 x E32), E32 = what the reference's own fp32
arithmetic loses on the case (fp32 against fp64 restatement, computed here from the restatement, never from the kernel).  Threshold
pixels (image_cases.py) have zero upstream weight and are held to finiteness in the gradients; their values are compared."""
import numpy as np
import pytest
import torch

import image_cases as ic
from oracle import epilogue_oracle as eo

pytestmark = pytest.mark.gpu
_id = lambda r: r["id"]  # noqa: E731
SVGSS_RUNS = [r for r in ic.UNPACK_RUNS if r["mode"] != "rgss"]
RGSS_RUNS = [r for r in ic.UNPACK_RUNS if r["mode"] == "rgss"]


def _dev():
    return torch.device("cuda:0")


def _cmp(name, a, b, keep=None, tol=2e-4):
    """|a - b| <= tol (max |b| + |b|) on every compared entry (tests/test_gpu_render_view.py::_cmp with flip_frac = 0)."""
    a = a.detach().double().cpu().numpy()
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    if keep is not None:
        a, b = a[..., keep], b[..., keep]
    if b.size == 0:
        return
    assert np.isfinite(a).all(), f"{name}: non-finite entries on compared pixels"
    scale = max(np.abs(b).max(), 1e-30)
    bad = np.abs(a - b) > tol * (scale + np.abs(b))
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} entries off (max {np.abs(a - b).max():.3e}, scale {scale:.3e})"


def _values(name, got, ref):
    """The forward rule: the NaN and the Inf pattern equal the oracle's, every other entry within rtol 2e-5 / atol 2e-6."""
    got = got.detach().cpu().numpy()
    ref = np.broadcast_to(np.asarray(ref, dtype=np.float64), got.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{name}: NaN pattern differs ({np.isnan(got).sum()} vs {np.isnan(ref).sum()} in the oracle)"
    assert np.array_equal(np.isinf(got), np.isinf(ref)), f"{name}: Inf pattern differs ({np.isinf(got).sum()} vs {np.isinf(ref).sum()} in the oracle)"
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-6, err_msg=name)


def _svgss_tuple(dev, op, fe, vf):
    z = torch.zeros(1, device=dev)
    return (0, z, z, op, z, fe, vf, z, torch.zeros(1, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("run", SVGSS_RUNS, ids=_id)
def test_svgss_unpack_on_edge_inputs(built, run):
    from svgir_harness import render_view
    dev = _dev()
    d = ic.build_unpack(run)
    training = run["mode"] == "train"
    bg = ic.BACKGROUNDS[run["bg"]]
    names = [g[0] for g in ic.GROUPS[run["mode"]]]
    thr, bad = ic.threshold_pixels(ic.probe(d, run["mode"], bg)), ic.nonfinite_pixels(d)
    keep = ~(thr | bad)
    lv = {k: torch.from_numpy(d[k]).to(dev).requires_grad_(True) for k in ("opacity", "feature", "vfeature")}
    got = render_view.unpack(_svgss_tuple(dev, lv["opacity"], lv["feature"], lv["vfeature"]), torch.tensor(bg, device=dev), training)
    ref = eo.unpack_svgss(d["opacity"], d["feature"], d["vfeature"], bg, training)
    for k in names:
        _values(k, got[k], ref[k])
    # backward: random upstream weights, zero on threshold and non-finite pixels; the tie pixels are compared like every other
    w = ic.unpack_weights(run, {k: tuple(got[k].shape) for k in names}, keep)
    sum((got[k] * w[k].float().to(dev)).sum() for k in names).backward()
    ld = {k: torch.from_numpy(d[k]).double().requires_grad_(True) for k in lv}
    rt = eo.unpack_svgss_torch(ld["opacity"], ld["feature"], ld["vfeature"], torch.tensor(bg, dtype=torch.float64), training)
    sum((rt[k] * w[k]).sum() for k in names).backward()
    ordinary = keep & (d["opacity"][0] >= 0.25)        # a second pass without the 1e5-fold gradients of the small opacities in the scale
    for k in lv:
        _cmp("d_" + k, lv[k].grad, ld[k].grad.numpy(), keep)
        _cmp("d_" + k + " (opacity >= 0.25)", lv[k].grad, ld[k].grad.numpy(), ordinary)
        assert torch.isfinite(lv[k].grad.cpu()[..., torch.from_numpy(~bad)]).all(), f"d_{k}: non-finite on a finite pixel"


@pytest.mark.parametrize("run", RGSS_RUNS, ids=_id)
def test_rgss_unpack_on_edge_inputs(built, run):
    from svgir_harness import render_view
    dev = _dev()
    d = ic.build_unpack(run)
    keep = ~ic.nonfinite_pixels(d)
    z = torch.zeros(1, device=dev)
    nc = torch.from_numpy(d["num_contrib"]).to(dev)
    lv = {k: torch.from_numpy(d[k]).to(dev).requires_grad_(True) for k in ("opacity", "depth", "feature")}
    got = render_view.unpack_rgss((0, nc, z, z, lv["opacity"], lv["depth"], lv["feature"], z, z, z, torch.zeros(1, dtype=torch.int32, device=dev)))
    ref = eo.unpack_rgss(d["num_contrib"], d["opacity"], d["depth"], d["feature"])
    for k in ic.RGSS_KEYS:
        _values(k, got[k], ref[k])
    w = ic.unpack_weights(run, {k: tuple(got[k].shape) for k in ic.RGSS_KEYS}, keep)
    sum((got[k] * w[k].float().to(dev)).sum() for k in ic.RGSS_KEYS).backward()
    ld = {k: torch.from_numpy(d[k]).double().requires_grad_(True) for k in lv}
    rt = eo.unpack_rgss_torch(torch.from_numpy(d["num_contrib"]), ld["opacity"], ld["depth"], ld["feature"])
    sum((rt[k] * w[k]).sum() for k in ic.RGSS_KEYS).backward()
    ordinary = keep & (d["opacity"][0] >= 0.25)
    for k in lv:
        _cmp("d_" + k, lv[k].grad, ld[k].grad.numpy(), keep)
        _cmp("d_" + k + " (opacity >= 0.25)", lv[k].grad, ld[k].grad.numpy(), ordinary)


@pytest.mark.parametrize("run", ic.D2N_RUNS, ids=_id)
def test_depth2normal_on_edge_inputs(built, run):
    from svgir_harness import render_view
    dev = _dev()
    depth, mask, n_ref, g_ref, excl = ic.d2n_reference(run)
    dt = torch.from_numpy(depth).to(dev).requires_grad_(True)
    n = render_view.depth2normal(dt, torch.from_numpy(mask).to(dev), ic.FOVX, ic.FOVY, run["prcp"])
    got = n.detach().cpu().numpy()
    np.testing.assert_allclose(got, n_ref, rtol=0, atol=3e-5)
    (n * ic.d2n_upstream(run).float().to(dev)).sum().backward()
    gd = dt.grad.cpu().numpy()
    assert gd.shape == g_ref.shape and np.isfinite(gd).all()
    all_degenerate = min(run["H"], run["W"]) == 1 or run["mask"] == "zeros"
    if all_degenerate:
        assert not got.any()
        if run["H"] * run["W"] == 1 or run["mask"] == "zeros":
            assert not gd.any()
    elif run["grad"]:
        ok = ~excl[None]
        err = np.abs(gd - g_ref)[ok].max() / np.abs(g_ref[ok]).max()
        assert err <= 2e-4, err


def _ssim_tolerances(run):
    r64, r32 = ic.ssim_reference(run), ic.ssim_reference(run, torch.float32)
    if run["content"] == "nan":
        return r64, r32, 1e-5, 1e-6
    ev, _, lv, _ = ic.ssim_e32(r64, r32)
    return r64, r32, max(1e-5, 4 * ev), max(1e-6, 4 * lv)


def _grad_check(name, got, r64, r32, g_l1, g_ssim):
    """got against g_l1 d_l1 + g_ssim d_ssim of the fp64 restatement, within max(1e-4, 4 x E32 of this combination) x max |ref|; the
    NaN pattern (the `nan` case) equals the oracle's."""
    ref = g_l1 * r64["d_l1"] + g_ssim * r64["d_ssim"]
    r32c = g_l1 * r32["d_l1"] + g_ssim * r32["d_ssim"]
    got = got.detach().double().cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{name}: NaN pattern differs"
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0, 0.0
    m = max(np.abs(ref[fin]).max(), 1e-300)
    fin32 = fin & np.isfinite(r32c)
    e32 = np.abs(r32c - ref)[fin32].max() / m
    err = np.abs(got - ref)[fin].max() / m
    print(f"{name}: kernel {err:.2e}, E32 {e32:.2e}, ratio {err / max(e32, 1e-30):.2f}")
    assert err <= max(1e-4, 4 * e32), (name, err, e32)
    return err, e32


@pytest.mark.parametrize("run", ic.SSIM_RUNS, ids=_id)
def test_l1_ssim_on_edge_inputs(built, run):
    from svgir_harness import losses
    dev = _dev()
    img, gt = ic.build_ssim(run)
    r64, r32, tol_s, tol_l1 = _ssim_tolerances(run)
    a = img.to(dev).requires_grad_(True)
    b = gt.to(dev)
    l1, s = losses.l1_ssim(a, b)
    sv_, l1v_ = float(s.detach()), float(l1.detach())
    print(f"{run['id']}: ssim kernel {abs(sv_ - r64['ssim']):.2e} (fp32 reference {abs(r32['ssim'] - r64['ssim']):.2e}), "
          f"l1 kernel {abs(l1v_ - r64['l1']):.2e}")
    if run["content"] == "nan":
        assert np.isnan(sv_) and np.isnan(l1v_) and np.isnan(r64["ssim"]) and np.isnan(r64["l1"])
    else:
        assert abs(sv_ - r64["ssim"]) <= tol_s and abs(l1v_ - r64["l1"]) <= tol_l1
    for g_l1, g_ssim in ic.UPSTREAMS:
        g, = torch.autograd.grad(g_l1 * l1 + g_ssim * s, a, retain_graph=True)
        _grad_check(f"{run['id']} upstream ({g_l1}, {g_ssim})", g, r64, r32, g_l1, g_ssim)
        if run["content"] == "equal" and g_ssim == 0:
            assert not g.cpu().numpy()[(img == gt).numpy()].any()          # sign(0) = 0
    sv = losses.ssim(a.detach(), b)
    assert float(sv) == sv_ or (np.isnan(float(sv)) and np.isnan(sv_))
    s4 = losses.ssim(a.detach()[None], b[None])                          # the reference's ssim also takes [1,C,H,W]
    assert float(s4) == sv_ or (np.isnan(float(s4)) and np.isnan(sv_))
    for lam in ic.LAMBDAS:
        a2 = img.to(dev).requires_grad_(True)
        loss = losses.l1_ssim_loss(a2, b, lam)
        if run["content"] == "nan":
            assert np.isnan(float(loss))
        else:
            assert abs(float(loss) - ((1 - lam) * r64["l1"] + lam * (1 - r64["ssim"]))) <= (1 - lam) * tol_l1 + lam * tol_s
        (3.0 * loss).backward()
        _grad_check(f"{run['id']} lambda {lam}", a2.grad, r64, r32, 3.0 * (1 - lam), -3.0 * lam)


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_svgss_unpack_writes_every_element(built, mode):
    from gaussian_renderer import _native as N
    from svgir_harness import render_view
    dev = _dev()
    H, W = 37, 29
    run = next(r for r in SVGSS_RUNS if r["mode"] == mode and r["case"] == "opacity_ends" and (r["H"], r["W"]) == (H, W))
    d = ic.build_unpack(run)
    training = int(mode == "train")
    bg = torch.tensor(ic.BACKGROUNDS["colour"], device=dev)
    op, fe, vf = (torch.from_numpy(d[k]).to(dev).requires_grad_(True) for k in ("opacity", "feature", "vfeature"))
    planes = N.lib.svgir_unpack_planes(training)
    out = _nan((planes, H, W), dev)
    N.check(N.lib.svgir_unpack_forward(W, H, training, bg.data_ptr(), op.data_ptr(), fe.data_ptr(), vf.data_ptr(), out.data_ptr(),
                                       N.stream_ptr(dev)), "unpack_forward")
    assert not torch.isnan(out).any()
    res = render_view.unpack(_svgss_tuple(dev, op, fe, vf), bg, bool(training))
    names = render_view.TRAIN_PLANES if training else render_view.EVAL_PLANES
    assert torch.equal(torch.cat([res[k] for k in names]), out)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    d_op, d_fe, d_vf = _nan(op.shape, dev), _nan(fe.shape, dev), _nan(vf.shape, dev)
    N.check(N.lib.svgir_unpack_backward(W, H, training, bg.data_ptr(), op.data_ptr(), fe.data_ptr(), vf.data_ptr(), g.data_ptr(),
                                        d_op.data_ptr(), d_fe.data_ptr(), d_vf.data_ptr(), N.stream_ptr(dev)), "unpack_backward")
    (torch.cat([res[k] for k in names]) * g).sum().backward()
    for name, raw, wrapped in (("opacity", d_op, op.grad), ("feature", d_fe, fe.grad), ("vfeature", d_vf, vf.grad)):
        assert not torch.isnan(raw).any() and torch.equal(raw, wrapped), name


def test_rgss_unpack_writes_every_element(built):
    from gaussian_renderer import _native as N
    from svgir_harness import render_view
    dev = _dev()
    H, W = 37, 29
    run = next(r for r in RGSS_RUNS if r["case"] == "opacity_ends" and (r["H"], r["W"]) == (H, W))
    d = ic.build_unpack(run)
    nc = torch.from_numpy(d["num_contrib"]).to(dev)
    op, de, fe = (torch.from_numpy(d[k]).to(dev).requires_grad_(True) for k in ("opacity", "depth", "feature"))
    out = _nan((6, H, W), dev)
    N.check(N.lib.svgir_unpack_rgss_forward(W, H, nc.data_ptr(), op.data_ptr(), de.data_ptr(), fe.data_ptr(), out.data_ptr(), N.stream_ptr(dev)),
            "unpack_rgss")
    assert not torch.isnan(out).any()
    planes = render_view._UnpackRgss.apply(nc, op, de, fe)
    assert torch.equal(planes, out)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(8)).to(dev)
    d_op, d_de, d_fe = _nan(op.shape, dev), _nan(de.shape, dev), _nan(fe.shape, dev)
    N.check(N.lib.svgir_unpack_rgss_backward(W, H, nc.data_ptr(), op.data_ptr(), de.data_ptr(), fe.data_ptr(), g.data_ptr(), d_op.data_ptr(),
                                             d_de.data_ptr(), d_fe.data_ptr(), N.stream_ptr(dev)), "unpack_rgss_backward")
    (planes * g).sum().backward()
    for name, raw, wrapped in (("opacity", d_op, op.grad), ("depth", d_de, de.grad), ("feature", d_fe, fe.grad)):
        assert not torch.isnan(raw).any() and torch.equal(raw, wrapped), name


def test_depth2normal_writes_every_element(built):
    from gaussian_renderer import _native as N
    from svgir_harness import render_view
    dev = _dev()
    run = next(r for r in ic.D2N_RUNS if r["id"].startswith("37x29-plane1-disc"))
    depth, mask = ic.build_d2n(run)
    H, W = run["H"], run["W"]
    dt, mt = torch.from_numpy(depth).to(dev).requires_grad_(True), torch.from_numpy(mask).to(dev)
    out = _nan((3, H, W), dev)
    N.check(N.lib.svgir_depth2normal(W, H, dt.data_ptr(), mt.data_ptr(), ic.FOVX, ic.FOVY, run["prcp"][0], run["prcp"][1], out.data_ptr(),
                                     N.stream_ptr(dev)), "depth2normal")
    assert not torch.isnan(out).any()
    n = render_view.depth2normal(dt, mt, ic.FOVX, ic.FOVY, run["prcp"])
    assert torch.equal(n, out)
    g = ic.d2n_upstream(run).float().to(dev)
    gd = _nan((H, W), dev)
    N.check(N.lib.svgir_depth2normal_backward(W, H, dt.data_ptr(), mt.data_ptr(), g.data_ptr(), ic.FOVX, ic.FOVY, run["prcp"][0],
                                              run["prcp"][1], gd.data_ptr(), N.stream_ptr(dev)), "depth2normal_backward")
    assert not torch.isnan(gd).any()
    (n * g).sum().backward()
    # (the adjoint scatters with float atomics: the order of the additions is not fixed, the values agree to rounding)
    assert float((gd - dt.grad[0]).abs().max()) <= 1e-5 * float(gd.abs().max())


def test_l1_ssim_writes_every_element(built):
    from gaussian_renderer import _native as N
    from svgir_harness import losses
    dev = _dev()
    run = next(r for r in ic.SSIM_RUNS if r["id"] == "rand-3x17x33")
    img, gt = ic.build_ssim(run)
    C_, H, W = run["C"], run["H"], run["W"]
    a, b = img.to(dev).requires_grad_(True), gt.to(dev)
    nblk = N.lib.svgir_l1_ssim_partials(C_, H, W)
    assert nblk == ic.partials(run) == 18
    partial, dmaps, means = _nan((nblk, 2), dev), _nan((3, C_, H, W), dev), _nan((2,), dev)
    N.check(N.lib.svgir_l1_ssim_forward(a.data_ptr(), b.data_ptr(), C_, H, W, partial.data_ptr(), dmaps.data_ptr(), means.data_ptr(),
                                        N.stream_ptr(dev)), "l1_ssim forward")
    for name, t in (("partial", partial), ("dmaps", dmaps), ("means2", means)):
        assert not torch.isnan(t).any(), name
    l1, s = losses.l1_ssim(a, b)
    assert float(means[0]) == float(s) and float(means[1]) == float(l1)
    out = _nan((C_, H, W), dev)
    N.check(N.lib.svgir_l1_ssim_backward(a.data_ptr(), b.data_ptr(), dmaps.data_ptr(), C_, H, W, 1.0, 1.0, None, out.data_ptr(),
                                         N.stream_ptr(dev)), "l1_ssim backward")
    assert not torch.isnan(out).any()
    (l1 + s).backward()
    assert torch.equal(out, a.grad)


def test_l1_ssim_takes_non_contiguous_and_fp64_images(built):
    from svgir_harness import losses
    dev = _dev()
    run = next(r for r in ic.SSIM_RUNS if r["id"] == "rand-3x17x33")
    img, gt = ic.build_ssim(run)
    a = img.to(dev).requires_grad_(True)
    l1, s = losses.l1_ssim(a, gt.to(dev))
    (l1 + s).backward()
    wide = torch.zeros(3, 17, 66, device=dev)
    wide[:, :, ::2] = img.to(dev)
    wide.requires_grad_(True)
    strided = wide[:, :, ::2]
    assert not strided.is_contiguous()
    l1n, sn = losses.l1_ssim(strided, gt.to(dev))
    (l1n + sn).backward()
    assert float(l1n) == float(l1) and float(sn) == float(s)
    assert torch.equal(wide.grad[:, :, ::2], a.grad) and not wide.grad[:, :, 1::2].any()
    a64 = img.double().to(dev).requires_grad_(True)
    l1d, sd = losses.l1_ssim(a64, gt.double().to(dev))
    (l1d + sd).backward()
    assert float(l1d) == float(l1) and float(sd) == float(s)
    assert a64.grad.dtype == torch.float64 and torch.equal(a64.grad.float(), a.grad)


def test_l1_ssim_with_only_the_ground_truth_requiring_grad(built):
    """Only the rendered image is differentiable.  With gradients requested for the ground truth alone the forward keeps no derivative
    maps; the backward must say so (or hand back None) -- never pass a null pointer to the kernel."""
    from svgir_harness import losses
    dev = _dev()
    run = next(r for r in ic.SSIM_RUNS if r["id"] == "rand-3x16x16")
    img, gt = ic.build_ssim(run)
    g = gt.to(dev).requires_grad_(True)
    for fn in (lambda: sum(losses.l1_ssim(img.to(dev), g)), lambda: losses.l1_ssim_loss(img.to(dev), g, 0.2)):
        loss = fn()
        assert loss.requires_grad
        try:
            grads = torch.autograd.grad(loss, g, allow_unused=True)
        except RuntimeError as e:
            assert "ground truth" in str(e), str(e)
        else:
            assert grads[0] is None
    torch.cuda.synchronize()
    # the device is still healthy and the ordinary direction still works
    a = img.to(dev).requires_grad_(True)
    l1, s = losses.l1_ssim(a, g)
    (l1 + s).backward()
    assert a.grad is not None and torch.isfinite(a.grad).all() and g.grad is None
