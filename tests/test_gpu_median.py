"""The exact column median and its two consumers on the GPU (csrc/select.hip through svgir_harness/metrics.py and losses.py) against the
oracles of tests/median_cases.py.  Every output and the scratch are poisoned first (NaN / -7 by the binding layer, 0xA5 bytes on the raw
second run), and the second run must give the same bits.

Bounds, eps32 = 2^-23, E32 = what the reference's own fp32 lines lose on the case against their fp64 evaluation (computed from the
restatements on the CPU, never from a kernel):
  column_median                    values bit for bit (NaN where the oracle has NaN), indices and both counts exact.
  albedo_scale_median, no srgb     bit for bit: the ratio is one correctly rounded fp32 division and a clamp, the selection is exact.
  albedo_scale_median, srgb        4 max(E32, eps32) relative to the fp64 lower median.  Order statistics are monotone: keys within t
                                   (relative) of their fp64 values put the median within t of the fp64 median, and the clamp keeps that.
  surface_center_loss              loss: 4 max(E32, eps32) relative to the fp64 oracle; the kernel's own double sum (stats[0]) against the
                                   double sum of the same fp32 values |x - c|: 3 P 2^-52 relative (the order of a double summation).
                                   dL_dxyz, rows that do not hold the median value: 4 eps32 |g L| / (3 P) per element, signs exact.
                                   Rows that hold it, summed per column (torch and the kernel may pick different rows): the sum is ONE
                                   fp32 element of magnitude |g L| |n_greater - n_less| / (3 P), so 4 eps32 |g L| max(1, |n_greater -
                                   n_less|) / (3 P).  A tie-free case is the same check with one holding row."""
import numpy as np
import pytest
import torch

import median_cases as mc

pytestmark = pytest.mark.gpu
_id = lambda c: c["id"]  # noqa: E731


def _dev():
    return torch.device("cuda:0")


def _to(dev):
    return lambda a: torch.from_numpy(a).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _same_float_bits(got, want):
    """Bit for bit, except that a NaN need only be a NaN."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _raw_column_median(view):
    """svgir_column_median straight through the C ABI, scratch and outputs filled with 0xA5 bytes first."""
    from gaussian_renderer import _native as N
    dev = view.device
    n, Cn = int(view.shape[0]), int(view.shape[1])
    scratch = torch.full((max(N.lib.svgir_column_median_scratch_bytes(n, Cn), 4),), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((4, Cn), -1515870811, dtype=torch.int32, device=dev)   # 0xA5A5A5A5
    N.check(N.lib.svgir_column_median(N.ptr(view), n, Cn, view.stride(0), view.stride(1), scratch.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                      out[2].data_ptr(), out[3].data_ptr(), N.stream_ptr(dev)), "column_median")
    return out.cpu().numpy()


@pytest.mark.parametrize("case", mc.COLUMN_CASES, ids=_id)
def test_column_median(built, case):
    from svgir_harness import metrics
    dev = _dev()
    view = mc.column_view(case, _to(dev))
    val, idx, less, greater = metrics.column_median(view, with_counts=True)
    rv, ri, rl, rg = mc.column_reference(case)
    got = val.cpu().numpy()
    print(case["id"], "values", got, rv, "indices", idx.cpu().numpy(), ri, "less", less.cpu().numpy(), rl, "greater", greater.cpu().numpy(), rg)
    assert idx.dtype == torch.int64 and val.dtype == torch.float32 and val.device == view.device
    assert _same_float_bits(got, rv)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(less.cpu().numpy(), rl) and np.array_equal(greater.cpu().numpy(), rg)
    again = _raw_column_median(view)   # other poison, same bits
    assert np.array_equal(again[0], _bits(val)) and np.array_equal(again[1], ri) and np.array_equal(again[2], rl) and np.array_equal(again[3], rg)
    v2, i2 = metrics.column_median(view)   # the drop-in form
    assert np.array_equal(_bits(v2), _bits(val)) and torch.equal(i2, idx)


@pytest.mark.parametrize("case", mc.ALBEDO_CASES, ids=_id)
def test_albedo_scale_median(built, case):
    from svgir_harness import metrics
    from gaussian_renderer import _native as N
    dev = _dev()
    r, g = (torch.from_numpy(a).to(dev) for a in mc.build_albedo(case))
    scale, count = metrics.albedo_scale_median(r, g, lo=mc.LO, hi=mc.HI, render_srgb=case["srgb"])
    ref = mc.albedo_reference(case)
    got = scale.cpu().numpy()
    tol = 4 * max(ref["e32"], mc.EPS32)
    with np.errstate(invalid="ignore"):
        print(case["id"], "count", int(count), ref["count"], "scale", got, "fp32 lines", ref["scale32"], "fp64", ref["scale64"],
              "rel", np.abs(got - ref["scale64"]) / np.abs(ref["scale64"]), "tol", tol)
    assert scale.dtype == torch.float32 and count.dtype == torch.int32 and int(count) == ref["count"]
    assert np.array_equal(np.isnan(got), np.isnan(ref["scale64"]))   # NaN exactly in the 0 / 0 channel (every channel when nothing is selected)
    if not case["srgb"]:
        assert _same_float_bits(got, ref["scale32"])
    ok = ~np.isnan(ref["scale64"])
    assert (np.abs(got[ok] - ref["scale64"][ok]) <= tol * np.abs(ref["scale64"][ok])).all()
    # a second run, straight through the C ABI over 0xA5 scratch: the same bits
    H, W = case["H"], case["W"]
    scratch = torch.full((N.lib.svgir_albedo_scale_median_scratch_bytes(W, H),), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((4,), -1515870811, dtype=torch.int32, device=dev)
    N.check(N.lib.svgir_albedo_scale_median(W, H, r.data_ptr(), g.data_ptr(), int(case["srgb"]), mc.LO, mc.HI, scratch.data_ptr(), out[:3].data_ptr(),
                                            out[3:].data_ptr(), N.stream_ptr(dev)), "albedo_scale_median")
    out = out.cpu().numpy()
    assert np.array_equal(out[:3], _bits(scale)) and out[3] == ref["count"]


def test_albedo_scale_median_takes_other_bounds(built):
    """lo, hi are arguments: the variant's bounds (1e-6, 1) give the lower median of the same ratios clamped there."""
    from svgir_harness import metrics
    dev = _dev()
    case = next(c for c in mc.ALBEDO_CASES if c["id"] == "partial-17x33")
    r, g = (torch.from_numpy(a) for a in mc.build_albedo(case))
    q, m = mc.albedo_lines(r, g, False, mc.srgb_to_rgb, lo=1e-6, hi=1.0)
    scale, count = metrics.albedo_scale_median(r.to(dev), g.to(dev), lo=1e-6, hi=1.0, render_srgb=False)
    assert int(count) == int(m.sum()) and _same_float_bits(scale.cpu().numpy(), mc.column_oracle(q.numpy())[0])


@pytest.mark.parametrize("case", mc.LOSS_CASES, ids=_id)
def test_surface_center_loss(built, case):
    from svgir_harness import losses
    dev = _dev()
    x_np = mc.build_loss(case)
    P = x_np.shape[0]
    ref = mc.loss_reference(case)

    def run():
        x = torch.from_numpy(x_np.copy()).to(dev).requires_grad_(True)
        loss, stats = losses.surface_center_loss(x, with_stats=True)
        (loss * mc.UPSTREAM).backward()
        return loss.detach(), stats, x.grad

    loss, stats, grad = run()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and tuple(grad.shape) == (P, 3)
    L, st, gr = float(loss), stats.cpu().numpy(), grad.cpu().numpy().astype(np.float64)
    tol_loss = 4 * max(ref["e32"], mc.EPS32)
    print(case["id"], "loss", L, "fp64", ref["loss64"], "tol", tol_loss, "sum", st[0], ref["sum32"], "stats", st[1:])
    assert st[1] == 3 * P
    assert np.array_equal(st[2:].reshape(3, 3), np.stack([ref["index"], ref["less"], ref["greater"]], axis=1))
    if np.isnan(ref["loss64"]):   # a NaN coordinate: the loss and every gradient element
        assert np.isnan(L) and np.isnan(st[0]) and np.isnan(gr).all()
    else:
        assert abs(st[0] - ref["sum32"]) <= 3 * P * 2.0 ** -52 * ref["sum32"]
        assert abs(L - ref["loss64"]) <= tol_loss * ref["loss64"]
        if case["shape"] == "equal" or P == 1:
            assert L == 1.0 and st[0] == 0.0
        assert not np.isnan(gr).any()                                   # written completely (the buffer was NaN)
        held, unit = ref["held"], 4 * mc.EPS32 * abs(mc.UPSTREAM * ref["loss64"]) / (3 * P)
        free = ~held
        err = np.abs(gr - ref["grad"])
        print("  grad: max err off the median rows", err[free].max(initial=0.0), "bound", unit)
        assert (err[free] <= unit).all() and np.array_equal(np.sign(gr[free]), np.sign(ref["grad"][free]))
        sums, want = mc.tie_sum(gr, held), mc.tie_sum(ref["grad"], held)
        bound = unit * np.maximum(1, np.abs(ref["greater"] - ref["less"]))
        print("  grad: sums over the median rows", sums, want, "bound", bound)
        assert (np.abs(sums - want) <= bound).all() and np.array_equal(np.sign(sums), np.sign(want))
        if not case["ties"]:
            assert (err <= unit).all() and np.array_equal(np.sign(gr), np.sign(ref["grad"]))
    loss2, stats2, grad2 = run()   # two runs give the same bits
    assert np.array_equal(_bits(loss2.reshape(1)), _bits(loss.reshape(1))) and np.array_equal(_bits(grad2), _bits(grad))
    assert np.array_equal(stats2.cpu().numpy().view(np.int64), st.view(np.int64))


def test_surface_center_loss_of_no_points(built):
    """P == 0: the loss is NaN, nothing else is written, and the backward returns an empty gradient."""
    from gaussian_renderer import _native as N
    from svgir_harness import losses, metrics
    dev = _dev()
    x = torch.zeros((0, 3), device=dev, requires_grad=True)
    loss, stats = losses.surface_center_loss(x, with_stats=True)
    loss.backward()
    assert torch.isnan(loss) and tuple(x.grad.shape) == (0, 3)
    assert (torch.isnan(stats).all() if N.POISON else True)             # the poison stands: stats were not written
    v, i, less, greater = metrics.column_median(torch.zeros((0, 2), device=dev), with_counts=True)
    assert torch.isnan(v).all() and i.tolist() == [-1, -1] and less.tolist() == [0, 0] and greater.tolist() == [0, 0]


def test_median_agrees_with_torch_on_the_device(built):
    """The drop-in claim on the device itself: torch.median's values on a planar view, and an index that points at a row holding them."""
    from svgir_harness import metrics
    dev = _dev()
    case = next(c for c in mc.COLUMN_CASES if c["id"] == f"generic-{2 * mc.T + 1}-planar")
    view = mc.column_view(case, _to(dev))
    val, idx = metrics.column_median(view)
    tv, _ = torch.median(view, dim=0)
    assert torch.equal(val, tv) and torch.equal(view[idx, torch.arange(3, device=dev)], val)
