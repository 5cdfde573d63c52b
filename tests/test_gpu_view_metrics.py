"""The eval view's tail on the GPU (csrc/view_metrics.hip through svgir_harness/metrics.py) against the oracle of tests/metrics_cases.py.

Every output buffer is poisoned first (NaN rows, 0xA5 bytes).  Bounds, eps32 = 2^-23, E32 = what the reference's own fp32 arithmetic
loses on the case against the fp64 evaluation of the same fp32 operands (computed from the restatements, never from a kernel):
  mse_c   4 max(E32, eps32) mse_c.  The kernel forms d = a - b in fp32 from operands that have torch's bits, squares and sums in double:
          it carries no rounding of its own beyond the one of d, which the oracle shares; a CPU model of it deviates from fp64 by <= 3e-8
          relative on the rand cases (test_metrics_edge_inputs.py), against the floor 4 eps32 = 4.8e-7.  A term with an sRGB operand adds
          2 l1 delta + delta^2, delta = 4 E_SRGB: the first-order bound of perturbing one operand by delta (powf differs from torch's pow
          by ulps), mean |2 d delta + delta^2| <= 2 l1 delta + delta^2.
  psnr_c  (10 / ln 10) tol_mse / mse_c (the derivative of -10 log10); +inf expected exactly where the mse is exactly 0.
  means   the mean of their parts' bounds.
  ssim    max(1e-5, 4 E32), l1 max(1e-6, 4 E32): the rule of tests/test_gpu_image_edges.py::_ssim_tolerances.
NaN / inf patterns equal the oracle's.  The bytes of captures_u8 are compared bit for bit."""

import numpy as np
import pytest
import torch

import image_cases as ic
import metrics_cases as mc

pytestmark = pytest.mark.gpu
_id = lambda c: c["id"]  # noqa: E731


def _dev():
    return torch.device("cuda:0")


def _plane(o, dev):
    from svgir_harness import metrics
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    return metrics.plane(t(o["src"]), mask=t(o["mask"]), bg=o["bg"], fill=t(o["fill"]), scale=o["scale"], offset=o["offset"], srgb=o["srgb"])


def _term(case, dev):
    oa, ob = case["ops"] if "ops" in case else mc.build(case)
    return (_plane(oa, dev), _plane(ob, dev), case["ssim"])


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64).numpy()


def _poisoned_table(n, dev):
    return torch.full((3, n, mc.COLS), float("nan"), dtype=torch.float64, device=dev)


@pytest.mark.parametrize("case", mc.METRIC_CASES, ids=_id)
def test_view_metrics_on_edge_inputs(built, case):
    from svgir_harness import metrics
    dev = _dev()
    term = _term(case, dev)
    table = _poisoned_table(1, dev)
    table[0].fill_(7.0)
    out = metrics.view_metrics([term], out=table[1])
    assert out.data_ptr() == table[1].data_ptr()
    row = out[0].cpu().numpy()
    mc.check_row(case["id"], row, case)
    # rows of the caller's table that were not addressed keep what they held
    assert (table[0] == 7.0).all() and torch.isnan(table[2]).all()
    # a second run (into a fresh poisoned row) gives identical bits
    again = metrics.view_metrics([term])
    assert np.array_equal(_bits(again), _bits(table[1]))


COMPOSED = [c for c in mc.METRIC_CASES if c["comp"] != "none" and c["comp"] != "srgb"]


@pytest.mark.parametrize("case", COMPOSED, ids=_id)
def test_composed_operands_have_torchs_bits(built, case):
    """The operand formed on load against the same operand formed by torch and handed in as a plain plane: every difference is exactly 0
    (one fused multiply-add in the composition would show on the fractional masks and the fill plane).  sRGB is left out: its bits are
    powf's, not torch's."""
    from svgir_harness import metrics
    dev = _dev()
    n = 0
    for o in mc.build(case):
        if o["mask"] is None and o["scale"] == 1.0:
            continue
        o = dict(o, srgb=False)
        row = metrics.view_metrics([(_plane(o, dev), mc.compose(o).to(dev), False)])[0].cpu().numpy()
        assert (row[[0, 1, 2, 6, 9]] == 0).all() and np.isposinf(row[[3, 4, 5, 7]]).all(), (case["id"], row)
        n += 1
    assert n >= 1


@pytest.mark.parametrize("launch", mc.LAUNCHES, ids=lambda l: "+".join(l))
def test_multi_term_launch_equals_single_term_calls(built, launch):
    from svgir_harness import metrics
    dev = _dev()
    cases = [mc.BY_ID[i] for i in launch]
    terms = [_term(c, dev) for c in cases]
    multi = metrics.view_metrics(terms)
    assert tuple(multi.shape) == (len(launch), mc.COLS)
    for k, c in enumerate(cases):
        single = metrics.view_metrics([terms[k]])
        assert np.array_equal(_bits(single[0]), _bits(multi[k])), c["id"]
        mc.check_row(c["id"] + " (in a launch of %d)" % len(launch), multi[k].cpu().numpy(), c)
    # the same launch in another order: every term's row is its own
    rev = metrics.view_metrics(terms[::-1])
    assert np.array_equal(_bits(rev.flip(0)), _bits(multi))


@pytest.mark.parametrize("rid", ["rand-3x1x1", "rand-3x16x16", "rand-3x17x33", "rand-3x150x161", "flat-3x17x33", "sat-3x17x33", "nan-3x17x33"])
def test_plain_term_agrees_with_l1_ssim(built, rid):
    """The same planes through losses.l1_ssim (csrc/loss.hip) and through a plain term: within the sum of both kernels' bounds."""
    from svgir_harness import losses, metrics
    dev = _dev()
    run = next(r for r in ic.SSIM_RUNS if r["id"] == rid)
    img, gt = ic.build_ssim(run)
    case = dict(id="ssim-run-" + rid, ssim=True, ops=(mc.op(img.numpy()), mc.op(gt.numpy())))
    row = metrics.view_metrics([(img.to(dev), gt.to(dev))])[0].cpu().numpy()
    l1, s = losses.l1_ssim(img.to(dev), gt.to(dev))
    mc.check_row(case["id"], row, case)
    if run["content"] == "nan":
        assert np.isnan(row[8]) and np.isnan(row[9]) and np.isnan(float(s)) and np.isnan(float(l1))
        return
    tol = mc.tolerances(case)
    print(f"{rid}: ssim {row[8]!r} vs l1_ssim {float(s)!r}; l1 {row[9]!r} vs {float(l1)!r}")
    assert abs(row[8] - float(s)) <= 2 * tol[8] and abs(row[9] - float(l1)) <= 2 * tol[9]


def test_mse_and_psnr_drop_ins(built):
    from svgir_harness import metrics
    dev = _dev()
    for cid in ("rand-17x33", "equal-ch1-17x33", "nan-17x33"):
        case = mc.BY_ID[cid]
        oa, ob = mc.build(case)
        a, b = torch.from_numpy(oa["src"]).to(dev), torch.from_numpy(ob["src"]).to(dev)
        m, p = metrics.mse(a, b), metrics.psnr(a, b)
        for t in (m, p):
            assert tuple(t.shape) == (3, 1) and t.dtype == torch.float32 and t.device.type == "cuda"
        r64 = mc.reference(case)[0]
        tol = mc.tolerances(case)
        got = np.concatenate([m.double().cpu().numpy()[:, 0], p.double().cpu().numpy()[:, 0]])
        assert np.array_equal(np.isnan(got), np.isnan(r64[:6])) and np.array_equal(np.isinf(got), np.isinf(r64[:6]))
        fin = np.isfinite(r64[:6])
        # (the drop-ins round the double row to fp32, as the reference's results are)
        assert (np.abs(got - r64[:6])[fin] <= (tol[:6] + np.abs(r64[:6]) * 2.0 ** -24)[fin]).all()
        ref_m, ref_p = mc.torch_mse(a, b), mc.torch_psnr(a, b)
        assert tuple(ref_m.shape) == tuple(m.shape) and tuple(ref_p.shape) == tuple(p.shape)
        assert np.array_equal(metrics.psnr(a, b).cpu().numpy().view(np.int32), p.cpu().numpy().view(np.int32))
    with pytest.raises(ValueError, match=r"\[3,H,W\]"):
        metrics.psnr(torch.rand(1, 5, 7, device=dev), torch.rand(1, 5, 7, device=dev))
    with pytest.raises(ValueError, match=r"\[3,H,W\]"):
        metrics.mse(torch.rand(2, 3, 5, 7, device=dev), torch.rand(2, 3, 5, 7, device=dev))


@pytest.mark.parametrize("case", mc.BYTE_CASES, ids=_id)
def test_captures_u8_bit_for_bit(built, case):
    from gaussian_renderer import _native as N
    from svgir_harness import metrics
    dev = _dev()
    planes = [_plane(o, dev) for o in mc.build_bytes(case)]
    ref = mc.bytes_reference(case)
    got = metrics.captures_u8(planes)                       # (the wrapper fills the buffer with 0xA5 first under SVGIR_POISON)
    assert got.dtype == torch.uint8 and tuple(got.shape) == ref.shape
    assert np.array_equal(got.cpu().numpy(), ref), case["id"]
    # the raw entry point into a buffer that starts off a 4-byte boundary, guard bytes on both sides: every byte written, none beyond
    n, H, W = case["n"], case["H"], case["W"]
    total = n * H * W * 3
    arr = (N.PlaneOp * n)()
    for k, p in enumerate(planes):
        metrics._fill_op(arr[k], p)
    for shift in (1, 2, 3):
        buf = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=dev)
        off = 32 + shift
        N.check(N.lib.svgir_capture_u8(W, H, n, arr, buf.data_ptr() + off, N.stream_ptr(dev)), "capture_u8")
        host = buf.cpu().numpy()
        assert np.array_equal(host[off:off + total], ref.reshape(-1)), (case["id"], shift)
        assert (host[:off] == 0xA5).all() and (host[off + total:] == 0xA5).all(), (case["id"], shift)
    # a result that is all 0xA5 would pass for "written": the table's images never are
    assert (ref.reshape(n, -1) != 0xA5).any(axis=1).all()


@pytest.mark.parametrize("case", mc.ALBEDO_CASES, ids=_id)
def test_albedo_scale(built, case):
    from svgir_harness import metrics
    dev = _dev()
    r, g = mc.build_albedo(case)
    s64, s32, count, _, _ = mc.albedo_reference(case)
    scale, n = metrics.albedo_scale(torch.from_numpy(r).to(dev), torch.from_numpy(g).to(dev), gt_srgb=case["srgb"])
    assert scale.dtype == torch.float32 and tuple(scale.shape) == (3,) and n.dtype == torch.int32 and scale.device.type == "cuda"
    assert int(n) == count
    got = scale.double().cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(s64)), (got, s64)
    fin = np.isfinite(s64)
    if fin.any():
        with np.errstate(invalid="ignore"):
            e32 = np.where(fin, np.abs(s32 - s64) / np.abs(s64), 0.0)
            err = np.where(fin, np.abs(got - s64) / np.abs(s64), 0.0)
        print(f"{case['id']}: err {err.max():.2e}, E32 {e32.max():.2e}")
        assert (err <= 4 * np.maximum(e32, mc.EPS32)).all(), (got, s64)
    again, n2 = metrics.albedo_scale(torch.from_numpy(r).to(dev), torch.from_numpy(g).to(dev), gt_srgb=case["srgb"])
    assert np.array_equal(again.cpu().numpy().view(np.int32), scale.cpu().numpy().view(np.int32)) and int(n2) == count


@pytest.mark.parametrize("size", mc.FRAME_SIZES, ids=lambda s: "%dx%d" % s)
def test_relighting_frame_against_the_eager_restatement(built, size):
    from svgir_harness import metrics
    dev = _dev()
    H, W = size
    fr = mc.build_frame(H, W)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    pkg = {k: t(v) for k, v in fr["render_pkg"].items()}
    before = {k: v.clone() for k, v in pkg.items()}
    gt_image, gt_albedo, gt_normal, mask = (t(fr[k]) for k in ("gt_image", "gt_albedo", "gt_normal", "mask"))
    assert set(np.unique(fr["mask"])) == {0.0, 1.0}
    images, rows = metrics.relighting_frame(pkg, gt_image, gt_albedo, gt_normal, mask, mc.FRAME_BG, mc.FRAME_CAPTURES)
    assert all(torch.equal(pkg[k], before[k]) for k in pkg)
    saved = {}
    eager = mc.eager_relighting_frame(pkg, gt_image, gt_albedo, gt_normal, mask, mc.FRAME_BG, mc.FRAME_CAPTURES,
                                      lambda name, img: saved.__setitem__(name, mc.torch_quantise(img)), mc.srgb32, mc.torch_psnr, mc.torch_ssim,
                                      mc.torch_mse)
    assert set(images) == set(mc.FRAME_CAPTURES) | {"gt"} == set(saved)
    for name in saved:
        assert images[name].dtype == torch.uint8 and tuple(images[name].shape) == (H, W, 3)
        assert torch.equal(images[name], saved[name]), name
    assert tuple(rows.shape) == (3, mc.COLS) and rows.dtype == torch.float64
    got = rows.cpu().numpy()
    for k, (term, name) in enumerate(zip(mc.frame_terms(H, W), ("pbr", "albedo", "normal"))):
        mc.check_row(term["id"], got[k], term)
        tol = mc.tolerances(term)
        # the eager fp32 values on the same GPU: within twice the bounds (they carry E32 themselves)
        e = eager[name]
        assert abs(float(e["mse"]) - got[k][6]) <= 2 * tol[6] + got[k][6] * 2.0 ** -23, (name, float(e["mse"]), got[k][6])
        if name != "normal":
            assert abs(float(e["ssim"]) - got[k][8]) <= 2 * tol[8], (name, float(e["ssim"]), got[k][8])
            assert abs(float(e["psnr"]) - got[k][7]) <= 2 * tol[7] + abs(got[k][7]) * 2.0 ** -22, (name, float(e["psnr"]), got[k][7])
    assert np.isnan(got[2][8]) and np.isfinite(got[:2, 8]).all()


def test_invalid_arguments_raise_with_the_librarys_message(built):
    from svgir_harness import metrics
    dev = _dev()
    x = torch.rand(3, 5, 7, device=dev)
    m = torch.ones(1, 5, 7, device=dev)
    with pytest.raises(RuntimeError, match="terms per call"):
        metrics.view_metrics([(x, x)] * 5)
    with pytest.raises(RuntimeError, match="fill plane but no mask"):
        metrics.view_metrics([(metrics.plane(x, fill=x), x)])
    with pytest.raises(RuntimeError, match="fill plane but no mask"):
        metrics.captures_u8([metrics.plane(x, fill=x)])
    with pytest.raises(RuntimeError, match="operands per call"):
        metrics.captures_u8([x] * 17)
    with pytest.raises(RuntimeError, match="operand 1: srgb"):
        metrics.captures_u8([x, metrics.plane(x, mask=m, bg=1.0, srgb=True)])
    with pytest.raises(ValueError, match="one image size"):
        metrics.view_metrics([(x, torch.rand(3, 5, 8, device=dev))])
    with pytest.raises(RuntimeError, match="read on the host"):
        metrics.plane(x, mask=m, bg=torch.ones(3, device=dev))
    with pytest.raises(ValueError, match="float64"):
        metrics.view_metrics([(x, x)], out=torch.empty(1, 10, device=dev))
    torch.cuda.synchronize()
    # the device is healthy and the ordinary call still works
    assert np.isposinf(metrics.psnr(x, x).cpu().numpy()).all()
