"""CPU checks of the eval view's tail: the oracle of tests/metrics_cases.py is pinned by the reference's own results
(tests/golden/view_metrics.npz, scripts/make_golden_metrics.py), the table is proven to hold what it claims, E32 / E_SRGB are measured
per case (DESIGN.md section 5 quotes them), the byte oracle equals torch's own mul / add_ / clamp_ / to(uint8) bit for bit, and the
header's new symbols are exported."""
import os
import re

import numpy as np
import pytest
import torch

import metrics_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "view_metrics.npz")
_id = lambda c: c["id"]  # noqa: E731


def _same(a, b, rtol, atol=0.0):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), (a, b)
    fin = np.isfinite(b)
    np.testing.assert_allclose(a[fin], b[fin], rtol=rtol, atol=atol)


@pytest.mark.parametrize("cid", mc.GOLDEN_CASES)
def test_metrics_oracle_is_the_references(cid):
    """mse / psnr: the same expression, equal to the last bits; ssim: the reference's window is the fp32 outer product in both
    precisions, the fp64 oracle's the double one (a 1e-7 matter)."""
    g = np.load(GOLD)
    r64, r32, _ = mc.reference(mc.BY_ID[cid])
    _same(r32[0:3], g[cid + ".mse32"], 1e-7)
    _same(r32[3:6], g[cid + ".psnr32"], 0, 1e-5)
    _same(r64[0:3], g[cid + ".mse64"], 1e-7)       # (the fp64 sRGB knee is the fp32 constant in the oracle, the double one in the reference)
    _same(r64[3:6], g[cid + ".psnr64"], 0, 1e-6)
    _same(r32[8], g[cid + ".ssim32"], 0, 5e-7)
    _same(r64[8], g[cid + ".ssim64"], 0, 5e-7)
    assert abs(r32[6] - float(g[cid + ".mse32"].mean())) <= 1e-7 * abs(r32[6]) or np.isnan(r32[6])


def test_srgb_oracles_are_the_references():
    g = np.load(GOLD)
    lad = np.resize(mc.srgb_ladder(), 48).reshape(3, 4, 4)
    assert np.array_equal(mc.srgb32(torch.from_numpy(lad)).numpy(), g["srgb_ladder_32"])
    np.testing.assert_allclose(mc.eo.rgb_to_srgb(lad), g["srgb_ladder_64"], rtol=0, atol=1e-7)


@pytest.mark.parametrize("cid", mc.GOLDEN_ALBEDO)
def test_albedo_oracle_is_the_references(cid):
    g = np.load(GOLD)
    case = next(c for c in mc.ALBEDO_CASES if c["id"] == cid)
    s64, s32, count, _, _ = mc.albedo_reference(case)
    assert count == int(g[f"albedo.{cid}.count32"]) == int(g[f"albedo.{cid}.count64"])
    _same(s32, g[f"albedo.{cid}.scale32"], 1e-7)
    _same(s64, g[f"albedo.{cid}.scale64"], 1e-7)


def test_table_ids_are_unique_and_launches_share_a_size():
    assert len(mc.BY_ID) == len(mc.METRIC_CASES)
    assert {(c["H"], c["W"]) for c in mc.METRIC_CASES} == set(mc.SIZES)
    for launch in mc.LAUNCHES:
        assert 1 < len(launch) <= 4 and len({(mc.BY_ID[i]["H"], mc.BY_ID[i]["W"]) for i in launch}) == 1
    assert sorted(len(l) for l in mc.LAUNCHES)[::2] == [3, 4]
    assert any(mc.BY_ID[i]["ssim"] for i in mc.LAUNCHES[0]) and not all(mc.BY_ID[i]["ssim"] for i in mc.LAUNCHES[0])


@pytest.mark.parametrize("case", mc.METRIC_CASES, ids=_id)
def test_metric_cases_hold_what_they_claim(case):
    oa, ob = mc.build(case)
    a, b = mc.compose(oa).numpy(), mc.compose(ob).numpy()
    r64, r32, es = mc.reference(case)
    H, W = case["H"], case["W"]
    assert a.shape == b.shape == (3, H, W) and a.dtype == b.dtype == np.float32
    content, comp = case["content"], case["comp"]
    if content == "equal_all":
        assert (r64[0:3] == 0).all() and np.isposinf(r64[3:6]).all() and np.isposinf(r64[7]) and r64[9] == 0
        assert r64[8] == 1.0 or not case["ssim"]
    elif content == "equal_ch1":
        assert r64[1] == 0 and np.isposinf(r64[4]) and r64[0] > 0 and r64[2] > 0 and np.isposinf(r64[7]) and np.isfinite(r64[6])
    elif content == "nan":
        assert np.isnan(a).sum() == 1 and np.isnan(a[2]).sum() == 1
        assert np.isnan(r64[[2, 5, 6, 7, 9]]).all() and np.isfinite(r64[[0, 1, 3, 4]]).all()
        assert np.isnan(r64[8])
    elif content == "inf":
        assert np.isposinf(a).sum() == 1 and np.isposinf(r64[0]) and np.isneginf(r64[3]) and np.isfinite(r64[[1, 2, 4, 5]]).all()
        assert np.isposinf(r64[9])
    else:
        assert np.isfinite(r64[[0, 1, 2, 3, 4, 5, 6, 7, 9]]).all() and (r64[0:3] > 0).all()
    assert np.isnan(r64[8]) == (not case["ssim"] or content in ("nan", "inf"))
    if content == "flat":
        assert len(np.unique(b)) == 1 and len(np.unique(a)) == (2 if W > 1 else 1)
    if content == "sat":
        assert set(np.unique(b)) == {0.0, 1.0}
    if comp.startswith("binary") or comp == "affine":
        assert set(np.unique(oa["mask"])) == {0.0, 1.0}
    if comp.startswith("frac"):
        m = oa["mask"]
        assert ((m > 0) & (m < 1)).any() or H * W == 1
    if comp.startswith("edge16"):
        m = oa["mask"][0]
        assert W > 16 and (m[:, :16] == 1).all() and (m[:, 16:] == 0).all()
    if comp == "fill":
        assert oa["fill"] is not None and oa["fill"].shape == (3, H, W)
    if comp == "affine":
        assert oa["scale"] == 0.5 and oa["offset"] == 0.5 and oa["src"].min() < -0.5
    if content == "knee":
        assert ob["srgb"] and es > 0
        pre = mc.compose(ob, with_srgb=False).numpy()
        if comp == "srgb" and H * W >= 35:
            k = mc.KNEE
            for v in (k, np.nextafter(k, np.float32(0)), np.nextafter(k, np.float32(1))):
                assert (pre == v).any()
            assert (pre < 0).any() and (pre > 1).any()
        assert es < 2.5e-7          # a few ulps of 1: delta = 4 E_SRGB stays a rounding-size perturbation
    else:
        assert es == 0
    e = mc.e32(case)
    tol = mc.tolerances(case)
    print(f"{case['id']}: E32 mse {e[0:3].max():.2e} (rel) psnr {e[3:6].max():.2e} ssim {e[8]:.2e} l1 {e[9]:.2e}  E_SRGB {es:.2e}  "
          f"bounds mse {tol[0:3].max():.2e} psnr {tol[3:6].max():.2e} ssim {tol[8]:.2e} l1 {tol[9]:.2e}")
    # the reference's own fp32 arithmetic sits inside the bounds the kernels are held to (its psnr columns apart: an fp32 number near 50
    # is rounded to 4e-6, which the double rows of the kernels are not)
    mc.check_row(case["id"] + " (fp32 reference)", r32, case, cols=(0, 1, 2, 6, 8, 9))


def test_a_model_of_the_kernel_sits_near_the_floor():
    """fp32 difference, double square and double sum (what the kernel does) against the fp64 row, on the rand cases: far below the
    4 eps32 floor of the mse bound."""
    worst = 0.0
    for case in mc.METRIC_CASES:
        if case["content"] != "rand" or case["comp"] != "none":
            continue
        oa, ob = mc.build(case)
        d = (mc.compose(oa) - mc.compose(ob)).double()
        model = (d * d).reshape(3, -1).mean(1).numpy()
        worst = max(worst, float(np.abs(model / mc.reference(case)[0][0:3] - 1).max()))
    print(f"kernel model vs fp64: {worst:.2e} relative (floor {4 * mc.EPS32:.2e})")
    assert worst <= 4 * mc.EPS32 / 4


@pytest.mark.parametrize("case", mc.BYTE_CASES, ids=_id)
def test_byte_oracle_is_torchs_quantisation(case):
    ops = mc.build_bytes(case)
    assert len(ops) == case["n"]
    ref = mc.bytes_reference(case)
    assert ref.shape == (case["n"], case["H"], case["W"], 3) and ref.dtype == np.uint8
    for k, o in enumerate(ops):
        x = mc.compose(o)
        t = x.clone().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()   # torchvision.utils.save_image's line
        ok = ~np.isnan(x.permute(1, 2, 0).numpy())            # (the cast of NaN is undefined in torch: the oracle says 0)
        assert np.array_equal(t[ok], ref[k][ok]), (case["id"], k)
        assert (ref[k][~ok] == 0).all()


def test_byte_ladder_holds_the_flip_points():
    lad = mc.byte_ladder()
    q = mc.quantise(np.resize(lad, 3 * 18 * 20).reshape(3, 18, 20)).transpose(2, 0, 1).reshape(-1)[: lad.size]
    k = np.arange(256)
    assert np.array_equal(q[:256], k)                                        # k / 255 -> k
    lo, hi = q[512:768], q[768:1024]                                         # the fp32 neighbours of (k + 0.5) / 255
    assert (hi >= lo).all() and ((hi - lo) >= 0).all() and (lo == k).sum() > 200 and (hi == np.minimum(k + 1, 255)).sum() > 200
    tail = lad[1024:]
    assert np.isnan(tail).any() and np.isposinf(tail).any() and np.isneginf(tail).any() and (tail < 0).any() and (tail > 1).any()
    qt = q[1024:]
    assert qt[np.isnan(tail)].tolist() == [0] and qt[np.isposinf(tail)].tolist() == [255] and qt[np.isneginf(tail)].tolist() == [0]
    assert {c["n"] for c in mc.BYTE_CASES} == {1, 12, 16} and (1, 257) in {(c["H"], c["W"]) for c in mc.BYTE_CASES}
    # image bases of an [n,H,W,3] array at every residue mod 4
    assert {(k * 3 * 5 * 7) % 4 for k in range(12)} == {0, 1, 2, 3} and {(k * 771) % 4 for k in range(12)} == {0, 1, 2, 3}


@pytest.mark.parametrize("case", mc.ALBEDO_CASES, ids=_id)
def test_albedo_cases_hold_what_they_claim(case):
    r, g = mc.build_albedo(case)
    s64, s32, count, m32, m64 = mc.albedo_reference(case)
    # only zero or clearly signed sums: the selection is exact in both precisions and in every summation order
    s = r.astype(np.float64).sum(0)
    assert ((s == 0) | (np.abs(s) > 0.1)).all()
    f = np.float32
    assert np.array_equal(m32, m64) and np.array_equal(m32, ((r[0] + r[1]).astype(f) + r[2]).astype(f) / f(3) > 0)
    N = case["H"] * case["W"]
    if case["sel"] == "empty":
        assert count == 0 and np.isnan(s64).all() and (s < 0).any()
    elif case["sel"] == "all":
        assert count == N
    else:
        assert 0 < count < N and (s < 0).any() and (s == 0).any()
    if case["special"]:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = g.astype(np.float64)[:, m64] / r.astype(np.float64)[:, m64]
        if not case["srgb"]:
            assert np.isposinf(ratio).any() and ((ratio < 1e-6) & (ratio > 0)).any() and (ratio < 0).any()
        assert (ratio[np.isfinite(ratio)] > 1).any()
        assert np.isnan(s64[0]) == (case["special"] == "nan") and np.isfinite(s64[1:]).all()
        assert np.isnan(ratio).any() == (case["special"] == "nan")
    if count and not np.isnan(s64).any():
        e = np.abs(s32 - s64) / s64
        print(f"{case['id']}: count {count}, scale {s64}, E32 {e.max():.2e}")
        assert e.max() < 1e-6


def test_header_symbols_are_exported(built):
    from gaussian_renderer import _native as N
    hdr = open(os.path.join(ROOT, "include", "svgir_raster.h")).read()
    new = ("svgir_view_metrics_partials", "svgir_view_metrics", "svgir_capture_u8", "svgir_albedo_scale_partials", "svgir_albedo_scale")
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in N.EXPORTS and hasattr(N.lib, name), name
    assert re.search(r"#define SVGIR_METRIC_MAX_TERMS (\d+)", hdr).group(1) == "4"
    assert re.search(r"#define SVGIR_METRIC_COLS (\d+)", hdr).group(1) == str(mc.COLS) == "10"
    assert re.search(r"#define SVGIR_CAPTURE_MAX (\d+)", hdr).group(1) == "16"
    assert re.search(r"#define SVGIR_ABI_VERSION (\d+)", hdr).group(1) == "14" and N.lib.svgir_abi_version() == 14
    body = re.search(r"typedef struct svgir_plane_op \{(.*?)\} svgir_plane_op;", hdr, re.S).group(1)
    order = [m for m in re.findall(r"\b(src|mask|fill|bg|scale|offset|srgb)\b", body)]
    assert order == [f[0] for f in N.PlaneOp._fields_]
    import ctypes as C
    assert C.sizeof(N.PlaneOp) == 48 and C.sizeof(N.MetricTerm) == 104
    from svgir_harness import metrics
    assert (metrics.MAX_TERMS, metrics.CAPTURE_MAX, len(metrics.COLS)) == (4, 16, 10)


def test_invalid_arguments_are_rejected_before_any_hip_call(built):
    """No GPU is needed: every rejection happens on the host, with a message."""
    from gaussian_renderer import _native as N
    t = (N.MetricTerm * 5)()
    for k in range(5):
        t[k].a.src = t[k].b.src = 4096
    bad = 0xdead000
    for n in (0, 5, -1):
        assert N.lib.svgir_view_metrics(8, 8, n, t, bad, bad, None) == -1 and "terms per call" in N.last_error()
    assert N.lib.svgir_view_metrics(0, 8, 1, t, bad, bad, None) == -1 and "bad image size" in N.last_error()
    assert N.lib.svgir_view_metrics(8, -2, 1, t, bad, bad, None) == -1 and "bad image size" in N.last_error()
    t[1].b.src = None
    assert N.lib.svgir_view_metrics(8, 8, 2, t, bad, bad, None) == -1 and "term 1: an operand has no src" in N.last_error()
    t[0].a.fill = 4096
    assert N.lib.svgir_view_metrics(8, 8, 1, t, bad, bad, None) == -1 and "fill plane but no mask" in N.last_error()
    t[0].a.fill = None
    assert N.lib.svgir_view_metrics(8, 8, 1, t, None, bad, None) == -1 and "must be provided" in N.last_error()
    ops = (N.PlaneOp * 17)()
    for k in range(17):
        ops[k].src = 4096
    for n in (0, 17):
        assert N.lib.svgir_capture_u8(8, 8, n, ops, bad, None) == -1 and "operands per call" in N.last_error()
    assert N.lib.svgir_capture_u8(8, 0, 1, ops, bad, None) == -1 and "bad image size" in N.last_error()
    ops[2].srgb = 1
    assert N.lib.svgir_capture_u8(8, 8, 3, ops, bad, None) == -1 and "operand 2: srgb" in N.last_error()
    ops[1].fill = 4096
    assert N.lib.svgir_capture_u8(8, 8, 2, ops, bad, None) == -1 and "fill plane but no mask" in N.last_error()
    assert N.lib.svgir_capture_u8(8, 8, 1, ops, None, None) == -1 and "must be provided" in N.last_error()
    assert N.lib.svgir_albedo_scale(0, 3, bad, bad, 0, bad, bad, bad, None) == -1 and "bad image size" in N.last_error()
    assert N.lib.svgir_albedo_scale(4, 3, bad, None, 0, bad, bad, bad, None) == -1 and "must be provided" in N.last_error()
    assert N.lib.svgir_view_metrics_partials(33, 17, 3) == 3 * 3 * 2 * 3 * 3 and N.lib.svgir_albedo_scale_partials(56, 40) == 3 * 4


def test_cpu_tensors_fail_loudly(built):
    from svgir_harness import metrics
    x = torch.rand(3, 5, 7)
    for fn in (lambda: metrics.plane(x), lambda: metrics.view_metrics([(x, x)]), lambda: metrics.mse(x, x), lambda: metrics.psnr(x, x),
               lambda: metrics.captures_u8([x]), lambda: metrics.albedo_scale(x, x)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            fn()
    with pytest.raises(ValueError, match=r"\[3,H,W\]"):
        metrics.mse(torch.rand(4, 5, 7), torch.rand(4, 5, 7))
