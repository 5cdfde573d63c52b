"""LPIPS on the CPU: the oracle of tests/lpips_cases.py pinned by the reference's own run (tests/golden/lpips.npz), the properties of the case
table proven on the oracle, the constants the GPU bounds are made of (E32_k, EM_k) measured, and everything of the Python and C surface
that needs no GPU: the weight loader in both key forms, the argument errors, the four symbols at ABI 14.  No kernel runs here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import lpips_cases as lc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_id = lambda c: c["id"]  # noqa: E731


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the oracle is the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ("base", "dead5", "signed"))
def test_generated_weights_have_the_recorded_checksum(golden, variant):
    got, want = lc.weight_checksum(variant), golden[f"weights_{variant}"]
    print(variant, got, want)
    assert np.allclose(got, want, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("cid", ("size_16x16", "size_17x19", "const_0_vs_1_17x19"))
def test_case_builder_rebuilds_the_recorded_inputs(golden, cid):
    x, y = lc.operands(lc.BY_ID[cid])
    assert np.array_equal(_bits(x.numpy()), _bits(golden[f"{cid}/x"])) and np.array_equal(_bits(y.numpy()), _bits(golden[f"{cid}/y"]))


@pytest.mark.parametrize("cid", lc.GOLDEN_CASES)
def test_fp32_restatement_has_the_reference_bits(golden, cid):
    got = lc.oracle(cid, "f32")
    print(cid, got["score"], golden[f"{cid}/score"], got["taps"], golden[f"{cid}/taps"])
    assert np.array_equal(_bits(got["score"]), _bits(golden[f"{cid}/score"]))
    assert np.array_equal(_bits(got["taps"]), _bits(golden[f"{cid}/taps"]))


# ---- the table's properties, on the oracle ---------------------------------------------------------------------------------------------------
def test_table_covers_the_sizes_and_levels():
    sizes = {(c["H"], c["W"]) for c in lc.CASES}
    assert {(16, 16), (17, 19), (31, 31), (32, 32), (33, 47), (16, 150), (150, 16), (150, 161)} <= sizes
    m = lc.oracle("size_16x16")["maps"]
    assert [a.shape for a in m] == [(2, 64, 16, 16), (2, 128, 8, 8), (2, 256, 4, 4), (2, 512, 2, 2), (2, 512, 1, 1)]
    m = lc.oracle("size_33x47")["maps"]   # a floor in every pool
    assert [a.shape[2:] for a in m] == [(33, 47), (16, 23), (8, 11), (4, 5), (2, 2)]
    m = lc.oracle("size_150x161")["maps"]
    assert [a.shape[2:] for a in m] == [(150, 161), (75, 80), (37, 40), (18, 20), (9, 10)]
    assert {len(b) for b in lc.BATCHES} == {1, 2, 4}
    for b in lc.BATCHES:
        assert len({(lc.BY_ID[c]["H"], lc.BY_ID[c]["W"], lc.BY_ID[c]["variant"]) for c in b}) == 1


@pytest.mark.parametrize("case", [c for c in lc.CASES if c["expect"] == "zero"], ids=_id)
@pytest.mark.parametrize("kind", ("f64", "f32", "f32cl"))
def test_equal_operands_give_exact_zeros(case, kind):
    r = lc.oracle(case["id"], kind)
    assert np.all(r["taps"] == 0.0) and r["score"] == 0.0


@pytest.mark.parametrize("kind", ("f64", "f32", "f32cl"))
def test_swapped_operands_give_the_same_bits(kind):
    a, b = lc.oracle("size_33x47", kind), lc.oracle("swapped_33x47", kind)
    assert np.array_equal(a["taps"], b["taps"]) and a["score"] == b["score"]
    assert np.all(a["taps"] > 0.0)


@pytest.mark.parametrize("kind", ("f64", "f32", "f32cl"))
def test_dead_relu5_3_gives_an_exact_zero_not_nan(kind):
    r = lc.oracle("dead_relu5_3_32x32", kind)
    assert not r["maps"][4].any()                      # every relu5_3 vector is zero: 0 / (0 + 1e-10)
    assert r["taps"][4] == 0.0 and np.all(r["taps"][:4] > 0.0) and np.isfinite(r["score"])


def test_signed_linear_weights_have_both_signs():
    _, lin = lc.weights("signed")
    for w in lin.values():
        assert (w > 0).any() and (w < 0).any()
    _, lin = lc.weights("base")
    assert all((w >= 0).all() for w in lin.values())


@pytest.mark.parametrize("cid", ("nan_pixel_33x47", "inf_pixel_33x47"))
@pytest.mark.parametrize("kind", ("f64", "f32", "f32cl"))
def test_a_non_finite_pixel_gives_a_nan_score_in_torch(cid, kind):
    r = lc.oracle(cid, kind)
    assert np.isnan(r["score"]) and np.isnan(r["taps"][0])


def test_constants_and_out_of_range_values_are_finite_and_positive():
    for cid in ("const_0_vs_1_17x19", "range_-2_3_31x31"):
        r = lc.oracle(cid)
        assert np.all(np.isfinite(r["taps"])) and r["score"] > 0.0
    x, y = lc.operands(lc.BY_ID["range_-2_3_31x31"])
    assert x.min() < -1.5 and x.max() > 2.5


def test_plane_cases_exercise_every_operand_feature():
    feats = set()
    for c in lc.CASES:
        for o in (c["a"], c["b"]):
            if o["mask"] is not None:
                feats.add("fill" if o["fill"] is not None else "bg")
                assert ((o["mask"] > 0) & (o["mask"] < 1)).any()    # a soft edge: both products of the composite matter
            if o["scale"] != 1.0 or o["offset"] != 0.0:
                feats.add("affine")
            if o["srgb"]:
                feats.add("srgb")
    assert feats == {"bg", "fill", "affine", "srgb"}
    assert len(lc.SRGB_CASES) == 1


# ---- the constants of the GPU bounds ---------------------------------------------------------------------------------------------------------
def test_measure_fp32_deviation_from_fp64():
    """E32_k and EM_k: what torch's own two fp32 orders lose against fp64 over the table.  Printed; sanity-bounded from the number
    format only: at least one rounding must show somewhere (> 0) and nothing may exceed sqrt(K) roundings of a K = 4608 sum chained over
    13 layers by orders of magnitude (1e-4)."""
    e32, em = lc.measured_errors()
    print("E32_k", " ".join(f"{v:.3e}" for v in e32))
    print("EM_k ", " ".join(f"{v:.3e}" for v in em))
    assert np.all(e32 > 0.0) and np.all(e32 < 1e-4)
    assert np.all(em > 0.0) and np.all(em < 1e-4)
    for cid in lc.FINITE_CASES:   # an exactly-zero fp64 tap is exactly zero in fp32 too, so it needs no relative bound
        ref, a, b = lc.oracle(cid), lc.oracle(cid, "f32"), lc.oracle(cid, "f32cl")
        zero = ref["taps"] == 0.0
        assert np.all(a["taps"][zero] == 0.0) and np.all(b["taps"][zero] == 0.0)


# ---- the loader ------------------------------------------------------------------------------------------------------------------------------
def _forms():
    vgg, lin = lc.weights("base")
    bare_vgg = {k[len("features."):]: v for k, v in vgg.items()}
    renamed_lin = {k.replace("lin", "").replace("model.", ""): v for k, v in lin.items()}   # what lpipsPyTorch's get_state_dict makes
    assert "0.weight" in bare_vgg and "0.1.weight" in renamed_lin
    return (vgg, lin), (bare_vgg, renamed_lin)


def test_loader_accepts_both_key_forms_as_dicts_and_as_files(tmp_path):
    from svgir_harness import metrics
    (vgg, lin), (bare_vgg, renamed_lin) = _forms()
    nets = [metrics.LPIPS(vgg, lin), metrics.LPIPS(bare_vgg, renamed_lin)]
    torch.save(vgg, tmp_path / "vgg16.pth"); torch.save(renamed_lin, tmp_path / "lin.pth")
    torch.save(bare_vgg, tmp_path / "features.pth"); torch.save(lin, tmp_path / "vgg_lin.pth")
    nets.append(metrics.LPIPS(str(tmp_path / "vgg16.pth"), tmp_path / "lin.pth"))
    nets.append(metrics.LPIPS(tmp_path / "features.pth", str(tmp_path / "vgg_lin.pth")))
    for net in nets:
        assert [tuple(w.shape) for w in net._w] == [(co, ci, 3, 3) for co, ci in lc.CONV_SHAPE]
        for i, w, b in zip(lc.CONV_INDEX, net._w, net._b):
            assert torch.equal(w, vgg[f"features.{i}.weight"]) and torch.equal(b, vgg[f"features.{i}.bias"])
        for k, w in enumerate(net._lin):
            assert torch.equal(w, lin[f"lin{k}.model.1.weight"].reshape(-1))


def test_loader_refuses_missing_keys_and_wrong_shapes():
    from svgir_harness import metrics
    vgg, lin = lc.weights("base")
    with pytest.raises(KeyError, match="28"):
        metrics.LPIPS({k: v for k, v in vgg.items() if not k.startswith("features.28.")}, lin)
    with pytest.raises(KeyError, match="lin4"):
        metrics.LPIPS(vgg, {k: v for k, v in lin.items() if not k.startswith("lin4")})
    bad = dict(vgg)
    bad["features.5.weight"] = vgg["features.7.weight"]
    with pytest.raises(ValueError, match="features.5.weight"):
        metrics.LPIPS(bad, lin)
    # the right element count in another layout is refused too (a reshape would accept it and give wrong scores)
    for perm in ((1, 0, 2, 3), (0, 2, 3, 1)):
        bad = dict(vgg)
        bad["features.2.weight"] = vgg["features.2.weight"].permute(*perm).contiguous()    # (64 x 64: [Cin,Cout,3,3] has the same shape, undetectable)
        bad["features.5.weight"] = vgg["features.5.weight"].permute(*perm).contiguous()
        with pytest.raises(ValueError, match=r"features\.[25]\.weight"):
            metrics.LPIPS(bad, lin)
    bad = dict(vgg)
    bad["features.0.bias"] = vgg["features.0.bias"].reshape(1, 64)
    with pytest.raises(ValueError, match="features.0.bias"):
        metrics.LPIPS(bad, lin)
    bad = dict(lin)
    bad["lin1.model.1.weight"] = lin["lin0.model.1.weight"]
    with pytest.raises(ValueError, match="lin1"):
        metrics.LPIPS(vgg, bad)
    with pytest.raises(TypeError):
        metrics.LPIPS(3, lin)


# ---- argument errors -------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_batches_and_shapes_are_refused():
    from svgir_harness import metrics
    net = metrics.LPIPS(*lc.weights("base"))
    x = torch.rand(3, 32, 32)
    with pytest.raises(RuntimeError, match="GPU"):
        net(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.lpips_terms(net, [(x, x)])
    with pytest.raises(ValueError, match="batch of 2"):
        net(torch.rand(2, 3, 32, 32), torch.rand(2, 3, 32, 32))
    with pytest.raises(ValueError, match=r"\[3,H,W\]"):
        net(torch.rand(1, 32, 32), torch.rand(1, 32, 32))
    with pytest.raises(ValueError, match="1 ... 4"):
        metrics.lpips_terms(net, [])
    with pytest.raises(ValueError, match="1 ... 4"):
        metrics.lpips_terms(net, [(x, x)] * 5)
    with pytest.raises(RuntimeError, match="GPU"):
        net.packed("cpu")


def test_drop_in_refuses_other_networks_and_missing_weights(monkeypatch):
    import lpipsPyTorch
    assert os.path.abspath(lpipsPyTorch.__file__).startswith(os.path.join(ROOT, "svg-ir_amd"))
    x = torch.rand(3, 32, 32)
    for net_type in ("alex", "squeeze"):
        with pytest.raises(NotImplementedError, match="'vgg'"):
            lpipsPyTorch.lpips(x, x, net_type=net_type)
    with pytest.raises(NotImplementedError, match="'vgg'"):
        lpipsPyTorch.lpips(x, x)                       # the reference's default is 'alex'
    monkeypatch.delenv(lpipsPyTorch.ENV_VGG, raising=False)
    monkeypatch.delenv(lpipsPyTorch.ENV_LIN, raising=False)
    lpipsPyTorch.set_weights()
    with pytest.raises(RuntimeError, match="SVGIR_LPIPS_VGG_WEIGHTS.*SVGIR_LPIPS_LIN_WEIGHTS"):
        lpipsPyTorch.lpips(x, x, net_type="vgg")
    with pytest.raises(ValueError, match="both"):
        lpipsPyTorch.set_weights(vgg=lc.weights("base")[0])
    try:
        lpipsPyTorch.set_weights(*lc.weights("base"))
        with pytest.raises(ValueError, match="batch of 2"):
            lpipsPyTorch.lpips(torch.rand(2, 3, 32, 32), torch.rand(2, 3, 32, 32), net_type="vgg")
        with pytest.raises(RuntimeError, match="GPU"):
            lpipsPyTorch.lpips(x, x, net_type="vgg")
    finally:
        lpipsPyTorch.set_weights()


def test_drop_in_reads_the_environment(monkeypatch, tmp_path):
    import lpipsPyTorch
    vgg, lin = lc.weights("base")
    torch.save(vgg, tmp_path / "vgg16.pth"); torch.save(lin, tmp_path / "lin.pth")
    monkeypatch.setenv(lpipsPyTorch.ENV_VGG, str(tmp_path / "vgg16.pth"))
    monkeypatch.setenv(lpipsPyTorch.ENV_LIN, str(tmp_path / "lin.pth"))
    lpipsPyTorch.set_weights()
    try:
        net = lpipsPyTorch._network()
        assert torch.equal(net._w[12], vgg["features.28.weight"]) and lpipsPyTorch._network() is net   # built once
    finally:
        lpipsPyTorch.set_weights()


def test_library_refuses_bad_arguments_before_any_launch():
    from gaussian_renderer import _native as N
    pairs = (N.LpipsPair * 5)()
    for p in pairs:
        p.a.src = p.b.src = 16       # never dereferenced: every call below is refused first
        p.a.scale = p.b.scale = 1.0
    one = C.c_void_p(256)
    call = lambda W, H, n, packed=one, work=one, taps=one, score=one, maps=None: N.lib.svgir_lpips(  # noqa: E731
        W, H, n, pairs, packed, work, taps, score, maps, None)
    for W, H in ((15, 16), (16, 15), (0, 0), (-3, 64)):
        assert call(W, H, 1) == -1 and "smaller than 16 x 16" in N.last_error()
        assert N.lib.svgir_lpips_work_bytes(W, H, 1) == 0
    for n in (0, 5, -1):
        assert call(32, 32, n) == -1 and "pairs per call" in N.last_error()
        assert N.lib.svgir_lpips_work_bytes(32, 32, n) == 0
    for W, H in ((50000, 50000), (16, 1 << 27), (1 << 27, 16)):     # H W beyond an int; more patches / blocks than a grid holds
        assert call(W, H, 1) == -1 and "exceeds the supported size" in N.last_error()
        assert N.lib.svgir_lpips_work_bytes(W, H, 1) == 0
    for kw in ("packed", "work", "taps", "score"):
        assert call(32, 32, 1, **{kw: None}) == -1 and "must be provided" in N.last_error()
    assert call(32, 32, 1, work=C.c_void_p(260)) == -1 and "aligned" in N.last_error()
    maps = (C.c_void_p * 5)(256, 256, None, 256, 256)
    assert call(32, 32, 1, maps=maps) == -1 and "entry 2" in N.last_error()
    pairs[1].b.src = None
    assert call(32, 32, 2) == -1 and "pair 1" in N.last_error() and "no src" in N.last_error()
    pairs[1].b.src = 16
    pairs[0].a.fill = 16
    assert call(32, 32, 1) == -1 and "fill plane but no mask" in N.last_error()
    # the workspace: two [2 n][H][W][64] fp32 buffers and the records
    for W, H, n in ((16, 16, 1), (161, 150, 4), (800, 800, 1)):
        b = N.lib.svgir_lpips_work_bytes(W, H, n)
        assert 2 * (2 * n * H * W * 64 * 4) <= b <= 2 * (2 * n * H * W * 64 * 4) + 8 * n * (H * W // 32 + 16) + 1024
    null13, null5 = (C.c_void_p * 13)(), (C.c_void_p * 5)()
    assert N.lib.svgir_lpips_pack(null13, null13, null5, one, None) == -1 and "convolution 0" in N.last_error()
    assert N.lib.svgir_lpips_pack(None, null13, null5, one, None) == -1
    assert N.lib.svgir_lpips_packed_floats() == sum(co * ci * 9 + co for co, ci in lc.CONV_SHAPE) + sum(lc.TAP_C)


def test_header_exports_and_library_agree_at_abi_14():
    from gaussian_renderer import _native as N
    names = ("svgir_lpips_packed_floats", "svgir_lpips_pack", "svgir_lpips_work_bytes", "svgir_lpips")
    hdr = open(os.path.join(ROOT, "include", "svgir_raster.h")).read()
    assert re.search(r"#define SVGIR_ABI_VERSION (\d+)", hdr).group(1) == "14" and N.lib.svgir_abi_version() == 14
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in N.EXPORTS
        assert getattr(N.lib, name) is not None
    assert re.search(r"typedef struct svgir_lpips_pair \{\s*svgir_plane_op a, b;\s*\} svgir_lpips_pair;", hdr)
    assert C.sizeof(N.LpipsPair) == 2 * C.sizeof(N.PlaneOp)
    assert int(re.search(r"#define SVGIR_METRIC_MAX_TERMS (\d+)", hdr).group(1)) == 4
