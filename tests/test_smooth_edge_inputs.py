"""The smoothness-loss case table (tests/smooth_cases.py) on the host: its oracle reproduces the reference's recorded results
(tests/golden/smooth_losses.npz: the reference's own first_order_edge_aware_loss / second_order_edge_aware_loss / tv_loss with autograd over
a stubbed kornia, scripts/make_golden_smooth.py), a second construction in numpy (np.pad(mode="edge") and shifted slices, no conv2d) and
central finite differences; every case holds what it is named for; E32 per case and G32 over the table -- what the reference's own fp32
arithmetic loses -- are measured and the threshold-element cap is proven; the C ABI carries the three new entry points at version 14 and
refuses bad arguments before any GPU work."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import smooth_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "smooth_losses.npz")
_id = lambda c: c["id"] if isinstance(c, dict) else str(c)   # noqa: E731
CASES = {c["id"]: c for c in sc.CASES}
FINITE = [c for c in sc.CASES if c["id"].split("-")[0] not in sc.NONFINITE]
_cache = {}


def evaluated(cid):
    """[(term, oracle, torch_eval fp64, torch_eval fp32)] of a case, computed once."""
    if cid not in _cache:
        _cache[cid] = [(t, sc.oracle(t), sc.torch_eval(t), sc.torch_eval(t, torch.float32)) for t in sc.build(CASES[cid])]
    return _cache[cid]


def _same(a, b, tol):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol


# ---- the oracle against the reference's recorded results ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_is_small_data(gold):
    assert os.path.getsize(GOLD) < 400 * 1024
    assert all(gold[k].dtype.kind in "fU" for k in gold.files)
    assert {str(c).split("-")[0] for c in gold["recorded"]} >= {"sizes", "four", "shared", "light", "stage2", "envmap"}


def test_oracle_reproduces_the_reference(gold):
    kinds = set()
    for cid in (str(c) for c in gold["recorded"]):
        for k, (term, o, r64, r32) in enumerate(evaluated(cid)):
            g = lambda name: gold[f"{cid}.{k}.{name}"]   # noqa: E731
            kinds.add((term["kind"], term["data"].shape[0], 0 if term["img"] is None else term["img"].shape[0]))
            assert _same(o["loss"], float(g("f64.loss")), 1e-14), (cid, k)
            assert _same(r64["loss"], float(g("f64.loss")), 1e-14), (cid, k)
            assert _same(r32["loss"], float(g("f32.loss")), 2e-6 * abs(float(g("f32.loss")))), (cid, k)   # (fp32 sums in conv2d's order)
            for nm, mask in (("d_data", term["data_mask"]), ("d_img", term["img_mask"])):
                if o[nm] is None:
                    continue
                ref = g("f64." + nm) * (1.0 if mask is None else mask.astype(np.float64))   # recorded w.r.t. the masked product
                np.testing.assert_allclose(o[nm], ref, rtol=0, atol=1e-14, err_msg=f"{cid} {k} {nm}")
    assert {k[0] for k in kinds} == {"first", "second", "tv"} and {(1, 3), (3, 1), (3, 3), (4, 4)} <= {k[1:] for k in kinds}


# ---- a second construction: numpy, edge padding and shifted slices ----------------------------------------------------------------
def np_gradient(x, order):
    """[C,H,W] fp64 -> [C,2,H,W]: the contract's derivative without conv2d."""
    smooth, deriv, norm = (([1, 2, 1], [-1, 0, 1], 8.0) if order == 1 else ([1, 4, 6, 4, 1], [-1, 0, 2, 0, -1], 64.0))
    Cc, H, W = x.shape
    xp = np.pad(x, ((0, 0), (order, order), (order, order)), mode="edge")
    out = np.zeros((Cc, 2, H, W))
    n = 2 * order + 1
    with np.errstate(invalid="ignore"):
        for i in range(n):
            for j in range(n):
                win = xp[:, i:i + H, j:j + W]
                out[:, 0] += (smooth[i] * deriv[j] / norm) * win
                out[:, 1] += (deriv[i] * smooth[j] / norm) * win
    return out


def np_loss(kind, D, I=None):   # noqa: E741
    """The term on fp64 arrays D [C,H,W], I [Ci,H,W] (masks already applied)."""
    if kind == "tv":
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.float64(np.square(D[:, 1:] - D[:, :-1]).sum()) / D[:, 1:].size + np.float64(np.square(D[:, :, 1:] - D[:, :, :-1]).sum()) / D[:, :, 1:].size
    order, s = (1, 1.0) if kind == "first" else (2, 10.0)
    with np.errstate(invalid="ignore"):
        v = np.abs(np_gradient(D, order)) * np.exp(-s * np.abs(np_gradient(I, 1)))
    return v.sum(1).mean()


def _products(term):
    D = term["data"] if term["data_mask"] is None else term["data"] * term["data_mask"]
    I = None if term["img"] is None else (term["img"] if term["img_mask"] is None else term["img"] * term["img_mask"])   # noqa: E741
    return D.astype(np.float64), None if I is None else I.astype(np.float64)


@pytest.mark.parametrize("case", sc.CASES, ids=_id)
def test_oracle_equals_the_numpy_construction(case):
    for k, (term, o, _, _) in enumerate(evaluated(case["id"])):
        D, I = _products(term)   # noqa: E741
        ref = float(np_loss(term["kind"], D, I))
        assert _same(o["loss"], ref, 1e-14 * max(1.0, abs(ref))), (case["id"], k, o["loss"], ref)
        if term["kind"] != "tv":
            order = 1 if term["kind"] == "first" else 2
            np.testing.assert_allclose(o["gd"], np_gradient(D, order), rtol=0, atol=1e-13 * max(1.0, np.nanmax(np.abs(D[np.isfinite(D)]))), equal_nan=True)
            np.testing.assert_allclose(o["gi"], np_gradient(I, 1), rtol=0, atol=1e-13 * max(1.0, np.nanmax(np.abs(I[np.isfinite(I)]))), equal_nan=True)


@pytest.mark.parametrize("cid", ["sizes-1x7", "sizes-5x1", "sizes-2x2", "sizes-3x3", "sizes-5x5"])
def test_gradients_equal_central_differences(cid):
    """fp64 central differences of the numpy construction, every element of data and img (no masks in these cases).  A derivative that is
    exactly 0 (one row, one column) sits on the kink of abs: the central difference there is 0, which is sign(0) = 0."""
    h = 2.0 ** -20

    def value(kind, D, I):   # noqa: E741
        if kind != "tv":
            return np_loss(kind, D, I)
        H, W = D.shape[1:]                                        # an empty mean is NaN in the value; the other mean's gradient is real
        return (np.square(D[:, 1:] - D[:, :-1]).sum() / D[:, 1:].size if H > 1 else 0.0) + \
               (np.square(D[:, :, 1:] - D[:, :, :-1]).sum() / D[:, :, 1:].size if W > 1 else 0.0)

    for k, (term, o, _, _) in enumerate(evaluated(cid)):
        D, I = _products(term)   # noqa: E741
        for nm, arr in (("d_data", D), ("d_img", I)):
            if arr is None:
                continue
            fd = np.zeros_like(arr)
            for idx in np.ndindex(arr.shape):
                x0 = arr[idx]
                arr[idx] = x0 + h
                up = value(term["kind"], D, I)
                arr[idx] = x0 - h
                dn = value(term["kind"], D, I)
                arr[idx] = x0
                fd[idx] = (up - dn) / (2 * h)
            np.testing.assert_allclose(o[nm], fd, rtol=0, atol=2e-9, err_msg=f"{cid} {k} {nm}")   # (the kinks of abs lie further off than h here)


# ---- every case holds what it is named for --------------------------------------------------------------------------------------------
def test_table_covers_the_sizes_kinds_and_channel_pairs():
    sizes = [c for c in sc.CASES if c["id"].startswith("sizes-")]
    assert [(c["H"], c["W"]) for c in sizes] == list(sc.SIZES)
    assert set(sc.SIZES) == {(1, 1), (1, 7), (5, 1), (2, 2), (3, 3), (5, 5), (8, 32), (7, 31), (9, 33), (21, 70), (150, 161)}
    for c in sizes:
        assert [t["kind"] for t in c["terms"]] == ["first", "second", "tv"]
    pairs = {(t["C"], t["Ci"]) for c in sc.CASES for t in c["terms"] if t["kind"] != "tv"}
    assert pairs == {(1, 1), (1, 3), (3, 1), (3, 3), (4, 4)}
    assert sum((t["C"], t["Ci"]) == (4, 4) for c in sc.CASES for t in c["terms"]) == 2 and len(CASES["four-7x31"]["terms"]) == 3
    assert all(len(c["terms"]) <= 4 for c in sc.CASES)
    th, tw = sc.TILE
    assert (150 + th - 1) // th * ((161 + tw - 1) // tw) > 64 and 21 % th and 70 % tw and 70 > 2 * tw
    masks = {t["data_mask"] for c in sc.CASES for t in c["terms"]}
    assert masks >= {"ones", "zeros", "disc", "fractions", "border_edge"}
    assert any(t["img_grad"] for t in CASES["stage2-21x70"]["terms"]) and [t["C"] for t in CASES["stage2-21x70"]["terms"]] == [3, 1, 3]
    terms = sc.build(CASES["stage2-21x70"])
    assert terms[0]["img"] is terms[1]["img"] and terms[2]["img"] is not terms[0]["img"]
    terms = sc.build(CASES["shared-9x33"])
    assert terms[0]["img"] is terms[1]["img"]
    env = sc.build(CASES["envmap-16x32"])[0]
    assert env["kind"] == "tv" and env["data"].shape == (3, 16, 32)


def test_flat_step_and_plane_are_exact():
    for term, o, r64, r32 in evaluated("flat-21x70")[:3]:          # one dyadic value: every derivative exactly 0
        assert o["loss"] == 0.0 and r32["loss"] == 0.0 and not o["d_data"].any() and not r32["d_data"].any()
        if o["d_img"] is not None:
            assert not o["d_img"].any() and not o["aabs_img"].any()
        assert not o["aabs_data"].any()
    term, o, _, r32 = evaluated("flat-21x70")[3]                     # a flat img: weight exactly 1, no gradient into img
    assert not o["gi"].any() and not o["d_img"].any() and o["loss"] > 0 and o["d_data"].any()
    term, o, _, _ = evaluated("step-21x70")[0]                       # the edge lies on the tile border at x = 32
    assert (term["data"][:, :, :32] == 0.25).all() and (term["data"][:, :, 32:] == 0.75).all()
    gx = o["gd"][:, 0]
    assert (gx[:, :, 31:33] == 0.25).all() and not gx[:, :, :31].any() and not gx[:, :, 33:].any() and not o["gd"][:, 1].any()
    term, o, _, r32 = evaluated("step-21x70")[1]                     # second order: -1/8, +1/8 ... across the edge, 0 elsewhere
    assert o["gd"][:, 0, :, 30:34].all() and not o["gd"][:, 0, :, :30].any() and not o["gd"][:, 0, :, 34:].any()
    term, o, _, r32 = evaluated("plane-21x70")[0]                    # a x + b y: second derivative 0 in the interior, not on the replicate border
    assert not o["gd"][:, :, 2:-2, 2:-2].any() and o["gd"][:, 0, :, :2].all() and o["gd"][:, 1, :2, :].all() and o["loss"] > 0
    gd32 = sc.spatial_gradient(torch.from_numpy(term["data"]), 2).numpy()
    assert np.array_equal(gd32, o["gd"])                             # dyadic: the fp32 evaluation is exact too


def test_masks_hold_what_they_are_named_for():
    ones, zeros, disc, frac = evaluated("masks-21x70")
    plain = sc.oracle(dict(ones[0], data_mask=None, img_mask=None))
    assert ones[1]["loss"] == plain["loss"] and np.array_equal(ones[1]["d_data"], plain["d_data"])
    assert zeros[1]["loss"] == 0.0 and not zeros[1]["d_data"].any() and not zeros[1]["d_img"].any()
    m = disc[0]["data_mask"][0]
    assert 0 < m.mean() < 1 and set(np.unique(m)) == {0.0, 1.0}
    assert not disc[1]["d_data"][:, m == 0].any() and disc[1]["d_data"][:, m == 1].all()   # the outgoing gradient is multiplied by the mask
    f = frac[0]["data_mask"][0]
    assert ((f > 0) & (f < 1)).mean() > 0.99
    b = evaluated("mask_border-21x70")[0][0]["data_mask"][0]
    assert not b[0].any() and not b[:, 0].any() and not b[-2:].any() and not b[:, -2:].any() and b[1:-2, 1:-2].all()


@pytest.mark.parametrize("cid", ["nan_data-9x33", "nan_img-9x33", "inf_img-9x33"])
def test_non_finite_cases(cid):
    y, x = sc.POKE_AT
    for term, o, r64, r32 in evaluated(cid):
        which = "data" if cid.startswith("nan_data") else "img"
        a = term[which]
        bad = ~np.isfinite(a)
        assert bad.sum() == 1 and bad[min(1, a.shape[0] - 1), y, x] and (np.isnan(a[bad]).all() if cid.startswith("nan") else (a[bad] == np.inf).all())
        assert np.isnan(o["loss"]) and np.isnan(r64["loss"]) and np.isnan(r32["loss"])          # torch puts the NaN into the loss too
        for nm in ("d_data", "d_img", "aabs_data", "aabs_img"):
            assert np.isfinite(o[nm]).all(), nm                                                    # ... the convention keeps it out of every gradient
        assert o["d_data"].any() and o["d_img"].any()
        assert not np.isfinite(r64["d_data"]).all() or not np.isfinite(r64["d_img"]).all()        # (torch's autograd would spread it)


def test_empty_tv_means():
    one = evaluated("sizes-1x1")[2][1]
    assert np.isnan(one["loss"]) and not one["d_data"].any()
    for cid in ("sizes-1x7", "sizes-5x1"):
        term, o, r64, _ = evaluated(cid)[2]
        assert np.isnan(o["loss"]) and np.isnan(r64["loss"]) and 0 in sc.counts(term)
        assert np.isfinite(o["d_data"]).all() and o["d_data"].any()                               # the other mean's gradient flows, as in torch
        np.testing.assert_allclose(o["d_data"], r64["d_data"], rtol=0, atol=1e-15)


# ---- E32, G32 and the threshold elements -----------------------------------------------------------------------------------------------
def _signs_agree_outside(term, o):
    """The fp32 evaluation of a derivative disagrees in sign with fp64 only at threshold elements."""
    t = sc._tensors(term, torch.float32)
    D = t["data"] if t["data_mask"] is None else t["data"] * t["data_mask"]
    I = t["img"] if t["img_mask"] is None else t["img"] * t["img_mask"]   # noqa: E741
    for g32, g64, thr in ((sc.spatial_gradient(D, 1 if term["kind"] == "first" else 2).numpy(), o["gd"], o["thr_gd"]),
                          (sc.spatial_gradient(I, 1).numpy(), o["gi"], o["thr_gi"])):
        with np.errstate(invalid="ignore"):
            differ = np.sign(g32) != np.sign(g64)
        differ &= ~(np.isnan(g32) & np.isnan(g64))
        assert not (differ & ~thr).any(), int((differ & ~thr).sum())


def _g_ratio(o, r32):
    worst = 0.0
    for nm in ("data", "img"):
        if o["d_" + nm] is None:
            continue
        keep = ~o["thr_" + nm]
        ratio = np.abs(r32["d_" + nm] - o["d_" + nm]) / (sc.EPS32 * np.maximum(o["aabs_" + nm], sc.AABS_FLOOR))
        worst = max(worst, float(ratio[keep].max()) if keep.any() else 0.0)
    return worst


@pytest.mark.parametrize("case", FINITE, ids=_id)
def test_e32_g32_and_threshold_caps(case):
    for k, (term, o, r64, r32) in enumerate(evaluated(case["id"])):
        for nm in ("data", "img"):                       # on finite inputs the conventions change nothing: oracle == torch's fp64 autograd
            if o["d_" + nm] is not None:
                np.testing.assert_allclose(o["d_" + nm], r64["d_" + nm], rtol=0, atol=1e-14 * max(1.0, np.abs(r64["d_" + nm]).max()))
                share = o["thr_" + nm].mean()
                assert share <= sc.MAX_THRESHOLD_SHARE, (case["id"], k, nm, share)
                assert (np.abs(o["d_" + nm]) <= o["aabs_" + nm] * (1 + 1e-12) + 1e-300).all()
        assert _same(o["loss"], r64["loss"], 1e-14)
        if np.isnan(o["loss"]):
            assert term["kind"] == "tv" and 0 in sc.counts(term)
            e32 = float("nan")
        else:
            e32 = abs(r32["loss"] - o["loss"])
            assert e32 <= 2e-6 * max(abs(o["loss"]), 1e-3), (case["id"], k, e32)      # the fp32 restatement is the same function
            assert o["A"] == pytest.approx(abs(o["loss"]), rel=1e-12, abs=1e-300)   # every contribution is >= 0
        if term["kind"] != "tv":
            _signs_agree_outside(term, o)
        g = _g_ratio(o, r32)
        print(f"{case['id']} term {k} {term['kind']}: loss {o['loss']:.6g}, E32 {e32:.2e}, bound {sc.loss_bound(o, e32) if e32 == e32 else float('nan'):.2e}, G {g:.2f}")
        assert g <= sc.G32, (case["id"], k, g)


def test_g32_is_the_measured_constant():
    """G32 of tests/smooth_cases.py is not below what the whole table measures here, and not more than twice it."""
    worst = max(_g_ratio(o, r32) for c in FINITE for _, o, _, r32 in evaluated(c["id"]))
    rest = max(_g_ratio(o, r32) for c in FINITE if not c["id"].startswith("strong") for _, o, _, r32 in evaluated(c["id"]))
    print(f"G32 measured {worst:.1f} (without the strong case {rest:.1f}); constant {sc.G32}")
    assert worst <= sc.G32 <= 2 * worst
    strong = evaluated("strong-21x70")[0]
    w32 = np.exp(np.float32(-10) * np.abs(strong[1]["gi"]).astype(np.float32))
    assert (w32 == 0).mean() > 0.5 and (np.abs(strong[1]["gi"]) > 10).mean() > 0.5      # the weights underflow in fp32, the derivatives are large
    assert (strong[1]["aabs_data"] < sc.AABS_FLOOR).any() and 0 < strong[1]["loss"] < 1e-2


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
NAMES = ("svgir_smooth_loss_partials", "svgir_smooth_loss_forward", "svgir_smooth_loss_backward")


def test_header_exports_and_library_agree(built):
    from gaussian_renderer import _native as N
    hdr = open(os.path.join(ROOT, "include", "svgir_raster.h")).read()
    declared = set(re.findall(r"\b(svgir_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(N.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in N.EXPORTS and hasattr(lib, name), name
        assert getattr(N.lib, name).argtypes is not None
    assert lib.svgir_abi_version() == N.ABI_VERSION == 14
    assert re.search(r"#define SVGIR_ABI_VERSION (\d+)", hdr).group(1) == "14"
    body = re.search(r"typedef struct svgir_smooth_term \{(.*?)\} svgir_smooth_term;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in re.sub(r"^(const\s+)?\w+\s", "", decl.strip()).replace("*", " ").split(",")]
    assert fields == [f[0] for f in N.SmoothTerm._fields_]
    from svgir_harness import losses
    assert re.search(r"#define SVGIR_SMOOTH_MAX_TERMS (\d+)", hdr).group(1) == str(losses.SMOOTH_MAX_TERMS) == "4"
    assert losses.SMOOTH_KINDS == sc.KINDS


def test_partials(built):
    from gaussian_renderer import _native as N
    f = N.lib.svgir_smooth_loss_partials
    assert f(161, 150, 1) == 6 * 19 and f(161, 150, 3) == 3 * 6 * 19 and f(1, 1, 1) == 1 and f(1, 1, 4) == 4
    assert f(32, 8, 2) == 2 and f(33, 9, 1) == 4 and f(0, 5, 1) == 0 and f(5, 5, 0) == 0


def test_cpu_tensors_and_bad_arguments_are_refused(built):
    """No CPU path behind the smoothness losses, and the C entry points validate before any launch (no GPU is touched here)."""
    from gaussian_renderer import _native as N
    from svgir_harness import losses
    z3, z1 = torch.zeros(3, 4, 4), torch.ones(1, 4, 4)
    for call in (lambda: losses.first_order_edge_aware_loss(z3, z3), lambda: losses.second_order_edge_aware_loss(z1, z3), lambda: losses.tv_loss(z3),
                 lambda: losses.tv_loss(z3[0]), lambda: losses.smoothness_losses([dict(kind="first", data=z3, img=z3, data_mask=z1)])):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()
    with pytest.raises(RuntimeError, match="gets no gradient"):
        losses.smoothness_losses([dict(kind="first", data=z3, img=z3, img_mask=z1.clone().requires_grad_(True))])
    for terms, msg in (([], "terms per launch"), ([dict(kind="tv", data=z3)] * 5, "terms per launch"), ([dict(kind="third", data=z3)], "unknown kind"),
                       ([dict(kind="first", data=z3)], "no img"), ([dict(kind="tv", data=z3, img=z3)], "data only"),
                       ([dict(kind="first", data=z3, img=torch.zeros(2, 4, 4))], "cannot broadcast"),
                       ([dict(kind="first", data=z3, img=torch.zeros(3, 4, 5))], "every plane of a launch"),
                       ([dict(kind="first", data=z3, img=z3, data_mask=z3)], r"\[1,H,W\]"), ([dict(kind="tv", data=z3, weight=z1)], "unknown keys")):
        with pytest.raises(ValueError, match=msg):
            losses.smoothness_losses(terms)

    def term(kind, Cc, Ci, data=1, img=1, **kw):
        t = N.SmoothTerm()
        t.kind, t.C, t.Ci, t.data, t.img = kind, Cc, Ci, data or None, img or None     # (pointers that are never dereferenced: nothing is launched)
        for key, v in kw.items():
            setattr(t, key, v)
        return (N.SmoothTerm * 1)(t)

    buf = 8   # a non-NULL value for partial / stats / losses: every call below is refused before it is used
    fwd = lambda W, H, n, t: N.lib.svgir_smooth_loss_forward(W, H, n, t, buf, buf, buf, None)   # noqa: E731
    for args, msg in (((-1, 4, 1, term(1, 3, 3)), "bad image size"), ((4, 4, 0, term(1, 3, 3)), "n_terms"), ((4, 4, 5, term(1, 3, 3)), "n_terms"),
                      ((4, 4, 1, None), "descriptors"), ((4, 4, 1, term(0, 3, 3)), "unknown kind"), ((4, 4, 1, term(4, 3, 3)), "unknown kind"),
                      ((4, 4, 1, term(1, 5, 1)), "C=5"), ((4, 4, 1, term(1, 0, 1)), "C=0"), ((4, 4, 1, term(2, 3, 0)), "Ci=0"),
                      ((4, 4, 1, term(1, 2, 3)), "cannot broadcast"), ((4, 4, 1, term(1, 3, 3, data=0)), "data plane"),
                      ((4, 4, 1, term(2, 3, 3, img=0)), "img plane"), ((4, 4, 1, term(3, 3, 3, img=0)), "tv term"), ((4, 4, 1, term(3, 3, 0)), "tv term"),
                      ((4, 4, 1, term(3, 3, 0, img=0, data_mask=8)), "tv term")):
        assert fwd(*args) == -1 and msg in N.last_error(), (msg, N.last_error())
    assert N.lib.svgir_smooth_loss_forward(4, 4, 1, term(1, 3, 3), None, buf, buf, None) == -1 and "must be provided" in N.last_error()
    assert N.lib.svgir_smooth_loss_backward(4, 4, 1, term(1, 3, 3), buf, buf, None) == -1 and "no gradient requested" in N.last_error()
    assert N.lib.svgir_smooth_loss_backward(4, 4, 1, term(1, 3, 3, d_data=8), None, buf, None) == -1 and "must be provided" in N.last_error()
    assert N.lib.svgir_smooth_loss_backward(4, 4, 1, term(3, 3, 0, img=0, d_img=8), buf, buf, None) == -1 and "tv term" in N.last_error()
    # W * H == 0 launches nothing and succeeds
    assert fwd(0, 4, 1, term(1, 3, 3)) == 0 and N.lib.svgir_smooth_loss_backward(4, 0, 1, term(1, 3, 3, d_data=8), buf, buf, None) == 0
