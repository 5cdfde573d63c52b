"""The per-surfel kernels -- csrc/preprocess.hip, csrc/geom_bwd.hip, and csrc/grad_reduce.hip between them -- held to the scenes of
tests/surfel_cases.py (proved on the CPU oracle by tests/test_surfel_edge_inputs.py), element by element.

(a) exact state, every case: radii, num_rendered, the depth-sorted instance list and the tile ranges equal the fp32 oracle's, the images
    pass the forward check of tests/test_gpu_parity.py.  For the cull ladders this is the whole test.
(b) element-wise parity on the lattices, coop_rows and listed: for every blended surfel and gradient tensor
    |gpu - o64| <= 4 max(E32, eps32) rowmax|o64| + FLT_MIN, E32 the fp32 oracle's own largest deviation of that tensor in that case under
    the same normalisation (surfel_cases.row_deviation / e32: the surfel's row of the tensor over the row's max |o64| -- the oracle has no
    per-element sum of absolute pixel contributions).  Rows of surfels that were not blended are exactly zero.
(c) closed forms on the kernel's own outputs (no summation order in them: bounds in eps32):
      dL_dsh[i, k, c] == cf_k(dir_i) (clamped_ic ? 0 : dL_dcolors[i, c]) to 16 eps32 A_k |dL_dcolors| for k < nk (16: the rounding count of
      the longest chain -- normalise 4, cubic monomial 3, bracket 3, constant 1, product 1 -- with margin; the fp32 oracle stays below 4);
      dL_dsh[i, k, :] == 0.0 exactly for k >= nk (SVGIR_POISON: an unwritten element is NaN);  dL_dscales[:, 2] == 0.0 exactly;
      dL_dscales[:, :2] from the returned dL_dcov3D to 16 eps32 of the sum of absolute terms (surfel_cases.scale_grad_from_cov).
(d) M / D and storage-offset twins: images, radii, R bit-identical; gradients bit-identical (svgss) or within the rule of
    tests/test_gpu_blended_only.py (rgss: the spread of two runs + ATOMIC_ULPS eps32 max|.|).
(e) listed: see test_listed.
(f) a second (rgss: third) backward of every case: the same bits (svgss) / within the spread (rgss); no output element is NaN."""
import functools
import time

import numpy as np
import pytest
import torch

import surfel_cases as sf
import test_gpu_parity as tp
from svgir_harness import runner
from test_gpu_blended_only import ATOMIC_ULPS, RGSS_OUT, SVGSS_OUT
from test_surfel_edge_inputs import BACKWARD, LATTICE, LATTICE_IDS

pytestmark = pytest.mark.gpu
EPS, TINY = sf.EPS, sf.TINY
SCOPE = 9400     # the workload scope of this file: its image sizes share no launch-speculation history with other tests
INPUTS = ("means3D", "scales", "rotations", "opacities", "shs", "colors_precomp", "features", "vfeatures", "viewmatrix", "projmatrix",
          "campos", "bg", "patch_bbox", "prcppoint", "config")
SCALARS = ("W", "H", "tanfovx", "tanfovy", "cx", "cy", "sh_degree", "scale_modifier", "backward_geometry", "computer_pseudo_normal")


@pytest.fixture(scope="module", autouse=True)
def _own_history(built):
    from gaussian_renderer import _native
    _native.reset_workload_history(SCOPE)
    with _native.workload_scope(SCOPE):
        yield


def _to_torch(sc):
    """The scene on the GPU; `offset` floats in front of the coefficients inside their storage (a contiguous view the bindings pass on)."""
    sct = runner.to_torch({k: sc[k] for k in INPUTS + SCALARS if k in sc}, tp._dev())
    off = sc.get("offset", 0)
    if off:
        shs = sct["shs"]
        buf = torch.full((off + shs.numel(),), float("nan"), dtype=torch.float32, device=shs.device)
        buf[off:] = shs.reshape(-1)
        sct["shs"] = buf[off:].view(shs.shape)
        assert sct["shs"].is_contiguous() and sct["shs"].data_ptr() % 16 == 4 * off
    elif "shs" in sct:
        assert sct["shs"].data_ptr() % 16 == 0
    return sct


def _backward(sct, variant, fw, grads):
    """One `_C` backward on the forward `fw` (runner.forward_raw) with the forward's weights; {name: array}."""
    dev = sct["means3D"].device
    st = runner.settings(sct, variant)
    empty = torch.empty(0, dtype=torch.float32, device=dev)
    up = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in grads.items()}
    gb, bb, ib = fw["blobs"]
    col, shs = sct.get("colors_precomp", empty), sct.get("shs", empty)
    if variant == "svgss":
        from gaussian_renderer.svgss_rasterization import _C
        res = _C.rasterize_gaussians_backward(st.bg, sct["means3D"], sct["features"], sct["vfeatures"], fw["radii"], col, sct["scales"],
                                              sct["rotations"], st.scale_modifier, empty, st.viewmatrix, st.projmatrix, st.prcppoint,
                                              st.patch_bbox, st.tanfovx, st.tanfovy, up["color"], up["normal"], up["depth"], up["opacity"],
                                              up["feature"], up["vfeature"], shs, st.sh_degree, st.campos, gb, fw["num_rendered"], bb, ib,
                                              False, st.config, out_weights=fw["weights"])
        names = SVGSS_OUT
    else:
        from gaussian_renderer.rgss_rasterization import _C
        res = _C.rasterize_gaussians_backward(st.bg, sct["means3D"], sct["features"], fw["radii"], col, sct["scales"], sct["rotations"],
                                              st.scale_modifier, empty, st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy, up["color"],
                                              up["normal"], up["opacity"], up["depth"], up["feature"], shs, st.sh_degree, st.campos, gb,
                                              fw["num_rendered"], bb, ib, True, False, out_weights=fw["weights"])
        names = RGSS_OUT
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in zip(names, res)}


def _run(sc, variant, grads, runs):
    sct = _to_torch(sc)
    fw = runner.forward_raw(sct, variant)
    return fw, [_backward(sct, variant, fw, grads) for _ in range(runs)]


@functools.lru_cache(maxsize=None)
def _gpu(case):
    """(forward, backwards) of a case of surfel_cases.host: run once, shared.  rgss: three backwards -- the spread of the first two
    is what the third is held to."""
    sc, grads, _, _ = sf.host(case)
    return _run(sc, case[1], grads, 2 if case[1] == "svgss" else 3)


# ---- the checks ------------------------------------------------------------------------------------------------------------------

def _check_state(fw, o32):
    """(a)"""
    assert np.array_equal(fw["radii"].cpu().numpy(), o32.get("radii")), "radii differ from the fp32 oracle's"
    tp._check_binning_raw(fw, o32, o32.num_rendered)
    tp._check_forward(fw, o32, o32.num_rendered, "svgss" if "vfeature" in fw else "rgss")


def _per_surfel(got, P):
    return {k: v.reshape(P, -1) for k, v in got.items() if k in sf.PER_SURFEL and v.size and v.shape[0] == P}


def _check_elementwise(got, g32, g64, rows, what):
    """(b)"""
    P = g64["means3D"].shape[0]
    E = sf.e32(g32, g64, rows)
    for k, a in _per_surfel(got, P).items():
        ref = g64[k].reshape(P, -1)
        bound = 4 * max(E[k], EPS) * np.abs(ref).max(1, keepdims=True) + TINY
        d = np.abs(a.astype(np.float64) - ref)
        worst = float((d[rows] / bound[rows]).max())
        print(f"{what}: {k} E32 {E[k]:.1e}, worst |gpu - o64| / bound {worst:.2f}")
        assert (d[rows] <= bound[rows]).all(), f"{what}: {k} is {worst:.2f} x its bound (E32 {E[k]:.1e}) on surfel {rows[int((d[rows] / bound[rows]).max(1).argmax())]}"


def _check_unblended_zero(got, blended, what):
    P = len(blended)
    for k, a in _per_surfel(got, P).items():
        assert (a[~blended] == 0).all(), f"{what}: {k} has non-zero rows of surfels that were not blended"


def _check_closed_forms(sc, got, clamped, rows, what):
    """(c)"""
    P = len(sc["means3D"])
    assert (got["scales"][:, 2] == 0).all(), f"{what}: dL_dscales[:, 2] under config[0]"
    val, mag = sf.scale_grad_from_cov(sc, got["cov3D"])
    err = float((np.abs(got["scales"][:, :2] - val)[rows] / mag[rows]).max()) / EPS
    print(f"{what}: dL_dscales against dL_dcov3D {err:.2f} eps32")
    assert err <= 16, f"{what}: dL_dscales is {err:.1f} eps32 of the sum of absolute terms from the closed form on dL_dcov3D"
    if "shs" in sc:
        nk = sf.nk_of(sc["sh_degree"])
        dsh = got["sh"].reshape(P, -1, 3)
        assert dsh.shape[1] == sc["shs"].shape[1]
        assert (dsh[:, nk:] == 0).all(), f"{what}: dL_dsh above the active degree is not exactly zero"
        err = sf.sh_identity_error(sc, dsh, got["colors"], clamped, rows)
        print(f"{what}: dL_dsh against dL_dcolors {err:.2f} eps32")
        assert err <= 16, f"{what}: dL_dsh is {err:.1f} eps32 A_k |dL_dcolors| from cf_k(dir) dL_dcolors"


def _check_same(variant, got, base, spread_of, what):
    """(d), (f): `got` against base[0] -- bit for bit (svgss) or within the spread of spread_of[0], spread_of[1] + ATOMIC_ULPS eps32 max|.|"""
    for k in got:
        assert np.isfinite(got[k]).all(), f"{what}: {k} is not finite"
        a, b = got[k], base[0][k]
        if a.ndim == 3 and a.shape != b.shape:     # dL_dsh at another stride: the active coefficients
            n = min(a.shape[1], b.shape[1])
            a, b = a[:, :n], b[:, :n]
        if variant == "svgss":
            assert np.array_equal(a, b), f"{what}: {k} differs"
        elif a.size:
            s0, s1 = spread_of[0][k], spread_of[1][k]
            bound = float(np.abs(s0 - s1).max()) + ATOMIC_ULPS * EPS * float(np.abs(b).max())
            assert float(np.abs(a - b).max()) <= bound, f"{what}: {k} differs by {np.abs(a - b).max():.3e}, bound {bound:.3e}"


# ---- lattices, coop_rows, clamp ladders ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,case", BACKWARD, ids=[b[0] for b in BACKWARD])
def test_state_elements_and_closed_forms(built, name, case):
    sc, grads, o32, o64 = sf.host(case)
    variant = case[1]
    fw, runs = _gpu(case)
    _check_state(fw, o32)
    P = len(sc["means3D"])
    blended = fw["weights"].cpu().numpy().reshape(-1) > 0
    assert np.array_equal(blended, o32.get("out_weights") > 0)
    rows = np.nonzero(blended)[0]
    c32 = o32.get("clamped").reshape(-1, 3) > 0
    agree = (c32 == (o64.get("clamped").reshape(-1, 3) > 0)).all(1)     # (all but the threshold surfels of a clamp ladder)
    for i, got in enumerate(runs):
        for k, a in got.items():
            assert not np.isnan(a).any(), f"{name} run {i}: {k} holds NaN"
        _check_elementwise(got, o32.grads(), o64.grads(), rows[agree[rows]], f"{name} run {i}")
        _check_unblended_zero(got, blended, f"{name} run {i}")
        _check_closed_forms(sc, got, c32, rows, f"{name} run {i}")
    _check_same(variant, runs[-1], runs, runs, f"{name}: repeated backward")     # (f)
    if case[0] == "colors":
        assert runs[0]["sh"].size == 0 or (runs[0]["sh"] == 0).all()


TWINS = [(i, c) for i, c in zip(LATTICE_IDS, LATTICE) if sf.twin_of(*c[1:])]


@pytest.mark.parametrize("name,row", TWINS, ids=[t[0] for t in TWINS])
def test_stride_and_offset_twins(built, name, row):
    """(d)"""
    variant = row[0]
    fw, runs = _gpu(("lattice",) + row)
    fw2, runs2 = _gpu(("lattice", variant) + sf.twin_of(*row[1:]))
    assert fw["num_rendered"] == fw2["num_rendered"]
    for k in ("radii", "color", "normal", "depth", "opacity", "feature") + (("vfeature",) if variant == "svgss" else ()):
        assert torch.equal(fw[k], fw2[k]), f"{name}: {k} differs from the twin's"
    assert torch.equal(fw["weights"] > 0, fw2["weights"] > 0)     # (the weights themselves are accumulated with float atomics)
    assert np.array_equal(fw["point_list"], fw2["point_list"]) and np.array_equal(fw["ranges"], fw2["ranges"])
    _check_same(variant, runs[0], runs2, runs, f"{name} against its twin")


# ---- cull ladders -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,variant", sf.CULL_CASES, ids=[f"{k}_{v}" for k, v in sf.CULL_CASES])
def test_cull_ladder(built, kind, variant):
    """(a) on 33 surfels whose parameter steps through consecutive fp32 values across one decision of the preprocess."""
    sc = sf.cull_ladder(kind, variant)
    o32 = sf.oracle(sc, variant)
    fw = runner.forward_raw(_to_torch(sc), variant)
    torch.cuda.synchronize()
    got, want = fw["radii"].cpu().numpy(), o32.get("radii")
    assert np.array_equal(got, want), f"{kind}: radii {got} against the fp32 oracle's {want} (parameter {sc['ladder']})"
    _check_state(fw, o32)


# ---- list sizes ---------------------------------------------------------------------------------------------------------------------

# (variant, P, M, D).  api.hip: with the forward's weights the per-Gaussian kernels walk a blended LIST from kListMinPRows = 50 000
# (svgss, gradient rows) / kListMinP = 400 000 (rgss) surfels on -- geom_bwd_kernel<1>, grad_reduce with a list; below, geom_bwd_kernel<2>
# tests the weights itself.  grad_reduce.hip: grad_reduce_kernel<1> below P = 500 000, <2> from there, <4> from 1 000 000.  The list holds
# 61 surfels: the last wave of <2> sums one Gaussian, the last of <4> one of four (first + k < n, list[min(first + k, n - 1)]).
LISTED = [("svgss", 49_999, 1, 0), ("svgss", 49_999, 16, 1), ("svgss", 50_000, 1, 0), ("svgss", 500_000, 1, 0), ("svgss", 1_000_000, 1, 0),
          ("rgss", 399_999, 16, 2), ("rgss", 400_000, 16, 2)]
_listed_base = {}


def _listed_run(variant, P, M, D):
    sc = sf.listed(variant, P, M, D)
    grads = sf.br.upstream(sc, variant)
    fw, runs = _run(sc, variant, grads, 2 if variant == "svgss" else 3)
    return sc, grads, fw, runs


@pytest.mark.parametrize("variant,P,M,D", LISTED, ids=[f"{v}_P{p}_M{m}" for v, p, m, _ in LISTED])
def test_listed(built, variant, P, M, D):
    """(e) rows of the blended surfels: bit-identical (svgss) to the same scene at the smallest P -- no list, GK = 1 --, within the
    spread for rgss; all other rows exactly zero; every blended row, the wide surfels' too (more than 16 tiles each: the `rest` loop
    of grad_reduce, three ballot rounds), held to (b) and (c); exact state against the fp32 oracle at every P."""
    t0 = time.perf_counter()
    sc, grads, fw, runs = _listed_run(variant, P, M, D)
    o32 = sf.oracle(sc, variant, grads=grads)
    _check_state(fw, o32)
    blended = fw["weights"].cpu().numpy().reshape(-1) > 0
    assert np.array_equal(blended, sc["blended"])
    rows = np.nonzero(blended)[0]
    for i, got in enumerate(runs):
        for k, a in got.items():
            assert not np.isnan(a).any(), f"run {i}: {k} holds NaN"
        _check_unblended_zero(got, blended, f"listed P {P} run {i}")
        _check_closed_forms(sc, got, o32.get("clamped").reshape(-1, 3) > 0, rows, f"listed P {P} run {i}")
    w = sc["where"]
    core = lambda got: {k: a[w] for k, a in got.items() if a.shape[:1] == (P,)}
    P0 = min(p for v, p, m, _ in LISTED if v == variant and m == M)
    if P == P0:
        o64 = sf.oracle(sc, variant, fp64=True, grads=grads)
        for i, got in enumerate(runs):
            _check_elementwise(got, o32.grads(), o64.grads(), rows, f"listed P {P} run {i}")
        _listed_base[(variant, M)] = [core(g) for g in runs]
    else:
        if (variant, M) not in _listed_base:     # (this case run alone)
            _listed_base[(variant, M)] = [core(g) for g in _listed_run(variant, P0, M, D)[3]]
        base = _listed_base[(variant, M)]
        _check_same(variant, core(runs[0]), base, base, f"listed P {P} against P {P0}")
    mine = [core(g) for g in runs]
    _check_same(variant, mine[-1], mine, mine, f"listed P {P}: repeated backward")
    print(f"listed {variant} P {P}: {time.perf_counter() - t0:.2f} s")
