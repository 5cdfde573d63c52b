"""The backward's per-Gaussian kernel (csrc/geom_bwd.hip) processes a surfel only if the forward blended it (out_weights > 0), also
where no blended list is built, and compacts those surfels inside each wave.  Scenes: tests/blended_only_cases.py.

On the host (no GPU): the scenes hold the classes they are built for, by the CPU oracle's own forward.
On the GPU, through the `_C` bindings (one forward, several backwards on it):
  * rows of blended surfels: every per-Gaussian gradient tensor against the oracle, budgets of tests/test_gpu_parity.py;
  * rows of all other surfels: exactly zero in every tensor;
  * the same backward without the weights, without the clear_base hint, on a NaN-filled scratch, and a second time: the same result.
"The same": svgss sums its gradient rows in a fixed order, so `==`.  rgss accumulates with float atomics: two runs WITHOUT weights give
`spread`, their difference per tensor, and a result passes if it lies within spread + ATOMIC_ULPS * eps * max|tensor| of the first of
them.  The second term: on these tiny scenes two identical calls are often bit-identical (spread 0) while anything that shifts the
timing -- a side-stream clear, another scratch -- lets the composite's atomics meet in another order.  An entry of a packed row is the
sum of at most 64 addends here (one per 8 x 8 sub-tile of the 64 x 64 image), so two orders differ by at most 63 eps of the sum of
their magnitudes; the factor 16 on top covers that sum exceeding the entry (cancellation) and the few products and sums by which geom_bwd
turns a row into a gradient.  1024 eps = 6.1e-5 of the tensor's largest entry is below the 1e-4 the parity tests grant any fp32
evaluation; a row that is wrong -- not cleared, not written, another surfel's -- is off by its own size, and the oracle comparison
and the exact zeros of the unblended rows hold besides."""
import functools

import numpy as np
import pytest
import torch

import blended_only_cases as bc
import test_gpu_parity as tp
from oracle import oracle as orc
from svgir_harness import runner, scenes

gpu = pytest.mark.gpu
ATOMIC_ULPS = 1024     # (module docstring)
EPS = float(np.finfo(np.float32).eps)
# ("rgss_generic": S = 2 has no specialised composite -- the run-time-width kernels add into the gradient tensors themselves)
CASES = [("rgss", 300), ("rgss", 65), ("rgss", 1), ("svgss", 300), ("rgss_generic", 300)]
IDS = [f"{v}_P{p}" for v, p in CASES]
ORACLE_KEYS = dict(means2D="means2D", colors="colors", opacity="opacity", means3D="means3D", features="features", vfeatures="vfeatures",
                   cov3D="cov3D", sh="sh", scales="scales", rotations="rotations")
RGSS_OUT = ("means2D", "colors", "opacity", "means3D", "features", "cov3D", "sh", "scales", "rotations")
SVGSS_OUT = ("means2D", "colors", "opacity", "means3D", "features", "vfeatures", "cov3D", "sh", "scales", "rotations", "viewmat", "projmat",
             "campos")


@functools.lru_cache(maxsize=None)
def _host(variant, P, nothing=False):
    """(scene, upstream gradients, oracle after forward + backward): computed once, shared, never modified."""
    sc = bc.build(P, variant, nothing=nothing)
    variant = bc.kernel_variant(variant)
    grads = scenes.upstream_grads(sc, variant, seed=7)
    o = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS)
    o.forward()
    o.backward(grads["color"], grads["normal"], grads["depth"], grads["opacity"], grads["feature"], grads.get("vfeature"))
    return sc, grads, o


# ---- the scenes (host) ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant,P", [c for c in CASES if c[1] > 1], ids=[i for i, c in zip(IDS, CASES) if c[1] > 1])
def test_scene_holds_every_class(variant, P):
    sc, _, o = _host(variant, P)
    cl = bc.classes(sc, o)
    k = np.array(list(sc["kinds"]))
    for name in ("culled", "occluded", "faint", "blended"):
        assert cl[name].any(), name
    # ... and they are the surfels built for it
    assert np.array_equal(cl["culled"], k == "c") and np.array_equal(cl["faint"], k == "f")
    assert np.array_equal(cl["occluded"], k == "o") and np.array_equal(cl["blended"], (k == "b") | (k == "w"))
    assert cl["idle_waves"] == [64], cl["idle_waves"]
    if P == 300:   # one wave's two chunks hold more than 64 surfels to process: geom_bwd's body runs twice, with and without weights
        assert cl["blended"][128:256].sum() > 64 and (~cl["culled"])[128:256].sum() > 64
    assert o.num_rendered > 0


def test_scene_single_surfel_is_blended():
    sc, _, o = _host("rgss", 1)
    assert bc.classes(sc, o)["blended"].all() and o.num_rendered > 0


@pytest.mark.parametrize("variant", ["rgss", "svgss"])
def test_scene_nothing_renders_nothing(variant):
    sc, _, o = _host(variant, 300, True)
    assert o.num_rendered == 0 and bc.classes(sc, o)["culled"].all()


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

def _backward(sct, variant, fw, grads, weights=True):
    """One `_C` backward on the forward `fw` (runner.forward_raw); {name: tensor}."""
    variant = bc.kernel_variant(variant)
    dev = sct["means3D"].device
    st = runner.settings(sct, variant)
    empty = torch.empty(0, dtype=torch.float32, device=dev)
    up = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in grads.items()}
    gb, bb, ib = fw["blobs"]
    kw = dict(out_weights=fw["weights"] if weights else None)
    if variant == "svgss":
        from gaussian_renderer.svgss_rasterization import _C
        res = _C.rasterize_gaussians_backward(st.bg, sct["means3D"], sct["features"], sct["vfeatures"], fw["radii"], empty, sct["scales"],
                                              sct["rotations"], st.scale_modifier, empty, st.viewmatrix, st.projmatrix, st.prcppoint,
                                              st.patch_bbox, st.tanfovx, st.tanfovy, up["color"], up["normal"], up["depth"], up["opacity"],
                                              up["feature"], up["vfeature"], sct["shs"], st.sh_degree, st.campos, gb, fw["num_rendered"], bb, ib,
                                              False, st.config, **kw)
        names = SVGSS_OUT
    else:
        from gaussian_renderer.rgss_rasterization import _C
        res = _C.rasterize_gaussians_backward(st.bg, sct["means3D"], sct["features"], fw["radii"], empty, sct["scales"], sct["rotations"],
                                              st.scale_modifier, empty, st.viewmatrix, st.projmatrix, st.tanfovx, st.tanfovy, up["color"],
                                              up["normal"], up["opacity"], up["depth"], up["feature"], sct["shs"], st.sh_degree, st.campos, gb,
                                              fw["num_rendered"], bb, ib, True, False, **kw)
        names = RGSS_OUT
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in zip(names, res)}


@functools.lru_cache(maxsize=None)
def _gpu(variant, P, nothing=False):
    """The GPU side of a case: the forward, two backwards without weights and their spread (computed once, shared)."""
    sc, grads, _ = _host(variant, P, nothing)
    sct = runner.to_torch(sc, tp._dev())
    fw = runner.forward_raw(sct, bc.kernel_variant(variant))
    base = [_backward(sct, variant, fw, grads, weights=False) for _ in range(2)]
    spread = {k: float(np.abs(base[0][k] - base[1][k]).max()) if base[0][k].size else 0.0 for k in base[0]}
    return sct, fw, base, spread


def _assert_same(variant, got, base, spread, what):
    for k in got:
        assert np.isfinite(got[k]).all(), f"{what}: {k} is not finite"
    if bc.kernel_variant(variant) == "svgss":
        for k in got:
            assert np.array_equal(got[k], base[0][k]), f"{what}: {k} differs"
        return
    for k in got:
        if not got[k].size:
            continue
        d = float(np.abs(got[k] - base[0][k]).max())
        bound = spread[k] + ATOMIC_ULPS * EPS * float(np.abs(base[0][k]).max())
        print(f"{what}: {k} differs by {d:.3e}, bound {bound:.3e} (spread {spread[k]:.3e})")
        assert d <= bound, f"{what}: {k} differs by {d:.3e} from the run without weights, bound {bound:.3e}"


def _assert_unblended_zero(got, blended, what):
    P = len(blended)
    for k, t in got.items():
        if t.shape[:1] == (P,) and t.size:
            rows = t.reshape(P, -1)[~blended]
            assert (rows == 0).all(), f"{what}: {k} has non-zero rows of unblended surfels"


@gpu
@pytest.mark.parametrize("variant,P", CASES, ids=IDS)
def test_blended_rows_match_the_oracle_and_the_others_are_zero(built, variant, P):
    sc, grads, o = _host(variant, P)
    sct, fw, base, spread = _gpu(variant, P)
    assert fw["num_rendered"] == o.num_rendered
    blended = fw["weights"].cpu().numpy().reshape(-1) > 0
    assert np.array_equal(blended, bc.classes(sc, o)["blended"])
    got = _backward(sct, variant, fw, grads)
    gr = o.grads()
    for k, ok in ORACLE_KEYS.items():
        if k in got and got[k].size:
            ref = np.asarray(gr[ok]).reshape(P, -1)
            tp._cmp("grad_" + k, got[k].reshape(P, -1)[blended], ref[blended], flip_frac=tp.GRAD_FLIP_FRAC)
    _assert_unblended_zero(got, blended, "with weights")
    _assert_unblended_zero(base[0], blended, "without weights")


@gpu
@pytest.mark.parametrize("variant,P", CASES, ids=IDS)
def test_with_weights_equals_without(built, variant, P):
    _, grads, _ = _host(variant, P)
    sct, fw, base, spread = _gpu(variant, P)
    _assert_same(variant, _backward(sct, variant, fw, grads), base, spread, "with weights")


@gpu
@pytest.mark.parametrize("variant,P", CASES, ids=IDS)
def test_without_the_clear_hint(built, variant, P, monkeypatch):
    """svgir_backward clears the gradient tensors one by one on its side stream; geom_bwd runs behind the join."""
    from gaussian_renderer import _native
    _, grads, _ = _host(variant, P)
    sct, fw, base, spread = _gpu(variant, P)
    monkeypatch.setattr(_native, "CLEAR_HINT", False)
    got = _backward(sct, variant, fw, grads)
    _assert_same(variant, got, base, spread, "CLEAR_HINT off")
    _assert_unblended_zero(got, fw["weights"].cpu().numpy().reshape(-1) > 0, "CLEAR_HINT off")


def _poisoned_run_backward(dev, p, g, R, radii, geomBuffer, binningBuffer, imageBuffer, scratch_bytes):
    """_binding.run_backward with a scratch the caller made: every float of it NaN."""
    from gaussian_renderer import _native as N
    rad = radii.contiguous()
    scratch = torch.full(((scratch_bytes + 3) // 4,), float("nan"), dtype=torch.float32, device=dev)
    N.guarded(dev, "backward", N.lib.svgir_backward, p, g, int(R), rad.data_ptr(), geomBuffer.data_ptr(), binningBuffer.data_ptr(),
              binningBuffer.numel(), imageBuffer.data_ptr(), scratch.data_ptr(), scratch_bytes, N.stream_ptr(dev))


@gpu
@pytest.mark.parametrize("variant,P", CASES, ids=IDS)
def test_nan_filled_scratch(built, variant, P, monkeypatch):
    """Whatever the caller's scratch holds, nothing of it may reach a result: the library clears what it reads."""
    from gaussian_renderer import _binding
    _, grads, _ = _host(variant, P)
    sct, fw, base, spread = _gpu(variant, P)
    monkeypatch.setattr(_binding, "run_backward", _poisoned_run_backward)
    blended = fw["weights"].cpu().numpy().reshape(-1) > 0
    for weights in (True, False):
        got = _backward(sct, variant, fw, grads, weights=weights)
        _assert_same(variant, got, base, spread, f"NaN scratch, weights={weights}")
        _assert_unblended_zero(got, blended, f"NaN scratch, weights={weights}")


@gpu
@pytest.mark.parametrize("variant,P", CASES, ids=IDS)
def test_second_backward_on_the_same_forward(built, variant, P):
    _, grads, _ = _host(variant, P)
    sct, fw, base, spread = _gpu(variant, P)
    first = _backward(sct, variant, fw, grads)
    second = _backward(sct, variant, fw, grads)
    _assert_same(variant, first, base, spread, "first backward")
    _assert_same(variant, second, base, spread, "second backward")
    if bc.kernel_variant(variant) == "svgss":
        for k in first:
            assert np.array_equal(first[k], second[k]), k


@gpu
@pytest.mark.parametrize("variant", ["rgss", "svgss"])
def test_nothing_rendered(built, variant, monkeypatch):
    """R = 0: every weight is zero, every gradient stays at its cleared zero -- with and without the weights, on a NaN-filled scratch."""
    from gaussian_renderer import _binding
    _, grads, o = _host(variant, 300, True)
    sct, fw, base, _ = _gpu(variant, 300, True)
    assert fw["num_rendered"] == 0 == o.num_rendered and float(fw["weights"].abs().max()) == 0
    monkeypatch.setattr(_binding, "run_backward", _poisoned_run_backward)
    for got in base + [_backward(sct, variant, fw, grads), _backward(sct, variant, fw, grads, weights=False)]:
        for k, t in got.items():
            assert (t == 0).all(), k
