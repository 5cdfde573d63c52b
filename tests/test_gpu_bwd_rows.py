"""The plain backward composite (csrc/render_bwd_plain.hip) and its packed gradient rows (common.hpp packed_row_geom) on the scenes of
tests/bwd_rows_cases.py -- consumed counts around the 8-candidate blocks, their pairs and the 64-candidate segments, block pairs of
which one half blends nothing, replays that start past whole blocks, and the first rows of the scratch -- at every width the kernel is
built for.  tests/test_bwd_rows_scenes.py checks on the host that the scenes hold what they claim.

Every case: forward images and ALL per-Gaussian gradients against the CPU oracle with the fp64-anchored budgets of
tests/test_gpu_parity.py, and exactly zero gradient rows for the surfels without a blend weight.  Then, through the `_C` bindings: a
scratch of exactly svgir_backward_scratch_bytes inside a NaN-filled buffer whose guard words stay untouched, and the same call twice
within the noise bound tests/test_gpu_concurrency.py grants rgss."""
import functools

import numpy as np
import pytest
import torch

import bwd_rows_cases as rc
import test_gpu_blended_only as tb
import test_gpu_parity as tp
from oracle import oracle as orc
from svgir_harness import runner

pytestmark = pytest.mark.gpu
GUARD = 64      # guard words (256 bytes) on either side of the scratch: the scratch itself stays 256-byte aligned
RAW_CASES = [("align13", "rgss", 5), ("stack65", "rgss", 5), ("align13", "rgss", 3), ("align5", "svgss", 5), ("stack17", "rgss", 0)]
RAW_IDS = [f"{n}_{v}_S{s}" for n, v, s in RAW_CASES]


@functools.lru_cache(maxsize=None)
def _host(name, variant, S):
    """(scene, upstream gradients, fp32 oracle after forward + backward, fp64 gradients): computed once, shared, never modified."""
    sc = rc.build(name, variant, S)
    grads = rc.upstream(sc, variant)
    o = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS)
    R = o.forward()
    o.backward(grads["color"], grads["normal"], grads["depth"], grads["opacity"], grads["feature"], grads.get("vfeature"))
    return sc, grads, o, R, tp._exact_grads(sc, variant, grads, R)


def _assert_unblended_rows_zero(named, blended):
    P = len(blended)
    for k, t in named.items():
        if t is not None and t.shape[:1] == (P,) and t.size:
            assert (t.reshape(P, -1)[~blended] == 0).all(), f"{k}: non-zero rows of surfels without a blend weight"


@pytest.mark.parametrize("variant,S", rc.WIDTHS, ids=[f"{v}_S{s}" for v, s in rc.WIDTHS])
@pytest.mark.parametrize("name", rc.SCENES)
def test_scene_against_the_oracle(built, name, variant, S):
    sc, grads, o, R, exact = _host(name, variant, S)
    out, leaves = runner.render(runner.to_torch(sc, tp._dev()), variant, requires_grad=True)
    runner.backward(out, grads, variant)
    torch.cuda.synchronize()
    assert R > 0
    im = tp._check_forward(out, o, R, variant)
    if variant == "rgss":
        assert np.array_equal(out["n_contrib"].cpu().numpy(), im["n_contrib"])
    tp._check_backward(leaves, o, variant, exact=exact)
    w = out["weights"].cpu().numpy().reshape(-1)
    assert np.array_equal(w > 0, im["weights"].reshape(-1) > 0)
    for k, t in leaves.items():
        if t.grad is not None:
            assert torch.isfinite(t.grad).all(), k
    _assert_unblended_rows_zero({k: (None if t.grad is None else t.grad.cpu().numpy()) for k, t in leaves.items()}, w > 0)


@functools.lru_cache(maxsize=None)
def _raw(name, variant, S):
    """The forward of a raw case through the `_C` binding (computed once, shared)."""
    sc, grads, o, R, _ = _host(name, variant, S)
    sct = runner.to_torch(sc, tp._dev())
    fw = runner.forward_raw(sct, variant)
    assert fw["num_rendered"] == R
    return sct, fw


@pytest.mark.parametrize("name,variant,S", RAW_CASES, ids=RAW_IDS)
def test_scratch_of_exactly_the_reported_size(built, name, variant, S, monkeypatch):
    """The packed rows fit svgir_backward_scratch_bytes: a scratch of exactly that size inside a NaN-filled buffer, the words on either
    side of it untouched afterwards, every gradient right."""
    from gaussian_renderer import _binding, _native as N
    sc, grads, o, R, _ = _host(name, variant, S)
    sct, fw = _raw(name, variant, S)
    P = sc["means3D"].shape[0]
    want = int(N.lib.svgir_backward_scratch_bytes(N.SVGSS if variant == "svgss" else N.RGSS, P, fw["blobs"][1].numel(), sc["W"], sc["H"], S, 0))
    kept = []

    def run_backward(dev, p, g, R_, radii, geomBuffer, binningBuffer, imageBuffer, scratch_bytes):
        assert scratch_bytes == want and scratch_bytes % 4 == 0
        big = torch.full((scratch_bytes // 4 + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
        assert (big.data_ptr() + 4 * GUARD) % 256 == 0
        kept.append((big, scratch_bytes // 4))
        rad = radii.contiguous()
        N.guarded(dev, "backward", N.lib.svgir_backward, p, g, int(R_), rad.data_ptr(), geomBuffer.data_ptr(), binningBuffer.data_ptr(),
                  binningBuffer.numel(), imageBuffer.data_ptr(), big.data_ptr() + 4 * GUARD, scratch_bytes, N.stream_ptr(dev))

    monkeypatch.setattr(_binding, "run_backward", run_backward)
    got = tb._backward(sct, variant, fw, grads)
    assert len(kept) == 1
    big, n = kept[0]
    assert torch.isnan(big[:GUARD]).all() and torch.isnan(big[GUARD + n:]).all(), "the backward wrote outside its scratch"
    blended = fw["weights"].cpu().numpy().reshape(-1) > 0
    gr = o.grads()
    for k, ok in tb.ORACLE_KEYS.items():
        if k in got and got[k].size:
            assert np.isfinite(got[k]).all(), k
            tp._cmp("grad_" + k, got[k].reshape(P, -1)[blended], np.asarray(gr[ok]).reshape(P, -1)[blended], flip_frac=tp.GRAD_FLIP_FRAC)
    _assert_unblended_rows_zero(got, blended)


@pytest.mark.parametrize("name,variant,S", RAW_CASES, ids=RAW_IDS)
def test_the_same_call_twice(built, name, variant, S):
    """Float atomics meet in any order: two runs of one call differ by `noise`, a third lies within the bound
    tests/test_gpu_concurrency.py grants rgss (4 noise + 1e-6 max|tensor|)."""
    _, grads, _, _, _ = _host(name, variant, S)
    sct, fw = _raw(name, variant, S)
    a, a2, b = (tb._backward(sct, variant, fw, grads) for _ in range(3))
    for k in a:
        if not a[k].size:
            continue
        noise = float(np.abs(a[k] - a2[k]).max())
        d = float(np.abs(a[k] - b[k]).max())
        bound = 4.0 * noise + 1e-6 * float(np.abs(a[k]).max()) + 1e-12
        print(f"{k}: third run differs by {d:.3e}, noise {noise:.3e}, bound {bound:.3e}")
        assert d <= bound, f"{k}: {d:.3e} > {bound:.3e}"
