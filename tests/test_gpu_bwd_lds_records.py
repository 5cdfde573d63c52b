"""The record path of the plain backward composite (csrc/render_bwd_plain.hip) on the scenes of tests/bwd_lds_records_cases.py: records
that the LDS-DMA gathers from both ends of a 70 000-surfel model, segments with 5, 3 and 2 pad slots that replay a nearly opaque record,
and a launch with more segments than waves, so that waves reuse their record buffer for a second segment.
tests/test_bwd_lds_records_scenes.py checks on the host that the scenes hold what they claim.

Every case: forward images and ALL per-Gaussian gradients against the CPU oracle with the fp64-anchored budgets of
tests/test_gpu_parity.py, finite gradients, and exactly zero gradient rows for the surfels without a blend weight.  Then the same call
twice on `far_ids`, within the noise bound tests/test_gpu_concurrency.py grants rgss."""
import functools

import numpy as np
import pytest
import torch

import bwd_lds_records_cases as lc
import bwd_rows_cases as rc
import test_gpu_blended_only as tb
import test_gpu_parity as tp
from oracle import oracle as orc
from svgir_harness import runner

pytestmark = pytest.mark.gpu
CASES = [("far_ids", v, s) for v, s in rc.WIDTHS] + [("ragged", v, s) for v, s in lc.RAGGED_WIDTHS] + [("second_item", "rgss", 5)]
IDS = [f"{n}_{v}_S{s}" for n, v, s in CASES]


@functools.lru_cache(maxsize=None)
def _host(name, variant, S):
    """(scene, upstream gradients, fp32 oracle after forward + backward, fp64 gradients): computed once, shared, never modified."""
    sc = lc.build(name, variant, S)
    grads = rc.upstream(sc, variant)
    o = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS)
    R = o.forward()
    o.backward(grads["color"], grads["normal"], grads["depth"], grads["opacity"], grads["feature"], grads.get("vfeature"))
    return sc, grads, o, R, tp._exact_grads(sc, variant, grads, R)


@pytest.mark.parametrize("name,variant,S", CASES, ids=IDS)
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
    P = len(w)
    for k, t in leaves.items():
        if t.grad is None:
            continue
        assert torch.isfinite(t.grad).all(), k
        g = t.grad.cpu().numpy()
        if g.shape[:1] == (P,) and g.size:
            assert (g.reshape(P, -1)[~(w > 0)] == 0).all(), f"{k}: non-zero rows of surfels without a blend weight"


def test_the_same_call_twice_on_far_ids(built):
    """Float atomics meet in any order: two runs of one call differ by `noise`, a third lies within the bound
    tests/test_gpu_concurrency.py grants rgss (4 noise + 1e-6 max|tensor|)."""
    sc, grads, o, R, _ = _host("far_ids", "rgss", 5)
    sct = runner.to_torch(sc, tp._dev())
    fw = runner.forward_raw(sct, "rgss")
    assert fw["num_rendered"] == R
    a, a2, b = (tb._backward(sct, "rgss", fw, grads) for _ in range(3))
    for k in a:
        if not a[k].size:
            continue
        assert np.isfinite(b[k]).all(), k
        noise = float(np.abs(a[k] - a2[k]).max())
        d = float(np.abs(a[k] - b[k]).max())
        bound = 4.0 * noise + 1e-6 * float(np.abs(a[k]).max()) + 1e-12
        print(f"{k}: third run differs by {d:.3e}, noise {noise:.3e}, bound {bound:.3e}")
        assert d <= bound, f"{k}: {d:.3e} > {bound:.3e}"
