"""The single-pass tile sort (csrc/binning.hip launch_tile_sort12), whose kernels bound their work by the instance count they read on
the device, on the GPU against the oracle: tests/tile_bin_cases.py lists the cases, tests/test_tile_bin_scenes.py proves on the host that
each has the property it is named for.  num_rendered, radii, the instance list and the tile ranges are compared for equality
(tests/test_gpu_parity.py).

Every forward-only case is rendered four times on a workload scope of its own: the first view gets the exact instance capacity, the later
ones a speculative capacity above the count, so the count is read on the device and key blocks past it exist."""
import pytest
import torch

import tile_bin_cases as tb
import test_gpu_binning as gb
import test_gpu_parity as tp
from oracle import oracle as orc
from svgir_harness import runner, scenes

pytestmark = pytest.mark.gpu
SCOPE0 = 7600       # workload scopes 7600 ... : one per case
VIEWS = 4


def check_case(name):
    """One case of tests/tile_bin_cases.py against the oracle on a workload of its own."""
    from gaussian_renderer import _native
    case = tb.CASES[name]
    variant = case["variant"]
    sc = scenes.binning_scene(variant, **case["kw"])
    scope = SCOPE0 + list(tb.CASES).index(name)
    _native.reset_workload_history(scope)
    with _native.workload_scope(scope):
        if case["backward"]:
            grads = scenes.upstream_grads(sc, variant, seed=19)
            out, leaves, o, R = tp._run_both(sc, variant, grads)
            assert R == sc["plan"]["R"]
            tp._check_forward(out, o, R, variant)
            tp._check_binning(sc, variant, o, R)
            tp._check_backward(leaves, o, variant, exact=tp._exact_grads(sc, variant, grads, R))
            for k in ("means3D", "opacities", "features", "vfeatures"):      # a wrong first-instance record puts gradients on the wrong surfels
                assert float(leaves[k].grad.abs().max()) > 0, k
            return
        o = orc.OracleRun(sc, orc.RGSS)
        R = o.forward()
        assert R == sc["plan"]["R"]
        sct = runner.to_torch(sc, tp._dev())
        before = _native.speculation_stats()
        for view in range(VIEWS):
            raw = runner.forward_raw(sct, variant)
            torch.cuda.synchronize()
            try:
                gb._where(raw, o, R)
                tp._check_forward(raw, o, R, variant)          # num_rendered, radii (exact), the images
                tp._check_binning_raw(raw, o, R)               # instance list, ranges (exact), n_contrib
            except AssertionError as e:
                raise AssertionError(f"view {view + 1} of {VIEWS}: {e}") from e
            del raw
        after = _native.speculation_stats()
    d = {k: after[k] - before[k] for k in after}
    assert d["forwards"] == VIEWS and d["rerun_capacity"] == 0, d


@pytest.mark.parametrize("name", list(tb.CASES))
def test_tile_bin_case_matches_the_oracle(built, name):
    check_case(name)


def test_count_beyond_the_speculative_capacity_is_rerun(built):
    """Two views of equal surfel count on one workload; the second has three whole-grid splats, so its instance count lies beyond the
    capacity guessed from the first: the speculative launch must not produce a position at or past its capacity (the blob ends there), the
    dependent stages run again for the exact count, and both lists are exact."""
    from gaussian_renderer import _native
    scope = SCOPE0 + 900
    _native.reset_workload_history(scope)
    before = _native.speculation_stats()
    with _native.workload_scope(scope):
        for kw in tb.RERUN:
            sc = scenes.binning_scene("rgss", **kw)
            o = orc.OracleRun(sc, orc.RGSS)
            R = o.forward()
            assert R == sc["plan"]["R"]
            raw = runner.forward_raw(runner.to_torch(sc, tp._dev()), "rgss")
            torch.cuda.synchronize()
            gb._where(raw, o, R)
            tp._check_forward(raw, o, R, "rgss")
            tp._check_binning_raw(raw, o, R)
    after = _native.speculation_stats()
    assert after["forwards"] - before["forwards"] == 2
    assert after["rerun_capacity"] - before["rerun_capacity"] == 1

