"""The instance offsets, the instance count and the visible span from the depth sort's last pass (csrc/binning.hip, the weighted radix
pass) on the GPU, with weights that differ: tests/depth_offsets_cases.py lists the cases, tests/test_depth_offsets_scenes.py proves on
the host that each has the size and the weights it is named for.

One wrong offset scrambles the instance list: num_rendered, radii, the depth-sorted instance list and the tile ranges are compared
with the oracle for exact equality (the checks of tests/test_gpu_parity.py, as tests/test_gpu_binning.py uses them).  Every case has
a workload scope of its own."""
import os

import numpy as np
import pytest
import torch

import depth_offsets_cases as dc
import test_gpu_binning as tb
import test_gpu_parity as tp
from oracle import oracle as orc
from svgir_harness import runner, scenes

pytestmark = pytest.mark.gpu
SCOPE0 = 8200       # workload scopes 8200 ... : one per case
KEY_SPEC = os.environ.get("SVGIR_NO_KEY_SPEC") is None


def _view(sct, o, R, variant="rgss"):
    raw = runner.forward_raw(sct, variant)
    torch.cuda.synchronize()
    tb._where(raw, o, R)
    tp._check_forward(raw, o, R, variant)          # num_rendered, radii (exact), the images
    tp._check_binning_raw(raw, o, R)               # instance list, ranges (exact), n_contrib
    return raw


def _oracle(sc, variant="rgss"):
    o = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS)
    R = o.forward()
    assert R == sc["plan"]["R"]
    return o, R


@pytest.mark.parametrize("name", list(dc.CASES))
def test_case_matches_the_oracle(built, name):
    from gaussian_renderer import _native
    case = dc.CASES[name]
    sc = scenes.binning_scene("rgss", **case["kw"])
    o, R = _oracle(sc)
    if case["R"] is not None:
        assert R == case["R"]
    scope = SCOPE0 + list(dc.CASES).index(name)
    _native.reset_workload_history(scope)
    sct = runner.to_torch(sc, tp._dev())
    before = _native.speculation_stats()
    with _native.workload_scope(scope):
        for view in range(case["views"]):
            try:
                _view(sct, o, R)
            except AssertionError as e:
                raise AssertionError(f"view {view + 1} of {case['views']}: {e}") from e
    after = _native.speculation_stats()
    if case["views"] == 4 and KEY_SPEC:
        d = {k: after[k] - before[k] for k in after}
        assert d["forwards"] == 4 and d["rerun_capacity"] == 0 and d["rerun_depth_key"] == 0, d
        # visible keys that share their top byte: the fourth view is sorted in three passes (its third one weighted); otherwise none is
        assert d["three_pass"] == (1 if len(dc.top_bytes(sc)) == 1 else 0), d


def test_all_culled_view_between_two_that_are_not(built):
    """R = 0 and an empty visible span, published by the pass for an order in which no key weighs anything -- inside the capacity
    guessed from the view before, and the view after it is right again."""
    from gaussian_renderer import _native
    full = scenes.binning_scene("rgss", **dc.EMPTY_BETWEEN)
    none = scenes.binning_scene("rgss", **dict(dc.EMPTY_BETWEEN, n_culled=dc.EMPTY_BETWEEN["P"]))
    runs = {id(sc): _oracle(sc) for sc in (full, none)}
    scope = SCOPE0 + 100
    _native.reset_workload_history(scope)
    before = _native.speculation_stats()
    with _native.workload_scope(scope):
        for sc in (full, none, full):
            o, R = runs[id(sc)]
            raw = _view(runner.to_torch(sc, tp._dev()), o, R)
            if sc is none:
                assert R == 0 and raw["num_rendered"] == 0 and not raw["ranges"].any() and not raw["radii"].any()
            else:
                assert R > sc["means3D"].shape[0]
    after = _native.speculation_stats()
    assert after["rerun_capacity"] == before["rerun_capacity"]


def test_broken_top_byte_speculation_is_rerun_with_four_weighted_passes(built):
    """Three views whose visible keys share their top byte, then one of the same size whose keys do not: its three-pass order (and the
    offsets that came with it) is wrong, the summary the pass publishes says so, and the re-run with four passes matches the oracle."""
    from gaussian_renderer import _native
    one, many = (scenes.binning_scene("rgss", **kw) for kw in dc.BROKEN_SPECULATION)
    scope = SCOPE0 + 101
    _native.reset_workload_history(scope)
    o1, R1 = _oracle(one)
    o2, R2 = _oracle(many)
    t1, t2 = runner.to_torch(one, tp._dev()), runner.to_torch(many, tp._dev())
    before = _native.speculation_stats()
    with _native.workload_scope(scope):
        for _ in range(3):
            _view(t1, o1, R1)
        _view(t2, o2, R2)
    after = _native.speculation_stats()
    if KEY_SPEC:
        d = {k: after[k] - before[k] for k in after}
        assert d["forwards"] >= 4 and d["three_pass"] == 1 and d["rerun_depth_key"] == 1 and d["rerun_capacity"] == 0, d


def test_svgss_backward_rows_follow_the_offsets(built):
    """R_IBASE of the records -- the first gradient row of a surfel -- comes from the offsets: a wrong prefix puts gradient rows on the
    wrong surfels.  Gradients against the oracle, non-zero on the four leaves."""
    from gaussian_renderer import _native
    sc = scenes.binning_scene("svgss", **dc.SVGSS)
    scope = SCOPE0 + 102
    _native.reset_workload_history(scope)
    with _native.workload_scope(scope):
        grads = scenes.upstream_grads(sc, "svgss", seed=19)
        out, leaves, o, R = tp._run_both(sc, "svgss", grads)
        assert R == sc["plan"]["R"]
        tp._check_forward(out, o, R, "svgss")
        tp._check_binning(sc, "svgss", o, R)
        tp._check_backward(leaves, o, "svgss", exact=tp._exact_grads(sc, "svgss", grads, R))
        for k in ("means3D", "opacities", "features", "vfeatures"):
            assert float(leaves[k].grad.abs().max()) > 0, k


@pytest.mark.parametrize("culled", [300, 0])
def test_prefilter_violation_reaches_the_host_with_the_count(built, culled):
    """`prefiltered` set: the violation bit travels in the second host word the pass publishes next to R -- an error with a culled
    surfel, a normal render without."""
    from gaussian_renderer import _native
    from gaussian_renderer.rgss_rasterization import GaussianRasterizer
    kw = dict(dc.CASES["block_edge_above"]["kw"], n_culled=culled)
    sc = scenes.binning_scene("rgss", **kw)
    sct = runner.to_torch(sc, tp._dev())
    st = runner.settings(sct, "rgss")._replace(prefiltered=True)
    args = dict(means3D=sct["means3D"], means2D=torch.zeros_like(sct["means3D"]), opacities=sct["opacities"], shs=sct["shs"],
                scales=sct["scales"], rotations=sct["rotations"], features=sct["features"])
    with _native.workload_scope(SCOPE0 + 103 + (1 if culled else 0)):
        if culled:
            with pytest.raises(RuntimeError, match="filtered although prefiltered"):
                GaussianRasterizer(st)(**args)
        else:
            res = GaussianRasterizer(st)(**args)
            assert res[0] == sc["plan"]["R"]
            assert np.array_equal(res[-1].cpu().numpy(), (dc.weights(sc) > 0) * 3)      # radii: the 0.3 px^2 low-pass alone
    torch.cuda.synchronize()
