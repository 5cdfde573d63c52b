"""The bucket plan of the geometry depth sort (csrc/depth_sort_plan.hpp; csrc/binning.hip launch_depth_bucket_sort) on the GPU:
tests/depth_bucket_cases.py lists the cases, tests/test_depth_bucket_scenes.py proves on the host that each has the buckets it is named
for.  Every case runs four views on a workload of its own -- the fourth is sorted under the speculated byte, by the bucket plan -- and
every view's num_rendered, radii, instance list, tile ranges (exact) and images are compared with the oracle (the checks of
tests/test_gpu_depth_offsets.py).  The same fourth view sorted by the LSD passes (SVGIR_DEPTH_SORT=lsd, a child process: the switch is
read once) gives the same instance list and ranges; the oversize paths of the bucket kernel run in a second child under
SVGIR_DEPTH_BUCKET_CAP=256."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_bucket_cases as bk
import test_gpu_binning as tb
import test_gpu_parity as tp
from oracle import oracle as orc
from svgir_harness import runner, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCOPE0 = 8600       # workload scopes 8600 ... : one per case
KEY_SPEC = os.environ.get("SVGIR_NO_KEY_SPEC") is None
_oracles = {}       # id(scene dict) is not stable across builds: keyed by the case's name


def _oracle(key, sc, variant="rgss"):
    """(OracleRun, R) of a scene, computed once."""
    if key not in _oracles:
        o = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS)
        R = o.forward()
        assert R == sc["plan"]["R"]
        _oracles[key] = (o, R)
    return _oracles[key]


def _view(sct, o, R, variant="rgss"):
    raw = runner.forward_raw(sct, variant)
    torch.cuda.synchronize()
    tb._where(raw, o, R)
    tp._check_forward(raw, o, R, variant)          # num_rendered, radii (exact), the images
    tp._check_binning_raw(raw, o, R)               # instance list, ranges (exact), n_contrib
    return raw


def check_case(case, scope):
    """Four views of one case against the oracle + the speculation statistics; returns the fourth view."""
    from gaussian_renderer import _native
    sc = bk.build(case)
    o, R = _oracle(("case", scope), sc)
    _native.reset_workload_history(scope)
    sct = runner.to_torch(sc, tp._dev())
    before = _native.speculation_stats()
    with _native.workload_scope(scope):
        for view in range(case["views"]):
            try:
                raw = _view(sct, o, R)
            except AssertionError as e:
                raise AssertionError(f"view {view + 1} of {case['views']}: {e}") from e
    after = _native.speculation_stats()
    if KEY_SPEC:
        d = {k: after[k] - before[k] for k in after}
        assert d["forwards"] == 4 and d["rerun_capacity"] == 0 and d["rerun_depth_key"] == 0, d
        assert d["three_pass"] == (1 if case["one_byte"] else 0), d      # (counts every view sorted under the speculated byte, whichever plan)
    return raw


def _child(which, env, outdir):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "depth_bucket_paths.py"), which, str(outdir)], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "failed: 0" in out.stdout, out.stdout[-3000:] + out.stderr[-1500:]
    return out.stdout


@pytest.fixture(scope="module")
def lsd_views(built, tmp_path_factory):
    """<case>.npz of every case, CASES and FORCED: the fourth view's instance list and ranges as the LSD passes sort it."""
    d = tmp_path_factory.mktemp("lsd")
    out = _child("lsd", dict(SVGIR_DEPTH_SORT="lsd"), d)
    assert f"cases: {len(bk.CASES) + len(bk.FORCED)}" in out
    return d


def _same_as_lsd(raw, lsd_views, name):
    ref = np.load(os.path.join(lsd_views, name + ".npz"))
    assert np.array_equal(raw["point_list"], ref["point_list"]) and np.array_equal(raw["ranges"], ref["ranges"]), "differs from the LSD passes' view"


@pytest.mark.parametrize("name", list(bk.CASES))
def test_case_matches_the_oracle_and_the_lsd_passes(built, lsd_views, name):
    raw = check_case(bk.CASES[name], SCOPE0 + list(bk.CASES).index(name))
    _same_as_lsd(raw, lsd_views, name)


def test_forced_paths_in_a_child_process(built, lsd_views, tmp_path):
    """SVGIR_DEPTH_BUCKET_CAP=256: in LDS at the capacity, oversize with equal keys, two and three chunks through global memory, ties
    across the chunk boundaries -- each against the oracle in the child, and against the LSD passes' view here."""
    out = _child("cap", dict(SVGIR_DEPTH_BUCKET_CAP=str(bk.FORCED_CAP)), tmp_path)
    assert f"cases: {len(bk.FORCED)}" in out
    for name in bk.FORCED:
        _same_as_lsd(np.load(os.path.join(tmp_path, name + ".npz")), lsd_views, name)


def test_all_culled_view_on_a_speculating_workload(built):
    """Three full views arm the speculation; then no surfel is visible: no bucket has a key, R = 0 and span 0 come from the pass's first
    workgroup, inside the capacity guessed from the views before; and the view after it is right again."""
    from gaussian_renderer import _native
    full = scenes.binning_scene("rgss", **bk.EMPTY_BETWEEN)
    none = scenes.binning_scene("rgss", **dict(bk.EMPTY_BETWEEN, n_culled=bk.EMPTY_BETWEEN["P"]))
    scope = SCOPE0 + 100
    _native.reset_workload_history(scope)
    before = _native.speculation_stats()
    with _native.workload_scope(scope):
        for i, sc in enumerate((full, full, full, none, full)):
            o, R = _oracle(("empty", sc is none), sc)
            raw = _view(runner.to_torch(sc, tp._dev()), o, R)
            if sc is none:
                assert R == 0 and raw["num_rendered"] == 0 and not raw["ranges"].any() and not raw["radii"].any()
            else:
                assert R > sc["means3D"].shape[0]
    after = _native.speculation_stats()
    d = {k: after[k] - before[k] for k in after}
    assert d["rerun_capacity"] == 0 and d["rerun_depth_key"] == 0, d
    if KEY_SPEC:
        assert d["three_pass"] >= 1, d


def test_svgss_backward_rows_follow_the_offsets(built):
    """R_IBASE of the records -- the first gradient row of a surfel -- comes from the offsets the bucket kernel writes: three forwards arm
    the speculation, the fourth view runs forward and backward.  Gradients against the oracle, non-zero on the four leaves."""
    from gaussian_renderer import _native
    sc = scenes.binning_scene("svgss", **bk.SVGSS)
    scope = SCOPE0 + 101
    _native.reset_workload_history(scope)
    before = _native.speculation_stats()
    with _native.workload_scope(scope):
        o, R = _oracle(("svgss",), sc, "svgss")
        sct = runner.to_torch(sc, tp._dev())
        for _ in range(3):
            _view(sct, o, R, "svgss")
        grads = scenes.upstream_grads(sc, "svgss", seed=19)
        out, leaves, o2, R2 = tp._run_both(sc, "svgss", grads)
        assert R2 == R == sc["plan"]["R"]
        tp._check_forward(out, o2, R2, "svgss")
        tp._check_binning(sc, "svgss", o2, R2)
        tp._check_backward(leaves, o2, "svgss", exact=tp._exact_grads(sc, "svgss", grads, R2))
        for k in ("means3D", "opacities", "features", "vfeatures"):
            assert float(leaves[k].grad.abs().max()) > 0, k
    after = _native.speculation_stats()
    if KEY_SPEC:
        d = {k: after[k] - before[k] for k in after}
        assert d["three_pass"] >= 1 and d["rerun_depth_key"] == 0 and d["rerun_capacity"] == 0, d
