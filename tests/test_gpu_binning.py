"""The binning stage (csrc/binning.hip: depth sort, offsets scan, emit, tile sort, tile ranges, sub-tile order) on the GPU, AT the sizes
where its code changes behaviour -- tests/binning_cases.py lists them; tests/test_binning_scenes.py proves on the host that every case
has the size it is named for and that the oracle's integer state equals an independent numpy construction.

Everything the binning produces is an integer: num_rendered, radii, the depth-sorted instance list and the tile ranges are compared with
the oracle for exact equality; n_contrib and the images with the helpers and budgets of tests/test_gpu_parity.py.  Cases with 32 767
surfels or more are rendered four times on one workload: the first view gets the exact instance capacity, the later ones a speculative
capacity above the count (the count is then read on the device), the fourth sorts the depth keys in three passes where they share their
top byte.  Every case has its own workload scope, so that neighbouring sizes (1023 / 1024 / 1025) do not feed each other's guesses.
The switches that are read once per process (SVGIR_TILE_SORT12, SVGIR_FWD_FILL, SVGIR_FWD_XCD) run in child processes
(scripts/binning_paths.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import binning_cases as bc
import test_gpu_parity as tp
from oracle import oracle as orc
from svgir_harness import cameras, runner, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCOPE0 = 7000       # workload scopes 7000 ... : one per case


def _where(raw, o, R):
    """Names the first instance at which the list differs from the oracle's (its tile, and the key blocks it falls in)."""
    if raw["num_rendered"] != R:
        return
    a, b = raw["point_list"], o.get("point_list")[:R]
    bad = np.nonzero(a != b)[0]
    if len(bad):
        i = int(bad[0])
        rg = o.get("ranges").reshape(-1, 2)
        tile = int(np.searchsorted(np.maximum.accumulate(rg[:, 1]), i, side="right"))     # (empty tiles are (0, 0))
        raise AssertionError(f"instance list differs at {len(bad)} of {R} positions, first at {i} (tile {tile}; key block of 1024: {i // 1024}, of 2048: "
                             f"{i // 2048}, of 4096: {i // 4096}; group of 32768: {i // 32768}, of 131072: {i // 131072}): {a[i]} instead of {b[i]}")


def check_case(name):
    """One case of tests/binning_cases.py against the oracle, `views` times on a workload of its own."""
    from gaussian_renderer import _native
    case = bc.CASES[name]
    variant, views = case["variant"], case["views"]
    sc = scenes.binning_scene(variant, **case["kw"])
    scope = SCOPE0 + list(bc.CASES).index(name)
    _native.reset_workload_history(scope)
    with _native.workload_scope(scope):
        if case["backward"]:
            grads = scenes.upstream_grads(sc, variant, seed=19)
            out, leaves, o, R = tp._run_both(sc, variant, grads)
            assert R == sc["plan"]["R"]
            tp._check_forward(out, o, R, variant)
            tp._check_binning(sc, variant, o, R)
            tp._check_backward(leaves, o, variant, exact=tp._exact_grads(sc, variant, grads, R))
            for k in ("means3D", "opacities", "features", "vfeatures"):      # a wrong row prefix puts gradients on the wrong surfels
                assert float(leaves[k].grad.abs().max()) > 0, k
            return
        o = orc.OracleRun(sc, orc.SVGSS if variant == "svgss" else orc.RGSS)
        R = o.forward()
        assert R == sc["plan"]["R"]
        sct = runner.to_torch(sc, tp._dev())
        before = _native.speculation_stats()
        for view in range(views):
            raw = runner.forward_raw(sct, variant)
            torch.cuda.synchronize()
            try:
                _where(raw, o, R)
                tp._check_forward(raw, o, R, variant)          # num_rendered, radii (exact), the images
                tp._check_binning_raw(raw, o, R)               # instance list, ranges (exact), n_contrib
            except AssertionError as e:
                raise AssertionError(f"view {view + 1} of {views}: {e}") from e
            del raw
        after = _native.speculation_stats()
    if views == 4 and os.environ.get("SVGIR_NO_KEY_SPEC") is None:
        d = {k: after[k] - before[k] for k in after}
        assert d["forwards"] == 4 and d["rerun_capacity"] == 0 and d["rerun_depth_key"] == 0, d
        # keys that share their top byte: the fourth view (after a streak of three) is sorted in three passes; otherwise none is
        assert d["three_pass"] == (1 if case["expect"]["top"] == 1 else 0), d


@pytest.mark.parametrize("name", list(bc.CASES))
def test_binning_case_matches_the_oracle(built, name):
    check_case(name)


def test_nonempty_empty_nonempty_views_of_one_workload(built):
    """A view in which every surfel is culled, between two views that are not: it runs inside the capacity guessed from the first
    (count 0 read on the device), renders the background, leaves every range (0, 0) -- and the view after it is right again."""
    from gaussian_renderer import _native
    full = scenes.binning_scene("rgss", P=3000, seed=3, **bc.GRID)
    none = scenes.binning_scene("rgss", P=3000, n_culled=3000, seed=3, **bc.GRID)
    scope = SCOPE0 + 900
    _native.reset_workload_history(scope)
    before = _native.speculation_stats()
    with _native.workload_scope(scope):
        for sc in (full, none, full):
            o = orc.OracleRun(sc, orc.RGSS)
            R = o.forward()
            raw = runner.forward_raw(runner.to_torch(sc, tp._dev()), "rgss")
            torch.cuda.synchronize()
            _where(raw, o, R)
            tp._check_forward(raw, o, R, "rgss")
            tp._check_binning_raw(raw, o, R)
            if sc is none:
                assert R == 0 and raw["num_rendered"] == 0 and not raw["ranges"].any() and not raw["n_contrib"].any()
                assert not raw["radii"].any()
                # the background: one value everywhere, bit-equal to the oracle's (rgss starts a pixel at T = 1 - 1e-6, so it is
                # 0.4999995 for a background of 0.5, and the opacity image 1e-6, not 0)
                im = o.images()
                assert np.array_equal(raw["color"].cpu().numpy(), im["color"]) and np.array_equal(raw["opacity"].cpu().numpy(), im["opacity"])
                assert np.unique(im["color"]).size == 1 and abs(float(im["color"].flat[0]) - 0.5) < 2e-6 and float(im["opacity"].max()) < 2e-6
            else:
                assert R == 3000
    after = _native.speculation_stats()
    assert after["rerun_capacity"] == before["rerun_capacity"]


@pytest.mark.parametrize("gx,gy", [(1023, 1), (1, 1023)])
def test_largest_grid_side_is_accepted(built, gx, gy):
    """1023 tiles per side, either way round (tests/binning_cases.py has the 1023 x 33 grid with whole-grid splats)."""
    from gaussian_renderer import _native
    sc = scenes.binning_scene("rgss", P=4000, gx=gx, gy=gy, edge_frac=0.2, seed=4)
    o = orc.OracleRun(sc, orc.RGSS)
    R = o.forward()
    assert R == sc["plan"]["R"]
    with _native.workload_scope(SCOPE0 + 910 + gy % 2):
        raw = runner.forward_raw(runner.to_torch(sc, tp._dev()), "rgss")
    _where(raw, o, R)
    tp._check_forward(raw, o, R, "rgss")
    tp._check_binning_raw(raw, o, R)


@pytest.mark.parametrize("W,H", [(16 * 1024, 16), (16, 16 * 1024), (16 * 1023, 16 * 65)], ids=["1024_wide", "1024_high", "4T_2p18"])
def test_grid_beyond_the_limits_is_refused(built, W, H):
    """csrc/api.hip validate: more than 1023 tiles per side, or 4 T >= 2^18 sub-tiles (1023 x 65 tiles), is an argument error of the
    binding -- with the library's message, and before anything is launched (no forward is counted)."""
    from gaussian_renderer import _native
    sc = scenes.binning_scene("rgss", P=10, seed=1, **bc.GRID)
    sc.update(cameras.make_camera(W, H, np.array(scenes.BINNING_EYE)))
    before = _native.speculation_stats()
    with pytest.raises(RuntimeError, match=r"exceeds the supported size \(at most 1023 tiles per side, 65535 tiles in total\)"):
        runner.forward_raw(runner.to_torch(sc, tp._dev()), "rgss")
    torch.cuda.synchronize()
    assert _native.speculation_stats() == before


@pytest.mark.parametrize("which,env", [("radix", dict(SVGIR_TILE_SORT12="0")), ("xcd", dict(SVGIR_FWD_FILL="1", SVGIR_FWD_XCD="1"))], ids=["radix", "xcd"])
def test_forced_paths_in_a_child_process(built, which, env):
    """The two-kernel radix passes as the tile sort of the small grids (1 ... 8 tile bits in one pass, 9 ... 12 in two), and the per-XCD
    dispatch lists at 4 T = 1024, 1028, 8192, 8196, 12 296 with the svgss backward: switches read once per process."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "binning_paths.py"), which], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "failed: 0" in out.stdout, out.stdout[-3000:] + out.stderr[-1500:]
    assert f"cases: {len(bc.FORCED[which])}" in out.stdout
