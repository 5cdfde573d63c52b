"""The rows of the depth sort's bucket plan on the GPU (csrc/preprocess.hip groups every row of DEPTH_ROW surfels by key bits 16..23,
csrc/binning.hip depth_bucket_sort_kernel gathers a bucket from the rows): tests/depth_gather_cases.py lists the cases,
tests/test_depth_gather_scenes.py proves on the host that each has the rows it is named for.  Every case runs four views on a workload
of its own -- the fourth is sorted under the speculated byte, by the bucket plan -- and every view's num_rendered, radii, instance list,
tile ranges (exact) and images are compared with the oracle (the checks of tests/test_gpu_depth_buckets.py).  The same fourth view sorted
by the LSD passes (SVGIR_DEPTH_SORT=lsd, a child process: the switch is read once) gives the same instance list and ranges; oversize
buckets gathered from several rows run in a second child under SVGIR_DEPTH_BUCKET_CAP=256.  All integer outputs: no tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_gather_cases as gc
import test_gpu_depth_buckets as G
import test_gpu_parity as tp
from svgir_harness import runner, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCOPE0 = 8900       # workload scopes 8900 ... : one per case


def check_case(case, scope):
    """Four views of one case against the oracle + the speculation statistics; returns the fourth view."""
    from gaussian_renderer import _native
    sc = gc.build(case)
    o, R = G._oracle(("gather", scope), sc)
    _native.reset_workload_history(scope)
    sct = runner.to_torch(sc, tp._dev())
    before = _native.speculation_stats()
    with _native.workload_scope(scope):
        for view in range(case["views"]):
            try:
                raw = G._view(sct, o, R)
            except AssertionError as e:
                raise AssertionError(f"view {view + 1} of {case['views']}: {e}") from e
    after = _native.speculation_stats()
    if G.KEY_SPEC:
        d = {k: after[k] - before[k] for k in after}
        assert d["forwards"] == 4 and d["rerun_capacity"] == 0 and d["rerun_depth_key"] == 0 and d["three_pass"] == 1, d
    # the order itself, beyond what the oracle's instance list shows: inside a tile, equal keys in index order
    want_list, want_ranges = scenes.binning_expected(sc)
    assert np.array_equal(raw["point_list"][:R], want_list) and np.array_equal(raw["ranges"].reshape(-1, 2), want_ranges)
    return raw


def _child(which, env, outdir):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "depth_gather_paths.py"), which, str(outdir)], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "failed: 0" in out.stdout, out.stdout[-3000:] + out.stderr[-1500:]
    return out.stdout


@pytest.fixture(scope="module")
def lsd_views(built, tmp_path_factory):
    """<case>.npz of every case, CASES and FORCED: the fourth view's instance list and ranges as the LSD passes sort it."""
    d = tmp_path_factory.mktemp("lsd_gather")
    out = _child("lsd", dict(SVGIR_DEPTH_SORT="lsd"), d)
    assert f"cases: {len(gc.CASES) + len(gc.FORCED)}" in out
    return d


@pytest.mark.parametrize("name", list(gc.CASES))
def test_case_matches_the_oracle_and_the_lsd_passes(built, lsd_views, name):
    raw = check_case(gc.CASES[name], SCOPE0 + list(gc.CASES).index(name))
    G._same_as_lsd(raw, lsd_views, name)


def test_oversize_buckets_gathered_from_several_rows(built, lsd_views, tmp_path):
    """SVGIR_DEPTH_BUCKET_CAP=256: one bucket above the capacity whose keys lie in four rows, with differing low bits (the chunked passes
    read the rows) and with equal ones (the gathered order is the order); and the same rows inside the capacity -- each against the oracle
    in the child, and against the LSD passes' view here."""
    out = _child("cap", dict(SVGIR_DEPTH_BUCKET_CAP=str(gc.FORCED_CAP)), tmp_path)
    assert f"cases: {len(gc.FORCED)}" in out
    for name in gc.FORCED:
        G._same_as_lsd(np.load(os.path.join(tmp_path, name + ".npz")), lsd_views, name)


def test_fused_shading_clears_every_culled_surfel(built):
    """svgss with the fused shading under the speculated byte: the shading clears the packed rows of the surfels the view does not shade
    by walking the BACK of the depth order, which the bucket kernel assembles from the tails of the rows (the ids without a tile, by
    index).  Output rows are NaN-poisoned beforehand: an id missing from that tail leaves NaN in its feature / vfeature row, or in its
    gradient rows after the backward."""
    import test_gpu_fused_shade as fs
    from gaussian_renderer import _native as N
    from gaussian_renderer import shading
    from gaussian_renderer.svgss_rasterization import _C
    from svgir_harness import shade_inputs
    assert N.POISON
    dev = torch.device(fs.DEV)
    kw = gc.SVGSS
    P, S, VS = kw["P"], kw["S"], kw["VS"]
    sc = scenes.binning_scene("svgss", **kw)
    sct = runner.to_torch(sc, dev)
    st = runner.settings(sct, "svgss")
    d = fs._materials(sct, st, 32, True, seed=5)
    scope = SCOPE0 + 100
    N.reset_workload_history(scope)
    before = N.speculation_stats()
    empty = torch.empty(0, device=dev)
    culled_plan = torch.from_numpy(~sc["plan"]["visible"]).to(dev)
    assert int(culled_plan.sum()) == kw["n_culled"]
    with N.workload_scope(scope):
        for view in range(4):
            shade, keep = shading.fused_shade(d["base_color"], d["roughness"], d["normals"], d["viewdirs"], d["radiance"], shade_inputs.Light(d["env"]),
                                              d["visibility"], d["dirs"], d["areas"], st.viewmatrix, True)
            f2, vf2 = N.out_tensor((P, S), torch.float32, dev), N.out_tensor((P, VS), torch.float32, dev)
            assert torch.isnan(f2).all() and torch.isnan(vf2).all()
            out = _C.rasterize_gaussians(st.bg, sct["means3D"], f2, vf2, empty, sct["opacities"], sct["scales"], sct["rotations"], st.scale_modifier,
                                         empty, st.viewmatrix, st.projmatrix, st.prcppoint, st.patch_bbox, st.tanfovx, st.tanfovy, st.image_height,
                                         st.image_width, sct["shs"], st.sh_degree, st.campos, False, False, st.config, shade=shade)
            torch.cuda.synchronize()
            radii = out[8]
            assert torch.equal(radii == 0, culled_plan), f"view {view + 1}"
            assert not torch.isnan(f2).any() and not torch.isnan(vf2).any(), f"view {view + 1}: a row the shading neither wrote nor cleared"
            assert float(f2[culled_plan].abs().max()) == 0.0 and float(vf2[culled_plan].abs().max()) == 0.0, f"view {view + 1}"
            assert float(vf2[~culled_plan].abs().sum(1).min()) > 0.0, f"view {view + 1}: every surfel with a tile is shaded"
        # forward + backward on the same workload: the gradient rows of the culled surfels
        gt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in scenes.upstream_grads(sc, "svgss", seed=7).items()}
        lv = fs._leaves(sct, d)
        out, m2, _ = fs._fused(sct, st, d, lv, True)
        fs._loss(out, gt).backward()
        torch.cuda.synchronize()
    for k, g in [(k, v.grad) for k, v in lv.items()] + [("means2D", m2.grad)]:
        assert g is not None and torch.isfinite(g).all(), k
        if g.shape[0] == P:
            assert float(g[culled_plan].abs().max()) == 0.0, k
    assert float(lv["base_color"].grad.abs().max()) > 0 and float(lv["means3D"].grad.abs().max()) > 0
    if G.KEY_SPEC:
        after = N.speculation_stats()
        dd = {k: after[k] - before[k] for k in after}
        assert dd["three_pass"] >= 2 and dd["rerun_depth_key"] == 0 and dd["rerun_capacity"] == 0, dd
