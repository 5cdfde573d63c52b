"""`submodules.bvh.RayTracer` (csrc/bvh.hip) and `pbgi.renderer.Renderer` (csrc/pbgi.hip) held to the tracer case table
(tests/tracer_cases.py; tests/test_tracer_edge_inputs.py proves the table on the CPU oracles).

The rule, for every case: a ray that is not a threshold ray (oracle margin, tracer_cases.py) must have `contribute` / `hit_indices` and
blocked / open IDENTICAL to the oracle's and its values within the case's tolerance; threshold rays are counted, not compared, and may
not exceed the 1 % the host test holds the oracle to; the exact-tie cases have none.  There is no flat allowance for rays that "took
another branch".  Every element of every output must have been written: the suite runs with SVGIR_POISON=1 (NaN / -7 in every output
buffer before the call); a NaN may survive only where the oracle's own result is NaN (the zero and NaN directions).
"""
import numpy as np
import pytest
import torch

from oracle import pbgi_oracle as po
from tests import tracer_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON_INT = -7


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("name", list(tc.VIS))
def test_visibility_case(built, name):
    from submodules.bvh import RayTracer
    c, e = tc.VIS[name](), tc.vis_expected(name)
    rt = RayTracer(t(c["means"]), t(c["scales"]), t(c["rots"]))
    out = rt.trace_visibility(t(c["rays_o"]), t(c["rays_d"]), t(c["means"]), t(c["symm"]), t(c["opacity"]), t(c["normals"]))
    n = c["rays_d"].shape[0]
    assert out["visibility"].shape == (n, 1) and out["contribute"].shape == (n, 1) and out["contribute"].dtype == torch.int32
    vis, cnt = out["visibility"].cpu().numpy()[:, 0], out["contribute"].cpu().numpy()[:, 0]
    ovis, ocnt, thr = e["visibility"], e["contribute"], e["threshold"]
    # every element written; NaN only where the oracle's result is NaN
    assert (cnt != POISON_INT).all() and (cnt >= 0).all()
    assert np.array_equal(np.isnan(vis), np.isnan(ovis)), f"NaN visibility at rays {np.flatnonzero(np.isnan(vis) != np.isnan(ovis))[:8]}"
    assert thr.mean() <= tc.MAX_THRESHOLD_SHARE and not ("exact" in c and thr.any())
    keep = ~thr
    print(f"{name}: {n} rays, {thr.sum()} threshold rays, contribute differs on {(cnt != ocnt)[keep].sum()}")
    assert np.array_equal(cnt[keep], ocnt[keep]), f"contribute differs at rays {np.flatnonzero((cnt != ocnt) & keep)[:8]}"
    assert np.array_equal(vis[keep] > 0, ovis[keep] > 0), f"blocked / open differs at rays {np.flatnonzero(((vis > 0) != (ovis > 0)) & keep)[:8]}"
    fin = keep & np.isfinite(ovis)
    err = float(np.abs(vis[fin] - ovis[fin]).max()) if fin.any() else 0.0
    assert err <= c["tol"], f"visibility differs by {err:.3e} (tolerance {c['tol']:.1e}: {c['tol_source']})"
    if "exact" in c:        # exact arithmetic on both sides: bit for bit
        assert np.array_equal(cnt, c["exact"]["contribute"]) and np.array_equal(vis, c["exact"]["visibility"])


def _renderer(c):
    from pbgi.renderer import Renderer
    R = Renderer()
    R.set_proxy(t(c["xyz"]), t(c["scales"]), t(c["rot"]), t(c["normals"]), t(c["opacity"]), t(c["shs"]))
    R.build_bvh()
    return R


@pytest.mark.parametrize("name", list(tc.RAD))
def test_radiance_case(built, name):
    c, e = tc.RAD[name](), tc.rad_expected(name)
    N, S = c["ray_o"].shape[0], c["S"]
    R = _renderer(c)
    info, aabb, _ = po.build(c["xyz"], c["scales"])
    assert np.array_equal(R.LBVHNode_info.cpu().numpy(), info) and np.array_equal(R.LBVHNode_aabb.cpu().numpy(), aabb)
    out = R.render_radiance_with_sampling_SH(t(c["ray_o"]), t(c["ray_d"]), t(c["cov_inv"]), S)
    assert [tuple(o.shape) for o in out] == [(N, S, 3), (N, S, 1), (N, S, 1), (N, S, 2)] and out[2].dtype == torch.int32
    rad, vis, hit, uvs = (o.cpu().numpy() for o in out)
    thr = e["threshold"]
    # every element written (the oracle's results of this table are all finite: the host test asserts it)
    assert np.isfinite(rad).all() and np.isfinite(vis).all() and np.isfinite(uvs).all() and (hit != POISON_INT).all() and (hit >= -1).all()
    assert thr.mean() <= tc.MAX_THRESHOLD_SHARE and not ("exact" in c and thr.any())
    keep = ~thr
    hit, ohit, vis1, ovis1 = hit[..., 0], e["hit"][..., 0], vis[..., 0], e["visibility"][..., 0]
    print(f"{name}: {N} x {S} rays, {thr.sum()} threshold rays, hit index differs on {(hit != ohit)[keep].sum()}")
    assert np.array_equal(hit[keep], ohit[keep]), f"hit index differs at (row, ray) {np.argwhere((hit != ohit) & keep)[:8].tolist()}"
    assert np.array_equal(vis1[keep] > 0, ovis1[keep] > 0), f"blocked / open differs at {np.argwhere(((vis1 > 0) != (ovis1 > 0)) & keep)[:8].tolist()}"
    for what, a, b in (("radiance", rad, e["radiance"]), ("visibility", vis, e["visibility"]), ("uv", uvs, e["uvs"])):
        err = float(np.abs(a[keep] - b[keep]).max()) if keep.any() else 0.0
        assert err <= c["tol"], f"{what} differs by {err:.3e} (tolerance {c['tol']:.1e}: {c['tol_source']})"
    if "exact" in c:
        x = c["exact"]
        assert hit[x["row"]].tolist() == x["hit"]
        if x["visibility"] is not None:
            assert np.array_equal(vis1[x["row"]], np.asarray(x["visibility"], dtype=np.float32))


@pytest.mark.parametrize("layout", tc.SORT_LAYOUTS)
@pytest.mark.parametrize("P", tc.SORT_SIZES)
def test_radiance_tree_at_the_sort_thresholds(built, P, layout):
    """The 30-bit sort plan (8 + 8 + 8 + 6) at the radix sort's size thresholds: node table, boxes and sorted pairs identical to the oracle's."""
    from pbgi.bvhhelpers import GsBvh
    xyz, scales = tc.sort_tree_inputs(P, layout)
    info, aabb, srt = GsBvh(t(xyz), t(scales)).tensors(with_sorted=True)
    oinfo, oaabb, osrt = po.build(xyz, scales)
    assert np.array_equal(srt.cpu().numpy(), osrt)
    assert np.array_equal(info.cpu().numpy(), oinfo)
    assert np.array_equal(aabb.cpu().numpy(), oaabb)
