"""GPU parity on the scenes where the composite kernels leave their common path (svgir_harness.scenes; tests/test_edge_scenes.py shows
that each scene holds its case): indefinite conics whose exp overflows next to blending pixels, the most edge-on near surfels the cull
admits, stacks of exact lengths at the forward / backward batch and segment boundaries (with and without termination at them, with
tied depths), and Gaussians at the edges of the view frustum.  The budgets are test_gpu_parity.py's, unchanged; gradients are anchored
on the fp64 oracle.  SVGIR_POISON is on (tests/conftest.py): an element a kernel leaves unwritten is NaN."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_parity as gp
from svgir_harness import scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _finite(out, leaves):
    for k, v in out.items():
        if torch.is_tensor(v) and v.is_floating_point():
            assert bool(torch.isfinite(v).all()), f"output {k} is not finite"
    for k, v in leaves.items():
        if v.grad is not None:
            bad = (~torch.isfinite(v.grad)).reshape(v.shape[0], -1).any(1).nonzero().reshape(-1).tolist()
            assert not bad, f"grad_{k} is not finite for Gaussians {bad[:8]} ({len(bad)} in all)"


def _full_check(sc, variant, seed=7):
    grads = scenes.upstream_grads(sc, variant, seed=seed)
    out, leaves, o, R = gp._run_both(sc, variant, grads)
    assert R > 0
    _finite(out, leaves)
    gp._check_forward(out, o, R, variant)
    gp._check_binning(sc, variant, o, R)
    return out, leaves, o, R, grads


@pytest.mark.parametrize("variant,S,VS", [("svgss", 3, 8), ("rgss", 5, 0), ("svgss", 9, 72), ("rgss", 7, 0)],
                         ids=["svgss_S3_VS8", "rgss_S5", "svgss_S9_VS72_runtime", "rgss_S7_runtime"])
def test_indefinite_conics(built, variant, S, VS):
    """det < 0 conics (cov3D_precomp): pixels with power > 88.7 (exp = inf) share 8x8 sub-tiles with pixels that blend the splat."""
    sc = scenes.indefinite_conic_scene(variant, S=S, VS=VS)
    out, leaves, o, R, grads = _full_check(sc, variant)
    gp._check_backward(leaves, o, variant, exact=gp._exact_grads(sc, variant, grads, R))


class _Masked:
    """The gradients of one oracle run with the rows of `drop` zeroed (the interface _check_backward reads)."""

    def __init__(self, gr, drop):
        self.gr = {k: v.copy() for k, v in gr.items()}
        for k, v in self.gr.items():
            if v.ndim >= 1 and v.shape[0] == drop.size:
                v[drop] = 0

    def grads(self):
        return self.gr


@pytest.mark.parametrize("variant,S,VS", [("svgss", 3, 8), ("rgss", 5, 0)])
def test_edge_on_near_surfels(built, variant, S, VS):
    """Flat surfels at depth 0.21-0.35 at the most grazing angle the cull admits.  Images and integer state as everywhere; gradients
    with the normal budgets on every Gaussian except the ill-conditioned ones (|det| / (ca cc) < 1e-4 from the oracle's conic), which
    are only required finite -- and must be few (<= 1 % of P)."""
    sc = scenes.edge_on_near_scene(variant, S=S, VS=VS)
    out, leaves, o, R, grads = _full_check(sc, variant)
    co = o.get("conic_opacity").reshape(-1, 4).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.abs(co[:, 0] * co[:, 2] - co[:, 1] ** 2) / np.abs(co[:, 0] * co[:, 2])
    drop = (o.get("radii") > 0) & (cond < 1e-4)
    P = sc["means3D"].shape[0]
    assert drop.sum() <= 0.01 * P, drop.sum()
    exact = gp._exact_grads(sc, variant, grads, R)
    if drop.any():
        keep = torch.from_numpy(~drop).to(leaves["means3D"].device)

        class _Leaf:
            def __init__(self, g):
                self.grad = None if g is None else g * keep.reshape(-1, *([1] * (g.dim() - 1)))
        leaves = {k: _Leaf(v.grad) for k, v in leaves.items()}
        o = _Masked(o.grads(), drop)
        exact = _Masked(exact, drop).grads()
    gp._check_backward(leaves, o, variant, exact=exact)


@pytest.mark.parametrize("terminate", [False, True], ids=["all_blend", "terminate"])
@pytest.mark.parametrize("variant,S,VS", [("svgss", 3, 8), ("rgss", 5, 0)])
def test_stack_boundaries(built, variant, S, VS, terminate):
    """List lengths 1..193 around every KB / CH / SEG / SB / CHB boundary, termination on and next to ranks 64 and 128, a tied-depth
    block per stack: instance list (tie order included), ranges and n_contrib exact, images and fp64-anchored gradients."""
    sc = scenes.stack_scene(variant, terminate=terminate, S=S, VS=VS)
    out, leaves, o, R, grads = _full_check(sc, variant)
    gp._check_backward(leaves, o, variant, exact=gp._exact_grads(sc, variant, grads, R))


def test_stack_boundaries_forced_forward_variants(built):
    """The stack scenes under the high-fill / per-XCD forward (read once per process: a child process)."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n" % (os.path.join(ROOT, "svg-ir_amd"), ROOT, os.path.join(ROOT, "tests")) +
            "import test_gpu_edge_cases as T\n"
            "for v, S, VS in (('svgss', 3, 8), ('rgss', 5, 0)):\n"
            "    for term in (False, True):\n"
            "        sc = T.scenes.stack_scene(v, terminate=term, S=S, VS=VS)\n"
            "        out, leaves, o, R, grads = T._full_check(sc, v)\n"
            "        T.gp._check_backward(leaves, o, v, exact=T.gp._exact_grads(sc, v, grads, R))\n"
            "print('stack variants OK')\n")
    env = dict(os.environ, SVGIR_FWD_FILL="1", SVGIR_FWD_XCD="1")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0 and "stack variants OK" in res.stdout, res.stdout[-1500:] + res.stderr[-3000:]


@pytest.mark.parametrize("variant,S,VS", [("svgss", 3, 8), ("rgss", 5, 0)])
def test_frustum_edge_gaussians(built, variant, S, VS):
    """Centres beyond the 1.3 tan clamp (the clamped mean gradient) with footprints reaching the image, and near Gaussians (depth
    0.21-0.25) covering it: radii exact, means3D / scales / rotations gradients fp64-anchored."""
    sc = scenes.surface_scene(P=3000, W=160, H=120, seed=91, sh_degree=1, variant=variant, S=S, VS=VS, scale_lo=0.01, scale_hi=0.05)
    scenes.frustum_extras(sc, variant, seed=5, n_side=16)
    out, leaves, o, R, grads = _full_check(sc, variant)
    P, m = sc["means3D"].shape[0], sc["n_frustum"]
    assert (out["radii"][P - m:].cpu().numpy() > 0).all()
    gp._check_backward(leaves, o, variant, exact=gp._exact_grads(sc, variant, grads, R))
    for k in ("means3D", "scales", "rotations"):
        assert float(leaves[k].grad[P - m:].abs().max()) > 0, k
