"""Case table of the fused shading under a spherical-Gaussian light (svgir_forward_sg / svgir_backward_sg; tests/test_gpu_fused_sg.py,
tests/test_fused_sg_edge_inputs.py).  Seeded builders only: a case names its scene, its shading inputs and its lobes; nothing here runs
a kernel.

The small view is 64 surfels on 32 x 32 pixels: about half of them pass the preprocess culls, so the working set of the fused call (the
front of the depth order, or the contribution pre-pass's list from Ns >= 128 on) and the blended list of its backward are proper subsets
of 0..P-1 and the kernels' zero-fill of the other rows has rows to fill.  The lobe counts cover the lane groups of the lobes' share of
the backward (sg_chunk_adjoint: groups of 2, 4, 32 and 64 lanes; above 64 two lobes per lane): 1, 3, 32, 33 and 128 lobes."""
import math

import torch

from svgir_harness import scenes, shade_inputs

# (training widths, in-kernel lattice, Ns, lobes, radiance_ratio, view_gradient).  Ns 7 and 24: the quad forward kernel (7: a step of four
# samples that ends inside the list); 200: one wave per surfel, four chunks of 64 samples of which the last holds 8, and the
# contribution pre-pass.  128 lobes once per forward kernel.
SMALL = (
    (True, True, 7, 1, False, False),
    (True, False, 24, 3, True, False),
    (True, True, 24, 32, False, True),
    (True, False, 7, 33, True, True),
    (True, True, 24, 128, False, False),
    (True, False, 200, 33, False, True),
    (True, True, 200, 1, True, False),
    (False, True, 200, 32, False, False),
    (False, False, 200, 3, True, False),
    (False, True, 200, 128, False, True),
    (False, False, 24, 33, False, False),
    (False, True, 7, 1, True, True),
)

# (P, Ns, training): the partition of the working set is built per chunk of 2048 surfels (csrc/subset.hip)
CHUNK_EDGES = tuple((P, Ns, tr) for Ns, tr in ((64, True), (200, False)) for P in (2047, 2048, 2049, 4097))


def case_id(c):
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in c)


def small_scene(training):
    S, VS = (4, 52) if training else (7, 64)
    return scenes.surface_scene(P=64, W=32, H=32, seed=13, sh_degree=2, variant="svgss", S=S, VS=VS, scale_lo=0.05, scale_hi=0.2)


def chunk_scene(P, training):
    S, VS = (4, 52) if training else (7, 64)
    return scenes.surface_scene(P=P, W=64, H=64, seed=41, sh_degree=2, variant="svgss", S=S, VS=VS, scale_lo=0.01, scale_hi=0.06)


def train_scene():
    """the 2 000-surfel scene of tests/test_gpu_sg_light.py::test_train_step_with_an_sg_light"""
    return scenes.surface_scene(P=2000, W=96, H=80, seed=71, sh_degree=3, variant="svgss", S=4, VS=52, scale_lo=0.02, scale_hi=0.07)


def lobes(M, seed=8, device="cpu"):
    """DirectLightSG's initial lobes with the sharpness column at 5 instead of 100: every lobe then lights a good part of the sphere, and
    every lobe's gradient is far from zero."""
    lb = shade_inputs.sg_lobes(M, seed=seed, device=device)
    lb[:, 3] *= 0.05
    return lb


def geo_normals(rotations):
    q = torch.nn.functional.normalize(rotations, dim=-1)
    r, x, y, z = q.unbind(-1)
    return torch.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], dim=-1)


def materials(sct, campos, Ns, training, seed, lattice, offsets=None):
    """The shading inputs of the scene `sct` (torch, on its device): view directions towards the camera; `lattice`: the in-kernel
    Fibonacci lattice (random azimuths at the training widths, seeded) instead of explicit directions and areas."""
    from gaussian_renderer import shading
    dev = sct["means3D"].device
    P = sct["means3D"].shape[0]
    gn = geo_normals(sct["rotations"])
    d = shade_inputs.make(P, Ns, seed=seed, device=dev, geo_normals=gn, with_dirs=not lattice)
    d["viewdirs"] = torch.nn.functional.normalize(campos[None, :] - sct["means3D"], dim=-1)
    if lattice:
        offs = offsets
        if offs is None and training:
            offs = (torch.rand(P, generator=torch.Generator().manual_seed(seed)) * (2 * math.pi)).to(dev)
        d["dirs"], d["areas"] = shading.FibonacciLattice(torch.nn.functional.normalize(gn, dim=-1), Ns, offs), None
    return d
