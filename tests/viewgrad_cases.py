"""The case matrix of the view-direction gradient tests (svgir_shade_backward_view; DESIGN.md "View-direction gradient"): one table for
tests/test_viewgrad_edge_inputs.py (the fp64 oracle alone) and tests/test_gpu_viewgrad.py (the HIP kernels against it).

It extends tests/shading_cases.py (imported, not edited): the same builders, probe, per-row error, weights and oracle run, with
`viewdirs` a leaf of the oracle.

Runs.  Every entry of shading_cases.RUNS (the lattice ones take the directions the kernels generate: GPU tests only), plus
  * `view_alignment` (Ns = 65, n = 197), the inputs at which the adjoint of V has its own clamps: every row but the `zero_view` ones has
    one sample with dirs == -viewdirs bit for bit (L = -V: h = 0, H = 0 exactly, under the norm clamp); `aligned` rows (a minority:
    thresholds by construction) also have one sample with dirs == viewdirs bit for bit (V.H = 1, the upper bound of the Schlick
    term's clamp); `zero_view` rows have viewdirs = 0 (a surfel at the camera: V = 0 under the norm clamp); `all_h0` rows face the
    viewer and have EVERY sample at -viewdirs (n.l < 0 everywhere: the row's outputs and all its gradients are exactly zero); the
    rest is random.  The view directions are fp32 values, so "bit for bit" also holds for the kernels' inputs.  The L = -V samples
    lie behind the surface of their (viewer-facing) rows and carry no weight, as in shading_cases' `opposed` rows: the kernels form
    (L + V) / 2 with a fused multiply-add, which leaves the rounding residual of L instead of 0 there ("View-direction
    gradient": known limits), so a weighted sample at L = -V would test the forward's arithmetic, not this gradient;
  * Ns = 1 and Ns = 65 on an ordinary case: either side of the backward's 64-sample chunk;
  * Ns = 8 with 12 301 surfels: more than grid workgroups x waves x KB_G of the backward launch on 256 CUs (256 x 12 x 4 = 12 288, for
    the plain kernel and the view pass alike), so that a wave walks a second batch of surfel records.

Threshold rows: shading_cases.threshold_rows, plus the rule its docstring leaves out because V had no adjoint there: a row with
V.H >= 1 - 1e-6 on a (sample, corner) pair whose GGX denominator is not under its lower clamp, is a threshold row like the rows of the
other three cosines (x = 1 is the closed end of the clamp's pass band, and fp32 rounds the dot product of two equal unit vectors to
either side of 1).  Exact zeros (H = 0, V = 0) are not thresholds: the oracle gives exactly zero there in both precisions."""
import numpy as np
import torch

import shading_cases as sc
from svgir_harness import shade_inputs

MAX_THRESHOLD_SHARE = sc.MAX_THRESHOLD_SHARE
LEAVES = sc.LEAVES + ("viewdirs",)
BATCH_SURFELS = 12301   # > 256 workgroups x 12 waves x 4 surfels per batch (csrc/shade.hip: shade_backward_impl's grid rule)


def _runs():
    out = [dict(r) for r in sc.RUNS]
    out += [dict(sc._run("view_alignment", 65)), dict(sc._run("grazing_view", 1)), dict(sc._run("grazing_view", 65)),
            dict(sc._run("material_ends", 65, ratio=0.83))]
    big = dict(sc._run("grazing_view", 8), n=BATCH_SURFELS)
    big["id"] += f"-n{BATCH_SURFELS}"
    return out + [big]


RUNS = _runs()
CPU_RUNS = [r for r in RUNS if not r["lattice"]]


def view_alignment(n=197, Ns=65, seed=0, He=32, We=64):
    """(inputs fp64, labels, options) of the `view_alignment` case (module docstring)."""
    g = torch.Generator().manual_seed(7000 + seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    d = shade_inputs._ordinary(n, Ns, g, He, We)
    d["viewdirs"] = d["viewdirs"].float().double()          # fp32 values: dirs == +-viewdirs survives the cast to the kernels' inputs
    lab = np.array(["ordinary"] * n, dtype=object)
    opt = dict(softplus=True, scale=2.0, transform=None, radiance_ratio=None)
    rows = torch.randperm(n, generator=g)
    groups, at = {}, 0
    for label, k in (("aligned", 6), ("zero_view", 5), ("all_h0", 5)):
        groups[label] = rows[at:at + k]
        lab[groups[label].numpy()] = label
        at += k
    s_minus, s_plus = 3, 40
    d["dirs"][:, s_minus] = -d["viewdirs"]
    d["dirs"][groups["aligned"], s_plus] = d["viewdirs"][groups["aligned"]]
    i = groups["all_h0"]
    d["normals"][i] = shade_inputs._unit(d["viewdirs"][i][:, None] + 0.1 * rnd(i.numel(), 4, 3))
    d["dirs"][i] = -d["viewdirs"][i][:, None].expand(-1, Ns, -1)
    i = groups["zero_view"]
    d["viewdirs"][i] = 0.0
    d["dirs"][i, s_minus] = shade_inputs._unit(d["geo_normals"][i] + 0.9 * rnd(i.numel(), 3))
    return d, lab.astype(str), opt


def build(run, dirs=None):
    """shading_cases.build for the runs of this table."""
    if run["case"] != "view_alignment" and "n" not in run:
        return sc.build(run, dirs)
    if run["case"] == "view_alignment":
        d, lab, opt = view_alignment(Ns=run["Ns"], He=run["He"], We=run["We"])
    else:
        d, lab, opt = shade_inputs.edge_case(run["case"], run["n"], run["Ns"], He=run["He"], We=run["We"], transform=run["transform"],
                                             hdr=run["hdr"])
    assert dirs is None
    opt["radiance_ratio"] = run["ratio"]
    return d, lab, opt


def threshold_rows(p):
    """shading_cases.threshold_rows plus the V.H <= 1 rule (module docstring), from a probe of the fp64 oracle."""
    n = p["sgn_arg"].shape[0]
    live = p["nom"] >= 1e-6 * (1 - sc.REL)                                   # [n,Ns,4]
    return sc.threshold_rows(p) | ((p["VoH"] >= 1 - 1e-6)[:, :, None] & live).reshape(n, -1).any(1)


def exact_zero_rows(lab):
    """Rows whose d_viewdirs is exactly zero: a zero view direction, or every sample at H = 0 behind the surface."""
    return torch.from_numpy((lab == "zero_view") | (lab == "all_h0"))


def oracle_run(d, opt, w, dtype=torch.float64, view=None, training=None):
    """shading_cases.oracle_run with `viewdirs` a leaf: its `cv(d["viewdirs"])` keeps the graph of the fp64 leaf handed in here (the
    cast to fp32 is differentiable and exact in the adjoint), so the gradient arrives in that leaf.  Returns (outputs, gradients with
    "viewdirs", in fp64 for both dtypes of the arithmetic)."""
    leaf = d["viewdirs"].detach().double().clone().requires_grad_(True)
    out, grads = sc.oracle_run(dict(d, viewdirs=leaf), opt, w, dtype, view, training)
    grads["viewdirs"] = (leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)).to(dtype)
    return {k: v.detach() for k, v in out.items()}, grads


def e32(d, opt, w, thr, view=None, training=None):
    """shading_cases.e32 over the gradients with `viewdirs`: (fp64 outputs, fp64 gradients, E32)."""
    o64, g64 = oracle_run(d, opt, w, torch.float64, view, training)
    o32, g32 = oracle_run(d, opt, w, torch.float32, view, training)
    E = {}
    for tag, r64, r32 in (("", o64, o32), ("d_", g64, g32)):
        for k in r64:
            if k == "mean_vis":
                continue
            assert torch.isfinite(r64[k]).all() and torch.isfinite(r32[k]).all(), f"oracle {tag}{k} is not finite"
            if r64[k].dim() == 0 or k == "env":
                E[tag + k] = float(sc.row_err(r32[k].reshape(1, -1), r64[k].reshape(1, -1), whole=True))
            else:
                e = sc.row_err(r32[k], r64[k])[~thr]
                E[tag + k] = float(e.max()) if e.numel() else 0.0
    return o64, g64, E
