"""HIP-event times of a training step under a spherical-Gaussian light with the shading fused into the rasterizer calls
(svgir_forward_sg / svgir_backward_sg) against the unfused sequence (svgir_shade_forward_sg over all P surfels, the rasterizer, its
backward, svgir_shade_backward_sg) -- what `workloads.TrainStep(sg_lobes=M)` ran before `fused` was honoured.  For the record only:
bench.py does not time an SG-lit model.

  train   TrainStep on cfg3_train (P = 200 000, 800 x 800), Ns = 64, M = 32 and 128: fused=True against fused=False, the two alternated
          in one process: warm-up, then `--reps` rounds of one event-timed step each; median, min and max; the stage table of both;
  eval    the cfg3_eval widths at Ns = 384, forward only (no_grad), M = 32: render_shaded against shade_and_pack + the rasterizer;
  shares  the working sets the fused path shades / differentiates: surfels with a written vfeatures row / P in the forward, surfels with
          a blend weight / P in the backward -- the ratio of the shading stages can be checked against them.
Acceptance: the fused step is faster than the unfused one by more than the unfused side's own spread (max - min).

`--dump FILE`: the outputs and gradients of one texture fused case (tests/test_gpu_fused_shade.py's small training view) on the library
the process loaded (SVGIR_RASTER_LIB: the parent commit's build, or this one); `--compare A B` records which arrays are byte-identical.
`--bench-ab DIR`: folds bench.py result lines (DIR/{parent,new}_<workload>_<i>.json from alternating runs) into the record.
    python scripts/fused_sg_timing.py [--out profiles/fused_sg_timing.json]   (on the GPU box)"""
import argparse
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd"))
sys.path.insert(0, ROOT)


def timed(fns, reps, warmup):
    """{name: ms stats}: the callables alternated, one event pair per call."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}


def geo_normals(rotations):
    q = torch.nn.functional.normalize(rotations, dim=-1)
    r, x, y, z = q.unbind(-1)
    return torch.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], dim=-1)


def train_group(dev, M, Ns, reps, warmup):
    from svgir_harness import workloads
    steps = {name: workloads.TrainStep(dev, seed=5, name="cfg3_train", Ns=Ns, fused=fused, sg_lobes=M)
             for name, fused in (("fused", True), ("unfused", False))}
    assert steps["fused"].fused and not steps["unfused"].fused
    res = timed({k: ts.step for k, ts in steps.items()}, reps, warmup)
    tables = {k: ts.stage_table(5) for k, ts in steps.items()}
    ts = steps["fused"]
    blended = float((ts.last["weights"] > 0).float().mean())
    f, u = res["fused"], res["unfused"]
    return {"P": ts.P, "Ns": Ns, "M": M, "step_ms": res, "stage_table_ms": tables,
            "ratio_unfused_over_fused": u["median"] / f["median"],
            "faster_by_more_than_the_unfused_spread": bool(u["median"] - f["median"] > u["max"] - u["min"]),
            "blended_share_backward": blended}


def view_inputs(dev, name, Ns, training):
    from gaussian_renderer import shading
    from svgir_harness import runner, scenes, shade_inputs
    sc = scenes.make(name)
    sct = runner.to_torch(sc, dev)
    st = runner.settings(sct, "svgss")
    gn = geo_normals(sct["rotations"])
    d = shade_inputs.make(sct["means3D"].shape[0], Ns, seed=5, device=dev, geo_normals=gn, with_dirs=False)
    d["viewdirs"] = torch.nn.functional.normalize(st.campos[None, :] - sct["means3D"], dim=-1)
    d["dirs"], d["areas"] = shading.FibonacciLattice(torch.nn.functional.normalize(gn, dim=-1), Ns, None), None
    return sct, st, d


def forward_shares(dev, sct, st, d, light, training):
    """(surfels whose vfeatures row the fused forward wrote / P, surfels with a blend weight / P)"""
    from gaussian_renderer import _native as N, shading
    from gaussian_renderer.svgss_rasterization import _C
    P = sct["means3D"].shape[0]
    S, VS = (4, 52) if training else (7, 64)
    fs, lt, keep = shading.fused_shade_sg(d["base_color"], d["roughness"], d["normals"], d["viewdirs"], d["radiance"], light, d["visibility"],
                                          d["dirs"], d["areas"], st.viewmatrix, training)
    f, vf = torch.empty((P, S), device=dev), torch.empty((P, VS), device=dev)
    empty = torch.empty(0, device=dev)
    out = _C.rasterize_gaussians(st.bg, sct["means3D"], f, vf, empty, sct["opacities"], sct["scales"], sct["rotations"], st.scale_modifier, empty,
                                 st.viewmatrix, st.projmatrix, st.prcppoint, st.patch_bbox, st.tanfovx, st.tanfovy, st.image_height,
                                 st.image_width, sct["shs"], st.sh_degree, st.campos, False, False, st.config, shade=fs, sg_light=lt,
                                 forward_only=True)
    torch.cuda.synchronize()
    return float((vf.abs().sum(1) > 0).float().mean()), float((out[7] > 0).float().mean())


def eval_group(dev, M, Ns, reps, warmup):
    from gaussian_renderer import shading
    from gaussian_renderer.svgss_rasterization import GaussianRasterizer
    from svgir_harness import shade_inputs
    sct, st, d = view_inputs(dev, "cfg3_eval", Ns, False)
    light = shade_inputs.SGLight(shade_inputs.sg_lobes(M, seed=11, device=dev))
    m2 = torch.zeros_like(sct["means3D"])
    geo = (sct["opacities"], sct["shs"], sct["scales"], sct["rotations"])
    mat = (d["base_color"], d["roughness"], d["normals"], d["viewdirs"], d["radiance"])

    def fused():
        with torch.no_grad():
            shading.render_shaded(st, sct["means3D"], m2, *geo, *mat, light, d["visibility"], d["dirs"], d["areas"], False)

    def unfused():
        with torch.no_grad():
            f, vf, _ = shading.shade_and_pack(*mat, light, d["visibility"], d["dirs"], d["areas"], st.viewmatrix, False)
            GaussianRasterizer(st)(means3D=sct["means3D"], means2D=m2, opacities=geo[0], shs=geo[1], scales=geo[2], rotations=geo[3],
                                   features=f, vfeatures=vf)

    res = timed({"fused": fused, "unfused": unfused}, reps, warmup)
    shaded, blended = forward_shares(dev, sct, st, d, light, False)
    f, u = res["fused"], res["unfused"]
    return {"P": int(sct["means3D"].shape[0]), "Ns": Ns, "M": M, "forward_ms": res, "ratio_unfused_over_fused": u["median"] / f["median"],
            "faster_by_more_than_the_unfused_spread": bool(u["median"] - f["median"] > u["max"] - u["min"]),
            "shaded_share_forward": shaded, "blended_share": blended}


def train_forward_share(dev, M, Ns):
    from svgir_harness import shade_inputs
    sct, st, d = view_inputs(dev, "cfg3_train", Ns, True)
    return forward_shares(dev, sct, st, d, shade_inputs.SGLight(shade_inputs.sg_lobes(M, seed=11, device=dev)), True)[0]


def dump_texture_case(dev, path):
    """the small training view of tests/test_gpu_fused_shade.py under the texture light, forward + backward, every array to `path`"""
    from gaussian_renderer import shading
    from svgir_harness import runner, scenes, shade_inputs
    sc = scenes.surface_scene(P=6000, W=176, H=144, seed=41, sh_degree=2, variant="svgss", S=4, VS=52, scale_lo=0.01, scale_hi=0.06)
    sct = runner.to_torch(sc, dev)
    st = runner.settings(sct, "svgss")
    gn = geo_normals(sct["rotations"])
    d = shade_inputs.make(6000, 64, seed=3, device=dev, geo_normals=gn, with_dirs=False)
    d["viewdirs"] = torch.nn.functional.normalize(st.campos[None, :] - sct["means3D"], dim=-1)
    offs = (torch.rand(6000, generator=torch.Generator().manual_seed(3)) * 6.2831855).to(dev)
    lat = shading.FibonacciLattice(torch.nn.functional.normalize(gn, dim=-1), 64, offs)
    lv = {k: sct[k].detach().clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    lv.update({k: d[k].detach().clone().requires_grad_(True) for k in ("base_color", "roughness", "normals", "radiance", "env")})
    m2 = torch.zeros_like(lv["means3D"], requires_grad=True)
    out, _ = shading.render_shaded(st, lv["means3D"], m2, lv["opacities"], lv["shs"], lv["scales"], lv["rotations"], lv["base_color"],
                                   lv["roughness"], lv["normals"], d["viewdirs"], lv["radiance"], shade_inputs.Light(lv["env"]),
                                   d["visibility"], lat, None, True)
    gt = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in scenes.upstream_grads(sc, "svgss", seed=6).items()}
    names = ("color", "normal", "opacity", "depth", "feature", "vfeature")
    sum((o * gt[n]).sum() for n, o in zip(names, out[1:7])).backward()
    torch.cuda.synchronize()
    arrays = {n: o.detach().cpu().numpy() for n, o in zip(names + ("weights", "radii"), out[1:9])}
    arrays.update({"grad_" + k: v.grad.cpu().numpy() for k, v in lv.items()})
    arrays["grad_means2D"] = m2.grad.cpu().numpy()
    np.savez(path, **arrays)


def compare(a, b):
    """{array: byte-identical?}; weights and grad_env are sums of float atomics in both libraries (listed, not expected to be equal)"""
    A, B = np.load(a), np.load(b)
    assert set(A.files) == set(B.files)
    return {k: bool(A[k].tobytes() == B[k].tobytes()) for k in sorted(A.files)}


def bench_ab(d):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.json"))):
        side, rest = os.path.basename(path)[:-5].split("_", 1)
        workload = rest.rsplit("_", 1)[0]
        line = [ln for ln in open(path).read().splitlines() if ln.startswith("{")][-1]
        out.setdefault(workload, {}).setdefault(side, []).append(json.loads(line))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_sg_timing.json"))
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--dump")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--unchanged")
    ap.add_argument("--bench-ab")
    a = ap.parse_args()
    if a.compare:
        print(json.dumps(compare(*a.compare), indent=1))
        return
    dev = torch.device("cuda:0")
    if a.dump:
        dump_texture_case(dev, a.dump)
        return
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "train": [], "eval": []}
    for M in (32, 128):
        g = train_group(dev, M, 64, a.reps, a.warmup)
        torch.cuda.empty_cache()
        g["shaded_share_forward"] = train_forward_share(dev, M, 64)
        rec["train"].append(g)
        print(json.dumps(g), flush=True)
        torch.cuda.empty_cache()
    g = eval_group(dev, 32, 384, a.reps, a.warmup)
    rec["eval"].append(g)
    print(json.dumps(g), flush=True)
    if a.unchanged:
        rec["texture_fused_case_byte_identical_to_parent"] = json.load(open(a.unchanged))
    if a.bench_ab:
        rec["bench_ab"] = bench_ab(a.bench_ab)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
