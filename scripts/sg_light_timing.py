"""HIP-event times of the shading kernels with the spherical-Gaussian direct light (csrc/shade.hip LIGHT_SG, csrc/sg_light.hpp) next to
(b) the texture-light shading on the same inputs -- the existing kernels through the same build -- and (c) the reference's way of getting
the SG light: `render_envmap_sg` (scene/direct_light_sg.py:10-46) restated in torch on the GPU in its 10 000-row batches (without its
per-batch empty_cache), timed alone; it materialises [rows, Ns, M, 3] temporaries and a [P, Ns, 3] light that the kernels never build.
For the record only (bench.py does not time these calls).

Geometry: the cfg3 shading inputs (svgir_harness.shade_inputs.make), explicit directions: P = 200 000, Ns = 64 with M = 32 and 128 lobes, and
P = 100 000, Ns = 384, M = 32; the lobes are the reference's initialisation (randn, sharpness x 100).
Per call: the three variants alternated in one process, warm-up, the median of `--reps` event-timed calls, output allocation included.
`max_abs_diff`: the kernels' per-surfel mean of the global light against the torch composition clamp(L, 0, 64) * visibility.
Acceptance (a sanity bound with no margin): SG forward <= texture forward + (c) -- the fused evaluation must not lose to materialising the
light, which it replaces together with the lookup.
`--bench-ab DIR`: folds the `bench.py` result lines of the unchanged workloads (files DIR/{parent,new}_<workload>_<i>.json, written by
alternating runs of the parent commit's build and this one in one GPU session) into the record, with the spread of the parent's repeats.
    python scripts/sg_light_timing.py [--out profiles/sg_light_timing.json]   (on the GPU box)"""
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
from gaussian_renderer import shading  # noqa: E402
from svgir_harness import shade_inputs  # noqa: E402


def render_envmap_sg(lgtSGs, viewdirs, batch_size=10000):
    M = lgtSGs.shape[0]
    lgtSGs = lgtSGs.view((1,) * (len(viewdirs.shape) - 1) + (M, 7))
    lobes = lgtSGs[..., :3] / (torch.norm(lgtSGs[..., :3], dim=-1, keepdim=True))
    lambdas, mus = torch.abs(lgtSGs[..., 3:4]), torch.abs(lgtSGs[..., -3:])
    out = []
    for i in range(0, viewdirs.shape[0], batch_size):
        vb = viewdirs[i:i + batch_size].unsqueeze(-2)
        dot = torch.sum(vb * lobes.expand(vb.shape[:-2] + (M, 3)), dim=-1, keepdim=True)
        out.append(torch.sum(mus.expand(vb.shape[:-2] + (M, 3)) * torch.exp(lambdas.expand(vb.shape[:-2] + (M, 1)) * (dot - 1.)), dim=-2))
    return torch.cat(out, dim=0)


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


def one(P, Ns, M, reps, warmup, dev):
    d = shade_inputs.make(P, Ns, seed=3, device=dev)
    lobes = shade_inputs.sg_lobes(M, seed=11, device=dev)
    lights = {"sg": shade_inputs.SGLight(lobes), "texture": shade_inputs.Light(d["env"])}
    names = ("base_color", "roughness", "normals", "radiance")

    def call(kind, grad):
        lv = {k: d[k].detach().requires_grad_(grad) for k in names}
        light = lights[kind]
        if grad:
            light = shade_inputs.SGLight(lobes.detach().requires_grad_(True)) if kind == "sg" else shade_inputs.Light(d["env"].detach().requires_grad_(True))
        pbr, ex = shading.rendering_equation4(lv["base_color"], lv["roughness"], lv["normals"], d["viewdirs"], lv["radiance"], light,
                                              visibility_precompute=d["visibility"], incident_dirs_precompute=d["dirs"],
                                              incident_areas_precompute=d["areas"])
        if grad:
            (pbr.sum() + ex["diffuse_light"].sum()).backward()
        return ex

    with torch.no_grad():
        L = render_envmap_sg(lobes, d["dirs"])
        ref = (L.clamp(0, 64) * d["visibility"]).mean(1)
        got = call("sg", False)["global_incident_lights"][:, 0]
    rec = {"P": P, "Ns": Ns, "M": M, "max_abs_diff": float((got - ref).abs().max()), "max_global_light": float(ref.max()),
           "samples_clamped_fraction": float((L > 64).any(-1).float().mean())}
    del L, ref, got
    fns = {"sg_forward": lambda: call("sg", False), "texture_forward": lambda: call("texture", False),
           "torch_render_envmap_sg": lambda: render_envmap_sg(lobes, d["dirs"]),
           "sg_forward_backward": lambda: call("sg", True), "texture_forward_backward": lambda: call("texture", True)}
    with torch.no_grad():
        t = timed({k: fns[k] for k in ("sg_forward", "texture_forward", "torch_render_envmap_sg")}, reps, warmup)
    t.update(timed({k: fns[k] for k in ("sg_forward_backward", "texture_forward_backward")}, reps, warmup))
    rec["ms"] = t
    rec["accepted"] = bool(t["sg_forward"]["median"] <= t["texture_forward"]["median"] + t["torch_render_envmap_sg"]["median"])
    return rec


def bench_ab(d):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.json"))):
        side, rest = os.path.basename(path)[:-5].split("_", 1)
        workload = rest.rsplit("_", 1)[0]
        lines = [l for l in open(path).read().splitlines() if l.startswith("{")]
        if lines:
            out.setdefault(workload, {}).setdefault(side, []).append(json.loads(lines[-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bench-ab", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sg_light_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sg_light_timing needs a GPU"
    dev = torch.device("cuda:0")
    results = [one(P, Ns, M, args.reps, args.warmup, dev) for P, Ns, M in ((200000, 64, 32), (200000, 64, 128), (100000, 384, 32))]
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events around one call (output allocation and every kernel of the call), variants alternated, median of reps",
              "acceptance": "sg_forward <= texture_forward + torch_render_envmap_sg (medians), per geometry",
              "accepted": all(r["accepted"] for r in results), "results": results}
    if args.bench_ab:
        result["unchanged_workloads"] = bench_ab(args.bench_ab)
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
