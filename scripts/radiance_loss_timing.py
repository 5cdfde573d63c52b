"""HIP-event times of the fused radiance-consistency loss (`svgir_harness.losses.fused_radiance_loss`: svgir_radiance_loss_forward /
_backward, csrc/irradiance.hip) next to the path it replaces on the same inputs: `svgir_harness.losses.radiance_loss` fed
envmap = direct_light(incident_dirs) * incident_areas composed in torch (arccos, atan2, grid_sample over N * S directions, a multiply;
the selection, the gather and l1_loss in torch around the irradiance kernel).  For the record only (bench.py does not time these calls):
the traced scene of scripts/radiance_timing.py -- N = 200 000 surfels of the cfg3 geometry, S = 64, first hits, uvs, radiances and
visibility from `Renderer.render_radiance_with_sampling_SH` as GaussianModel.update_radiace leaves them -- under a learnable
DirectLightMap-like map of 32 x 64 (the env gradient accumulates in the LDS table) and of 128 x 256 (the reference's default: global
float atomics).

Per call: the median of `--reps` event-timed calls after `--warmup`, allocation of the outputs included; forward, backward
(torch.autograd.grad from the retained forward) and forward + backward as one timed region.  Next to the times: the peak allocated bytes
of one forward + backward of either path above what the inputs hold, and for the 128 x 256 map the rate of the fallback's atomic bytes
(4 bytes per add: 12 per contributing sample, 13 per hit row) against the ~1.3 TB/s chip-wide float-atomic rate.
    python scripts/radiance_loss_timing.py [--out profiles/radiance_loss_timing.json]   (on the GPU box)"""
import argparse
import json
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd"))
sys.path.insert(0, ROOT)
from svgir_harness import losses, workloads  # noqa: E402

ATOMIC_RATE_TBS = 1.3


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def composed_light(env, dirs):
    """2 * bilinear(softplus(env)) along `dirs` [N,S,3] with torch's grid_sample: the lat-long lookup of a DirectLightMap"""
    d = dirs.reshape(-1, 3)
    lat = torch.arccos(d[:, 2]) - 1e-6
    lon = torch.atan2(d[:, 1], d[:, 0])
    grid = torch.stack((-lon / math.pi, lat / math.pi * 2 - 1), dim=-1)[None, None]
    tex = torch.nn.functional.softplus(env).permute(0, 3, 1, 2)
    return torch.nn.functional.grid_sample(tex, grid, align_corners=True)[0, :, 0].t().reshape(dirs.shape) * 2.0


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200000)
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance_loss_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "radiance_loss_timing needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    S = args.S
    tc = workloads.TracerCache(dev, "cfg3_train", S, P=args.N)
    N = tc.P
    R = tc.Renderer()
    R.set_proxy(tc.xyz, tc.scales, tc.rot, tc.normals, tc.opacity, tc.shs)
    R.build_bvh()
    chunk = N // ((S - 1) // 24 + 1)
    dirs, areas, rads, viss, hits, uvs = [], [], [], [], [], []
    for off in range(0, N, chunk):       # GaussianModel.update_radiace
        d, a = tc.shading.sample_incident_rays(tc.normals[off:off + chunk], True, S)
        rad, vis, h, uv = R.render_radiance_with_sampling_SH(tc.xyz[off:off + chunk], d, tc.cov_inv, S)
        dirs.append(d); areas.append(a); rads.append(rad); viss.append(vis); hits.append(h); uvs.append(uv)
    ray_d, areas, radiances, visibility = (torch.cat(x).contiguous() for x in (dirs, areas, rads, viss))
    ray_d[..., 2].clamp_(-1.0, 1.0)
    areas = areas.reshape(N, S, 1)
    R.hemi_index_buffers, R.uv_buffers = torch.cat(hits), torch.cat(uvs)
    hit = R.hemi_index_buffers.reshape(N, S)
    geo = torch.nn.functional.normalize(tc.normals, dim=-1)
    cam = torch.tensor([0.3, -2.5, 0.4], device=dev)
    normals12 = (tc.normals[:, :, None] + 0.1 * torch.randn(N, 3, 4, device=dev)).reshape(N, 12).contiguous()
    albedos = torch.rand(N, 12, device=dev).requires_grad_(True)
    rough = (torch.rand(N, 4, device=dev) * 0.9 + 0.09).requires_grad_(True)
    ratio = torch.ones((), device=dev).requires_grad_(True)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "N": N, "S": S,
              "timing": "HIP events around one call (output allocation and every kernel of the call), median of reps",
              "parent_path": "losses.radiance_loss with envmap = 2 * grid_sample(softplus(env)) * areas composed in torch", "results": []}
    for He, We in ((32, 64), (128, 256)):
        env = (0.5 * torch.randn(1, He, We, 3, device=dev)).requires_grad_(True)
        light = types.SimpleNamespace(env=env)
        leaves = (env, albedos, rough, ratio)

        def fused():
            return losses.fused_radiance_loss(R, tc.xyz, cam, geo, ray_d, areas, visibility, light, normals12, albedos, rough, radiances, ratio)

        def parent():
            envmap = composed_light(env, ray_d) * areas
            return losses.radiance_loss(R, tc.xyz, cam, geo, ray_d, visibility, envmap, normals12, albedos, rough, radiances, ratio)

        rec = {"env": [He, We]}
        lf, idx, _ = losses.fused_radiance_loss(R, tc.xyz, cam, geo, ray_d, areas, visibility, light, normals12, albedos, rough, radiances, ratio,
                                                with_rows=True)
        lp = parent()
        gf, gp = torch.autograd.grad(lf, leaves, retain_graph=True), torch.autograd.grad(lp, leaves, retain_graph=True)
        rec["loss"] = {"fused": float(lf), "parent": float(lp)}
        rec["grad_max_rel_diff_vs_parent"] = [float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(gf, gp)]
        h_s = hit[torch.arange(N, device=dev), idx.long()].long()
        rec["primary_hits"] = int((h_s >= 0).sum())
        rec["contributing_samples"] = int(((hit[h_s.clamp(0)] == -1) & (h_s >= 0)[:, None]).sum())
        for name, fn, l in (("fused", fused, lf), ("parent", parent, lp)):
            rec[name + "_forward_ms"] = event_ms(fn, args.reps, args.warmup)
            rec[name + "_backward_ms"] = event_ms(lambda: torch.autograd.grad(l, leaves, retain_graph=True), args.reps, args.warmup)
            rec[name + "_forward_backward_ms"] = event_ms(lambda: torch.autograd.grad(fn(), leaves), args.reps, args.warmup)
        del lf, lp, gf, gp, l
        for name, fn in (("fused", fused), ("parent", parent)):
            rec[name + "_peak_bytes"] = peak_bytes(lambda: torch.autograd.grad(fn(), leaves))
        rec["speedup_forward_backward"] = rec["parent_forward_backward_ms"]["median"] / rec["fused_forward_backward_ms"]["median"]
        rec["fused_median_below_parent_minimum"] = rec["fused_forward_backward_ms"]["median"] < rec["parent_forward_backward_ms"]["min"]
        if He * We * 24 + 64 > 160 * 1024:     # the global-atomic fallback of the env gradient
            nbytes = 4 * (12 * rec["contributing_samples"] + 13 * rec["primary_hits"])
            rec["backward_atomic_bytes"] = nbytes
            rec["backward_atomic_TBps"] = nbytes / (rec["fused_backward_ms"]["median"] * 1e-3) / 1e12
            rec["atomic_rate_reference_TBps"] = ATOMIC_RATE_TBS
        result["results"].append(rec)
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
