"""HIP-event times of the pbgi irradiance kernels (csrc/irradiance.hip: `Renderer.render_irradiance_sample` forward and backward,
`Renderer.render_irradiance`) next to the same formulas composed from eager torch gathers on the GPU -- what a user of the reference
would write without its slang kernels.  The comparison is against that and against nothing else.  For the record only (bench.py does
not time these calls): N = 200 000 surfels of the cfg3 geometry, S = 64, the first hits and uvs traced by
`Renderer.render_radiance_with_sampling_SH` as GaussianModel.update_radiace does.

Per call: the median of `--reps` event-timed calls after warm-up, output allocation included.  The eager full form is N * S * S * 4
corner terms: it is timed on `--eager-full-rows` rows and scaled to N (`eager_full_rows_timed` says so).  The backward keeps float
atomics; next to its time stands the rate of added bytes (4 bytes per atomic: every escaping sample's three d_envmap values and 13 per
row) against the ~1.3 TB/s chip-wide float-atomic rate of a 256-byte wave-instruction.
    python scripts/radiance_timing.py [--out profiles/radiance_timing.json]   (on the GPU box)"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd"))
sys.path.insert(0, ROOT)
from svgir_harness import workloads  # noqa: E402

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


def eager(view, h, ok, ray_d, env, normals, albedos, rough, hit, uvs, full):
    """entries E: view [E,3] = ray_d[i,p], h [E] (clamped), ok [E] -> [E,3]; plain torch fp32, one gather per input"""
    S = ray_d.shape[1]
    nz = torch.nn.functional.normalize
    V, L = nz(-view, dim=-1), nz(ray_d[h], dim=-1)
    H = nz(V[:, None] + L, dim=-1)
    nraw = normals[h].view(-1, 3, 4).transpose(1, 2)
    n = nz(nraw, dim=-1)
    cl = lambda x: x.clamp(1e-6, 1.0)
    NoL, NoH = cl(torch.einsum("nkc,nsc->nsk", n, L)), cl(torch.einsum("nkc,nsc->nsk", n, H))
    NoV, VoH = cl(torch.einsum("nkc,nc->nk", n, V))[:, None], cl((V[:, None] * H).sum(-1))[..., None]
    r = (rough[h] if full else rough[h][:, :1].expand(-1, 4))[:, None, :]
    a2 = r ** 4
    k = (r * r + 2 * r + 1) / 8
    fres = 0.04 + 0.96 * torch.exp2((-5.55473 * VoH - 6.98316) * VoH)
    den = (4 * math.pi * (NoH * NoH * (a2 - 1) + 1) ** 2 * (NoV * (1 - k) + k) * (NoL * (1 - k) + k)).clamp(1e-6, 4 * math.pi)
    brdf = (fres * a2 / den)[:, :, None, :] + albedos[h].view(-1, 1, 3, 4) / math.pi
    if full:
        brdf = brdf * cl(torch.einsum("nkc,nsc->nsk", nraw, L))[:, :, None, :]
    u, v = uvs[h][..., 0], uvs[h][..., 1]
    w = torch.stack([(1 - u) * (1 - v), u * (1 - v), (1 - u) * v, u * v], -1)
    free = (hit[h] == -1) & ok[:, None]
    return ((brdf * w[:, :, None, :]).sum(-1) * env[h] * free[..., None]).sum(1) / S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200000)
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eager-full-rows", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "radiance_timing needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    S = args.S
    tc = workloads.TracerCache(dev, "cfg3_train", S, P=args.N)
    N = tc.P
    R = tc.Renderer()
    R.set_proxy(tc.xyz, tc.scales, tc.rot, tc.normals, tc.opacity, tc.shs)
    R.build_bvh()
    chunk = N // ((S - 1) // 24 + 1)
    dirs, areas, hits, uvs = [], [], [], []
    for off in range(0, N, chunk):       # GaussianModel.update_radiace
        d, a = tc.shading.sample_incident_rays(tc.normals[off:off + chunk], True, S)
        _, _, h, uv = R.render_radiance_with_sampling_SH(tc.xyz[off:off + chunk], d, tc.cov_inv, S)
        dirs.append(d); areas.append(a); hits.append(h); uvs.append(uv)
    ray_d, areas = torch.cat(dirs), torch.cat(areas)
    R.hemi_index_buffers, R.uv_buffers = torch.cat(hits), torch.cat(uvs)
    hit = R.hemi_index_buffers.reshape(N, S)
    env = (torch.rand(N, S, 3, device=dev) * 2.0 * areas.reshape(N, S, 1)).contiguous()
    normals12 = (tc.normals[:, :, None] + 0.1 * torch.randn(N, 3, 4, device=dev)).reshape(N, 12).contiguous()
    albedos, rough = torch.rand(N, 12, device=dev), torch.rand(N, 4, device=dev) * 0.9 + 0.09
    sample = torch.randint(0, S, (N, 1), device=dev, dtype=torch.int32)
    g = torch.randn(N, 3, device=dev)
    ar = torch.arange(N, device=dev)
    h_s = hit[ar, sample[:, 0].long()].long()
    primary_hits = int((h_s >= 0).sum())
    free_of_hit = hit[h_s.clamp(0)] == -1
    contributing = int((free_of_hit & (h_s >= 0)[:, None]).sum())

    def kernel_fwd(leaves=None):
        e, a, r = leaves or (env, albedos, rough)
        return R.render_irradiance_sample(N, S, sample, e, ray_d, None, None, None, normals12, a, r, None, None, None)

    leaves = [t.clone().requires_grad_(True) for t in (env, albedos, rough)]
    out_k = kernel_fwd(leaves)
    eleaves = [t.clone().requires_grad_(True) for t in (env, albedos, rough)]
    eager_s = lambda lv: eager(ray_d[ar, sample[:, 0].long()], h_s.clamp(0), h_s >= 0, ray_d, lv[0], normals12, lv[1], lv[2], hit, uvs_t, False)
    uvs_t = R.uv_buffers
    out_e = eager_s(eleaves)
    rec = {"N": N, "S": S, "primary_hits": primary_hits, "contributing_terms_sample": contributing,
           "rays_missed_fraction": float((hit == -1).float().mean())}
    rec["sample_forward_max_abs_diff_vs_eager"] = float((out_k - out_e).abs().max())
    rec["sample_forward_ms"] = event_ms(lambda: kernel_fwd(), args.reps, args.warmup)
    rec["sample_backward_ms"] = event_ms(lambda: torch.autograd.grad(out_k, leaves, g, retain_graph=True), args.reps, args.warmup)
    rec["eager_sample_forward_ms"] = event_ms(lambda: eager_s((env, albedos, rough)), args.reps, args.warmup)
    rec["eager_sample_backward_ms"] = event_ms(lambda: torch.autograd.grad(out_e, eleaves, g, retain_graph=True), args.reps, args.warmup)
    gk, ge = torch.autograd.grad(out_k, leaves, g, retain_graph=True), torch.autograd.grad(out_e, eleaves, g, retain_graph=True)
    rec["sample_backward_max_rel_diff_vs_eager"] = [float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(gk, ge)]
    del out_e, eleaves, ge, gk
    torch.cuda.empty_cache()
    atomic_bytes = 4 * (3 * contributing + 13 * primary_hits)
    rec["sample_backward_atomic_bytes"] = atomic_bytes
    rec["sample_backward_atomic_TBps"] = atomic_bytes / (rec["sample_backward_ms"]["median"] * 1e-3) / 1e12
    rec["atomic_rate_reference_TBps"] = ATOMIC_RATE_TBS
    # the full form
    full = lambda: R.render_irradiance(N, S, env, ray_d, None, None, None, normals12, albedos, rough, None, None, None)
    out_f = full()
    rec["full_forward_ms"] = event_ms(full, args.reps, args.warmup)
    rows = min(N, args.eager_full_rows)
    hf = hit[:rows].reshape(-1).long()
    eager_f = lambda: eager(ray_d[:rows].reshape(-1, 3), hf.clamp(0), hf >= 0, ray_d, env, normals12, albedos, rough, hit, uvs_t, True)
    rec["full_forward_max_abs_diff_vs_eager"] = float((out_f[:rows].reshape(-1, 3) - eager_f()).abs().max())
    t = event_ms(eager_f, 5, 1)
    rec["eager_full_forward_ms"] = {k: v * N / rows for k, v in t.items()}
    rec["eager_full_rows_timed"] = rows
    for k in ("sample_forward", "sample_backward", "full_forward"):
        rec["speedup_" + k] = rec["eager_" + k + "_ms"]["median"] / rec[k + "_ms"]["median"]
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events around one call (output allocation and every kernel of the call), median of reps",
              "eager": "the same formulas as torch fp32 gathers / einsums on the GPU; the full form scaled from eager_full_rows_timed rows to N",
              "results": [rec]}
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
