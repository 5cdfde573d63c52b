"""HIP-event times of the spherical-Gaussian light's three paths around the shading, each next to what it replaces or mirrors, on the
same library (for the record only: bench.py does not time these calls):

  loss      `losses.fused_radiance_loss_sg` (svgir_radiance_loss_forward_sg / _backward_sg) forward + backward against the composed path
            `losses.radiance_loss(sg_direct_light(lgtSGs, dirs) * areas)` and, for orientation, the fused texture loss, at the traced scene
            of scripts/radiance_loss_timing.py: N = 200 000 surfels of the cfg3 geometry through TracerCache, S = 64, M = 32;
  eval      `svgir_sg_eval_backward` (through sg_direct_light, gradient to the lobes and the directions) against torch autograd of the
            reference's `render_envmap_sg` (its 10 000-row batches) at 200 000 x 64 directions, M = 32: the point of sg_light_timing.json;
  backdrop  `sg_environment_backdrop` against `environment_backdrop` (a 32 x 64 DirectLightMap) at 800 x 800.
The variants of a group are alternated in one process: warm-up, then `--reps` rounds of one event-timed call each; median, min and max.
Acceptance: the fused SG loss is not slower than the composed path, and the SG eval backward not slower than torch's, by more than the
spread (max - min) of the slower side; the ratios are reported.

`--dump FILE [--lib PATH]`: writes the outputs of svgir_radiance_loss_forward / _backward and svgir_env_backdrop on one existing case each
(radiance_loss_cases `random_70x64`, backdrop_cases `fixture_camera_8x16`) through raw ctypes on the library at PATH -- the parent
commit's build or this one; `--compare A B` records which arrays are byte-identical (`--unchanged FILE` folds that into the result).
`--bench-ab DIR`: folds bench.py result lines (DIR/{parent,new}_<workload>_<i>.json from alternating runs) into the record.
    python scripts/sg_paths_timing.py [--out profiles/sg_paths_timing.json]   (on the GPU box)"""
import argparse
import ctypes as C
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


def not_slower(new, old):
    """new's median within old's median + the spread of the slower side"""
    slow = new if new["median"] > old["median"] else old
    return bool(new["median"] <= old["median"] + (slow["max"] - slow["min"]))


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


def loss_group(dev, N, S, M, reps, warmup):
    import types
    from gaussian_renderer import shading
    from svgir_harness import losses, shade_inputs, workloads
    tc = workloads.TracerCache(dev, "cfg3_train", S, P=N)
    N = tc.P
    R = tc.Renderer()
    R.set_proxy(tc.xyz, tc.scales, tc.rot, tc.normals, tc.opacity, tc.shs)
    R.build_bvh()
    chunk = N // ((S - 1) // 24 + 1)
    parts = [[] for _ in range(6)]
    for off in range(0, N, chunk):       # GaussianModel.update_radiace
        d, a = tc.shading.sample_incident_rays(tc.normals[off:off + chunk], True, S)
        for lst, t in zip(parts, (d, a) + tuple(R.render_radiance_with_sampling_SH(tc.xyz[off:off + chunk], d, tc.cov_inv, S))):
            lst.append(t)
    ray_d, areas, radiances, visibility = (torch.cat(x).contiguous() for x in parts[:4])
    ray_d = torch.nn.functional.normalize(ray_d, dim=-1)
    ray_d[..., 2].clamp_(-1.0, 1.0)
    areas = areas.reshape(N, S, 1)
    R.hemi_index_buffers, R.uv_buffers = torch.cat(parts[4]), torch.cat(parts[5])
    geo = torch.nn.functional.normalize(tc.normals, dim=-1)
    cam = torch.tensor([0.3, -2.5, 0.4], device=dev)
    normals12 = (tc.normals[:, :, None] + 0.1 * torch.randn(N, 3, 4, device=dev)).reshape(N, 12).contiguous()
    albedos = torch.rand(N, 12, device=dev).requires_grad_(True)
    rough = (torch.rand(N, 4, device=dev) * 0.9 + 0.09).requires_grad_(True)
    ratio = torch.ones((), device=dev).requires_grad_(True)
    lobes = shade_inputs.sg_lobes(M, seed=11, device=dev)
    lobes[:, 3] *= 0.2          # sharpness |N(0,1)| * 20: lobes a hemisphere of 64 samples meets
    lobes.requires_grad_(True)
    env = (0.5 * torch.randn(1, 32, 64, 3, device=dev)).requires_grad_(True)
    sgl, texl = shade_inputs.SGLight(lobes), types.SimpleNamespace(env=env)
    common = (R, tc.xyz, cam, geo, ray_d)
    tail = (normals12, albedos, rough, radiances, ratio)

    def fused():
        return losses.fused_radiance_loss_sg(*common, areas, visibility, sgl, *tail)

    def composed():
        return losses.radiance_loss(*common, visibility, shading.sg_direct_light(lobes, ray_d) * areas, *tail)

    def texture():
        return losses.fused_radiance_loss(*common, areas, visibility, texl, *tail)

    sg_leaves, tex_leaves = (lobes, albedos, rough, ratio), (env, albedos, rough, ratio)
    lf, lc_ = fused(), composed()
    gf, gc = torch.autograd.grad(lf, sg_leaves), torch.autograd.grad(lc_, sg_leaves)
    rec = {"N": N, "S": S, "M": M, "loss": {"fused_sg": float(lf), "composed_sg": float(lc_), "fused_texture": float(texture())},
           "grad_max_rel_diff_fused_vs_composed": [float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(gf, gc)]}
    # the composed path selects with torch's own reduction: rows whose two best scores lie within an fp32 rounding of each other may
    # pick another sample there, and with it another hit surfel; the per-surfel gradients are compared outside those surfels as well
    with torch.no_grad():
        _, idx, _ = losses.fused_radiance_loss_sg(*common, areas, visibility, sgl, *tail, with_rows=True)
        view_dirs = torch.nn.functional.normalize(tc.xyz - cam, dim=-1)
        refl = 2 * torch.sum(geo * view_dirs, dim=-1, keepdim=True) * geo + view_dirs
        sel = torch.argmax(torch.sum(ray_d * refl[:, None], dim=-1) * (1 - visibility.reshape(N, S)), dim=-1)
        differs = sel != idx.long()
        hit = R.hemi_index_buffers.reshape(N, S).long()
        rows = torch.nonzero(differs)[:, 0]
        touched = torch.zeros(N, dtype=torch.bool, device=dev)
        for h in (hit[rows, sel[rows]], hit[rows, idx.long()[rows]]):
            touched[h[(h >= 0) & (h < N)]] = True
        rec["rows_selected_differently_by_torch"] = int(differs.sum())
        rec["grad_max_rel_diff_outside_their_hit_surfels"] = [float(((a - b).abs()[~touched]).max() / b.abs().max().clamp_min(1e-30))
                                                              for a, b in zip(gf[1:3], gc[1:3])]
    del lf, lc_, gf, gc
    rec["forward_backward_ms"] = timed({"fused_sg": lambda: torch.autograd.grad(fused(), sg_leaves),
                                        "composed_sg": lambda: torch.autograd.grad(composed(), sg_leaves),
                                        "fused_texture": lambda: torch.autograd.grad(texture(), tex_leaves)}, reps, warmup)
    with torch.no_grad():
        rec["forward_ms"] = timed({"fused_sg": fused, "composed_sg": composed, "fused_texture": texture}, reps, warmup)
    t = rec["forward_backward_ms"]
    rec["speedup_vs_composed"] = t["composed_sg"]["median"] / t["fused_sg"]["median"]
    rec["ratio_to_fused_texture"] = t["fused_sg"]["median"] / t["fused_texture"]["median"]
    rec["accepted"] = not_slower(t["fused_sg"], t["composed_sg"])
    return rec


def eval_group(dev, P, Ns, M, reps, warmup):
    from gaussian_renderer import shading
    from svgir_harness import shade_inputs
    d = shade_inputs.make(P, Ns, seed=3, device=dev)
    dirs = d["dirs"].contiguous()          # [P, Ns, 3]: the reference's batches are 10 000 rows of Ns directions
    up = torch.randn_like(dirs)
    lobes = shade_inputs.sg_lobes(M, seed=11, device=dev)

    def run(fn, want_dirs):
        lb, dd = lobes.detach().requires_grad_(True), dirs.detach().requires_grad_(want_dirs)
        return torch.autograd.grad((fn(lb, dd) * up).sum(), (lb, dd) if want_dirs else (lb,))

    a, b = run(shading.sg_direct_light, True), run(render_envmap_sg, True)
    rec = {"directions": int(dirs.numel() // 3), "M": M,
           "grad_max_rel_diff_vs_torch": [float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(a, b)]}
    del a, b
    rec["ms"] = timed({"hip_lobes": lambda: run(shading.sg_direct_light, False), "torch_lobes": lambda: run(render_envmap_sg, False),
                       "hip_lobes_and_dirs": lambda: run(shading.sg_direct_light, True),
                       "torch_lobes_and_dirs": lambda: run(render_envmap_sg, True)}, reps, warmup)
    with torch.no_grad():
        rec["ms"].update(timed({"hip_forward": lambda: shading.sg_direct_light(lobes, dirs), "torch_forward": lambda: render_envmap_sg(lobes, dirs)},
                               reps, warmup))
    t = rec["ms"]
    rec["note"] = "forward + backward in one timed region (torch cannot run its backward without its forward's graph)"
    rec["speedup_lobes"] = t["torch_lobes"]["median"] / t["hip_lobes"]["median"]
    rec["speedup_lobes_and_dirs"] = t["torch_lobes_and_dirs"]["median"] / t["hip_lobes_and_dirs"]["median"]
    rec["accepted"] = not_slower(t["hip_lobes"], t["torch_lobes"]) and not_slower(t["hip_lobes_and_dirs"], t["torch_lobes_and_dirs"])
    return rec


def backdrop_group(dev, W, H, M, reps, warmup):
    from svgir_harness import render_view, shade_inputs
    g = torch.Generator().manual_seed(5)
    image, opacity, vfeature = (torch.rand(*s, generator=g).to(dev) for s in ((3, H, W), (1, H, W), (3, H, W)))
    K = torch.tensor([[W * 0.9, 0, W / 2], [0, W * 0.9, H / 2], [0, 0, 1.0]])
    c2w = torch.eye(4)
    lobes = shade_inputs.sg_lobes(M, seed=11, device=dev)
    lobes[:, 3] *= 0.1
    sgl, texl = shade_inputs.SGLight(lobes), shade_inputs.Light(torch.randn(1, 32, 64, 3, device=dev) - 2.0)
    t = timed({"sg": lambda: render_view.sg_environment_backdrop(sgl, K, c2w, image, opacity, vfeature),
               "texture": lambda: render_view.environment_backdrop(texl, K, c2w, image, opacity, vfeature)}, reps, warmup)
    return {"W": W, "H": H, "M": M, "ms": t, "ratio_sg_to_texture": t["sg"]["median"] / t["texture"]["median"]}


# ---- outputs of the untouched texture entry points, through raw ctypes on any build of the library -----------------------------------
class _RLParams(C.Structure):   # svgir_radiance_loss_params
    _fields_ = [("N", C.c_int32), ("S", C.c_int32)] + [(n, C.c_void_p) for n in (
        "xyz", "camera_center", "geo_normal", "ray_d", "areas", "visibility", "normals", "albedos", "roughnesses", "hit_indices", "uvs",
        "radiances", "radiance_ratio", "env")] + [("env_h", C.c_int32), ("env_w", C.c_int32), ("env_softplus", C.c_int32),
                                                  ("env_scale", C.c_float), ("env_transform", C.c_void_p), ("work", C.c_void_p)]


def dump(path, libpath):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import backdrop_cases as bc
    from tests import radiance_loss_cases as lc
    lib = C.CDLL(libpath)
    lib.svgir_radiance_loss_work_bytes.restype = C.c_size_t
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)  # noqa: E731
    c = lc.case("random_70x64")
    N, S = c["N"], c["S"]
    keep = {k: t(c[v]) for k, v in dict(xyz="xyz", camera_center="camera_center", geo_normal="geo_normal", ray_d="ray_d", areas="areas",
                                        visibility="visibility", normals="normals", albedos="albedos", roughnesses="roughnesses", hit_indices="hit",
                                        uvs="uvs", radiances="radiances", radiance_ratio="radiance_ratio", env="env").items()}
    He, We = c["env"].shape[:2]
    keep["work"] = torch.empty(lib.svgir_radiance_loss_work_bytes(C.c_int32(N), C.c_int32(He), C.c_int32(We)), dtype=torch.uint8, device=dev)
    p = _RLParams()
    p.N, p.S, p.env_h, p.env_w, p.env_softplus, p.env_scale = N, S, He, We, 1, 2.0
    for k, v in keep.items():
        setattr(p, k, v.data_ptr())
    idx, R = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, 3, device=dev)
    total, loss = torch.empty((), dtype=torch.float64, device=dev), torch.empty((), device=dev)
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    assert lib.svgir_radiance_loss_forward(C.byref(p), vp(idx), vp(R), vp(total), vp(loss), None) == 0
    g = torch.ones(1, device=dev)
    d_env, d_alb, d_rough, d_ratio = (torch.empty(s, device=dev) for s in ((He, We, 3), (N, 12), (N, 4), (1,)))
    assert lib.svgir_radiance_loss_backward(C.byref(p), vp(idx), vp(R), vp(g), vp(d_env), vp(d_alb), vp(d_rough), vp(d_ratio), None) == 0
    case = bc.cases()[0]
    H, W = case["H"], case["W"]
    K, Rm = case["K"], case["R"]
    intr, rot = (C.c_float * 4)(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), (C.c_float * 9)(*Rm.reshape(-1))
    env = t(case["tex"])[0]
    work = torch.empty(env.shape[0] * env.shape[1] * 4, device=dev)
    out = torch.empty(9, H, W, device=dev)
    image, opacity, vfeature = t(case["image"]), t(case["opacity"]), t(case["vfeature"])
    assert lib.svgir_env_backdrop(C.c_int32(W), C.c_int32(H), intr, rot, None, vp(env), C.c_int32(env.shape[0]), C.c_int32(env.shape[1]), C.c_int32(1),
                                  C.c_float(2.0), vp(work), vp(image), vp(opacity), vp(vfeature), vp(out), None) == 0
    torch.cuda.synchronize()
    np.savez(path, **{k: v.cpu().numpy() for k, v in dict(
        loss_sample_indices=idx, loss_radiance=R, loss_sum=total, loss=loss, loss_d_ratio=d_ratio, atomic_d_env=d_env, atomic_d_albedos=d_alb,
        atomic_d_roughnesses=d_rough, backdrop_out=out).items()})


def compare(a, b):
    x, y = np.load(a), np.load(b)
    rec = {}
    for k in x.files:
        same = x[k].tobytes() == y[k].tobytes()
        rec[k] = {"byte_identical": bool(same)}
        if not same:
            den = float(np.abs(x[k]).max()) or 1.0
            rec[k]["max_abs_diff_over_max"] = float(np.abs(x[k].astype(np.float64) - y[k]).max() / den)
    return {"cases": "radiance_loss_cases random_70x64, backdrop_cases fixture_camera_8x16",
            "note": "atomic_*: accumulated with float atomics, repeatable only up to the order of the adds", "arrays": rec,
            "all_non_atomic_byte_identical": all(v["byte_identical"] for k, v in rec.items() if not k.startswith("atomic_"))}


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--N", type=int, default=200000)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--lib", default=os.path.join(ROOT, "svg-ir_amd", "libsvgir_raster.so"))
    ap.add_argument("--compare", nargs=2, default=None)
    ap.add_argument("--unchanged", default=None)
    ap.add_argument("--bench-ab", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sg_paths_timing.json"))
    args = ap.parse_args()
    if args.compare:
        print(json.dumps(compare(*args.compare), indent=1))
        return
    assert torch.cuda.is_available(), "sg_paths_timing needs a GPU"
    if args.dump:
        dump(args.dump, args.lib)
        return
    assert args.reps >= 5, "the acceptance needs at least five alternating repeats"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events around one call (output allocation and every kernel of the call), variants alternated, median of reps",
              "acceptance": "new median <= old median + (max - min) of the slower side: fused SG loss vs composed, SG eval backward vs torch"}
    result["radiance_loss"] = loss_group(dev, args.N, 64, 32, args.reps, args.warmup)
    torch.cuda.empty_cache()
    result["sg_eval_backward"] = eval_group(dev, 200000, 64, 32, args.reps, args.warmup)
    torch.cuda.empty_cache()
    result["backdrop"] = backdrop_group(dev, 800, 800, 32, args.reps, args.warmup)
    result["accepted"] = bool(result["radiance_loss"]["accepted"] and result["sg_eval_backward"]["accepted"])
    if args.unchanged:
        result["texture_entry_points_parent_vs_this"] = json.load(open(args.unchanged))
    if args.bench_ab:
        result["unchanged_workloads"] = bench_ab(args.bench_ab)
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
