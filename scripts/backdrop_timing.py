"""HIP-event times of the eval view's environment backdrop (csrc/backdrop.hip: `svgir_harness.render_view.environment_backdrop`) next to
the lines it replaces, run as eager torch fp32 on the same GPU -- `Camera.get_world_directions`, `DirectLightMap.direct_light` and the
three images of gaussian_renderer/svgss.py:255-260, i.e. what a user of the reference runs today at the end of every eval view.  The
comparison is against that and against nothing else.  For the record only (bench.py does not time this call).

Images of 800 x 800 and 1600 x 1600, a DirectLightMap of 32 x 64 and one of 256 x 512.  Per call: the median of `--reps` event-timed calls
after warm-up, output allocation, the table prologue and the host-side set-up included.  The kernel moves 28 B in and 36 B out per pixel;
`call_GBps` is that traffic over the call's median time (launch and host set-up included), `kernel_only_GBps` over the kernel's own time
(the library's stage events, svgir_set_profiling: `kernel_only_ms`, mean of reps), next to the chip's ~8 TB/s peak.
`kernel_beats_eager` is the condition; the ratio is recorded, none was fixed in advance.
    python scripts/backdrop_timing.py [--out profiles/backdrop_timing.json]   (on the GPU box)"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd"))
sys.path.insert(0, ROOT)
from gaussian_renderer import _native as N  # noqa: E402
from svgir_harness import render_view, shade_inputs  # noqa: E402

BYTES_PER_PIXEL = 64


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


def _srgb(img):
    img = torch.where(img > 0.0031308, torch.pow(torch.max(img, torch.tensor(0.0031308, device=img.device)), 1.0 / 2.4) * 1.055 - 0.055, 12.92 * img)
    return torch.clamp(img, 0.0, 1.0)


def eager(env, K, c2w, image, opacity, vfeature):
    """The reference's lines in its operation order, torch fp32 on the GPU (K, c2w: device tensors, as the reference's Camera holds them)."""
    H, W = image.shape[-2:]
    dev = image.device
    v, u = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    d = torch.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], torch.ones_like(u)], dim=0)
    d = F.normalize(d, dim=0)
    d = (c2w[:3, :3] @ d.reshape(3, -1)).reshape(3, H, W)
    dirs = d.permute(1, 2, 0).reshape(-1, 3)
    envir_map = F.softplus(env).permute(0, 3, 1, 2)
    phi = torch.arccos(dirs[:, 2]).reshape(-1) - 1e-6
    theta = torch.atan2(dirs[:, 1], dirs[:, 0]).reshape(-1)
    query_y = (phi / np.pi) * 2 - 1
    query_x = -theta / np.pi
    grid = torch.stack((query_x, query_y)).permute(1, 0).unsqueeze(0).unsqueeze(0)
    light = F.grid_sample(envir_map, grid, align_corners=True).squeeze().permute(1, 0).reshape(-1, 3) * 2.0
    direct_env = light.reshape(H, W, 3).permute(2, 0, 1)
    pbr = vfeature[:3] / opacity.clamp_min(1e-5)
    return dict(render_env=image + (1 - opacity) * _srgb(direct_env), pbr_env=_srgb(pbr * opacity + (1 - opacity) * direct_env),
                env_only=_srgb(direct_env))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backdrop_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "backdrop_timing needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    Q, _ = np.linalg.qr(torch.randn(3, 3, generator=g).double().numpy())
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    c2w = torch.eye(4)
    c2w[:3, :3] = torch.from_numpy(Q).float()
    results = []
    for size in (800, 1600):
        K = torch.tensor([[1.2 * size, 0, size / 2], [0, 1.2 * size, size / 2], [0, 0, 1]], dtype=torch.float32)
        image, opacity = torch.rand(3, size, size, generator=g).to(dev), torch.rand(1, size, size, generator=g).to(dev)
        vfeature = (1.2 * torch.rand(16, size, size, generator=g)).to(dev)
        Kd, c2wd = K.to(dev), c2w.to(dev)
        for He, We in ((32, 64), (256, 512)):
            light = shade_inputs.Light((-6.0 * torch.rand(1, He, We, 3, generator=g)).to(dev))
            kern = lambda: render_view.environment_backdrop(light, K, c2w, image, opacity, vfeature)  # noqa: E731
            eag = lambda: eager(light.env, Kd, c2wd, image, opacity, vfeature)  # noqa: E731
            a, b = kern(), eag()
            rec = {"W": size, "H": size, "env_h": He, "env_w": We,
                   "max_abs_diff_vs_eager": {k: float((a[k] - b[k]).abs().max()) for k in a}}
            rec["kernel_ms"] = event_ms(kern, args.reps, args.warmup)
            rec["eager_ms"] = event_ms(eag, args.reps, args.warmup)
            rec["kernel_ms_second_pass"] = event_ms(kern, args.reps, args.warmup)     # A B A: the order does not decide the result
            rec["ratio_eager_over_kernel"] = rec["eager_ms"]["median"] / rec["kernel_ms"]["median"]
            rec["kernel_beats_eager"] = bool(max(rec["kernel_ms"]["median"], rec["kernel_ms_second_pass"]["median"]) < rec["eager_ms"]["median"])
            rec["call_GBps"] = BYTES_PER_PIXEL * size * size / (rec["kernel_ms"]["median"] * 1e-3) / 1e9
            N.set_profiling(True)
            for _ in range(args.reps):
                kern()
            torch.cuda.synchronize()
            stages = dict(N.last_timings())
            N.set_profiling(False)
            rec["kernel_only_ms"] = {"backdrop": stages["backdrop"], "env_table": stages["backdrop_env_table"]}
            rec["kernel_only_GBps"] = BYTES_PER_PIXEL * size * size / (stages["backdrop"] * 1e-3) / 1e9
            results.append(rec)
            del a, b
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events around one call (output allocation, table prologue and every kernel of the call), median of reps",
              "eager": "Camera.get_world_directions + DirectLightMap.direct_light + svgss.py:258-260 as torch fp32 on the GPU",
              "bytes_per_pixel": BYTES_PER_PIXEL, "kernel_beats_eager": all(r["kernel_beats_eager"] for r in results), "results": results}
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
