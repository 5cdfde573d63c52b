"""HIP-event times of the fused geometry losses (csrc/geom_loss.hip) next to the composition they replace, forward + backward at 800 x 800.
For the record only (bench.py does not time these calls).

  surface : losses.surface_loss                       vs  render_view.depth2normal (its kernel) + eager cos_loss + autograd into the
                                                          depth2normal adjoint kernel
  all four: losses.geometry_losses, all four terms    vs  the same composition + the eager mono-normal cos_loss, MaxPool2d(9, 1, 4) and the
                                                          entropy lines (gaussian_renderer/render.py:157-188)

Same process, A B B A order per repetition pair; per variant the median of `--reps` event-timed forward + backward calls with the min ... max
range.  "Faster" = the two ranges do not overlap.  The fused kernels' bytes moved (every plane read or written once, halos not counted) and
the GB/s that figure implies are recorded next to the times.
    python scripts/geom_loss_timing.py [--out profiles/geom_loss_timing.json]   (on the GPU box)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd"))
sys.path.insert(0, ROOT)
from svgir_harness import losses, render_view  # noqa: E402

FOVX, FOVY, PRCP = 0.9, 0.6, (0.47, 0.55)


def eager_cos_loss(output, gt, weight=1):
    cos = torch.sum(output * gt * weight, 0)
    return (1 - cos[cos < 1]).mean()


def make_inputs(H, W, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = (3.0 + 0.001 * xx - 0.002 * yy + 0.3 * torch.sin(xx * 0.03) * torch.cos(yy * 0.02) + 0.002 * torch.rand(H, W, generator=g))[None]
    mask = ((yy - 0.5 * H) ** 2 + (xx - 0.5 * W) ** 2 <= (0.42 * min(H, W)) ** 2)[None].float()
    d2n = render_view.depth2normal(depth.to(dev), mask.to(dev), FOVX, FOVY, PRCP).cpu()
    normal = torch.nn.functional.normalize(d2n + 0.05 * torch.randn(3, H, W, generator=g), dim=0)
    target = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0) * mask
    opacity = torch.rand(1, H, W, generator=g).clamp(0.01, 0.99)
    t = dict(normal=normal, depth=depth, mask=mask, target=target, opacity=opacity)
    return {k: v.to(dev).contiguous() for k, v in t.items()}


def variants(t):
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("normal", "depth", "opacity")}
    n, d, o, m, tg = leaves["normal"], leaves["depth"], leaves["opacity"], t["mask"], t["target"]
    pool = torch.nn.MaxPool2d(9, stride=1, padding=4)

    def clear():
        for v in leaves.values():
            v.grad = None

    def fused_surface():
        clear()
        (0.02 * losses.surface_loss(n, d, m, FOVX, FOVY, PRCP)).backward()

    def composed_surface():
        clear()
        (0.02 * eager_cos_loss(n, render_view.depth2normal(d, m, FOVX, FOVY, PRCP))).backward()

    def fused_all():
        clear()
        r = losses.geometry_losses(normal=n, depth=d, mask=m, opacity=o, target=tg, weight=m, fovx=FOVX, fovy=FOVY, prcppoint=PRCP)
        (0.02 * r["surface"] + 0.03 * r["target"] + 0.01 * r["mask"] + 0.1 * r["entropy"]).backward()

    def composed_all():
        clear()
        loss = 0.02 * eager_cos_loss(n, render_view.depth2normal(d, m, FOVX, FOVY, PRCP)) + 0.03 * eager_cos_loss(n, tg, weight=m)
        loss = loss + 0.01 * (o * (1 - pool(m))).mean()
        oc = o.clamp(1e-6, 1 - 1e-6)
        loss = loss + 0.1 * -(m * torch.log(oc) + (1 - m) * torch.log(1 - oc)).mean()
        loss.backward()

    return dict(fused_surface=fused_surface, composed_surface=composed_surface, fused_all=fused_all, composed_all=composed_all), leaves


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def abba(fa, fb, reps, warmup):
    for _ in range(warmup):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for i in range(reps // 2):
        ta.append(event_ms(fa)); tb.append(event_ms(fb)); tb.append(event_ms(fb)); ta.append(event_ms(fa))
    s = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}   # noqa: E731
    return s(ta), s(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[800, 800], metavar=("H", "W"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geom_loss_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "geom_loss_timing needs a GPU"
    dev = torch.device("cuda:0")
    H, W = args.size
    fns, leaves = variants(make_inputs(H, W, dev))
    # the two forms agree before they are timed
    fns["fused_all"]()
    got = {k: v.grad.clone() for k, v in leaves.items()}
    fns["composed_all"]()
    agree = {k: float((got[k] - v.grad).abs().max() / v.grad.abs().max()) for k, v in leaves.items()}
    res = {}
    for name, planes in (("surface", 5 + 5 + 4), ("all", 10 + 10 + 5)):   # fp32 planes read forward + read backward + written backward
        f, c = abba(fns["fused_" + name], fns["composed_" + name], args.reps, args.warmup)
        nbytes = 4 * H * W * planes
        res[name] = {"fused_ms": f, "composed_ms": c, "fused_faster": bool(f["max"] < c["min"]), "speedup_median": c["median"] / f["median"],
                     "fused_bytes_moved": nbytes, "fused_GBps_at_median": nbytes / (f["median"] * 1e-3) / 1e9}
        print(json.dumps({name: res[name]}), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "size": [H, W], "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events around one forward + backward call (autograd and allocations included), A B B A order, median and min ... max",
              "bytes_moved": "fp32 planes the two fused kernels read (forward, backward) and write (backward), each counted once",
              "max_relative_gradient_difference_fused_vs_composed": agree, "results": res}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
