"""Times of the exact median's two consumers (csrc/select.hip) next to the reference's torch lines on the same device.  For the record
only (bench.py does not time these calls; nothing is gated on the result).

  albedo : metrics.albedo_scale_median(render, gt)   vs  eval_relighting_tensoIR.py:227-237 -- srgb_to_rgb, mean > 0, boolean indexing
           at 800 x 800                                   (nonzero: a host wait), clamp, sort-based median
  loss   : losses.surface_center_loss(xyz), forward  vs  gaussian_renderer/render.py:218-219 through torch autograd
           + backward, at P = 200 000 and 1 000 000

Same process, A B B A order per repetition pair.  Two clocks per variant, each over `--inner` calls in a row and divided by it:
  event_ms  HIP events around the calls: the device's time from the first enqueue to the last kernel's end
  host_ms   the host clock from the first call to the return of the last one, WITHOUT a synchronise: how long the host is held.  The
            library's calls only enqueue; the torch albedo lines wait for the device inside boolean indexing, so their host_ms contains
            that wait -- it is the figure the issue asks to be shown separately.
Per figure the median of `--reps` samples with the min ... max range; "faster" = the two ranges do not overlap.
    python scripts/median_timing.py [--out profiles/median_timing.json]   (on the GPU box)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd"))
sys.path.insert(0, ROOT)
from svgir_harness import losses, metrics  # noqa: E402


def srgb_to_rgb(img):   # utils/graphics_utils.py:218-229
    return torch.where(img <= 0.04045, img / 12.92, torch.pow((torch.max(img, torch.tensor(0.04045, device=img.device)) + 0.055) / 1.055, 2.4))


def torch_albedo(render, gt):   # eval_relighting_tensoIR.py:227-237
    render_albedo = srgb_to_rgb(render)
    img_mask = render_albedo.mean(dim=0) > 0
    render_albedo = render_albedo.permute(1, 2, 0)[img_mask]
    gt_albedo = gt.permute(1, 2, 0)[img_mask]
    return (gt_albedo / render_albedo).clamp(1e-6, 10).median(dim=0).values


def torch_loss(xyz):            # gaussian_renderer/render.py:218-219
    center, _ = torch.median(xyz, dim=0)
    return torch.exp(-(xyz - center[None, ...]).abs().mean())


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner, host / inner


def abba(fa, fb, reps, warmup, inner):
    for _ in range(warmup):
        fa(); fb()
    ta, tb = [], []
    for _ in range(reps // 2):
        ta.append(sample(fa, inner)); tb.append(sample(fb, inner)); tb.append(sample(fb, inner)); ta.append(sample(fa, inner))
    s = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}   # noqa: E731
    both = lambda t: {"event_ms": s([x[0] for x in t]), "host_ms": s([x[1] for x in t])}          # noqa: E731
    return both(ta), both(tb)


def entry(lib, ref):
    return {"library": lib, "torch": ref, "library_faster": bool(lib["event_ms"]["max"] < ref["event_ms"]["min"]),
            "speedup_median": ref["event_ms"]["median"] / lib["event_ms"]["median"],
            "torch_host_wait_ms_median": ref["host_ms"]["median"], "library_host_ms_median": lib["host_ms"]["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[800, 800], metavar=("H", "W"))
    ap.add_argument("--points", type=int, nargs="+", default=[200000, 1000000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "median_timing needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    H, W = args.size
    res = {}
    # a rendered albedo with a zero background (60 % of the pixels selected) and a ground truth that puts part of the ratios on the clamp
    render = (0.06 + 0.9 * torch.rand(3, H, W, generator=g)) * (torch.rand(1, H, W, generator=g) < 0.6)
    gt = torch.rand(3, H, W, generator=g) * torch.where(torch.rand(3, H, W, generator=g) < 0.5, 0.2, 1.0)
    render, gt = render.to(dev).contiguous(), gt.to(dev).contiguous()
    lib_scale, lib_count = metrics.albedo_scale_median(render, gt)
    ref_scale = torch_albedo(render, gt)
    agree = {"albedo_max_relative_difference": float(((lib_scale - ref_scale).abs() / ref_scale.abs()).max()), "albedo_selected": int(lib_count)}
    lib, ref = abba(lambda: metrics.albedo_scale_median(render, gt), lambda: torch_albedo(render, gt), args.reps, args.warmup, args.inner)
    res[f"albedo_{H}x{W}"] = entry(lib, ref)
    print(json.dumps({f"albedo_{H}x{W}": res[f"albedo_{H}x{W}"]}), flush=True)
    for P in args.points:
        x = (torch.randn(P, 3, generator=g) * torch.tensor([1.0, 0.5, 2.0])).to(dev).requires_grad_(True)

        def fused():
            x.grad = None
            losses.surface_center_loss(x).backward()

        def composed():
            x.grad = None
            torch_loss(x).backward()

        fused()
        got = x.grad.clone()
        composed()
        # the median's own rows apart: there torch holds an fp32 sum of P terms of +-g L / (3 P) that cancel, the kernel the exact count
        diff = (got - x.grad).abs()
        rows = losses.surface_center_loss(x.detach(), with_stats=True)[1][[2, 5, 8]].long()
        at_median = diff[rows, torch.arange(3, device=dev)].max()
        diff[rows, torch.arange(3, device=dev)] = 0
        agree[f"loss_{P}_max_gradient_difference_over_max"] = {"median_rows": float(at_median / x.grad.abs().max()),
                                                               "other_rows": float(diff.max() / x.grad.abs().max())}
        lib, ref = abba(fused, composed, args.reps, args.warmup, args.inner)
        res[f"loss_fwd_bwd_{P}"] = entry(lib, ref)
        print(json.dumps({f"loss_fwd_bwd_{P}": res[f"loss_fwd_bwd_{P}"]}), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "inner": args.inner,
              "timing": "per call, over `inner` calls in a row: event_ms = HIP events (device time), host_ms = host clock without a synchronise "
                        "(how long the host is held; the torch albedo lines wait for the device inside boolean indexing); A B B A order, "
                        "median and min ... max; allocations and autograd included",
              "agreement_before_timing": agree, "results": res}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
