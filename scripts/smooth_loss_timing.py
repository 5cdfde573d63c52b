"""HIP-event times of the fused smoothness losses (csrc/smooth_loss.hip) next to the eager composition they replace, forward + backward at
800 x 800.  For the record only (bench.py does not time these calls).

  stage2: losses.smoothness_losses, the three first-order terms of the stage-2 configuration (svgss.py:366-387: base colour [3] and
          roughness [1] against the masked ground truth, diffuse light [3] against the rendered normal, which requires grad)
                                                      vs  the same three terms from eager torch: mask products + replicate pad + conv2d + abs /
                                                          exp + .sum(1).mean() + autograd
  second: losses.second_order_edge_aware_loss on rendered_normal * mask against the ground truth (stage 1, svgss.py:395-396)
                                                      vs  its eager composition

Same process, A B B A order per repetition pair; per variant the median of `--reps` event-timed forward + backward calls with the min ... max
range.  "Faster" = the two ranges do not overlap.  The fused kernels' bytes moved (every plane read or written once, halos not counted) and
the GB/s that figure implies are recorded next to the times.
    python scripts/smooth_loss_timing.py [--out profiles/smooth_loss_timing.json]   (on the GPU box)"""
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
from svgir_harness import losses  # noqa: E402


def eager_gradient(x, order):
    """kornia's spatial_gradient(x[None], 'sobel', order, normalized=True)[0] (order 2: the xx and yy planes): [C,H,W] -> [C,2,H,W]."""
    if order == 1:
        k = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], device=x.device) / 8
    else:
        k = torch.tensor([[-1., 0., 2., 0., -1.], [-4., 0., 8., 0., -4.], [-6., 0., 12., 0., -6.], [-4., 0., 8., 0., -4.], [-1., 0., 2., 0., -1.]],
                         device=x.device) / 64
    return F.conv2d(F.pad(x[:, None], (order,) * 4, mode="replicate"), torch.stack([k, k.t()])[:, None])


def eager_first(data, img):
    return (eager_gradient(data, 1).abs() * torch.exp(-eager_gradient(img, 1).abs())).sum(1).mean()


def eager_second(data, img):
    return (eager_gradient(data, 2).abs() * torch.exp(-10 * eager_gradient(img, 1).abs())).sum(1).mean()


def make_inputs(H, W, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    mask = ((yy - 0.5 * H) ** 2 + (xx - 0.5 * W) ** 2 <= (0.42 * min(H, W)) ** 2)[None].float()
    smooth = lambda c: (0.5 + 0.3 * torch.sin(xx * 0.02 + c) * torch.cos(yy * 0.03 - c))[None]   # noqa: E731
    t = dict(mask=mask, gt=torch.cat([smooth(c) for c in range(3)]) + 0.02 * torch.rand(3, H, W, generator=g),
             base_color=torch.rand(3, H, W, generator=g), roughness=torch.rand(1, H, W, generator=g), diffuse=torch.rand(3, H, W, generator=g),
             normal=F.normalize(torch.randn(3, H, W, generator=g), dim=0))
    return {k: v.to(dev).contiguous() for k, v in t.items()}


def variants(t):
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("base_color", "roughness", "diffuse", "normal")}
    b, r, d, n, m, gt = leaves["base_color"], leaves["roughness"], leaves["diffuse"], leaves["normal"], t["mask"], t["gt"]

    def clear():
        for v in leaves.values():
            v.grad = None

    def fused_stage2():
        clear()
        out = losses.smoothness_losses([dict(kind="first", data=b, img=gt, data_mask=m, img_mask=m),
                                        dict(kind="first", data=r, img=gt, data_mask=m, img_mask=m), dict(kind="first", data=d, img=n, data_mask=m)])
        (0.01 * out[0] + 0.01 * out[1] + 0.005 * out[2]).backward()

    def composed_stage2():
        clear()
        (0.01 * eager_first(b * m, gt * m) + 0.01 * eager_first(r * m, gt * m) + 0.005 * eager_first(d * m, n)).backward()

    def fused_second():
        clear()
        (0.01 * losses.smoothness_losses([dict(kind="second", data=n, img=gt, data_mask=m)])[0]).backward()

    def composed_second():
        clear()
        (0.01 * eager_second(n * m, gt)).backward()

    return dict(fused_stage2=fused_stage2, composed_stage2=composed_stage2, fused_second=fused_second, composed_second=composed_second), leaves


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_loss_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "smooth_loss_timing needs a GPU"
    dev = torch.device("cuda:0")
    H, W = args.size
    fns, leaves = variants(make_inputs(H, W, dev))
    # the two forms agree before they are timed
    agree = {}
    for name, keys in (("stage2", ("base_color", "roughness", "diffuse", "normal")), ("second", ("normal",))):
        fns["fused_" + name]()
        got = {k: leaves[k].grad.clone() for k in keys}
        fns["composed_" + name]()
        agree[name] = {k: float((got[k] - leaves[k].grad).abs().max() / leaves[k].grad.abs().max()) for k in keys}
    res = {}
    # fp32 planes read forward + read backward + written backward.  stage2: (3 + 3 + 1 + 1) + (1 + 3 + 1 + 1) + (3 + 3 + 1) = 21 read each way,
    # 3 + 1 + 3 + 3 written; second: 3 + 3 + 1 = 7 read each way, 3 written
    for name, planes in (("stage2", 21 + 21 + 10), ("second", 7 + 7 + 3)):
        f, c = abba(fns["fused_" + name], fns["composed_" + name], args.reps, args.warmup)
        nbytes = 4 * H * W * planes
        res[name] = {"fused_ms": f, "composed_ms": c, "fused_faster": bool(f["max"] < c["min"]), "ranges_overlap": not (f["max"] < c["min"] or c["max"] < f["min"]),
                     "speedup_median": c["median"] / f["median"], "fused_bytes_moved": nbytes, "fused_GBps_at_median": nbytes / (f["median"] * 1e-3) / 1e9}
        print(json.dumps({name: res[name]}), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "size": [H, W], "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events around one forward + backward call (autograd and allocations included), A B B A order, median and min ... max",
              "bytes_moved": "fp32 planes the two fused kernels read (forward, backward) and write (backward), each counted once per term",
              "max_relative_gradient_difference_fused_vs_composed": agree, "results": res}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
