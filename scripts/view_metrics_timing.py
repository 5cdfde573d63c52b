"""HIP-event times of one eval frame's tail, fused (csrc/view_metrics.hip: `svgir_harness.metrics.relighting_frame` -- one capture launch,
one metrics call) next to the lines it replaces, run as eager torch fp32 on the same GPU in the same process: the capture loop, the
ground-truth composites, torchvision's quantisation line and psnr / ssim / mse of eval_relighting_tensoIR.py:333-378
(tests/metrics_cases.py `eager_relighting_frame`, LPIPS apart), i.e. what a user of the reference runs today after every eval render.  The
comparison is against that and against nothing else.  For the record only (bench.py does not time this call).

800 x 800 (cfg3_eval's size), 12 captures + the ground truth and the 3 metric terms.  Two figures per side, each the median of `--reps`
event-timed calls after `--warmup` warm-ups, allocations and host set-up included, A B A:
  device_ms  everything up to the device results (uint8 images and metric values on the device);
  tail_ms    the same plus the device-to-host copies that end in the arrays handed to the PNG writer: one `.to("cpu", torch.uint8)` per
             capture on the eager side (torchvision's own expression), one copy of the [13,H,W,3] block on the fused side.
`fused_beats_eager` is the expectation; the ratios are recorded, none was fixed in advance.
    python scripts/view_metrics_timing.py [--out profiles/view_metrics_timing.json]   (on the GPU box)"""
import argparse
import json
import os
import sys
from math import exp

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from svgir_harness import metrics  # noqa: E402
import metrics_cases as mc  # noqa: E402


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


def eager_ssim(img1, img2):
    """utils/loss_utils.py:21-64 as a user calls it: the window is rebuilt and uploaded on every call."""
    g = torch.Tensor([exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    C = img1.size(-3)
    window = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0).expand(C, 1, 11, 11).contiguous().to(img1.device).type_as(img1)
    mu1, mu2 = F.conv2d(img1, window, padding=5, groups=C), F.conv2d(img2, window, padding=5, groups=C)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(img1 * img1, window, padding=5, groups=C) - mu1_sq
    s2 = F.conv2d(img2 * img2, window, padding=5, groups=C) - mu2_sq
    s12 = F.conv2d(img1 * img2, window, padding=5, groups=C) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_metrics_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "view_metrics_timing needs a GPU"
    dev = torch.device("cuda:0")
    H = W = args.size
    fr = mc.build_frame(H, W)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    pkg = {k: t(v) for k, v in fr["render_pkg"].items()}
    gt_image, gt_albedo, gt_normal, mask = (t(fr[k]) for k in ("gt_image", "gt_albedo", "gt_normal", "mask"))
    caps, bg = mc.FRAME_CAPTURES, mc.FRAME_BG

    def fused(host):
        images, rows = metrics.relighting_frame(pkg, gt_image, gt_albedo, gt_normal, mask, bg, caps)
        if host:
            block = images[caps[0]]._base if images[caps[0]]._base is not None else torch.stack(list(images.values()))
            return block.cpu(), rows
        return images, rows

    def eager(host):
        saved = {}
        quant = (lambda x: mc.torch_quantise(x).to("cpu")) if host else mc.torch_quantise
        acc = mc.eager_relighting_frame(pkg, gt_image, gt_albedo, gt_normal, mask, bg, caps, lambda name, img: saved.__setitem__(name, quant(img)),
                                        mc.srgb32, mc.torch_psnr, eager_ssim, mc.torch_mse)
        return saved, {k: {m: v.double() for m, v in d.items()} for k, d in acc.items()}     # (`+= ....mean().double()`)

    # the two sides agree before they are timed
    images, rows = fused(False)
    saved, acc = eager(False)
    same_bytes = all(torch.equal(images[k], saved[k]) for k in saved)
    r = rows.cpu().numpy()
    diffs = {"pbr_mse": abs(float(acc["pbr"]["mse"]) - r[0][6]), "pbr_psnr": abs(float(acc["pbr"]["psnr"]) - r[0][7]),
             "pbr_ssim": abs(float(acc["pbr"]["ssim"]) - r[0][8]), "albedo_mse": abs(float(acc["albedo"]["mse"]) - r[1][6]),
             "albedo_psnr": abs(float(acc["albedo"]["psnr"]) - r[1][7]), "albedo_ssim": abs(float(acc["albedo"]["ssim"]) - r[1][8]),
             "normal_mse": abs(float(acc["normal"]["mse"]) - r[2][6])}
    rec = {"W": W, "H": H, "captures": len(caps) + 1, "terms": 3, "bytes_equal_eager": bool(same_bytes), "abs_diff_vs_eager": diffs}
    for key, host in (("device_ms", False), ("tail_ms", True)):
        a = event_ms(lambda: fused(host), args.reps, args.warmup)
        b = event_ms(lambda: eager(host), args.reps, args.warmup)
        a2 = event_ms(lambda: fused(host), args.reps, args.warmup)      # A B A: the order does not decide the result
        rec[key] = {"fused": a, "eager": b, "fused_second_pass": a2, "ratio_eager_over_fused": b["median"] / max(a["median"], a2["median"]),
                    "fused_beats_eager": bool(max(a["median"], a2["median"]) < b["median"])}
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events around one frame tail (allocations, host set-up and every kernel of the tail), median of reps",
              "eager": "eval_relighting_tensoIR.py:333-378 as torch fp32 on the GPU: capture loop, torchvision's quantisation line, psnr / ssim / mse "
                       "(LPIPS apart)",
              "fused_beats_eager": bool(rec["device_ms"]["fused_beats_eager"] and rec["tail_ms"]["fused_beats_eager"]), "results": [rec]}
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
