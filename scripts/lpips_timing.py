"""HIP-event times of LPIPS (csrc/lpips.hip through `svgir_harness.metrics.lpips_terms`) next to the same network run through torch's own
`F.conv2d` / `F.max_pool2d` in fp32 on the same GPU with the same weights -- what a user would otherwise run (lpipsPyTorch with
torchvision's VGG16, minus its per-call rebuild of the network, which is not timed here).  The comparison is against that and against
nothing else.  For the record only (bench.py does not time this call).

One pair and four pairs of 800 x 800 images, the seeded weights of tests/lpips_cases.py (the published ones are not available here: the
times do not depend on the values).  Per call: the median of `--reps` event-timed calls after warm-up, the workspace / output allocation and
the host-side set-up included; A B A, so the order does not decide the result.  FLOP: 2 * 305856 * H * W per image (the thirteen
convolutions); `TFLOPs` is that over the call's median time, `share_of_peak` over the 157.3 TF fp32 matrix peak.  The per-layer table comes
from the library's stage events (svgir_set_profiling), mean of reps, in a pass of its own.  The two paths must agree within the tap bound
of tests/test_gpu_lpips.py, 4 max(E32_k, 8 eps32) |tap_k|.  No ratio was fixed in advance; it is recorded as it comes out.
    python scripts/lpips_timing.py [--out profiles/lpips_timing.json]   (on the GPU box)"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "svg-ir_amd"), ROOT):
    sys.path.insert(0, p)
from gaussian_renderer import _native as N  # noqa: E402
from svgir_harness import metrics  # noqa: E402
import lpips_cases as lc  # noqa: E402

MACS_PER_PIXEL = 305856
PEAK_TF = 157.3
STAGES = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2",
          "conv5_3")
LEVEL = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)


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


class TorchLpips:
    """lpipsPyTorch's LPIPS('vgg') forward with torch's own operators, the weights resident on the device (built once)."""

    def __init__(self, vgg, lin, dev):
        self.w = {i: (vgg[f"features.{i}.weight"].to(dev), vgg[f"features.{i}.bias"].to(dev)) for i in lc.CONV_INDEX}
        self.lin = [lin[f"lin{k}.model.1.weight"].to(dev) for k in range(5)]
        self.mean = torch.tensor(lc.MEAN, device=dev)[None, :, None, None]
        self.std = torch.tensor(lc.STD, device=dev)[None, :, None, None]

    def feats(self, x):
        h = (x - self.mean) / self.std
        out = []
        for i in range(lc.TAP_INDEX[-1] + 1):
            if i in self.w:
                h = F.conv2d(h, self.w[i][0], self.w[i][1], padding=1)
            elif i in lc.POOL_INDEX:
                h = F.max_pool2d(h, 2, 2)
            else:
                h = torch.relu(h)
                if i in lc.TAP_INDEX:
                    out.append(h / (torch.sqrt(torch.sum(h ** 2, dim=1, keepdim=True)) + 1e-10))
        return out

    @torch.no_grad()
    def __call__(self, x, y):
        """x, y [n,3,H,W] -> taps [n,5] (the reference would sum the batch into one number; kept per pair here)."""
        fx, fy = self.feats(x), self.feats(y)
        return torch.cat([F.conv2d((a - b) ** 2, l).mean((2, 3)) for a, b, l in zip(fx, fy, self.lin)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lpips_timing needs a GPU"
    dev = torch.device("cuda:0")
    S = args.size
    vgg, lin = lc.weights("base")
    net = metrics.LPIPS(vgg, lin)
    net.packed(dev)
    ref = TorchLpips(vgg, lin, dev)
    e32, _ = lc.measured_errors()
    g = torch.Generator().manual_seed(0)
    results = []
    for n in (1, 4):
        x = torch.rand(n, 3, S, S, generator=g)
        y = (x + 0.2 * (torch.rand(n, 3, S, S, generator=g) - 0.5)).clamp(0, 1)
        x, y = x.to(dev), y.to(dev)
        pairs = [(x[i], y[i]) for i in range(n)]
        kern = lambda: metrics.lpips_terms(net, pairs, with_taps=True)  # noqa: E731
        eag = lambda: ref(x, y)  # noqa: E731
        flop = 2.0 * MACS_PER_PIXEL * S * S * 2 * n
        rec = {"W": S, "H": S, "pairs": n, "GFLOP": flop / 1e9, "work_MB": N.lib.svgir_lpips_work_bytes(S, S, n) / 2 ** 20}
        taps = kern()[1].double().cpu().numpy()
        rec["taps_hip"] = taps.tolist()
        rec["hip_ms"] = event_ms(kern, args.reps, args.warmup)
        want = eag().double().cpu().numpy()   # (a failure of torch's path ends the script: the comparison is part of its job)
        rec["torch_ms"] = event_ms(eag, args.reps, args.warmup)
        rec["hip_ms_second_pass"] = event_ms(kern, args.reps, args.warmup)
        med = max(rec["hip_ms"]["median"], rec["hip_ms_second_pass"]["median"])
        rec["hip_ms_per_pair"] = med / n
        rec["hip_TFLOPs"] = flop / (med * 1e-3) / 1e12
        rec["hip_share_of_peak"] = rec["hip_TFLOPs"] / PEAK_TF
        tol = 4.0 * np.maximum(e32, 8 * lc.EPS32)[None] * np.abs(want)
        rec["taps_torch"] = want.tolist()
        rec["max_err_over_tap_bound"] = float((np.abs(taps - want) / tol).max())
        rec["agree_within_tap_bound"] = bool(rec["max_err_over_tap_bound"] <= 1.0)
        rec["torch_ms_per_pair"] = rec["torch_ms"]["median"] / n
        rec["torch_TFLOPs"] = flop / (rec["torch_ms"]["median"] * 1e-3) / 1e12
        rec["ratio_torch_over_hip"] = rec["torch_ms"]["median"] / med
        rec["hip_beats_torch"] = bool(med < rec["torch_ms"]["median"])
        N.set_profiling(True)
        for _ in range(args.reps):
            kern()
        torch.cuda.synchronize()
        stages = {name: ms * cnt / args.reps for name, ms, cnt in N.last_timings(with_counts=True)}   # ms per call
        N.set_profiling(False)
        table = []
        for l, name in enumerate(STAGES):
            co, ci = lc.CONV_SHAPE[l]
            f = 2.0 * 9 * ci * co * (S >> LEVEL[l]) * (S >> LEVEL[l]) * 2 * n
            ms = stages["lpips_" + name]
            table.append({"stage": name, "ms": ms, "GFLOP": f / 1e9, "TFLOPs": f / (ms * 1e-3) / 1e12, "share_of_peak": f / (ms * 1e-3) / 1e12 / PEAK_TF})
        for name in ("lpips_tap", "lpips_pool", "lpips_reduce"):
            table.append({"stage": name[6:], "ms": stages[name]})
        rec["per_layer"] = table
        results.append(rec)
        del x, y, pairs
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events around one call (workspace and output allocation, host set-up and every kernel of the call), median of reps; "
                        "per_layer: the library's stage events, mean of reps; tap / pool: the sum over their 5 / 4 launches",
              "torch": "the same network through F.conv2d / F.max_pool2d / torch.relu in fp32, contiguous NCHW, weights resident, no_grad",
              "flop": "2 * 305856 * H * W per image", "peak_TF": PEAK_TF, "E32": e32.tolist(), "results": results}
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    assert all(r["agree_within_tap_bound"] for r in results), "the HIP path and torch's disagree beyond the tap bound"


if __name__ == "__main__":
    main()
