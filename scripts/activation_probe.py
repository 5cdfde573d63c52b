"""HIP-event times of the fused activation getters (csrc/activate.hip: `svgir_harness.activations.activate`) next to the lines they
replace, run as eager torch fp32 on the same GPU -- the `GaussianModel` getters, `viewdirs` and the normal regulariser of the reference
(tests/activation_cases.py `eager_activate`), i.e. what a user of the reference runs today in front of every render_view and again in
autograd's backward.  The comparison is against that and against nothing else.  For the record only (bench.py does not time this call).

P = 200 000 and 1 000 000 surfels, all nine outputs + normal_reg, forward + backward (a seeded upstream gradient per output).  Per case:
the median of `--reps` event-timed forward + backward pairs after `--warmup` warm-ups, allocations and host set-up included.  The kernel
pair moves 39 + 54 floats forward and 93 + 39 backward: 900 B per surfel; `effective_GBps` is that traffic over the pair's median time
(launch and host set-up included), next to the chip's ~8 TB/s peak.  `kernel_beats_eager` is the expectation; the ratio is recorded, none
was fixed in advance.
    python scripts/activation_probe.py [--out profiles/activation_timing.json]   (on the GPU box)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from gaussian_renderer import _native as N  # noqa: E402
from svgir_harness import activations  # noqa: E402
import activation_cases as ac  # noqa: E402

BYTES_PER_SURFEL = 4 * (39 + 54 + 93 + 39)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "activation_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "activation_probe needs a GPU"
    dev = torch.device("cuda:0")
    results = []
    for P in (200_000, 1_000_000):
        g = torch.Generator().manual_seed(P)
        raw = {k: v.to(dev).requires_grad_(True) for k, v in ac._random_rows(P, g).items()}
        campos, bcs = torch.tensor(ac.CAMPOS, device=dev), torch.tensor([1.0, 0.5, 2.0], device=dev)
        up = {k: torch.randn((P,) + activations.OUT_SHAPE[k], generator=g).to(dev) for k in ac.OUTPUTS}
        leaves = [raw[k] for k in ac.RAW]

        def pair(fn):
            out = fn(raw, campos, bcs, ac.OUTPUTS, True)
            return out, torch.autograd.grad([out[k] for k in ac.OUTPUTS] + [out["normal_reg"]],
                                            leaves, [up[k] for k in ac.OUTPUTS] + [torch.tensor(0.1, device=dev)])
        kern = lambda: pair(activations.activate)  # noqa: E731
        eag = lambda: pair(ac.eager_activate)  # noqa: E731
        (ko, kg), (eo, eg) = kern(), eag()
        diff = lambda a, b: float(torch.nan_to_num((a - b.reshape(a.shape)).abs(), nan=0.0).max())  # noqa: E731
        rec = {"P": P, "max_abs_diff_vs_eager": {k: diff(ko[k], eo[k]) for k in ac.OUTPUTS + ("normal_reg",)},
               "max_abs_grad_diff_vs_eager": {k: diff(a, b) for k, a, b in zip(ac.RAW, kg, eg)}}
        del ko, kg, eo, eg
        rec["kernel_ms"] = event_ms(kern, args.reps, args.warmup)
        rec["eager_ms"] = event_ms(eag, args.reps, args.warmup)
        rec["kernel_ms_second_pass"] = event_ms(kern, args.reps, args.warmup)     # A B A: the order does not decide the result
        rec["ratio_eager_over_kernel"] = rec["eager_ms"]["median"] / rec["kernel_ms"]["median"]
        rec["kernel_beats_eager"] = bool(max(rec["kernel_ms"]["median"], rec["kernel_ms_second_pass"]["median"]) < rec["eager_ms"]["median"])
        rec["effective_GBps"] = BYTES_PER_SURFEL * P / (rec["kernel_ms"]["median"] * 1e-3) / 1e9
        N.set_profiling(True)
        for _ in range(args.reps):
            kern()
        torch.cuda.synchronize()
        stages = dict(N.last_timings())
        N.set_profiling(False)
        rec["kernel_only_ms"] = {"activate_fwd": stages["activate_fwd"], "activate_bwd": stages["activate_bwd"]}
        rec["kernel_only_GBps"] = {"activate_fwd": 4 * 93 * P / (stages["activate_fwd"] * 1e-3) / 1e9,
                                   "activate_bwd": 4 * 132 * P / (stages["activate_bwd"] * 1e-3) / 1e9}
        results.append(rec)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events around one forward + backward pair (allocations, host set-up and every kernel of the pair), median of reps",
              "eager": "GaussianModel's getters, viewdirs and mse_loss(_normal, 0) as torch fp32 on the GPU, autograd backward",
              "bytes_per_surfel": BYTES_PER_SURFEL, "kernel_beats_eager": all(r["kernel_beats_eager"] for r in results), "results": results}
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
