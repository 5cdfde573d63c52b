"""HIP-event times of the view-direction gradient (csrc/shade.hip: the view pass of shade_bwd_kernel behind the plain kernel) on the
cfg3_train working set -- 200 000 surfels, 64 incident samples from the in-kernel lattice, a learned radiance ratio.  For the record
only (bench.py does not time the opt-in path).

  standalone: svgir_shade_backward against svgir_shade_backward_view on all P surfels, alternating (A B A B), the median of `--reps`
              event-timed calls each after `--warmup` warm-ups (prologue, kernel(s) and the env epilogue of one call);
  fused:      one TrainStep on cfg3_train with and without view_gradient, alternating: the `backward` phase of the step (loss,
              rasterizer, shading of the blended surfels, geometry) and the library's own stage times inside svgir_backward.

    python scripts/viewgrad_probe.py [--out profiles/viewgrad_timing.json]   (on the GPU box)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd"))
sys.path.insert(0, ROOT)
from gaussian_renderer import _native as N  # noqa: E402
from gaussian_renderer import shading  # noqa: E402
from svgir_harness import shade_inputs, workloads  # noqa: E402


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


def standalone(dev, P, Ns, reps, warmup):
    d = shade_inputs.make(P, Ns, seed=5, device=dev, with_dirs=False)
    geo = torch.nn.functional.normalize(d["normals"][:, 0].to(dev), dim=-1)
    lat = shading.FibonacciLattice(geo, Ns, torch.rand(P, device=dev) * 6.2831855)
    vm = torch.eye(4, device=dev)
    ratio = torch.ones((), device=dev)
    sp, keep, *_ = shading._params(d["base_color"], d["roughness"], d["normals"], d["viewdirs"], d["radiance"], d["visibility"], lat, None,
                                   d["env"], True, 2.0, viewmatrix=vm, training=True, ratio=ratio)
    g = torch.Generator(dev).manual_seed(1)
    gf, gvf = torch.randn(P, 4, device=dev, generator=g), torch.randn(P, 52, device=dev, generator=g)
    outs = [torch.empty_like(keep[i]) for i in (0, 1, 2, 8)]
    d_ratio, d_view = torch.empty(1, device=dev), torch.empty(P, 3, device=dev)
    gwork = torch.empty(keep[8].numel() + shading.RATIO_WORK, device=dev)
    head = (sp, None, gf.data_ptr(), gvf.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None, outs[3].data_ptr(),
            gwork.data_ptr(), d_ratio.data_ptr())
    plain = lambda: N.check(N.lib.svgir_shade_backward(*head, N.stream_ptr(dev)), "shade_backward")  # noqa: E731
    view = lambda: N.check(N.lib.svgir_shade_backward_view(*head, d_view.data_ptr(), N.stream_ptr(dev)), "shade_backward_view")  # noqa: E731
    rec = {"P": P, "Ns": Ns, "radiance_ratio": True, "lattice": True}
    for tag, fn in (("plain_ms", plain), ("view_ms", view), ("plain_ms_second_pass", plain), ("view_ms_second_pass", view)):
        rec[tag] = event_ms(fn, reps, warmup)
    rec["view_over_plain"] = rec["view_ms"]["median"] / rec["plain_ms"]["median"]
    N.set_profiling(True)
    for _ in range(reps):
        view()
    torch.cuda.synchronize()
    st = dict(N.last_timings())
    N.set_profiling(False)
    rec["kernel_only_ms"] = {k: st[k] for k in ("shade_bwd", "shade_bwd_view", "shade_env_grad") if k in st}
    assert bool(torch.isfinite(d_view).all())
    return rec


def fused(dev, steps, warmup):
    rec = {"workload": "cfg3_train", "steps": steps}
    ts = {vg: workloads.TrainStep(dev, name="cfg3_train", Ns=64, view_gradient=vg) for vg in (False, True)}
    rec["P"] = ts[False].P
    for t in ts.values():
        for _ in range(warmup):
            t.step()
    torch.cuda.synchronize()
    for tag, vg in (("default", False), ("view_gradient", True), ("default_second_pass", False), ("view_gradient_second_pass", True)):
        rec[tag + "_phase_ms"] = ts[vg].stage_table(steps)
    N.set_profiling(True)
    for vg, tag in ((False, "default"), (True, "view_gradient")):
        for _ in range(3):
            ts[vg].step()
        torch.cuda.synchronize()
        st = dict(N.last_timings())
        rec[tag + "_library_stage_ms"] = {k: v for k, v in st.items() if k.startswith("shade_")}
    N.set_profiling(False)
    rec["backward_phase_view_over_default"] = rec["view_gradient_phase_ms"]["backward"] / rec["default_phase_ms"]["backward"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viewgrad_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "viewgrad_probe needs a GPU"
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events around one call (standalone) / around the phases of one training step (fused), medians / means as named",
              "standalone": standalone(dev, 200_000, 64, args.reps, args.warmup), "fused": fused(dev, args.steps, args.warmup)}
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
