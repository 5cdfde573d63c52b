"""HIP-event times of the two nearest-neighbour calls (csrc/knn.hip: `simple_knn._C.distCUDA2`, `custom_knn._C.topKdistCUDA2`) next to
what a ROCm user would write without them: a chunked on-GPU torch brute force (`torch.cdist` + `topk`).  For the record only (bench.py
does not time these calls): P = 100 000, 200 000, 1 000 000 on a uniform cube and on the surface-like cloud of svgir_harness.scenes.

Per (cloud, P): the median of `--reps` event-timed calls after warm-up, each call including its scratch allocation and every kernel
(whole box, Morton codes, sort, gather, boxes, search).  The brute force is linear in the number of query rows: above `--brute-rows`
rows it is timed on that many rows (every chunk against ALL P points) and scaled to P; `brute_rows_timed` says so.  The brute force
computes k = 8 (the mean of 3 is a slice of it), so the same figure stands next to both calls.  At the smallest size the kernel's
neighbour sets are checked against the brute force's (distances within fp32 rounding of cdist's matmul form; the exact check is
tests/test_gpu_knn.py).
    python scripts/knn_timing.py [--out profiles/knn_timing.json]   (on the GPU box)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svg-ir_amd"))
sys.path.insert(0, ROOT)
from custom_knn._C import topKdistCUDA2  # noqa: E402
from simple_knn._C import distCUDA2  # noqa: E402
from svgir_harness import scenes  # noqa: E402


def clouds(P, seed):
    rng = np.random.default_rng(seed)
    yield "uniform_cube", rng.uniform(-1.0, 1.0, size=(P, 3)).astype(np.float32)
    yield "surface", scenes._surface_points(P, np.random.default_rng(seed + 1))[0].astype(np.float32)


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
    return float(np.median(times)), float(min(times)), float(max(times))


def brute_topk(pts, rows, chunk):
    """8 nearest other points of the first `rows` points against all of `pts`: cdist + topk per chunk of queries."""
    P = pts.shape[0]
    dist = torch.empty(rows, 8, device=pts.device)
    idx = torch.empty(rows, 8, dtype=torch.int64, device=pts.device)
    ar = torch.arange(chunk, device=pts.device)
    for lo in range(0, rows, chunk):
        hi = min(rows, lo + chunk)
        d = torch.cdist(pts[lo:hi], pts)
        d[ar[:hi - lo], ar[:hi - lo] + lo] = float("inf")
        v, i = torch.topk(d, min(8, P), dim=1, largest=False)
        dist[lo:hi, :v.shape[1]], idx[lo:hi, :i.shape[1]] = v * v, i
    return dist, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[100000, 200000, 1000000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--brute-rows", type=int, default=32768)
    ap.add_argument("--brute-chunk-elems", type=int, default=1 << 29, help="elements of one cdist block (fp32)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "knn_timing needs a GPU"
    dev = torch.device("cuda:0")
    rows_out = []
    for P in args.sizes:
        for name, cloud in clouds(P, seed=P % 9973):
            pts = torch.from_numpy(cloud).to(dev)
            mean_ms = event_ms(lambda: distCUDA2(pts), args.reps, args.warmup)
            topk_ms = event_ms(lambda: topKdistCUDA2(pts), args.reps, args.warmup)
            rows = min(P, args.brute_rows)
            chunk = max(1, min(rows, args.brute_chunk_elems // P))
            brute = event_ms(lambda: brute_topk(pts, rows, chunk), 3, 1)
            scale = P / rows
            rec = {"cloud": name, "P": P,
                   "distCUDA2_ms": {"median": mean_ms[0], "min": mean_ms[1], "max": mean_ms[2]},
                   "topKdistCUDA2_ms": {"median": topk_ms[0], "min": topk_ms[1], "max": topk_ms[2]},
                   "brute_force_ms": {"median": brute[0] * scale, "min": brute[1] * scale, "max": brute[2] * scale},
                   "brute_rows_timed": rows, "brute_chunk_rows": chunk,
                   "speedup_topk": brute[0] * scale / topk_ms[0], "speedup_mean": brute[0] * scale / mean_ms[0]}
            if P == min(args.sizes):
                # (cdist's distances differ from the contract's in the last bits: compare the neighbour SETS where the 8th and 9th
                # brute-force distances are clearly apart)
                _, bi = brute_topk(pts, rows, chunk)
                _, ki = topKdistCUDA2(pts)
                same = (torch.sort(bi, 1).values == torch.sort(ki[:rows].long(), 1).values).all(1)
                rec["rows_with_equal_neighbour_sets"] = float(same.float().mean())
            rec["kernel_beats_brute_force"] = bool(rec["speedup_topk"] > 1 and rec["speedup_mean"] > 1)
            print(json.dumps(rec), flush=True)
            rows_out.append(rec)
            del pts
            torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
              "timing": "HIP events around one call (scratch allocation and every kernel of the call), median of reps",
              "brute_force": "chunked torch.cdist + topk(8, largest=False) on the GPU, scaled from brute_rows_timed query rows to P",
              "results": rows_out}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
