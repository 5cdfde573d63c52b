"""bench.py --dump-outputs: what the last timed step returned, as DIR/<name>.npy within the 64 MB budget; an array beyond its share is
a fixed sample of its elements, so two runs (two builds) with the same arguments can be compared output for output."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        import bench
    finally:
        sys.argv = argv
    return bench


def test_host_outputs_types():
    bench = _bench()
    import torch
    h = bench.host_outputs({"a": torch.ones(2, 3, dtype=torch.float64), "r": 7, "i": torch.arange(4, dtype=torch.int32),
                            "b": torch.tensor([True, False]), "e": torch.empty(0), "n": None})
    assert sorted(h) == ["a", "b", "i", "r"]
    assert h["a"].dtype == np.float32 and h["a"].shape == (2, 3)
    assert h["r"].dtype == np.float64 and float(h["r"]) == 7.0
    assert h["i"].dtype == np.float64 and h["b"].dtype == np.float64


def test_dump_outputs_budget_and_fixed_sample(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(3)
    arrays = {"big": rng.random(16_800_000, dtype=np.float32).reshape(-1, 48), "mid": rng.random((3, 800, 800), dtype=np.float32),
              "small": np.arange(10, dtype=np.float64)}
    for d in ("x", "y"):
        bench.dump_outputs(arrays, str(tmp_path / d))
    total = sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x"))
    assert sorted(os.listdir(tmp_path / "x")) == ["big.npy", "mid.npy", "small.npy"] and total <= 64_000_000
    for k in ("mid", "small"):   # within their share: unchanged
        assert np.array_equal(np.load(tmp_path / "x" / f"{k}.npy"), arrays[k])
    a, b = np.load(tmp_path / "x" / "big.npy"), np.load(tmp_path / "y" / "big.npy")
    assert a.ndim == 1 and 0 < a.size < arrays["big"].size and np.array_equal(a, b)
    assert np.isin(a, arrays["big"]).all()
