"""CPU checks of the nearest-neighbour case table and its oracle (tests/knn_cases.py), and of the new surface: every case holds what it
is named for, the fp32 oracle is pinned against an fp64 brute force and against a box-pruned search, and the header, `_native.EXPORTS`,
the library and the two drop-in modules agree on the new names.  No GPU work is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import knn_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ("svgir_knn_bytes", "svgir_knn_mean_dist", "svgir_knn_topk")


def _missing(name):
    """padding slots per row of the list: dist = +inf and idx = the row"""
    _, dist, idx = kc.oracle(name)
    pad = np.isinf(dist)
    assert np.array_equal(idx[pad], np.broadcast_to(np.arange(len(idx), dtype=np.int32)[:, None], idx.shape)[pad])
    return pad.sum(1)


# ---- the table ------------------------------------------------------------------------------------------------------------------

def test_table_lists_the_sizes_and_thresholds():
    sizes = {len(kc.cloud(n)) for n in kc.CASES}
    for P in (1, 2, 3, 4, 8, 9, 10, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        assert P in sizes
    for t in (kc.GROUP, 256, kc.GROUP * kc.FAN, kc.WHOLE_BLOCKS * 256):   # csrc/knn.hip: fine box, BLOCK, coarse box, whole-box grid
        assert {t - 1, t, t + 1} <= sizes
    src = open(os.path.join(ROOT, "svg-ir_amd", "csrc", "knn.hip")).read()
    assert re.search(r"KNN_GROUP = (\d+)", src).group(1) == str(kc.GROUP) and re.search(r"KNN_FAN = (\d+)", src).group(1) == str(kc.FAN)
    assert re.search(r"KNN_WHOLE_BLOCKS = (\d+)", src).group(1) == str(kc.WHOLE_BLOCKS)
    assert len(kc.cloud("uniform_large")) >= 20000 and len(kc.cloud("two_clusters_large")) >= 20000
    for n in kc.CASES:
        assert kc.cloud(n).dtype == F32 and not kc.cloud(n).flags.writeable


@pytest.mark.parametrize("P", [1, 2, 3, 4, 8, 9, 10])
def test_small_clouds_miss_the_slots_they_are_named_for(P):
    name = "uniform_%d" % P
    mean, dist, idx = kc.oracle(name)
    assert np.array_equal(_missing(name), np.full(P, max(0, 8 - (P - 1))))
    with np.errstate(over="ignore"):
        if P <= 2:     # two FLT_MAX overflow the sum
            assert np.isinf(mean).all()
        elif P == 3:   # one FLT_MAX: about FLT_MAX / 3
            assert np.all((mean > 1.13e38) & (mean < 1.14e38))
        else:
            assert np.array_equal(mean, ((dist[:, 0] + dist[:, 1]) + dist[:, 2]) / F32(3))
    for i in range(P):   # the neighbours of a row are all the other points, nearest first
        if P <= 9:
            assert sorted(idx[i, :P - 1].tolist()) == [j for j in range(P) if j != i]
        assert np.all(np.diff(dist[i, :min(8, P - 1)]) >= 0)


def test_large_clouds_prune_some_coarse_boxes_and_keep_others():
    """per wave (64 Morton-consecutive queries) and coarse box: the box's lower bound against the wave's FINAL 8th distances --
    a box above every lane's bound can be skipped however the walk goes, one below some lane's must be visited."""
    for name in ("uniform_large", "two_clusters_large"):
        p = kc.cloud(name)
        order = np.argsort(kc.morton_codes(p), kind="stable")
        sp, kth = p[order], kc.oracle(name)[1][order, 7]
        span = kc.GROUP * kc.FAN
        nc = -(-len(p) // span)
        assert nc >= 4
        lo = np.stack([sp[c * span:(c + 1) * span].min(0) for c in range(nc)])
        hi = np.stack([sp[c * span:(c + 1) * span].max(0) for c in range(nc)])
        d = np.maximum(np.maximum(lo[None] - sp[:, None], sp[:, None] - hi[None]), 0).astype(F32)
        bound = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        need = bound <= kth[:, None]                                             # [P, nc]
        waves = [need[w:w + kc.GROUP].any(0) for w in range(0, len(p), kc.GROUP)]
        visited = np.array([w.sum() for w in waves])
        assert (visited < nc).mean() > 0.5, name      # most waves prune something
        assert (visited > 1).any(), name              # some need more than their own box
        assert visited.min() >= 1


def test_identical_points():
    p = kc.cloud("identical_4096")
    assert len(p) == 4096 and (p == p[0]).all() and len(np.unique(kc.morton_codes(p))) == 1
    mean, dist, idx = kc.oracle("identical_4096")
    assert (dist == 0).all() and (mean == 0).all()
    for i in (0, 1, 7, 8, 9, 4095):
        assert idx[i].tolist() == [j for j in range(10) if j != i][:8]


def test_lattice_ties_are_decided_by_index():
    p = kc.cloud("lattice_16")
    assert len(np.unique(p, axis=0)) == 4096 and (p == np.round(p)).all()
    _, dist, idx = kc.oracle("lattice_16")
    inner = ((p > 0) & (p < 15)).all(1)
    assert inner.sum() == 14 ** 3
    # an inner point: 6 neighbours at 1, then 2 of the 12 at distance 2 -- the two lowest indices among them
    assert (dist[inner, :6] == 1).all() and (dist[inner, 6:] == 2).all()
    for i in np.flatnonzero(inner)[:50]:
        assert np.all(np.diff(idx[i, :6]) > 0)
        at2 = np.flatnonzero(((p - p[i]) ** 2).sum(1) == 2)
        assert len(at2) == 12 and idx[i, 6:].tolist() == sorted(at2.tolist())[:2]


def test_flat_clouds_have_no_extent_where_named():
    p = kc.cloud("collinear")
    assert np.ptp(p[:, 0]) > 0 and np.ptp(p[:, 1]) == 0 and np.ptp(p[:, 2]) == 0
    assert (kc.morton_codes(p) & 0x36DB6DB6 == 0).all()        # only x bits
    p = kc.cloud("coplanar")
    assert np.ptp(p[:, 0]) > 0 and np.ptp(p[:, 1]) > 0 and np.ptp(p[:, 2]) == 0
    assert (kc.morton_codes(p) & 0x24924924 == 0).all()        # no z bits


def test_far_outlier_collapses_the_cube_into_one_cell():
    p = kc.cloud("far_outlier")
    code = kc.morton_codes(p)
    assert len(p) == 5001 and (np.delete(code, 2500) == 0).all() and code[2500] == 0x3FFFFFFF
    mean, dist, idx = kc.oracle("far_outlier")
    assert (idx != 2500).all() and dist[2500, 0] > 1e11 and np.isfinite(dist).all()


def test_offset_cube_cancels_to_a_coarse_grid_with_ties():
    p = kc.cloud("offset_cube")
    assert p.min() >= 1e6 and (p * 16 == np.round(p * 16)).all()      # fp32 spacing at 1e6 is 1/16
    _, dist, _ = kc.oracle("offset_cube")
    assert (dist[:, 1:] == dist[:, :-1]).mean() > 0.3 and np.isfinite(dist).all()


def test_coincident_pair():
    p = kc.cloud("coincident_pair")
    assert (p[1234] == p[77]).all() and len(np.unique(p, axis=0)) == len(p) - 1
    _, dist, idx = kc.oracle("coincident_pair")
    assert dist[77, 0] == 0 and idx[77, 0] == 1234 and dist[1234, 0] == 0 and idx[1234, 0] == 77
    assert (dist[:, 0] == 0).sum() == 2


def test_nonfinite_points_have_and_are_no_neighbours():
    p = kc.cloud("nonfinite")
    rows = sorted(kc.NONFINITE.values())
    assert np.isnan(p[kc.NONFINITE["nan"]]).any() and np.isinf(p[kc.NONFINITE["inf"]]).any() and p[kc.NONFINITE["huge"], 0] == F32(1e20)
    with np.errstate(over="ignore"):
        assert np.isinf(F32(1e20) * F32(1e20))
    mean, dist, idx = kc.oracle("nonfinite")
    missing = _missing("nonfinite")
    assert missing[rows].tolist() == [8, 8, 8] and np.delete(missing, rows).max() == 0
    assert np.isinf(mean[rows]).all() and np.isfinite(np.delete(mean, rows)).all()
    others = np.delete(idx, rows, axis=0)
    assert not np.isin(others, rows).any()


# ---- the oracle -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", kc.WELL_SEPARATED)
def test_oracle_agrees_with_fp64_on_well_separated_clouds(name):
    """Where no two candidates of a row are closer than fp32 can tell (checked: the fp64 gaps between consecutive neighbours exceed the
    fp32 error of a distance), the fp32 oracle picks the fp64 brute force's neighbour sets.  The mean is a 3-term fp32 sum of
    products of fp32 differences: each dist carries at most 3 roundings on top of the rounded differences, the sum 2 more and the
    divide 1 -- a few 2^-24 relative, far below 1e-5 (the differences themselves are exact here: the clouds sit in [-5, 5] and their
    neighbours are close, Sterbenz)."""
    p = kc.cloud(name)
    p64 = p.astype(np.float64)
    d64 = ((p64[None] - p64[:, None]) ** 2).sum(-1)
    np.fill_diagonal(d64, np.inf)
    order = np.argsort(d64, axis=1, kind="stable")[:, :9]
    near = np.take_along_axis(d64, order, 1)
    mean, dist, idx = kc.oracle(name)
    clear = (np.diff(near, axis=1) > 1e-6 * near[:, 1:]).all(1)      # rows whose first 9 fp64 distances are pairwise distinguishable in fp32
    assert clear.mean() > 0.95
    assert np.array_equal(np.sort(idx[clear], 1), np.sort(order[clear, :8], 1))
    assert np.array_equal(idx[clear], order[clear, :8])
    mean64 = near[:, :3].sum(1) / 3
    assert np.abs(mean - mean64).max() <= 1e-5 * mean64.max() and (np.abs(mean - mean64) <= 1e-5 * mean64).all()


def _pruned_search(p, queries, K):
    """The algorithm of the reference's kernel and of csrc/knn.hip, as plain sequential code: points in Morton order, one box per
    GROUP of them, per query a walk over ALL boxes that skips a box only when its fp32 lower bound is STRICTLY greater than the
    current K-th distance; inside a visited box every point except the query is offered to a K-best list ordered by (dist, index)."""
    order = np.argsort(kc.morton_codes(p), kind="stable")
    sp = p[order]
    nb = -(-len(p) // kc.GROUP)
    lo = np.stack([sp[b * kc.GROUP:(b + 1) * kc.GROUP].min(0) for b in range(nb)])
    hi = np.stack([sp[b * kc.GROUP:(b + 1) * kc.GROUP].max(0) for b in range(nb)])
    out = {}
    for i in queries:
        q = p[i]
        d = np.maximum(np.maximum(lo - q, q - hi), F32(0))
        bounds = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).tolist()
        best = []                                  # sorted (dist, index), at most K
        visited = 0
        for b in range(nb):
            if len(best) == K and bounds[b] > best[-1][0]:
                continue
            visited += 1
            ids = order[b * kc.GROUP:(b + 1) * kc.GROUP]
            e = sp[b * kc.GROUP:(b + 1) * kc.GROUP] - q
            dist = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
            for dj, j in zip(dist.tolist(), ids.tolist()):
                if j != i and dj < float("inf") and (len(best) < K or (dj, j) < best[-1]):
                    best.append((dj, j))
                    best.sort()
                    del best[K:]
        out[i] = (best, visited, nb)
    return out


@pytest.mark.parametrize("name", kc.TIE_HEAVY)
def test_box_pruned_search_equals_the_brute_force_on_ties(name):
    p = kc.cloud(name)
    mean, dist, idx = kc.oracle(name)
    queries = range(0, len(p), 16 if len(p) >= 2000 else 1)      # (every 16th query of the larger clouds: the walk is sequential Python)
    pruned_any = False
    for K in (kc.K_MEAN, kc.K_LIST):
        for i, (best, visited, nb) in _pruned_search(p, queries, K).items():
            n = min(K, int(np.isfinite(dist[i]).sum()))
            assert [j for _, j in best] == idx[i, :n].tolist(), (name, i)
            assert np.array_equal(np.array([d for d, _ in best], F32).view(np.int32), dist[i, :n].view(np.int32)), (name, i)
            pruned_any |= visited < nb
    if name in ("lattice_16", "coincident_pair"):
        assert pruned_any      # (the walk does skip boxes on these; identical points and the 1/16 grid tie with every bound)


# ---- the surface ----------------------------------------------------------------------------------------------------------------

def test_header_exports_and_library_agree_on_the_new_symbols(built):
    from gaussian_renderer import _native
    hdr = open(os.path.join(ROOT, "include", "svgir_raster.h")).read()
    lib = C.CDLL(_native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _native.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define SVGIR_ABI_VERSION (\d+)", hdr).group(1) == "14" and _native.ABI_VERSION == 14
    lib.svgir_knn_bytes.restype = C.c_size_t
    lib.svgir_knn_bytes.argtypes = [C.c_int32]
    b = [lib.svgir_knn_bytes(P) for P in (0, 1, 64, 65, 4096, 4097, 200000)]
    assert b[0] == b[1] == b[2] > 0 and all(x % 256 == 0 for x in b) and b == sorted(b) and b[3] > b[2] and b[5] > b[4]
    assert b[-1] >= 200000 * (16 + 16)      # the Morton-ordered copy and the sort's ping/pong arrays
    # argument checks come before any HIP call
    lib.svgir_knn_mean_dist.argtypes = [C.c_int32] + [C.c_void_p] * 4
    lib.svgir_knn_topk.argtypes = [C.c_int32] + [C.c_void_p] * 5
    assert lib.svgir_knn_mean_dist(-1, None, None, None, None) == -1 and lib.svgir_knn_mean_dist(5, None, None, None, None) == -1
    assert lib.svgir_knn_topk(-1, None, None, None, None, None) == -1 and lib.svgir_knn_topk(5, None, None, None, None, None) == -1
    assert lib.svgir_knn_mean_dist(0, None, None, None, None) == 0 and lib.svgir_knn_topk(0, None, None, None, None, None) == 0


def test_modules_import_under_the_reference_names(built):
    import torch
    from custom_knn._C import topKdistCUDA2
    from simple_knn._C import distCUDA2
    assert callable(distCUDA2) and callable(topKdistCUDA2)
    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        distCUDA2(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        topKdistCUDA2(x)
