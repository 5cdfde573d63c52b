"""The case table of the nearest-neighbour tests: one table for tests/test_knn_edge_inputs.py (CPU: every case holds what it is named
for, the oracle is pinned against fp64 and against a box-pruned search) and tests/test_gpu_knn.py (csrc/knn.hip through
`simple_knn._C.distCUDA2` and `custom_knn._C.topKdistCUDA2`, bit for bit against the oracle).

The oracle is a chunked numpy fp32 brute force in the contract's operation order (include/svgir_raster.h):
    d = p_j - p_i per component, dist = (d.x*d.x + d.y*d.y) + d.z*d.z, every operation a separate fp32 ufunc (no fused multiply-add);
    candidates j != i with a finite dist, ordered by np.lexsort on (index, dist);
    mean = ((b0 + b1) + b2) / 3 in fp32 over the three first dist, FLT_MAX where there is none;
    topk = the 8 first (dist, idx), padded with (+inf, i).
Per row only the candidates up to the row's K-th smallest dist (all of its ties included) reach the lexsort: the first K of that
order are the first K of the whole row's.

CASES[name]() builds the fp32 cloud [P,3]; `cloud(name)` and `oracle(name)` cache per process, so the tests of a session share one
reference per case and leave it unchanged (the arrays are read-only).

Sizes.  P = 1, 2, 3, 4 (fewer than 3 neighbours); 8, 9, 10 (fewer than, exactly, more than 8); 63, 64, 65; 255, 256, 257; 1023,
1024, 1025; and the thresholds of csrc/knn.hip, each with one either side:
    64    KNN_GROUP: points per fine box = queries per wave (63, 64, 65 above)
    256   BLOCK of the whole-box / Morton / gather kernels (255, 256, 257 above)
    4096  KNN_GROUP * KNN_FAN: points per coarse box, the second coarse box starts at 4097; also one block of the radix sort
          (SORT_ITEMS * BLOCK, common.hpp): 4095, 4096, 4097
    16384 KNN_WHOLE_BLOCKS * BLOCK: above it the whole-box kernel's threads take more than one point each: 16383, 16384, 16385
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

F32 = np.float32
K_MEAN, K_LIST = 3, 8
FLT_MAX = np.finfo(F32).max
GROUP, FAN, WHOLE_BLOCKS = 64, 64, 64      # csrc/knn.hip KNN_GROUP, KNN_FAN, KNN_WHOLE_BLOCKS
SIZES = (1, 2, 3, 4, 8, 9, 10, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385)
LARGE = 20000

CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def _uniform(P, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(P, 3)).astype(F32)


for _P in SIZES:
    CASES["uniform_%d" % _P] = functools.partial(_uniform, _P, 1000 + _P)


@case
def uniform_large():
    """20 000 points in a cube: 5 coarse boxes, most of them pruned for most waves."""
    return _uniform(LARGE, 7)


@case
def two_clusters_large():
    """two Gaussian blobs far apart: a wave of one cluster prunes the other cluster's coarse boxes and keeps its own."""
    rng = np.random.default_rng(8)
    a = rng.normal(0.0, 0.05, size=(LARGE // 2, 3)) + np.array([-1.0, 0.0, 0.0])
    b = rng.normal(0.0, 0.2, size=(LARGE - LARGE // 2, 3)) + np.array([3.0, 1.0, -2.0])
    pts = np.concatenate([a, b]).astype(F32)
    return pts[rng.permutation(LARGE)]


@case
def identical_4096():
    """every point the same: all distances 0, every Morton code equal, neighbours = the 8 lowest other indices."""
    return np.tile(np.array([[0.25, -1.5, 3.0]], F32), (4096, 1))


@case
def lattice_16():
    """integer lattice 16 x 16 x 16 in a seeded order: exact distances, up to 6 / 12 / 8 way ties decided by index."""
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3).astype(F32)
    return g[np.random.default_rng(9).permutation(len(g))]


@case
def collinear():
    """on a line along x: the whole box has no extent on two axes."""
    p = np.zeros((2000, 3), F32)
    p[:, 0] = np.random.default_rng(10).uniform(-5, 5, 2000)
    p[:, 1], p[:, 2] = 0.5, -2.0
    return p


@case
def coplanar():
    """in the plane z = 1: no extent on one axis."""
    p = _uniform(3000, 11)
    p[:, 2] = 1.0
    return p


@case
def far_outlier():
    """5 000 points in a unit cube and one at 1e6: the cube collapses into one Morton cell."""
    p = np.random.default_rng(12).uniform(0.0, 1.0, size=(5001, 3)).astype(F32)
    p[2500] = 1e6
    return p


@case
def offset_cube():
    """a unit cube at (1e6, 1e6, 1e6): coordinates on a 1/16 grid, differences cancel, ties everywhere -- still bit-defined."""
    return (np.random.default_rng(13).uniform(0.0, 1.0, size=(3000, 3)) + 1e6).astype(F32)


@case
def coincident_pair():
    """two equal points inside a random cloud: each is the other's nearest neighbour at distance 0."""
    p = _uniform(2000, 14)
    p[1234] = p[77]
    return p


NONFINITE = {"nan": 100, "inf": 900, "huge": 1700}


@case
def nonfinite():
    """one NaN point, one +inf point, one at 1e20 (its distances overflow): none has or is a neighbour."""
    p = _uniform(2000, 15)
    p[NONFINITE["nan"]] = (np.nan, 0.1, 0.2)
    p[NONFINITE["inf"]] = (0.3, np.inf, -0.4)
    p[NONFINITE["huge"]] = (1e20, 0.0, 0.0)
    return p


TIE_HEAVY = ("identical_4096", "lattice_16", "offset_cube", "coincident_pair", "uniform_9")
WELL_SEPARATED = ("uniform_257", "uniform_1025", "coplanar", "collinear")


@functools.lru_cache(maxsize=None)
def cloud(name):
    p = np.ascontiguousarray(CASES[name](), dtype=F32)
    assert p.ndim == 2 and p.shape[1] == 3
    p.setflags(write=False)
    return p


def dist_rows(p, lo, hi):
    """fp32 dist of queries lo..hi-1 to every point in the contract's operation order; self and non-finite -> +inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = p[None, :, :] - p[lo:hi, None, :]
        sq = d * d
        dist = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    dist[~np.isfinite(dist)] = np.inf
    dist[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
    return dist


def _rows(p, lo, hi):
    P = len(p)
    dist = dist_rows(p, lo, hi)
    out_d = np.full((hi - lo, K_LIST), np.inf, F32)
    out_i = np.repeat(np.arange(lo, hi, dtype=np.int32)[:, None], K_LIST, 1)
    if P > 1:
        kk = min(K_LIST, P - 1) - 1
        kth = np.partition(dist, kk, axis=1)[:, kk]
        for r in range(hi - lo):
            cand = np.flatnonzero((dist[r] <= kth[r]) & (dist[r] < np.inf))
            order = np.lexsort((cand, dist[r, cand]))[:K_LIST]
            out_d[r, :len(order)] = dist[r, cand[order]]
            out_i[r, :len(order)] = cand[order]
    return out_d, out_i


def brute_force(p, chunk=128):
    """(mean [P], dist [P,8], idx [P,8]) of the contract."""
    P = len(p)
    spans = [(lo, min(P, lo + chunk)) for lo in range(0, P, chunk)]
    if len(spans) > 4:
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            parts = list(ex.map(lambda s: _rows(p, *s), spans))
    else:
        parts = [_rows(p, *s) for s in spans]
    dist = np.concatenate([a for a, _ in parts]) if parts else np.zeros((0, K_LIST), F32)
    idx = np.concatenate([b for _, b in parts]) if parts else np.zeros((0, K_LIST), np.int32)
    b = np.where(np.isinf(dist[:, :K_MEAN]), FLT_MAX, dist[:, :K_MEAN]).astype(F32)
    with np.errstate(over="ignore"):
        mean = ((b[:, 0] + b[:, 1]) + b[:, 2]) / F32(3.0)
    return mean.astype(F32), dist, idx.astype(np.int32)


@functools.lru_cache(maxsize=None)
def oracle(name):
    out = brute_force(cloud(name))
    for a in out:
        a.setflags(write=False)
    return out


def morton_codes(p):
    """30-bit codes in the box of the finite points, as csrc/knn.hip orders the search (the result does not depend on them)."""
    fin = np.isfinite(p).all(1)
    lo, hi = (p[fin].min(0), p[fin].max(0)) if fin.any() else (np.zeros(3, F32), np.zeros(3, F32))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = (p - lo) / (hi - lo) * F32(1024.0)
    q = np.where(np.isnan(q), 0.0, q)
    q = np.clip(q, 0.0, 1023.0).astype(np.uint32)
    code = np.zeros(len(p), np.uint32)
    for bit in range(10):
        for c in range(3):
            code |= ((q[:, c] >> bit) & 1) << (3 * bit + c)
    return code
