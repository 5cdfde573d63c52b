"""The case table of the tracer edge tests: one table for tests/test_tracer_edge_inputs.py (the CPU oracles alone: every case holds what
it is named for, exercises both outcomes, and keeps its threshold rays under MAX_THRESHOLD_SHARE) and tests/test_gpu_tracer_edges.py
(csrc/bvh.hip `RayTracer` and csrc/pbgi.hip `pbgi.renderer.Renderer` against oracle/bvh_oracle.cpp and oracle/pbgi_oracle.cpp).

Every case is a seeded, named builder (VIS[name]() / RAD[name]()) that returns the fp32 arrays of ONE tracer call plus
  holds   what the case exists for (the host test asserts it)
  tol     the absolute value tolerance of the case and, in `tol_source`, where it comes from
  exact   (tie cases) the outcome stated by construction: the arithmetic of these rays is exact in fp32, fp64 and in the kernel

Threshold rays.  A ray whose oracle margin is below the bound is a threshold ray: it is counted, not compared, and a case may hold at
most MAX_THRESHOLD_SHARE of them.
  visibility tracer: margin = the smallest relative distance of any decision of the ray from its bound (oracle/bvh_oracle.cpp `Conj`,
      fp32 and fp64 mode; a ray's margin is the smaller of the two).  m is the smallest margin at which the fp32 and the fp64 oracle
      agree on `contribute` and on blocked / open for every ray above it, over every case of this table.  Measured
      (test_tracer_edge_inputs.py::test_visibility_margin_bound, which asserts it still holds): VIS_M_MEASURED = 0 -- the two oracles
      disagree on no ray of the table.  A margin below one fp32 ulp of the magnitudes it is relative to cannot be resolved by ANY
      fp32 evaluation, so the bound never goes below that: VIS_M = max(measured, 2^-23).  The kernel sums in another order and uses
      the fast exponential: the rule is margin < VIS_MARGIN = 4 x VIS_M = 4.8e-7.  (A ray THROUGH a surfel's mean has power = 0 up
      to rounding and is a threshold ray by construction: the builders aim beside the means.)
  radiance tracer: margin = distance of the closest expf-dependent comparison (alpha against 1/255 and 0.99, T against 0.2 and 0.001)
      from its bound in ulps of the bound per accumulated factor (oracle/pbgi_oracle.cpp `Margin`); the rule is margin < RAD_MARGIN
      = 4: both expf implementations are good to about 1 ulp.  Everything else in that oracle is IEEE-exact in the kernel's
      operation order, so every other difference is a fault.
  Exact ties are not threshold rays: their outcome is decided by exact arithmetic (`exact`), the margin rule is not applied to them.

Value tolerances.  VIS_TOL = 2e-4 and RAD_TOL = 2e-5 are the project's existing ones (tests/test_gpu_bvh.py, tests/test_gpu_pbgi.py).
A visibility case that needs more gets 2 x its own fp32-vs-fp64 oracle difference (never above 10 x VIS_TOL); long_ray would get
4 x the largest change of the oracle's outputs under a +-1 ulp expf (never above 10 x RAD_TOL).  The host test measures both for
every case and asserts the recorded `tol` covers them.  Measured: no case needs more than the existing numbers -- the largest
fp32-vs-fp64 oracle difference is 9.6e-5 (degenerate_far_coordinates), 8.7e-5 on the sort cases, 3.3e-5 elsewhere; a +-1 ulp expf
moves the long_ray outputs by 2.4e-7.

Stack occupancy.  `vis_peak_stack` walks a numpy Karras tree over morton << 31 | id (codes from the kernel's fp32 operations) with
bvh_trace_kernel's push rules and returns the largest number of pending entries; `rad_descent_stack` follows pbgi_trace_kernel's
first descent on the oracle's info / aabb (right child next, left child pushed: always while the direction is not fixed, after its
box test once it is) and returns the entries pending when the first leaf is reached -- a lower bound of the peak.
"""
import functools

import numpy as np

from oracle import bvh_oracle as bo
from oracle import pbgi_oracle as po
from tests import pbgi_scene
from tests.test_bvh_oracle import _scene

F32 = np.float32
MAX_THRESHOLD_SHARE = 0.01
VIS_M_MEASURED = 0.0
VIS_M = max(VIS_M_MEASURED, 2.0 ** -23)
VIS_MARGIN = 4 * VIS_M
RAD_MARGIN = 4.0
VIS_TOL, RAD_TOL = 2e-4, 2e-5
BVH_LDS_DEPTH, PBGI_LDS_DEPTH = 32, 20          # csrc/bvh.hip, csrc/pbgi.hip: stack levels kept in LDS
VIS_DEEP, RAD_DEEP = BVH_LDS_DEPTH + 4, PBGI_LDS_DEPTH + 4
RESIDENT_SLOTS = 256 * min(8 * 4, (160 * 1024) // (PBGI_LDS_DEPTH * 64 * 8))   # svgir_pbgi_trace_radiance: 4 096 waves

VIS, RAD = {}, {}


def _f(a):
    return np.ascontiguousarray(a, dtype=F32)


def _case(table, name):
    def deco(fn):
        assert name not in table
        table[name] = functools.lru_cache(maxsize=None)(fn)
        return fn
    return deco


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def down(x):
    return np.nextafter(F32(x), F32(-np.inf))


# ======================================================================================================================================
# fp32 helpers that restate the kernels' operations (numpy float32 arithmetic is IEEE and never contracted)
# ======================================================================================================================================
def unit3_f32(d):
    """normalize(v) = v / sqrt(dot(v, v)) in fp32, left to right (csrc/pbgi.hip unit3 / dot3)."""
    d = _f(d)
    l = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        return d / l[..., None]


def len_f32(d):
    d = _f(d)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def is_fixed(ray_d):
    """pbgi_trace_kernel's `fixed` at the start of a query: the fp32 length of the normalised direction is exactly 1."""
    return len_f32(unit3_f32(ray_d)) == F32(1)


def stays_unfixed(ray_d):
    """The length still differs from 1 after one re-normalisation (the first visited leaf leaves the direction changeable)."""
    u1 = unit3_f32(ray_d)
    u2 = unit3_f32(u1)
    return (len_f32(u1) != F32(1)) & (len_f32(u2) != F32(1))


def expand_bits(v):
    v = np.asarray(v, dtype=np.uint64)
    v = (v * np.uint64(0x00010001)) & np.uint64(0xFF0000FF)
    v = (v * np.uint64(0x00000101)) & np.uint64(0x0F00F00F)
    v = (v * np.uint64(0x00000011)) & np.uint64(0xC30C30C3)
    v = (v * np.uint64(0x00000005)) & np.uint64(0x49249249)
    return v


def vis_morton(boxes):
    """bvh_morton_kernel: codes of the box centroids in the whole box, fp32 operation by operation."""
    boxes = _f(boxes)
    with np.errstate(all="ignore"):
        wl = np.fmin.reduce(boxes[:, :3], axis=0)
        wu = np.fmax.reduce(boxes[:, 3:], axis=0)
        p = (boxes[:, 3:] + boxes[:, :3]) * F32(0.5)
        p = p - wl
        p = p / (wu - wl)
        p = np.fmin(np.fmax(p * F32(1024), F32(0)), F32(1023))          # fmaxf(NaN, 0) = 0
        cell = p.astype(np.uint64)
    return (expand_bits(cell[:, 0]) << np.uint64(2)) | (expand_bits(cell[:, 1]) << np.uint64(1)) | expand_bits(cell[:, 2])


def leading_ones30(code):
    code = np.asarray(code, dtype=np.uint64)
    n = np.zeros(code.shape, dtype=np.int64)
    alive = np.ones(code.shape, dtype=bool)
    for b in range(29, -1, -1):
        alive &= ((code >> np.uint64(b)) & np.uint64(1)) == 1
        n += alive
    return n


def karras(keys):
    """Karras 2012 over sorted unique integer keys (python ints): children[i] = (left, right), leaves encoded as ~position."""
    n = len(keys)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        return 64 - (keys[i] ^ keys[j]).bit_length()

    children = []
    for i in range(n - 1):
        first, last = 0, n - 1
        if i:
            ld, rd = delta(i, i - 1), delta(i, i + 1)
            d = 1 if rd > ld else -1
            dmin = min(ld, rd)
            lmax = 2
            while delta(i, i + d * lmax) > dmin:
                lmax <<= 1
            l, t = 0, lmax >> 1
            while t > 0:
                if delta(i, i + (l + t) * d) > dmin:
                    l += t
                t >>= 1
            j = i + l * d
            first, last = min(i, j), max(i, j)
        dnode = delta(first, last)
        split, stride = first, last - first
        while True:
            stride = (stride + 1) >> 1
            mid = split + stride
            if mid < last and delta(first, mid) > dnode:
                split = mid
            if stride <= 1:
                break
        children.append((~split if first == split else split, ~(split + 1) if last == split + 1 else split + 1))
    return children


def _slab_tmax(lo, hi, o, d):
    """slab_tmax of csrc/bvh.hip on fp32 scalars."""
    with np.errstate(all="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    tmin, tmax = t0[0], t1[0]
    if tmin > tmax:
        tmin, tmax = tmax, tmin
    tymin, tymax = t0[1], t1[1]
    if tymin > tymax:
        tymin, tymax = tymax, tymin
    if tmin > tymax or tymin > tmax:
        return F32(-1)
    if tymin > tmin:
        tmin = tymin
    if tymax < tmax:
        tmax = tymax
    tzmin, tzmax = t0[2], t1[2]
    if tzmin > tzmax:
        tzmin, tzmax = tzmax, tzmin
    if tmin > tzmax or tzmin > tmax:
        return F32(-1)
    if tzmax < tmax:
        tmax = tzmax
    return tmax


def vis_peak_stack(case, ray=0, t_offset=0.05):
    """Largest number of pending entries bvh_trace_kernel holds for one ray that is never cut off (the walk ignores the leaves: a case
    that uses this keeps every contribution negligible).  Returns (peak, leaves reached)."""
    boxes = bo.leaf_boxes(case["means"], case["scales"], case["rots"])
    P = boxes.shape[0]
    code = vis_morton(boxes)
    keys = sorted((int(code[i]) << 31) | i for i in range(P))
    order = [k & 0x7FFFFFFF for k in keys]
    ch = karras(keys)
    nb = np.zeros((max(P - 1, 1), 2, 6), dtype=F32)        # boxes of both children per internal node

    def box_of(c):                                           # post-order union, iterative
        if c < 0:
            return boxes[order[~c]]
        return np.concatenate([np.fmin(nb[c, 0, :3], nb[c, 1, :3]), np.fmax(nb[c, 0, 3:], nb[c, 1, 3:])])

    done, st = set(), [0] if P > 1 else []
    while st:
        n = st[-1]
        kids = [c for c in ch[n] if c >= 0 and c not in done]
        if kids:
            st.extend(kids)
            continue
        st.pop()
        nb[n, 0], nb[n, 1] = box_of(ch[n][0]), box_of(ch[n][1])
        done.add(n)
    d = _f(case["rays_d"]).reshape(-1, 3)[ray]
    o = _f(case["rays_o"]).reshape(-1, 3)[ray] + d * F32(t_offset)
    stack, peak, leaves = [0 if P > 1 else ~0], 1, 0
    while stack:
        n = stack.pop()
        if n < 0:
            leaves += 1
            continue
        tl, tr = _slab_tmax(nb[n, 0, :3], nb[n, 0, 3:], o, d), _slab_tmax(nb[n, 1, :3], nb[n, 1, 3:], o, d)
        seq = ((tl, ch[n][0]), (tr, ch[n][1])) if tl > tr else ((tr, ch[n][1]), (tl, ch[n][0]))
        for tm, c in seq:
            if tm > 0 and len(stack) < 64:
                stack.append(c)
        peak = max(peak, len(stack))
    return peak, leaves


def _box_entry(b, o, inv, t_min):
    """box_entry of csrc/pbgi.hip: (passes, entry')."""
    ex = F32(np.inf)
    with np.errstate(all="ignore"):
        for i in range(3):
            t0, t1 = (b[i] - o[i]) * inv[i], (b[3 + i] - o[i]) * inv[i]
            if inv[i] < 0:
                t0, t1 = t1, t0
            t_min = t0 if t0 > t_min else t_min
            ex = t1 if t1 < ex else ex
    return bool(ex > t_min), t_min


def rad_descent_stack(info, aabb, o, ray_d):
    """Entries pending when the first query of a ray reaches its first leaf, by pbgi_trace_kernel's rules: the root passes its own box
    (t in (0.042, 0.2)), then at every internal node the left child is pushed (untested while the direction is not fixed; if its box
    passes against closest = 0.2 once it is) and the right child is visited next while ITS box passes.  Nothing is popped before the
    first leaf, so this is a lower bound of the ray's peak occupancy.  Returns (pending, fixed)."""
    d = unit3_f32(ray_d)
    fixed = bool(len_f32(d) == F32(1))
    with np.errstate(all="ignore"):
        inv = F32(1) / np.where(d == 0, F32(0.000001), d).astype(F32)
    o = _f(o)
    t_min, closest = F32(0.042), F32(0.2)
    L = (info.shape[0] + 1) // 2 - 1
    ok, en = _box_entry(aabb[0], o, inv, t_min)
    if not (ok and closest > en):
        return 0, fixed
    cur, count = 0, 0
    while cur < L:
        left, right = int(info[cur, 0]), int(info[cur, 1])
        if fixed:
            ok, en = _box_entry(aabb[left], o, inv, t_min)
            if ok and closest > en:
                count += 1
        else:
            count += 1
        ok, en = _box_entry(aabb[right], o, inv, t_min)
        if not (ok and closest > en):
            return count, fixed                                  # the walk turns to the stack here: `count` entries were pending
        cur = right
    return count, fixed


def rad_chunks(N, S):
    """The scheduler's arithmetic for one block of rows (svgir_pbgi_trace_radiance): rays per chunk, chunks, rays per XCD part, waves."""
    chunk = max(S, (64 + S - 1) // S * S)
    rays = N * S
    nchunks = (rays + chunk - 1) // chunk
    part = (nchunks + 7) // 8 * chunk
    return dict(chunk=chunk, nchunks=nchunks, part=part, waves=min(nchunks, RESIDENT_SLOTS), empty_parts=8 - (rays + part - 1) // part)


# ======================================================================================================================================
# visibility tracer (csrc/bvh.hip)
# ======================================================================================================================================
def _surfels(means, scales, q, opacity):
    """The per-surfel arrays RayTracer takes, from means / scales / quaternions (the construction of tests/test_bvh_oracle._scene)."""
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T.astype(np.float64)
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                  np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                  np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    Linv = R * (1.0 / scales.astype(np.float64))[:, None, :]
    Cinv = Linv @ Linv.transpose(0, 2, 1)
    symm = np.stack([Cinv[:, 0, 0], Cinv[:, 0, 1], Cinv[:, 0, 2], Cinv[:, 1, 1], Cinv[:, 1, 2], Cinv[:, 2, 2]], -1)
    return dict(means=_f(means), scales=_f(scales), rots=_f(q), symm=_f(symm), opacity=_f(opacity), normals=_f(R[:, :, 2]))


def _vis(sc, rays_o, rays_d, holds, tol=VIS_TOL, tol_source="tests/test_gpu_bvh.py", **more):
    out = {k: sc[k] for k in ("means", "scales", "rots", "symm", "opacity", "normals")}
    out.update(rays_o=_f(rays_o), rays_d=_f(rays_d), holds=holds, tol=tol, tol_source=tol_source, **more)
    return out


def _unit_rays(rng, n):
    d = rng.normal(size=(n, 3)).astype(F32)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


# ---- wave_tails: bvh_trace_kernel runs one 64-lane wave per workgroup ----
WAVE_TAILS = (1, 63, 64, 65, 129)
for _n in WAVE_TAILS:
    @_case(VIS, f"wave_tails_{_n}")
    def _wave_tails(n=_n):
        sc = _scene(300, 50)
        sc["opacity"] = sc["opacity"] * F32(0.3)             # (so that about half of the rays stay open)
        rng = np.random.default_rng(51)                      # the same stream for every n: ray i is the same ray in every case
        pick = rng.integers(0, 300, size=129)
        d = _unit_rays(rng, 129)
        return _vis(sc, sc["means"][pick][:n], d[:n], f"{n} rays: {n // 64} full waves and a tail of {n % 64}")


# ---- deep_stack: a chain-shaped tree ----
CATERPILLAR_EPS = 2.0 ** -13          # offset between the three coordinates of the caterpillar's axis, in units of the scene extent
DEEP_CLUSTER = 128                    # coincident surfels at the deep end: 7 more levels through the index bits of morton << 31 | id


def _caterpillar_s():
    """Positions s_k, k = 0 .. 29, along the axis u(s) = (s, s - e, s - 2e) of the unit cube whose 30-bit Morton code (x bit first) has
    exactly k leading ones, and the position of the deep end (30 ones).  With b_j = 1 - 2^-(j+1): the axis is in the region of
    k = 3j while s is below b_j (x bit j still 0), of 3j + 1 between b_j and b_j + e (x has crossed, y has not), of 3j + 2 up to
    b_j + 2e.  Every position is the middle of its interval: at least e / 2 = 2^-14 of the extent from a cell boundary, 2^9 fp32 ulps."""
    e = CATERPILLAR_EPS
    s, low = [], 2 * e
    for j in range(10):
        b = 1 - 2.0 ** -(j + 1)
        s += [(low + b) / 2, b + e / 2, b + 1.5 * e]
        low = b + 2 * e
    return np.array(s), (low + 1) / 2


@_case(VIS, "deep_stack")
def _vis_deep_stack():
    """The scene extent is the unit cube, pinned by two transparent anchors in opposite corners.  Surfel k sits on the axis in the region
    of k leading ones (a left leaf of the chain), DEEP_CLUSTER coincident surfels at the deep end.  Ray 0 starts beyond the deep end
    and runs down the axis towards the root's side: at chain node k the leaf k lies farther along the ray than everything deeper, so
    its exit distance is the larger one, it is pushed first and stays pending while the walk goes on into the chain.  No ties: the
    positions are at least 2^-13 apart and the boxes 2^-15 wide.  Every surfel is displaced by 2^-16 across the axis under an inverse
    covariance of 2^39: power = -64, alpha < 1e-28, so every leaf reached counts and the product stays 1."""
    e = CATERPILLAR_EPS
    s, s_deep = _caterpillar_s()
    axis = lambda t: np.stack([t, t - e, t - 2 * e], -1)
    rho = 2.0 ** -16
    across = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0) * rho
    delta = 2.0 ** -12
    means = np.concatenate([axis(s) + across, np.tile(axis(np.array([s_deep])) + across, (DEEP_CLUSTER, 1)),
                            np.full((1, 3), delta), np.full((1, 3), 1 - delta)])
    P = means.shape[0]
    half = np.full(P, 2.0 ** -15)
    half[-2:] = delta
    scales = np.repeat((half / 3)[:, None], 3, axis=1)
    opacity = np.full(P, 0.5)
    opacity[-2:] = 0.0                                        # the anchors only pin the extent
    q = np.tile(np.array([1.0, 0, 0, 0]), (P, 1))
    sc = _surfels(means, scales, q, opacity)
    sc["symm"] = _f(np.tile(np.array([2.0 ** 39, 0, 0, 2.0 ** 39, 0, 2.0 ** 39]), (P, 1)))
    sc["normals"] = _f(np.tile(np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0), (P, 1)))   # faces the rays that run down the axis
    dn = -np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    start = axis(np.array([1.02]))[0]
    rng = np.random.default_rng(61)
    n = 64
    o = np.tile(start - 0.05 * dn, (n, 1))
    d = np.tile(dn, (n, 1))
    o[1], d[1] = axis(np.array([-0.05]))[0], -dn              # up the axis: the deep end exits last, the leaves are taken on the way
    o[2:40] += rng.normal(size=(38, 3)) * 2.0 ** -17          # beside the axis: some of the boxes are missed
    o[40:] += rng.normal(size=(n - 40, 3)) * 0.05             # far beside it: nothing is hit
    return _vis(sc, o, d, f"ray 0 leaves bvh_trace_kernel holding >= {VIS_DEEP} pending entries", deep_ray=0, min_peak=VIS_DEEP)


# ---- exact_ties: one or two surfels, axis-aligned rays through the mean; alpha equals the opacity bit for bit ----
def _tie_scene(mean_z=0.5, opacity=0.05, normal=(0.0, 0.0, -1.0)):
    """One surfel (the root is its leaf, entered untested), inverse covariance 4 I; the ray starts at z = -0.05 so that the origin
    after the 0.05 offset is exactly 0 (fl(1 * 0.05f) = 0.05f), and runs along +z: t = fl(4 mean_z) / 4 = mean_z exactly, the closest
    point is the mean, power = -0, __expf(-0) = 1, alpha = opacity."""
    sc = dict(means=_f([[0, 0, mean_z]]), scales=_f([[0.125, 0.125, 0.125]]), rots=_f([[1, 0, 0, 0]]), symm=_f([[4, 0, 0, 4, 0, 4]]),
              opacity=_f([opacity]), normals=_f([normal]))
    return sc, _f([[0, 0, -F32(0.05)]]), _f([[0, 0, 1]])


def _tie(name, holds, expect, **kw):
    @_case(VIS, f"exact_{name}")
    def build():
        sc, o, d = _tie_scene(**kw)
        return _vis(sc, o, d, holds, exact=dict(contribute=np.array([expect[0]], np.int32), visibility=_f([expect[1]])))


_OP = F32(1) / F32(255)
_tie("opacity_1_255", "opacity == float(1/255): not below it, the surfel counts", (1, F32(1) - _OP), opacity=_OP)
_tie("opacity_below_1_255", "opacity one ulp below float(1/255): skipped", (0, F32(1)), opacity=down(_OP))
_C9 = F32(0.9)
_tie("cutoff_0p9", "1 - opacity == 0.9f: (double)0.9f < 0.9, the ray is cut off", (0, F32(0)), opacity=F32(1) - _C9)
_tie("cutoff_below_0p9", "1 - opacity one ulp below 0.9f: cut off", (0, F32(0)), opacity=F32(1) - down(_C9))
_tie("cutoff_above_0p9", "1 - opacity one ulp above 0.9f: above the double 0.9, the ray stays open", (1, up(_C9)), opacity=F32(1) - up(_C9))
_T01 = F32(0.01)
_tie("t_0p01", "t == 0.01f: (double)0.01f < 0.01, skipped", (0, F32(1)), mean_z=_T01)
_tie("t_below_0p01", "t one ulp below 0.01f: skipped", (0, F32(1)), mean_z=down(_T01))
_tie("t_above_0p01", "t one ulp above 0.01f: above the double 0.01, counts", (1, F32(1) - F32(0.05)), mean_z=up(_T01))
_TINY = F32(2.0 ** -100)
_tie("facing_zero", "the ray lies in the surfel's plane: facing dot == 0, not back-facing", (1, F32(1) - F32(0.05)), normal=(1.0, 0.0, 0.0))
_tie("facing_plus", "facing dot = +2^-100: back-facing, skipped", (0, F32(1)), normal=(1.0, 0.0, _TINY))
_tie("facing_minus", "facing dot = -2^-100: counts", (1, F32(1) - F32(0.05)), normal=(1.0, 0.0, -_TINY))
assert F32(1) - (F32(1) - _C9) == _C9 and F32(1) - (F32(1) - up(_C9)) == up(_C9) and F32(1) - (F32(1) - down(_C9)) == down(_C9)


def _on_face(name, x, expect_count, holds):
    @_case(VIS, f"exact_{name}")
    def build():
        """Two surfels with boxes of half-width 0.375 (3 x 0.125): A at the origin, B at (0.375, 0, 1).  The ray runs along +z at
        x = `x`: on A's face x = 0.375 the slab test divides 0 by 0; the NaN exit distance fails `tmax > 0` and A is not entered.
        Inverse covariances 0 except zz: power = -0 for both, alpha = opacity = 0.03125 (1 - alpha and the product are exact)."""
        sc = dict(means=_f([[0, 0, 0.25], [0.375, 0, 1]]), scales=_f([[0.125] * 3] * 2), rots=_f([[1, 0, 0, 0]] * 2),
                  symm=_f([[0, 0, 0, 0, 0, 4]] * 2), opacity=_f([0.03125, 0.03125]), normals=_f([[0, 0, -1]] * 2))
        keep = F32(1) - F32(0.03125)
        return _vis(sc, _f([[x, 0, -F32(0.05)]]), _f([[0, 0, 1]]), holds,
                    exact=dict(contribute=np.array([expect_count], np.int32), visibility=_f([keep * keep if expect_count == 2 else keep])))


_on_face("origin_on_box_face", F32(0.375), 1, "origin on a box face, zero direction component: 0 / 0 in the slab test, the box is not entered")
_on_face("origin_inside_box_face", down(F32(0.375)), 2, "origin one ulp inside the face: -inf / +inf, the box is entered")
_on_face("origin_outside_box_face", up(F32(0.375)), 1, "origin one ulp outside the face: +inf / +inf, the box is missed")


# ---- degenerate_geometry: ordinary surfels and rays beside the degenerate ones ----
def _degenerate(name, holds, tol=VIS_TOL, tol_source="tests/test_gpu_bvh.py"):
    def deco(fn):
        @_case(VIS, f"degenerate_{name}")
        def build():
            sc = _scene(200, 70)
            sc["opacity"] = sc["opacity"] * F32(0.3)
            rng = np.random.default_rng(71)
            o = sc["means"][rng.integers(0, 200, size=300)].copy()
            d = _unit_rays(rng, 300)
            extra = fn(sc, o, d, rng) or {}
            return _vis(sc, o, d, holds, tol=tol, tol_source=tol_source, **extra)
        return fn
    return deco


@_degenerate("coincident", "60 surfels share one mean: equal Morton codes, six levels of the tree come from the index bits")
def _(sc, o, d, rng):
    sc["means"][:60] = sc["means"][0]
    o[:20] = sc["means"][0] + _f(rng.normal(size=(20, 3)) * 0.01) - d[:20] * F32(0.3)   # rays through the pile, beside its mean


@_degenerate("zero_extent", "every surfel on the x axis with zero scales: the whole box has zero width in y and z (0 / 0 in the Morton scaling)")
def _(sc, o, d, rng):
    sc["means"][:, 1:] = 0
    sc["scales"][:] = 0
    o[:20, 1:] = 0
    d[:20] = _f([1, 0, 0])                                   # along the axis: 0 / 0 in the y and z slabs; rays 0 and 1 ON it (through every mean:
    o[2:20, 2] = F32(0.01)                                   # power = 0, threshold rays by construction), the others beside it (-inf / -inf in z)


@_degenerate("zero_quaternion", "one zero quaternion: its box is NaN, it is never entered; the others are unaffected")
def _(sc, o, d, rng):
    sc["rots"][7] = 0
    return dict(nan_box=7)


@_degenerate("zero_scale_axis", "surfels with one zero scale axis: flat boxes")
def _(sc, o, d, rng):
    sc["scales"][:40, 2] = 0
    sc["scales"][40:60, 0] = 0


@_degenerate("far_coordinates", "coordinates near 1e4: fp32 keeps 1e-3 of a coordinate")
def _(sc, o, d, rng):
    big = _scene(200, 72, flat=False)                        # a scene 20 times the size: sigma 0.4 .. 3 against the 1e-3 fp32 keeps
    for k in ("means", "scales"):
        sc[k][:] = big[k] * F32(20)
    for k in ("rots", "normals"):
        sc[k][:] = big[k]
    sc["symm"][:] = big["symm"] / F32(400)
    sc["means"] += F32(1e4)
    o[:] = sc["means"][rng.integers(0, 200, size=300)]


@_degenerate("bad_directions", "a zero-length and a NaN direction: NaN results where the oracle's are NaN, every other ray unaffected")
def _(sc, o, d, rng):
    d[3] = 0
    d[64] = np.nan
    d[130, 1] = np.nan
    return dict(bad_rays=(3, 64, 130))


# ---- sort_sizes: the tracers' 30-bit sort plan (8 + 8 + 8 + 6) at the radix sort's size thresholds ----
SORT_SIZES = (1023, 1024, 1025, 2047, 2048, 2049, 32767, 32768, 32769)
SORT_LAYOUTS = ("spread", "low6")
SORT_RAYS = 2000
SORT_OPAQUE = 1500       # surfels with a non-zero opacity: a ray's threshold risk grows with the surfels that could count for it


def sort_means(P, layout, rng):
    """spread: codes over all 30 bits.  low6: every surfel but one anchor in the first 3.5 cells of each axis -- codes below 64, the
    first three passes of the sort see one digit."""
    if layout == "spread":
        return rng.uniform(-1, 1, size=(P, 3))
    m = rng.uniform(0, 3.5 / 1024, size=(P, 3)) * 2      # (next to the origin: fp32 resolves these surfels as well as the spread ones)
    m[P // 2] = 2.0
    return m


for _P in SORT_SIZES:
    for _lay in SORT_LAYOUTS:
        @_case(VIS, f"sort_P{_P}_{_lay}")
        def _vis_sort(P=_P, layout=_lay):
            rng = np.random.default_rng(P + len(layout))
            means = sort_means(P, layout, rng)
            size = (0.6 if layout == "spread" else 0.002) * P ** (-1 / 3)
            scales = size * np.exp(rng.uniform(np.log(0.3), 0, size=(P, 3)))
            scales[:, 2] *= 0.05
            q = rng.normal(size=(P, 4))
            opacity = rng.uniform(0, 0.3, size=P)
            if P > SORT_OPAQUE:
                opacity[rng.permutation(P)[SORT_OPAQUE:]] = 0
            sc = _surfels(means, scales, q, opacity)
            seen = np.flatnonzero(opacity > 0)
            o = sc["means"][rng.choice(seen, size=SORT_RAYS)].copy()
            d = _unit_rays(rng, SORT_RAYS)
            # the tracer starts 0.05 along the ray: 0.03 in front of a surfel (t > 0.01), a little beside its mean (a ray THROUGH a mean has
            # power = 0 up to rounding: a threshold ray by construction)
            o += (rng.normal(size=o.shape) * 0.3 * size).astype(F32) - d * F32(0.05 + 0.03)
            return _vis(sc, o, d, f"P = {P}, {layout} codes", layout=layout)


# ======================================================================================================================================
# radiance tracer (csrc/pbgi.hip)
# ======================================================================================================================================
def _rad(sc, ray_o, ray_d, holds, tol=RAD_TOL, tol_source="tests/test_gpu_pbgi.py", **more):
    out = {k: _f(sc[k]) for k in ("xyz", "scales", "rot", "normals", "opacity", "cov_inv", "shs")}
    ray_d = _f(ray_d)
    out.update(ray_o=_f(ray_o), ray_d=ray_d, S=ray_d.shape[1], holds=holds, tol=tol, tol_source=tol_source, **more)
    return out


def _take(sc, P):
    return {k: sc[k][:P] for k in ("xyz", "scales", "rot", "normals", "opacity", "cov_inv", "shs")}


for _P in (1, 2, 3):
    @_case(RAD, f"tiny_trees_P{_P}")
    def _tiny(P=_P):
        """N = 5 rows that are no surfel centres; half of the rays aim at a surfel, half anywhere."""
        sc = _take(pbgi_scene.make(P=20, shells=1, S=8, seed=80 + P), P)
        rng = np.random.default_rng(90 + P)
        o = sc["xyz"].mean(0) + sc["normals"][0] / np.linalg.norm(sc["normals"][0]) * 0.05 + rng.normal(size=(5, 3)) * 0.01
        d = rng.normal(size=(5, 8, 3))
        for r in range(5):
            for j in range(4):
                d[r, j] = sc["xyz"][(r + j) % P] - o[r] + rng.normal(size=3) * 0.004
        return _rad(sc, o, d, f"P = {P}: " + ("the root is a leaf, no pair record exists" if P == 1 else f"{P - 1} internal nodes"))


@_case(RAD, "more_rows_than_surfels")
def _more_rows():
    """P = 100, N = 2 P + 3: three blocks of rows (100, 100, 3).  Row r < P starts 0.1 in front of surfel r; its ray 0 runs straight at it:
    the hit is the row's own surfel and is rejected (Q-d).  Row P + r repeats row r: the same hit is now surfel r != row P + r and is kept."""
    sc = pbgi_scene.make(P=100, shells=1, S=4, seed=101)
    P = 100
    n = sc["normals"] / np.linalg.norm(sc["normals"], axis=1, keepdims=True)
    o = sc["xyz"] + n * F32(0.1)
    d = sc["ray_d"].copy()
    d[:, 0] = -n * F32(1.5)
    rng = np.random.default_rng(102)
    o3 = sc["xyz"][:3] + rng.normal(size=(3, 3)) * 0.01
    return _rad(_take(sc, P), np.concatenate([o, o, o3]), np.concatenate([d, d, d[:3]]), "N = 2 P + 3: the row of the self-hit test is the row in the call",
                P=P)


SAMPLE_COUNTS = {    # S: what svgir_pbgi_trace_radiance makes of N = 40 rows
    1: dict(chunk=64, nchunks=1, part=64, waves=1, empty_parts=7),
    3: dict(chunk=66, nchunks=2, part=66, waves=2, empty_parts=6),
    63: dict(chunk=126, nchunks=20, part=378, waves=20, empty_parts=1),
    64: dict(chunk=64, nchunks=40, part=320, waves=40, empty_parts=0),
    65: dict(chunk=65, nchunks=40, part=325, waves=40, empty_parts=0),
    200: dict(chunk=200, nchunks=40, part=1000, waves=40, empty_parts=0),
}
SAMPLE_ROWS = 40
for _S in SAMPLE_COUNTS:
    @_case(RAD, f"sample_counts_S{_S}")
    def _samples(S=_S):
        sc = pbgi_scene.make(P=200, shells=2, S=S, seed=110)
        return _rad(_take(sc, 200), sc["xyz"][:SAMPLE_ROWS], sc["ray_d"][:SAMPLE_ROWS], f"S = {S}: {SAMPLE_COUNTS[S]}", sched=SAMPLE_COUNTS[S])


QUEUE_REFILL = dict(chunk=64, nchunks=4200, part=33600, waves=RESIDENT_SLOTS, empty_parts=0)


@_case(RAD, "queue_refill")
def _refill():
    sc = pbgi_scene.make(P=4200, shells=42, S=64, seed=120)
    return _rad(_take(sc, 4200), sc["xyz"], sc["ray_d"], f"268 800 rays: 4 200 chunks for {RESIDENT_SLOTS} resident waves", sched=QUEUE_REFILL)


def _axis_dirs(fixed, want, rng):
    """Directions within 2^-16 of the cube diagonal whose normalised fp32 length is exactly 1 (fixed) or stays different from 1."""
    out = []
    while len(out) < want:
        d = _f(1 + rng.integers(-128, 129, size=(256, 3)) * 2.0 ** -23) * F32(rng.uniform(0.5, 2.0))
        ok = is_fixed(d) if fixed else stays_unfixed(d)
        out += list(d[ok])
    return _f(out[:want])


for _fixed in (False, True):
    @_case(RAD, "deep_stack_fixed" if _fixed else "deep_stack_unfixed")
    def _rad_deep(fixed=_fixed):
        """The caterpillar of the visibility case in the radiance tracer's tree: extent = a cube of side 3/32 pinned by one transparent
        anchor in its middle (scale 2^-6, box half-width 3 x 2^-6; its cell is 512 in every axis: it shares the code of surfel 3), surfel k
        ON ray 0 in the region of k leading ones, box half-width 2^-17.  Codes ascend along the right children: node k's left child is
        leaf k, its right child everything deeper.  Ray 0 runs up the axis (root's side first, 0.03 before the cube, 0.19 to its far
        corner): every right box contains the far end of the axis, every left box is pierced."""
        A = 3 * 2.0 ** -6
        e = CATERPILLAR_EPS
        s, s_deep = _caterpillar_s()
        rng = np.random.default_rng(130 + fixed)
        dirs = _axis_dirs(fixed, 16, rng)
        d0 = dirs[0].astype(np.float64)
        g = d0 / d0[0]                                         # du/ds per axis: within 2^-16 of (1, 1, 1)
        # the axis through (e', e' - e, e' - 2e) at s = 0 with slope g: the regions' borders move by less than 2^-16
        axis = lambda t: np.stack([t * g[0], t * g[1] - e, t * g[2] - 2 * e], -1)
        world = lambda u: (u * 2 - 1) * A
        pos = world(np.concatenate([axis(s), axis(np.array([s_deep]))]))
        P = pos.shape[0] + 1
        xyz = np.concatenate([np.zeros((1, 3)), pos[::-1]])    # ids: the anchor, then the deep end first -- no row (0 .. 5) starts at its own surfel's hit
        scales = np.full((P, 3), 2.0 ** -17 / 3)
        scales[:, 2] = 1e-4 * 2.0 ** -17
        scales[0] = 2.0 ** -6
        un = d0 / np.linalg.norm(d0)
        normals = np.tile(-un, (P, 1))                          # facing ray 0
        q = pbgi_scene.quat_from_z(normals.copy())
        opacity = np.full((P, 1), 0.3)
        opacity[0] = 0.0
        R = pbgi_scene.rotmat(q)
        inv = R @ (np.eye(3)[None] / (scales ** 2)[:, None, :]) @ np.transpose(R, (0, 2, 1))
        cov_inv = np.stack([inv[:, 0, 0], inv[:, 0, 1], inv[:, 0, 2], inv[:, 1, 1], inv[:, 1, 2], inv[:, 2, 2]], -1)
        shs = rng.normal(size=(P, 16, 3)) * 0.3
        shs[:, 0] += 1.0
        sc = dict(xyz=xyz, scales=scales, rot=q, normals=normals, opacity=opacity, cov_inv=cov_inv, shs=shs)
        start = world(axis(np.array([0.0])))[0] - un * 0.03
        N = 6
        o = np.tile(start, (N, 1))
        o[1:] += rng.normal(size=(N - 1, 3)) * 2.0 ** -18      # rows beside the axis: their rays pierce some of the boxes
        o[N - 1] = start + 0.2                                  # a row outside: nothing is hit
        d = np.tile(dirs[None], (N, 1, 1))
        return _rad(sc, o, d, f"ray 0 of row 0 holds >= {RAD_DEEP} pending entries; every direction is " + ("fixed" if fixed else "not fixed"),
                    deep_ray=(0, 0), min_peak=RAD_DEEP, fixed=fixed)


for _fixed in (True, False):
    @_case(RAD, "fixed_only" if _fixed else "unfixed_only")
    def _one_kind(fixed=_fixed):
        sc = pbgi_scene.make(P=400, shells=4, S=16, seed=140)
        rng = np.random.default_rng(141 + fixed)
        d = sc["ray_d"].copy()
        kind = is_fixed if fixed else stays_unfixed
        nrm = np.broadcast_to(sc["normals"][:, None], d.shape)
        for _ in range(1000):                                # redraw the rays of the other kind (same hemisphere about the normal)
            bad = ~kind(d)
            if not bad.any():
                break
            new = rng.normal(size=(int(bad.sum()), 3))
            new *= np.sign((new * nrm[bad]).sum(-1, keepdims=True)) * rng.uniform(0.5, 2.0, size=(new.shape[0], 1))
            d[bad] = new.astype(F32)
        assert kind(d).all()
        return _rad(_take(sc, 400), sc["xyz"], d, "every direction is " + ("fixed: children are box-tested when pushed" if fixed
                    else "still not fixed after one re-normalisation: children are pushed untested"), fixed=fixed)


LONG_RAY_SURFELS, LONG_RAY_MIN_QUERIES = 300, 200
for _lane in (0, 31, 63):
    @_case(RAD, f"long_ray_lane{_lane}")
    def _long_ray(lane=_lane):
        """An ordinary shell (surfels 0 .. 199, rows 0 .. 19) and, away from it, a row of 300 parallel surfels 0.0105 apart (a little more
        than the 0.01 restart distance) with opacity 0.02, facing -z.  Row 20 starts in front of the row of surfels; its ray `lane` runs along
        +z, 0.25 sigma beside the centres: one hit per query, T = 0.98^k stays above 0.001 for all 300.  The other 63 rays of the chunk
        point away and end after one query.  (Surfel ids 200 .. 499: no hit is the ray's own row.)"""
        sh = pbgi_scene.make(P=200, shells=2, S=64, seed=150)
        n = LONG_RAY_SURFELS
        rng = np.random.default_rng(151)
        base = np.array([3.0, 3.0, 3.0])
        xyz = base + np.stack([np.zeros(n), np.zeros(n), 0.05 + 0.0105 * np.arange(n)], -1)
        scales = np.tile(np.array([0.02, 0.02, 1e-3]), (n, 1))
        q = np.tile(np.array([1.0, 0, 0, 0]), (n, 1))
        cov = np.tile(np.array([1 / 0.02 ** 2, 0, 0, 1 / 0.02 ** 2, 0, 1e6]), (n, 1))
        shs = rng.normal(size=(n, 16, 3)) * 0.3
        shs[:, 0] += 1.0
        sc = dict(xyz=np.concatenate([sh["xyz"], xyz]), scales=np.concatenate([sh["scales"], scales]), rot=np.concatenate([sh["rot"], q]),
                  normals=np.concatenate([sh["normals"], np.tile(np.array([0, 0, -1.0]), (n, 1))]),
                  opacity=np.concatenate([sh["opacity"], np.full((n, 1), 0.02)]), cov_inv=np.concatenate([sh["cov_inv"], cov]),
                  shs=np.concatenate([sh["shs"], shs]))
        o = np.concatenate([sh["xyz"][:20], (base + np.array([0.005, 0, 0]))[None]])
        d = np.concatenate([sh["ray_d"][:20], np.zeros((1, 64, 3), F32)])
        away = rng.normal(size=(64, 3))
        away[:, 2] = -np.abs(away[:, 2]) - 0.5
        d[20] = away
        d[20, lane] = [0, 0, 1]
        return _rad(sc, o, d, f"ray {lane} of row 20 takes >= {LONG_RAY_MIN_QUERIES} queries beside one-query rays", long_ray=(20, lane))


# ---- exact ties of the radiance tracer ----
def _flat(P, z, opacity, sx=0.005, x=None, sy=None):
    """P surfels facing -z at (x, 0, z[i]), identity rotation (sqrt(1 + 1e-8) = 1 in fp32: the rotation matrix is exactly I), inverse
    covariance 0: power = -0, expf(-0) = 1, alpha = min(0.99, opacity) exactly."""
    x = np.zeros(P) if x is None else np.asarray(x)
    rng = np.random.default_rng(160)
    shs = rng.normal(size=(P, 16, 3)) * 0.3
    shs[:, 0] += 1.0
    return dict(xyz=np.stack([x, np.zeros(P), np.asarray(z, dtype=np.float64)], -1), scales=np.tile(np.array([sx, sx if sy is None else sy, 1e-3]), (P, 1)),
                rot=np.tile(np.array([1.0, 0, 0, 0]), (P, 1)), normals=np.tile(np.array([0, 0, -1.0]), (P, 1)),
                opacity=np.asarray(opacity, dtype=F32).reshape(P, 1), cov_inv=np.zeros((P, 6)), shs=shs)


def find_product(target):
    """Two fp32 opacities a, b >= 0.5 (so that 1 - a is exact) with fl((1 - a) * (1 - b)) == target, by search over the 2 048 fp32 values
    around 1 - sqrt(target)."""
    target = F32(target)
    root = np.sqrt(float(target))
    for ratio in (1.0, 1.03, 1.07, 1.12, 1.2, 1.3):          # (the products of one pair of binades need not contain the target)
        grid = lambda k0: F32(1 - k0) + (np.arange(2048, dtype=F32) - F32(1024)) * np.spacing(F32(1 - k0))
        a, b = grid(root * ratio), grid(root / ratio)
        found = np.argwhere((F32(1) - a)[:, None] * (F32(1) - b)[None, :] == target)
        if len(found):
            return a[found[0][0]], b[found[0][1]]
    raise AssertionError(f"no pair of opacities gives {target}")


def _rad_tie(name, holds, build):
    @_case(RAD, f"exact_{name}")
    def make():
        sc, o, d, exact = build()
        return _rad(sc, o, d, holds, exact=exact)


_Z2 = (0.125, 0.25, 3.0)     # two surfels 0.125 apart on the ray, a third far away so that the rays are never in row 0 .. 1's own surfel
_ROW = lambda: (np.zeros((3, 3)), np.tile(np.array([[[0, 0, 1.0], [0, 0, -1.0]]]), (3, 1, 1)))   # rows 0..2, ray 0 along +z, ray 1 away


def _alpha_tie(op, hit):
    def build():
        sc = _flat(3, _Z2, [op, 0.0, 0.0])
        o, d = _ROW()
        exact = dict(row=2, hit=[0 if hit else -1, -1], visibility=[F32(1) - F32(op) if hit else F32(1), F32(1)])
        return sc, o, d, exact
    return build


_rad_tie("alpha_1_255", "alpha == float(1/255): accepted", _alpha_tie(_OP, True))
_rad_tie("alpha_below_1_255", "alpha one ulp below float(1/255): not accepted", _alpha_tie(down(_OP), False))


def _T_tie(target, step):
    def build():
        a, b = find_product(target)
        b = {0: b, 1: down(b), -1: up(b)}[step]                # a smaller opacity: a larger T
        sc = _flat(3, _Z2, [a, b, 0.0])
        o, d = _ROW()
        T = (F32(1) - a) * (F32(1) - b)
        return sc, o, d, dict(row=2, hit=[0, -1], visibility=[T if not T < F32(0.2) else F32(0), F32(1)], T=T)
    return build


_rad_tie("T_0p2", "T == 0.2f after two hits: not below it, the ray stays visible", _T_tie(0.2, 0))
_rad_tie("T_above_0p2", "T just above 0.2f: visible", _T_tie(0.2, 1))
_rad_tie("T_below_0p2", "T just below 0.2f: visibility 0", _T_tie(0.2, -1))


def _T_end(step):
    def build():
        """Three surfels 0.125 apart: after two hits T is 0.001f (or a neighbour); `T > 0.001f` decides whether the third one is asked for."""
        a, b = find_product(0.001)
        b = {0: b, 1: down(b), -1: up(b)}[step]
        sc = _flat(4, (0.125, 0.25, 0.375, 3.0), [a, b, 0.5, 0.0])
        o = np.zeros((4, 3))
        d = np.tile(np.array([[[0, 0, 1.0], [0, 0, -1.0]]]), (4, 1, 1))
        T = (F32(1) - a) * (F32(1) - b)
        return sc, o, d, dict(row=3, hit=[0, -1], visibility=[F32(0), F32(1)], T=T, third_asked=bool(T > F32(0.001)))
    return build


_rad_tie("T_0p001", "T == 0.001f after two hits: not above it, the ray ends", _T_end(0))
_rad_tie("T_above_0p001", "T just above 0.001f: a third query", _T_end(1))
_rad_tie("T_below_0p001", "T just below 0.001f: the ray ends", _T_end(-1))


def _dis_tie(px, hit):
    def build():
        """The ray passes 3 sx beside the centre (sx = 2^-7: 3 sx and the squares are exact): dis == 9.  (sy = 2 sx: the box is 6 sx wide,
        the ray is inside it.)"""
        sc = _flat(3, _Z2, [0.5, 0.0, 0.0], sx=2.0 ** -7, sy=2.0 ** -6)
        o = np.tile(np.array([[px, 0, 0]], dtype=np.float64), (3, 1))
        d = np.tile(np.array([[[0, 0, 1.0], [0, 0, -1.0]]]), (3, 1, 1))
        return sc, o, d, dict(row=2, hit=[0 if hit else -1, -1], visibility=[F32(0.5) if hit else F32(1), F32(1)])
    return build


_rad_tie("dis_9", "dis == 9: inside the ellipse", _dis_tie(F32(3 * 2.0 ** -7), True))
_rad_tie("dis_above_9", "dis one step above 9: outside", _dis_tie(up(F32(3 * 2.0 ** -7)), False))


def _denom_tie(dz, hit):
    def build():
        """Direction (1, 0, dz): fl(1 + dz^2) = 1, the normalised direction is (1, 0, dz) and denom = dz.  The surfel's plane z = 1e-7 is
        met at t = 1e-7 / dz ~ 0.1, at its centre (0.1, 0, 1e-7) up to 1e-8."""
        sc = _flat(3, (1e-7, 2.0, 3.0), [0.5, 0.0, 0.0], sx=0.02, x=(F32(1e-7) / F32(1e-6), 0, 0))
        o = np.zeros((3, 3))
        d = np.tile(np.array([[[1.0, 0, dz], [-1.0, 0, -1.0]]]), (3, 1, 1))
        return sc, o, d, dict(row=2, hit=[0 if hit else -1, -1], visibility=[F32(0.5) if hit else F32(1), F32(1)])
    return build


_rad_tie("denom_1e-6", "|denom| == 1e-6f: not below it, the plane is intersected", _denom_tie(F32(1e-6), True))
_rad_tie("denom_below_1e-6", "|denom| one ulp below 1e-6f: parallel, no hit", _denom_tie(down(F32(1e-6)), False))


def _qb():
    """Q-b: surfel 1 lies 0.22 ahead, its box (half-width 0.06) starts before 0.2: it is visited and accepted although it is beyond t_max;
    the query reports the initial closest index 0 at t = 0.2.  Surfel 0 is far away."""
    sc = _flat(3, (5.0, 0.22, 3.0), [0.5, 0.5, 0.0], sx=0.02)
    o, d = _ROW()
    return sc, o, d, dict(row=2, hit=[0, -1], visibility=None)


_rad_tie("qb_beyond_t_max", "Q-b: an accepted leaf beyond 0.2 gives index 0", _qb)


def _qd(row):
    def build():
        sc = _flat(3, (5.0, 0.125, 3.0), [0.5, 0.5, 0.0])
        o, d = _ROW()
        return sc, o, d, dict(row=row, hit=[-1 if row == 1 else 1, -1], visibility=[F32(1) if row == 1 else F32(0.5), F32(1)])
    return build


_rad_tie("qd_self_hit", "Q-d: row 1 hits surfel 1: rejected, the ray ends", _qd(1))
_rad_tie("qd_other_row", "Q-d: the same ray in row 2 hits surfel 1: kept", _qd(2))


# ---- the radiance tracer's own tree at the sort thresholds (compared with po.build, no rays) ----
def sort_tree_inputs(P, layout):
    rng = np.random.default_rng(7 * P + len(layout))
    xyz = sort_means(P, layout, rng)
    scales = np.full((P, 3), 1e-4) * rng.uniform(0.5, 1.0, size=(P, 1))
    return _f(xyz), _f(scales)


def vis_reference(case, fp64=False):
    """(contribute, visibility, margin) of the oracle for a visibility case."""
    boxes = bo.leaf_boxes(case["means"], case["scales"], case["rots"])
    with np.errstate(all="ignore"):
        return bo.trace_visibility(boxes, case["rays_o"], case["rays_d"], case["means"], case["symm"], case["opacity"], case["normals"],
                                   fp64=fp64, with_margin=True)


@functools.lru_cache(maxsize=None)
def vis_expected(name):
    """fp32 oracle results of a visibility case + the threshold mask (margin of either precision below VIS_MARGIN; none on exact cases)."""
    case = VIS[name]()
    c32, v32, m32 = vis_reference(case)
    c64, v64, m64 = vis_reference(case, fp64=True)
    margin = np.fmin(m32, m64)
    thr = np.zeros(c32.shape, dtype=bool) if "exact" in case else margin < VIS_MARGIN
    return dict(contribute=c32, visibility=v32, contribute64=c64, visibility64=v64, margin=margin, threshold=thr)


def rad_reference(case, **kw):
    info, aabb, _ = po.build(case["xyz"], case["scales"])
    return po.trace(info, aabb, case["ray_o"], case["ray_d"], case["xyz"], case["scales"], case["rot"], case["normals"], case["opacity"],
                    case["cov_inv"], case["shs"], **kw)


@functools.lru_cache(maxsize=None)
def rad_expected(name):
    case = RAD[name]()
    rad, vis, hit, uvs, margin, queries = rad_reference(case, instruments=True)
    thr = np.zeros(margin.shape, dtype=bool) if "exact" in case else margin < RAD_MARGIN
    return dict(radiance=rad, visibility=vis, hit=hit, uvs=uvs, margin=margin, queries=queries, threshold=thr)
