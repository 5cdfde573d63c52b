"""The case table of the exact column median (csrc/select.hip) and its two consumers, with their numpy / torch-CPU oracles.  Shared by
tests/test_median_edge_inputs.py (CPU: proves the table and pins the oracles) and tests/test_gpu_median.py (the kernels).

COLUMN ORACLE (`column_oracle`): the contract of include/svgir_raster.h restated on the canonical uint32 keys -- NaN is one key above +inf,
-0 is +0 -- with a stable argsort: value = the key of rank (n - 1) / 2 (rank n - 1, the NaN key, when the column holds a NaN) turned back
into a float, index = the first row with that key, n_less / n_greater = the rows with a smaller / larger key.  test_median_edge_inputs
proves it equal to torch.median(dim=0).values on every case.

SIZES sit on the wave (64), the workgroup (256) and the rows one workgroup of the kernels covers (`T = metrics.SELECT_ROWS`, imported, not
retyped); 70 001 equal rows put one bin above 65 535 (a 16-bit packed counter would wrap) and span 35 workgroups.

HOT BIN.  With 99 % of the rows on one value the median cannot leave that value; the "outside" cases therefore give the hot value every
row short of the rank, and put the median on the value's fp32 neighbour: all digits but the last are shared with the hot bin.

ALBEDO: every selected pixel's mean is >= 1e-3 in magnitude and every other pixel is exactly 0 in all three channels (0 / 12.92 = 0 through
the linear branch), so a last-bit difference of pow cannot flip a selection (asserted by the CPU test).  E32 of a case is what the
reference's own fp32 arithmetic loses against fp64 on the selected, clamped ratios; the GPU test allows 4 max(E32, eps32): order statistics
are monotone, so keys within t (relative) of their fp64 values put the median within t of the fp64 median."""
import functools

import numpy as np
import torch

from svgir_harness.metrics import SELECT_ROWS as T

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
KEY_NAN = np.uint32(0xFFFFFFFF)


def _rng(tag):
    return np.random.default_rng(int.from_bytes(tag.encode(), "little") % (2 ** 63))


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def keys_of(col):
    col = np.ascontiguousarray(col, dtype=F32)
    u = col.view(np.uint32).copy()
    u[col == 0] = 0
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(col)] = KEY_NAN
    return k


def value_of(key):
    key = np.uint32(key)
    if key == KEY_NAN:
        return F32(np.nan)
    u = (key ^ np.uint32(0x80000000)) if key & np.uint32(0x80000000) else ~key
    return np.array([u], dtype=np.uint32).view(F32)[0]


def column_oracle(x):
    """(values [C] fp32, indices [C], n_less [C], n_greater [C]) of an [n, C] fp32 array."""
    x = np.asarray(x, dtype=F32)
    n, C = x.shape
    val, idx, less, greater = np.full(C, np.nan, F32), np.full(C, -1, np.int64), np.zeros(C, np.int64), np.zeros(C, np.int64)
    for c in range(C if n else 0):
        k = keys_of(x[:, c])
        rank = n - 1 if (k == KEY_NAN).any() else (n - 1) // 2
        med = k[np.argsort(k, kind="stable")[rank]]
        val[c], idx[c] = value_of(med), int(np.flatnonzero(k == med)[0])
        less[c], greater[c] = int((k < med).sum()), int((k > med).sum())
    return val, idx, less, greater


def lower_median64(x):
    """Per column of a float64 [n, C] array: the element of rank (n - 1) / 2, NaN where the column holds one, NaN for n == 0."""
    x = np.asarray(x, dtype=np.float64)
    n, C = x.shape
    out = np.full(C, np.nan)
    for c in range(C if n else 0):
        if not np.isnan(x[:, c]).any():
            out[c] = np.sort(x[:, c])[(n - 1) // 2]
    return out


# ---- column cases ----------------------------------------------------------------------------------------------------------------------
def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(F32)


def _generic(tag, n, C=3):
    """Column 0: a normal cloud; 1: the same quantised to 1/8 (ties); 2: coordinates that share an exponent; 3: small negatives."""
    g = _rng("generic" + tag)
    x = g.standard_normal((n, 4)).astype(F32)
    x[:, 1] = np.round(x[:, 1] * 8) / 8
    x[:, 2] = F32(9.0) + F32(0.25) * x[:, 2]
    x[:, 3] = -np.abs(x[:, 3]) * F32(1e-3)
    return x[:, :C].copy()


def _stack(*cols):
    return np.stack([np.asarray(c, dtype=F32) for c in cols], axis=1)


def _two_values(m, extra, a, b):
    return np.concatenate([np.full(m, a, F32), np.full(m + extra, b, F32)])


def _data(kind, n):
    g = _rng(kind + str(n))
    if kind == "generic":
        return _generic(str(n), n)
    if kind == "wide":          # every row equal: one bin holds n > 65 535 in every pass
        return _stack(np.full(n, 10.0), np.full(n, 1e-6), np.full(n, -3.25))
    if kind == "ascending":
        a = np.sort(g.standard_normal(n).astype(F32))
        return _stack(a, a[::-1], np.arange(n))
    if kind.startswith("ties"):  # m copies of a, then m (+ 1) of b: the rank sits on either side of the boundary, in both orders
        m, extra = n // 2, n % 2
        return _stack(_two_values(m, extra, 1.5, 2.5), _two_values(m, extra, 2.5, 1.5), _two_values(m, extra, -0.5, 0.5))
    if kind == "lowdigit":      # equal except in the lowest digit
        lo = g.integers(0, 256, (n, 3)).astype(np.uint32)
        return _bits(np.uint32(0x41234500) | lo) * np.array([1, -1, 1], F32)
    if kind == "highdigit":     # equal except in the highest digit (byte 2 = 0x34 keeps the exponent below 0xff: all finite)
        hi = g.integers(0, 256, (n, 3)).astype(np.uint32)
        return _bits((hi << np.uint32(24)) | np.uint32(0x00345678))
    if kind == "negatives":
        return -np.abs(_generic("neg", n)) - F32(0.5)
    if kind == "signmix":       # column 0: median negative; 1: median positive; 2: balanced
        x = _generic("mix", n)
        return x + np.array([-0.6, 0.6, 0.0], F32)
    if kind == "denormals":
        return _bits(g.integers(1, 0x800000, (n, 3)).astype(np.uint32) | (g.integers(0, 2, (n, 3)).astype(np.uint32) << np.uint32(31)))
    if kind == "zeros":         # the median is a zero of either sign; it comes out as +0
        q = n // 4
        z = np.where(g.integers(0, 2, n - 2 * q) == 1, F32(-0.0), F32(0.0)).astype(F32)
        col = lambda zz: g.permutation(np.concatenate([-np.ones(q, F32), zz, np.ones(q, F32)]))   # noqa: E731
        return _stack(col(z), col(np.full(n - 2 * q, -0.0, F32)), col(np.zeros(n - 2 * q, F32)))
    if kind == "inf":           # column 0: median +inf; 1: median -inf; 2: both infinities around a finite median
        x = _generic("inf", n)
        x[g.permutation(n)[: n // 2 + 3], 0] = np.inf
        x[g.permutation(n)[: n // 2 + 3], 1] = -np.inf
        p = g.permutation(n)
        x[p[:5], 2], x[p[5:11], 2] = np.inf, -np.inf
        return x
    if kind == "nan_one":       # one NaN in one column of three
        x = _generic("nan1", n)
        x[min(37, n - 1), 1] = np.nan
        return x
    if kind == "nan_all":       # column 0 all NaN (both signs of the payload); column 1: two NaNs, the first one is the index
        x = _generic("nanall", n)
        x[:, 0] = _bits(np.where(np.arange(n) % 2, np.uint32(0xFFC00001), np.uint32(0x7FC00000)))
        x[[5, 9], 1] = np.nan
        return x
    if kind.startswith("hot"):
        v = F32(10.0)
        up, dn = np.nextafter(v, F32(np.inf)), np.nextafter(v, F32(-np.inf))
        if kind == "hot_inside":     # 99 % equal, a few on each side
            few = max(n // 200, 1)
            col = np.full(n, v, F32)
            col[:few], col[few:2 * few] = F32(9.0) + g.random(few).astype(F32) * F32(0.5), F32(10.5) + g.random(few).astype(F32)
            cols = [g.permutation(col) for _ in range(3)]
            cols[1] = np.full(n, F32(1e-6), F32); cols[1][g.permutation(n)[:few]] = F32(0.5)     # the clamp's floor as the hot bin
            return _stack(*cols)
        k = (n - 1) // 2
        above = np.concatenate([np.full(k, v, F32), np.full(n - k, up, F32)])                     # rank k: the first row above the hot block
        below = np.concatenate([np.full(k + 1, dn, F32), np.full(n - k - 1, v, F32)])             # rank k: the last row below it
        return _stack(g.permutation(above), g.permutation(below), above)
    raise KeyError(kind)


def _column_cases():
    out = []

    def add(kind, n, layout="rows", C=3):
        out.append(dict(id=f"{kind}-{n}-{layout}" + (f"-C{C}" if C != 3 else ""), kind=kind, n=n, layout=layout, C=C))

    for n in (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1):
        add("generic", n)
    for n in (T + 1, 2 * T + 1):
        add("generic", n, "planar")
    add("wide", 70001)
    add("ascending", 257)
    for n in (6, 7, 128, 129):
        add("ties", n)
    for kind in ("lowdigit", "highdigit", "negatives", "signmix", "denormals", "zeros", "inf", "nan_one", "nan_all"):
        add(kind, 300)
    add("nan_one", T + 7)
    for kind in ("hot_inside", "hot_outside"):
        add(kind, 5000)
    add("hot_outside", 4999)
    for layout, C in (("planar", 3), ("rows", 1), ("rows", 4), ("planar", 4), ("sliced", 3), ("sliced", 2)):
        add("generic", 300, layout, C)
    add("empty", 0)
    return out


COLUMN_CASES = _column_cases()


@functools.lru_cache(maxsize=None)
def _column_data(kind, n, C):
    if kind == "empty":
        return np.zeros((0, C), F32)
    x = _generic(f"{n}c{C}", n, C) if kind == "generic" and C != 3 else _data(kind, n)
    x = np.ascontiguousarray(x[:, :C], dtype=F32)
    x.setflags(write=False)
    return x


def column_data(case):
    """The logical [n, C] fp32 array of a case (read-only, shared)."""
    return _column_data(case["kind"], case["n"], case["C"])


def column_view(case, to_tensor):
    """The case as the 2-D view the entry point is handed: `to_tensor(array)` makes the base tensor (on any device), the view has the
    layout of the case.  The padding of a sliced view is NaN: a read of it would show."""
    x = column_data(case)
    n, C = x.shape
    if case["layout"] == "rows":
        return to_tensor(x.copy())
    if case["layout"] == "planar":      # a [C, n] plane stack, handed over as its transpose
        return to_tensor(np.ascontiguousarray(x.T)).t()
    base = np.full((n + 5, C + 2), np.nan, F32)
    base[2:2 + n, 1:1 + C] = x
    return to_tensor(base)[2:2 + n, 1:1 + C]


@functools.lru_cache(maxsize=None)
def _column_reference(cid):
    return column_oracle(column_data(next(c for c in COLUMN_CASES if c["id"] == cid)))


def column_reference(case):
    return _column_reference(case["id"])


# ---- albedo cases ------------------------------------------------------------------------------------------------------------------------
LO, HI = 1e-6, 10.0          # what the eval passes
KNEE = F32(0.04045)


def knee_ladder():
    """Values on both sides of srgb_to_rgb's knee, its two fp32 neighbours included."""
    return np.array([-0.25, 0.0, 1e-4, np.nextafter(KNEE, F32(0)), KNEE, np.nextafter(KNEE, F32(1)), 0.05, 0.2, 0.5, 0.9, 1.0, 1.5], dtype=F32)


def srgb_to_rgb(img):
    """utils/graphics_utils.py:218-229 restated for a torch tensor of either dtype (pinned by tests/golden/median.npz)."""
    return torch.where(img <= 0.04045, img / 12.92, torch.pow((torch.max(img, torch.tensor(0.04045)) + 0.055) / 1.055, 2.4))


def albedo_lines(render, gt_albedo, srgb, to_rgb, lo=LO, hi=HI):
    """eval_relighting_tensoIR.py:227-237, literally, on torch tensors of one dtype -> (clamped ratios [count, 3], img_mask); the `.median(dim=0).values`
    of :237 is taken by the caller (torch raises on an empty selection)."""
    render_albedo = to_rgb(render) if srgb else render
    img_mask = render_albedo.mean(dim=0) > 0
    render_albedo = render_albedo.permute(1, 2, 0)[img_mask]
    gt_albedo = gt_albedo.permute(1, 2, 0)[img_mask]
    return (gt_albedo / render_albedo).clamp(lo, hi), img_mask


def _albedo_cases():
    out = []
    for H, W in ((1, 1), (5, 7), (17, 33), (150, 161)):   # 150 x 161 = 24 150 pixels: twelve workgroups, the last partial
        for sel in ("partial", "all"):
            if (H, W) == (1, 1) and sel == "partial":
                continue
            for srgb in (False, True):
                out.append(dict(id=f"{sel}-{H}x{W}" + ("-srgb" if srgb else ""), H=H, W=W, sel=sel, srgb=srgb, special=(H, W) in ((17, 33), (150, 161))))
    out += [dict(id="empty-17x33", H=17, W=33, sel="empty", srgb=False, special=False),
            dict(id="empty-5x7-srgb", H=5, W=7, sel="empty", srgb=True, special=False),
            dict(id="zero-over-zero-17x33", H=17, W=33, sel="partial", srgb=False, special="nan"),
            dict(id="zero-over-zero-150x161-srgb", H=150, W=161, sel="all", srgb=True, special="nan"),
            dict(id="knee-17x33-srgb", H=17, W=33, sel="partial", srgb=True, special="knee"),
            dict(id="knee-17x33", H=17, W=33, sel="partial", srgb=False, special="knee")]
    return out


ALBEDO_CASES = _albedo_cases()
GOLDEN_ALBEDO = ("partial-17x33-srgb", "all-5x7", "zero-over-zero-17x33", "knee-17x33-srgb", "all-150x161-srgb")   # recorded from the reference


@functools.lru_cache(maxsize=None)
def _build_albedo(cid):
    c = next(a for a in ALBEDO_CASES if a["id"] == cid)
    H, W = c["H"], c["W"]
    g = torch.Generator().manual_seed(int.from_bytes(("albedo" + cid).encode(), "little") % (2 ** 63))
    render = 0.06 + 0.9 * torch.rand(3, H, W, generator=g)              # above the knee: linear value >= 0.0048
    gt = torch.rand(3, H, W, generator=g) * torch.where(torch.rand(3, H, W, generator=g) < 0.5, 0.2, 1.0)   # ratios 0 ... > 10: many sit on hi
    if c["sel"] == "partial":      # background: exactly zero in all channels; a few pixels clearly negative
        render[:, torch.rand(H, W, generator=g) < 0.4] = 0.0
        render[:, torch.rand(H, W, generator=g) < 0.05] = -0.25
    elif c["sel"] == "empty":
        render = torch.zeros(3, H, W)
        render[:, ::2] = -0.5
    render, gt = render.float().contiguous(), gt.float().contiguous()
    if c["special"]:
        fr, fg = render.reshape(3, -1), gt.reshape(3, -1)
        pos = torch.nonzero((fr > 0.3).all(0))[:, 0]     # every channel large: the mean stays clearly positive after the edits below
        assert pos.numel() >= 8, cid
        p = [int(pos[i * (pos.numel() - 1) // 7]) for i in range(8)]
        if c["special"] == "knee":                        # both fp32 neighbours of the knee, and the knee itself, in every channel
            for q, v in zip(p[:3], (np.nextafter(KNEE, F32(0)), KNEE, np.nextafter(KNEE, F32(1)))):
                fr[:, q] = float(v)
        else:
            fr[0, p[0]], fg[0, p[0]] = 0.0, 0.5           # x / 0 = inf -> hi
            fg[1, p[1]] = 0.0                             # ratio 0 -> lo
            fr[1, p[2]] = -0.3                            # a negative channel inside a positive mean: ratio < 0 -> lo
            fr[2, p[3]], fg[2, p[3]] = 0.5, 5.0           # without srgb: exactly hi
            fr[2, p[4]], fg[2, p[4]] = 0.5, float(F32(LO) * F32(0.5))   # without srgb: exactly lo
            fg[0, p[5]] = -0.2                            # a negative ground truth -> lo
            if c["special"] == "nan":
                fr[0, p[6]], fg[0, p[6]] = 0.0, 0.0       # 0 / 0 -> NaN in channel 0 and in no other
    return render.numpy(), gt.numpy()


def build_albedo(case):
    """(render [3,H,W], gt [3,H,W]) fp32 arrays, shared: do not modify."""
    return _build_albedo(case["id"])


@functools.lru_cache(maxsize=None)
def _albedo_reference(cid):
    case = next(a for a in ALBEDO_CASES if a["id"] == cid)
    r, g = (torch.from_numpy(a) for a in build_albedo(case))
    q32, m32 = albedo_lines(r, g, case["srgb"], srgb_to_rgb)
    q64, m64 = albedo_lines(r.double(), g.double(), case["srgb"], srgb_to_rgb)
    q32, q64 = q32.numpy(), q64.numpy()
    s32 = column_oracle(q32)[0] if q32.shape[0] else np.full(3, np.nan, F32)
    s64 = lower_median64(q64)
    e32 = 0.0
    if q32.shape == q64.shape and q32.size:
        ok = np.isfinite(q64) & (q64 != 0)
        e32 = float(np.max(np.abs(q32.astype(np.float64) - q64)[ok] / np.abs(q64[ok]), initial=0.0))
    return dict(scale32=s32, scale64=s64, count=int(m64.sum()), mask32=m32.numpy(), mask64=m64.numpy(), e32=e32, q32=q32, q64=q64)


def albedo_reference(case):
    """scale32 (the fp32 lines + the column oracle: what the kernel gives bit for bit without srgb), scale64 (the fp64 lower median), count,
    the two masks, E32 and the clamped ratio matrices."""
    return _albedo_reference(case["id"])


# ---- loss cases --------------------------------------------------------------------------------------------------------------------------
def _loss_cases():
    out = []
    for P in (1, 2, 3, 257, 70001):
        out.append(dict(id=f"cloud-{P}", shape="cloud", P=P, ties=False))
    for P in (3, 257, 70001):
        out.append(dict(id=f"ties-{P}", shape="ties", P=P, ties=True))
    for P in (2, 257, 70001):
        out.append(dict(id=f"equal-{P}", shape="equal", P=P, ties=True))
    out.append(dict(id="nan-257", shape="nan", P=257, ties=False))
    for P in (257, 70001):
        out.append(dict(id=f"cube1e6-{P}", shape="cube", P=P, ties=True))
    return out


LOSS_CASES = _loss_cases()
GOLDEN_LOSS = ("cloud-2", "cloud-257", "ties-257", "equal-257", "nan-257", "cube1e6-257")   # recorded from the reference
UPSTREAM = 0.7   # the upstream gradient of the loss in every gradient check


@functools.lru_cache(maxsize=None)
def _build_loss(cid):
    c = next(a for a in LOSS_CASES if a["id"] == cid)
    P, g = c["P"], _rng("loss" + cid)
    if c["shape"] in ("cloud", "nan"):
        # a permutation of P distinct multiples of a power of two inside (-1, 1), plus an offset: no two rows of a column are equal,
        # every value is exact in fp32, and mean |x - c| stays near 0.3 (the fp32 subtraction's rounding stays below the tolerance)
        step = F32(2.0) ** -int(np.ceil(np.log2(P + 1)))
        x = _stack(*[(g.permutation(P).astype(F32) - F32(P // 2)) * step + F32(o) for o in (0.0, 2.0, -3.0)])
        if c["shape"] == "nan":
            x[100, 1] = np.nan
    elif c["shape"] == "ties":     # quarter steps: the median value is held by many rows
        x = (np.round(g.standard_normal((P, 3)) * 4) / 4).astype(F32)
    elif c["shape"] == "equal":
        x = np.tile(np.array([0.3, -1.7, 2.5], F32), (P, 1))
    else:                          # a unit cube at 1e6: the fp32 grid there is 1 / 16
        x = (F32(1e6) + g.uniform(-1, 1, (P, 3))).astype(F32)
    x = np.ascontiguousarray(x, dtype=F32)
    x.setflags(write=False)
    return x


def build_loss(case):
    return _build_loss(case["id"])


def loss_lines(xyz):
    """gaussian_renderer/render.py:218-219, literally, on a torch tensor of either dtype."""
    center, _ = torch.median(xyz, dim=0)
    return torch.exp(-(xyz - center[None, ...]).abs().mean())


@functools.lru_cache(maxsize=None)
def _loss_reference(cid):
    case = next(a for a in LOSS_CASES if a["id"] == cid)
    x = build_loss(case)
    P = x.shape[0]
    center, idx, less, greater = column_oracle(x)
    with np.errstate(invalid="ignore"):
        d32 = np.abs(x - center[None]).astype(F32)                    # the fp32 values the kernel sums ...
        sum32 = float(d32.astype(np.float64).sum())                   # ... in double
        d = x.astype(np.float64) - center.astype(np.float64)[None]
        loss64 = float(np.exp(-np.abs(d).mean()))
        coef = UPSTREAM * loss64 / (3 * P)
        grad = -coef * np.sign(d)                                      # (sign(0) = 0; NaN where the loss is NaN)
        if np.isnan(loss64):
            grad = np.full_like(grad, np.nan)
        else:
            for c in range(3):
                grad[idx[c], c] += coef * (greater[c] - less[c])
    with torch.no_grad():
        l32 = float(loss_lines(torch.from_numpy(x.copy())))
        l64 = float(loss_lines(torch.from_numpy(x.copy()).double()))
    e32 = abs(l32 - l64) / abs(l64) if np.isfinite(l64) and l64 != 0 else 0.0
    held = (keys_of(x.reshape(-1)).reshape(P, 3) == np.stack([keys_of(center[c:c + 1]) for c in range(3)], axis=1))   # rows holding the median
    return dict(center=center, index=idx, less=less, greater=greater, sum32=sum32, loss64=loss64, torch64=l64, grad=grad, coef=coef, e32=e32, held=held)


def loss_reference(case):
    """center / index / less / greater (the column oracle), sum32 (the kernel's double sum of the fp32 |x - c|), loss64 and grad (float64,
    upstream UPSTREAM, the gradient of `center` on the oracle's index row), torch64 (render.py's lines in fp64), E32 (what those lines lose
    in fp32), held [P,3] (True where a row holds its column's median value)."""
    return _loss_reference(case["id"])


def tie_sum(grad, held):
    """Per column the sum of `grad` over the rows that hold the median value (torch and the kernel may pick different rows among them)."""
    return np.where(held, np.asarray(grad, dtype=np.float64), 0.0).sum(axis=0)
