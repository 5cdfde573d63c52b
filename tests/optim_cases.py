"""The case table of the optimizer edge tests: one table for tests/test_optim_edge_inputs.py (the CPU oracle alone: every case reaches
the edge it is named for, the oracle reproduces the reference's fixtures and torch.optim.Adam) and tests/test_gpu_optim_edges.py
(csrc/optim.hip through svgir_harness/optim.py against oracle/optim_oracle.py).

Launch geometry the sizes are chosen around (csrc/optim.hip):
  adam_kernel          one workgroup per ADAM_CHUNK = 4096 elements of one tensor; the owning tensor is found by walking first_chunk[];
                       at most MAX_TENSORS = 32 tensors per launch (the harness splits longer lists)
  mask count / scatter (the front-only compaction of csrc/subset.hip) SCAN_ELEMS = 2048 mask entries per workgroup; the scatter kernel
                       sums the totals of the earlier blocks in a loop strided by SCAN_BLOCK = 256, so the loop's second trip needs more
                       than 256 blocks (P > 524288)
  gather / append      grid.x sized by the widest tensor of the launch (narrower ones return early), grid.y = tensor
  stats / masks / split one thread per row, 256 per workgroup

Kinds of expectation:
  exact   row movement, masks, kept lists, counts, step counts, gradient tensors left behind: raw bits
  values  arithmetic outputs: `same` = the criterion of tests/test_gpu_optim.py `_same` -- shapes equal, NaN / inf pattern equal, finite
          values within tol x the tensor's largest finite magnitude; TOL = 2e-6, TOL_DENSIFIED = 3e-6 (parameters after a densification),
          TOL_EXP_AVG_SQ = 4e-6.  No case of this table needs another bound: the split transform at its extreme scales (get_scaling =
          1e-6 and FLT_MAX) loses at most 2.3e-7 (xyz) and 4.2e-8 (scaling) of the tensor's scale in the reference's own fp32 arithmetic
          against the fp64 oracle (test_optim_edge_inputs.py::test_split_transform_fp32_error prints it and asserts 4 x it is inside
          TOL_DENSIFIED).  Positions beyond 1e30 (children of a row whose get_scaling is FLT_MAX) are measured among themselves.
          A split child's third log-scale (-1e10) is compared exactly and kept out of the tensor's scale, so the bound is not inflated.

Threshold rows.  Every comparison a mask makes in this table is an exact tie by construction (the tie scenes of the fixture) or clear
of its threshold: no mean gradient within 4 ulp of its threshold unless equal to it, no activated scale within 1e-5 (relative) of
its limit unless it is a constructed tie, no pruning quantity within 1e-5 of its threshold.  The host test asserts it from the
oracle's record of every comparison (`Model.compared`); with that, masks must be IDENTICAL on the GPU, no row excused.
"""
import functools
import os

import numpy as np

from oracle import optim_oracle as oo

F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL, TOL_DENSIFIED, TOL_EXP_AVG_SQ = 2e-6, 3e-6, 4e-6
EPS = 1e-15
# the reference's parameter block as the fixtures hold it: group name, shape per Gaussian, learning rate
SPEC = [("xyz", (3,), 1.6e-4), ("normal", (12,), 1e-3), ("rotation", (4,), 1e-3), ("scaling", (3,), 5e-3), ("opacity", (1,), 5e-2),
        ("f_dc", (1, 3), 2.5e-3), ("f_rest", (15, 3), 1.25e-4), ("base_color", (12,), 1e-2), ("roughness", (4,), 1e-2),
        ("incidents_dc", (1, 3), 2e-3), ("incidents_rest", (15, 3), 1e-4), ("visibility_dc", (1, 1), 2.5e-3),
        ("visibility_rest", (15, 1), 1.25e-4)]
NAMES = [n for n, _, _ in SPEC]
LRS = {n: lr for n, _, lr in SPEC}
BOOK = oo.BOOK
TIE_SCENES = ("tie_size", "nan_scale_at_limit")     # scenes whose activated scale EQUALS the limit, by construction


def same(a, b, what, tol=TOL):
    """tests/test_gpu_optim.py `_same` for arrays (or torch tensors) `a` against the expectation `b`."""
    a = np.asarray(a.detach().double().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.size == 0:
        return 0.0
    finite = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), finite) and np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN / inf pattern differs"
    assert np.array_equal(a[~finite & ~np.isnan(b)], b[~finite & ~np.isnan(b)]), f"{what}: sign of an infinity differs"
    scale = max(np.abs(b[finite]).max(), 1e-30) if finite.any() else 1.0
    err = np.abs(a[finite] - b[finite]).max() if finite.any() else 0.0
    assert err <= tol * scale, (what, err / scale, tol)
    return err / scale


def same_scaling(a, b, what, tol):
    """`same` for the log-scales: the -1e10 of a split child is compared exactly and stays out of the tensor's scale."""
    a = np.asarray(a.detach().double().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    flat = b.astype(F32) == F32(-1e10)            # (in fp32, where a later Adam step of 5e-3 leaves -1e10 as it is: its ulp is 1024)
    assert np.array_equal(a.astype(F32) == F32(-1e10), flat), f"{what}: the -1e10 axes differ"
    return same(a[~flat], b[~flat], what, tol)


def same_xyz(a, b, what, tol):
    """`same` for positions: rows that hold a NaN, an infinity or a magnitude above 1e30 (the children of a row whose get_scaling is
    FLT_MAX) are compared among themselves, so they do not set the scale the ordinary rows are measured by."""
    a = np.asarray(a.detach().double().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    with np.errstate(invalid="ignore"):
        wild = ~(np.abs(b) < 1e30).all(axis=1)
    same(a[wild], b[wild], what + " (rows beyond 1e30)", tol)
    return same(a[~wild], b[~wild], what, tol)


# ---- the reference's fixtures ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gold(fname):
    return dict(np.load(os.path.join(GOLD, fname)))


def scene_names():
    return [str(s) for s in gold("densify_edges.npz")["scenes"]]


def unpack_block(g, scene, block):
    """{group: array [rows, ...] or None} of a block stored as one flat vector (scripts/make_golden_densify.py `put_block`)."""
    flat, has = g[f"{scene}/{block}"], g[f"{scene}/{block}_has"]
    width = sum(int(np.prod(shp)) for (_, shp, _), h in zip(SPEC, has) if h)
    rows = flat.size // width if width else 0
    out, o = {}, 0
    for (n, shp, _), h in zip(SPEC, has):
        if not h:
            out[n] = None
            continue
        k = rows * int(np.prod(shp))
        out[n] = flat[o:o + k].reshape((rows,) + shp)
        o += k
    assert o == flat.size
    return out


def scene_inputs(scene):
    """Everything a run of one fixture scene is given: init {group: [P, ...]}, grads [per step {group: array or None}], stat {name:
    array}, op, args (max_grad, min_opacity, extent, max_screen_size or None, max_grad_normal), z, post_grad."""
    g = gold("densify_edges.npz")
    a = g[f"{scene}/args"]
    st = g[f"{scene}/stat"]
    return dict(init=unpack_block(g, scene, "init"), grads=[unpack_block(g, scene, f"grad{i}") for i in range(int(g[f"{scene}/pre"]))],
                stat={k: (st[i].reshape(-1, 1) if k != "max_radii2D" else st[i].copy()) for i, k in enumerate(BOOK)},
                op=str(g[f"{scene}/op"]), z=g[f"{scene}/split_z"], post_grad=unpack_block(g, scene, "post_grad"),
                args=dict(max_grad=float(a[0]), min_opacity=float(a[1]), extent=float(a[2]),
                          max_screen_size=None if np.isnan(a[3]) else float(a[3]), max_grad_normal=float(a[4])))


def scene_reference(scene, tag):
    """What the reference ended with after the densification (`dens`) or the step behind it (`post`), as a snapshot."""
    g = gold("densify_edges.npz")
    st = g[f"{scene}/{tag}_stat"]
    return dict(params=unpack_block(g, scene, tag), m=unpack_block(g, scene, tag + "_m"), v=unpack_block(g, scene, tag + "_v"),
                t={n: int(x) for n, x in zip(NAMES, g[f"{scene}/{tag}_t"])},
                book={k: (st[i].reshape(-1, 1) if k != "max_radii2D" else st[i]) for i, k in enumerate(BOOK)})


def snapshot(model):
    st = model.state
    return dict(params={n: p.copy() for n, p in model.params.items()},
                m={n: None if st[n] is None else st[n]["exp_avg"].copy() for n in st},
                v={n: None if st[n] is None else st[n]["exp_avg_sq"].copy() for n in st},
                t={n: -1 if st[n] is None else st[n]["step"] for n in st},
                book={k: getattr(model, k).copy() for k in BOOK},
                origin=model.origin.copy(), fresh=model.fresh.copy(), child=model.child.copy())


def run_densify(model, op, args, z):
    if op == "prune":
        return None, None, model.prune(args["min_opacity"], args["extent"], args["max_screen_size"], weights_threshold=1e-5)
    return model.densify_and_prune(args["max_grad"], args["min_opacity"], args["extent"], args["max_screen_size"], args["max_grad_normal"], z=z)


@functools.lru_cache(maxsize=None)
def scene_expected(scene):
    """The oracle's run of a scene: masks (clone, split, pruned; over the rows they were taken on), the snapshots `dens` and `post`
    (with the row movement since the densification began: origin / fresh / child), and every comparison made (`compared`)."""
    c = scene_inputs(scene)
    m = oo.Model(c["init"], LRS, percent_dense=0.01, use_pbr=True, eps=EPS)
    for gr in c["grads"]:
        m.step(gr)
    for k in BOOK:
        setattr(m, k, np.array(c["stat"][k], dtype=np.float64))
    m.mark()
    clone, split, pruned = run_densify(m, c["op"], c["args"], c["z"])
    dens = snapshot(m)
    m.step(c["post_grad"])
    return dict(clone=clone, split=split, pruned=pruned, dens=dens, post=snapshot(m), compared=m.compared)


def compare_snapshot(got, exp, what, densified=True):
    """values of a snapshot `got` (arrays or tensors) against `exp`: the project's bounds, step counts and missing state exact"""
    tol_p = TOL_DENSIFIED if densified else TOL
    for n in NAMES:
        (same_scaling if n == "scaling" else same_xyz if n == "xyz" else same)(got["params"][n], exp["params"][n], f"{what} {n}", tol_p)
        assert got["t"][n] == exp["t"][n], (what, n, "step count", got["t"][n], exp["t"][n])
        assert (got["m"][n] is None) == (exp["m"][n] is None), (what, n, "Adam state present")
        if exp["m"][n] is not None:
            same(got["m"][n], exp["m"][n], f"{what} exp_avg {n}", TOL)
            same(got["v"][n], exp["v"][n], f"{what} exp_avg_sq {n}", TOL_EXP_AVG_SQ)
    for k in BOOK:
        same(got["book"][k], exp["book"][k], f"{what} {k}", TOL)


def near_threshold(compared, ties_allowed):
    """Rows of the oracle's comparison record that sit too close to a threshold without being an allowed tie: [(kind, value, threshold)]."""
    bad = []
    for kind, vals, thr in compared:
        vals, thr = np.asarray(vals, dtype=np.float64), float(thr)
        with np.errstate(invalid="ignore"):
            if kind == "grad":
                near = (vals != thr) & (np.abs(vals - thr) <= 4 * float(np.spacing(F32(thr))))
            elif kind == "scale":
                near = np.abs(vals - thr) <= 1e-5 * abs(thr)
                if ties_allowed:
                    near &= vals != thr
            else:
                near = np.abs(vals - thr) <= 1e-5 * abs(thr)
        bad += [(kind, float(x), thr) for x in vals[near]]
    return bad


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------
ADAM = {}
ADAM_SIZES = (1, 63, 64, 255, 256, 257, 4095, 4096, 4097, 8192, 12289)
MAGNITUDES = (0.0, 1e-30, -1e-30, 1e-20, -1e-20, 3e-17, 1.0, 1e19, 1e20, 5e20, 1e21, float("inf"), float("-inf"), float("nan"))


def _adam_case(name):
    def deco(fn):
        assert name not in ADAM
        ADAM[name] = functools.lru_cache(maxsize=None)(fn)
        return fn
    return deco


def _adam(edge, sizes, seed, steps=2, lrs=None, start=None, nan_values=None, zero_grad=False, arbiter="fp64", nan_share=0.0, names=None):
    """A table of 1-d tensors.  `start`: per tensor None (no state yet) or the step count already taken (moments are then seeded)."""
    rng = np.random.default_rng(seed)
    k = len(sizes)
    c = dict(edge=edge, sizes=list(sizes), names=names or [f"t{i}" for i in range(k)], lrs=list(lrs or [10.0 ** -(2 + i % 4) for i in range(k)]),
             nan_values=nan_values, zero_grad=zero_grad, arbiter=arbiter)
    # magnitudes in [0.5, 2) with either sign and steps of at most 2e-2: the value a one-element tensor ends with is never the leftover
    # of a cancellation, so `same`'s "of the tensor's scale" stays a bound in units of the fp32 rounding of the operands
    c["params"] = [(rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)).astype(F32) for n in sizes]
    start = start or [None] * k
    c["state"] = [None if s is None else (s, (rng.standard_normal(n) * 1e-2).astype(F32), (rng.random(n) * 1e-3).astype(F32))
                  for s, n in zip(start, sizes)]
    c["grads"] = []
    for it in range(steps):
        gs = []
        for i, n in enumerate(sizes):
            g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 2)).astype(F32)
            if nan_share:
                g[rng.random(n) < nan_share] = np.nan
                if n:
                    g[(it + i) % n] = np.nan
            gs.append(g)
        c["grads"].append(gs)
    return c


@_adam_case("chunk_sizes")
def _():
    return _adam("n on both sides of 64, 256 and of one, two and three chunks of 4096, all in one table", ADAM_SIZES, 1)


@_adam_case("table_of_32")
def _():
    return _adam("exactly MAX_TENSORS tensors: the table is full, first_chunk[] is walked to its last entry",
                 [1, 4097, 1, 300] + [1 + 37 * i for i in range(27)] + [1], 2)


@_adam_case("table_of_40")
def _():
    return _adam("40 tensors: two launches, 32 + 8", [1, 5000] * 4 + [7 + 11 * i for i in range(31)] + [1], 3)


@_adam_case("empty_tensor_between")
def _():
    return _adam("a numel() == 0 parameter with a gradient between two others: skipped by the table, its step count still advances", [300, 0, 4097], 4)


@_adam_case("step_counts")
def _():
    return _adam("bias corrections at step 1, 2, 1000 and 100000; lr = 0 leaves the parameter alone", [257, 257, 257, 257, 257], 5, steps=1,
                 start=[None, 1, 999, 99999, 7], lrs=[1e-2, 1e-2, 1e-2, 1e-2, 0.0])


@_adam_case("gradient_magnitudes")
def _():
    k = len(MAGNITUDES)
    c = _adam("every gradient magnitude class side by side, two steps: (w2 g) g is finite at 1e20 where w2 (g g) is not; then each class in "
              "a tensor of its own, so that the bound is in units of that class's scale", [k * 3] + [3] * k, 6, lrs=[1e-3] * (k + 1), arbiter="torch32")
    start = np.array([0.5, -2.0, 0.0], dtype=F32)
    c["params"] = [np.repeat(start, k)] + [start.copy() for _ in range(k)]
    c["grads"] = [[np.tile(np.array(MAGNITUDES, dtype=F32), 3)] + [np.full(3, g, dtype=F32) for g in MAGNITUDES] for _ in range(2)]
    return c


@_adam_case("scrub_value_no_group_uses")
def _():
    return _adam("scrub on with the replacement 0.375 (group a) and 0 (group c), off on group b: its NaNs reach the parameter; the gradient "
                 "tensors keep the scrubbed values", [300, 300, 4097], 7, nan_values={"a": 0.375, "c": 0.0}, nan_share=0.02, names=["a", "b", "c"])


@_adam_case("scrub_and_fill")
def _():
    return _adam("SCRUB_NAN together with ZERO_GRAD: the update sees the replacement, the gradient tensor reads all zeros", [300, 300, 4097], 8,
                 nan_values={"a": 0.375, "c": 1e-6}, zero_grad="fill", nan_share=0.02, names=["a", "b", "c"])


def adam_geometry(c):
    """chunks per tensor, and the launch each tensor lands in (the harness batches the tensors that have a gradient by 32)"""
    return [-(-n // oo.ADAM_CHUNK) for n in c["sizes"]], [i // oo.MAX_TENSORS for i in range(len(c["sizes"]))]


@functools.lru_cache(maxsize=None)
def adam_expected(name):
    """The oracle's run: final (p, m, v) per tensor, step counts, and the gradient tensors as the LAST step leaves them."""
    c = ADAM[name]()
    p = [a.astype(np.float64) for a in c["params"]]
    m = [np.zeros(n) if s is None else s[1].astype(np.float64) for s, n in zip(c["state"], c["sizes"])]
    v = [np.zeros(n) if s is None else s[2].astype(np.float64) for s, n in zip(c["state"], c["sizes"])]
    t = [0 if s is None else s[0] for s in c["state"]]
    left = None
    for gs in c["grads"]:
        left = []
        for i, g in enumerate(gs):
            t[i] += 1
            nv = None if c["nan_values"] is None else c["nan_values"].get(c["names"][i])
            p[i], m[i], v[i], gl = oo.adam_step(p[i], g, m[i], v[i], t[i], c["lrs"][i], eps=EPS, nan_value=nv, fill=c["zero_grad"] == "fill")
            left.append(gl)
    return dict(p=p, m=m, v=v, t=t, grad_left=left)


def adam_torch(name, dtype):
    """torch.optim.Adam on the CPU in `dtype` over the same case (the scrub as the reference does it: in place, in front of step())."""
    import torch
    c = ADAM[name]()
    ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dtype)) for a in c["params"]]
    opt = torch.optim.Adam([{"params": [p], "lr": lr, "name": n} for p, lr, n in zip(ps, c["lrs"], c["names"])], lr=1e-4, eps=EPS)
    for p, s in zip(ps, c["state"]):
        if s is not None:
            opt.state[p] = {"step": torch.tensor(float(s[0])), "exp_avg": torch.from_numpy(s[1].copy()).to(dtype), "exp_avg_sq": torch.from_numpy(s[2].copy()).to(dtype)}
    for gs in c["grads"]:
        for p, g, n in zip(ps, gs, c["names"]):
            g = torch.from_numpy(g.copy()).to(dtype)
            if c["nan_values"] is not None and n in c["nan_values"]:
                g[torch.isnan(g)] = float(F32(c["nan_values"][n]))      # (the fp32 tensor of the reference holds fp32(value))
            p.grad = g
        opt.step()
    return dict(p=[p.detach().numpy() for p in ps], m=[opt.state[p]["exp_avg"].numpy() for p in ps],
                v=[opt.state[p]["exp_avg_sq"].numpy() for p in ps], t=[int(opt.state[p]["step"]) for p in ps])


def finiteness_class(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    a = np.asarray(a)
    return np.where(np.isnan(a), 3, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 0)))


# ---- mask scan and compaction ------------------------------------------------------------------------------------------------------------
MASK_P = (1, 7, 8, 9, 2047, 2048, 2049, 4096, 6145, 526337, 528389)
MASK_SHAPES = ("all", "none", "first", "last", "block_edge", "one_block", "one_empty_block", "alternating", "every_2048", "random_0.001",
               "random_0.5", "random_0.999")
MANY_TENSORS_P, MANY_TENSORS = 2049, 35      # two gather launches


def scan_blocks(P):
    return -(-P // oo.SCAN_ELEMS)


def block_sum_trips(P):
    """trips of the scatter kernel's `for (b = t; b < blockIdx.x; b += BLOCK)` loop taken by thread 0 of the LAST block"""
    return -(-(scan_blocks(P) - 1) // oo.SCAN_BLOCK)


def mask(P, shape):
    m = np.zeros(P, dtype=bool)
    nb = scan_blocks(P)
    b = min(1, nb - 1)       # the block singled out: the second one where there is one
    if shape == "all":
        m[:] = True
    elif shape == "first":
        m[0] = True
    elif shape == "last":
        m[P - 1] = True
    elif shape == "block_edge":          # the last element of block 0 and the first of block 1 (as far as they exist)
        m[[i for i in (oo.SCAN_ELEMS - 1, oo.SCAN_ELEMS) if i < P]] = True
    elif shape == "one_block":
        m[b * oo.SCAN_ELEMS:(b + 1) * oo.SCAN_ELEMS] = True
    elif shape == "one_empty_block":
        m[:] = True
        m[b * oo.SCAN_ELEMS:(b + 1) * oo.SCAN_ELEMS] = False
    elif shape == "alternating":
        m[1::2] = True
    elif shape == "every_2048":
        m[oo.SCAN_ELEMS - 1::oo.SCAN_ELEMS] = True
    elif shape.startswith("random_"):
        m = np.random.default_rng(P).random(P) < float(shape[7:])
    else:
        assert shape == "none"
    return m


def row_tensors(P, many=False):
    """[(what, array [P, ...])] compacted in ONE call; every word is distinct within its tensor, so a misplaced word shows.  The big
    sizes carry a handful of narrow tensors, the others every width of the parameter block."""
    def t(words, base, dtype=F32, shape=None):
        return (np.arange(P * words, dtype=np.int64) % (1 << 24) + base).astype(dtype).reshape((P,) + ((words,) if shape is None else shape))
    if many:
        return [(f"#{i} width {1 + 2 * (i % 2)}", t(1 + 2 * (i % 2), i)) for i in range(MANY_TENSORS)]
    out = [("fp32 [P,1]", t(1, 1)), ("fp32 [P,3]", t(3, 2)), ("int32 [P]", t(1, 3, np.int32, ()))]
    if P <= 8192:
        out += [("fp32 [P,4]", t(4, 4)), ("fp32 [P,4,3]", t(12, 5, shape=(4, 3))), ("fp32 [P,15,3]", t(45, 6, shape=(15, 3))),
                ("non-contiguous [P,3] of [P,6]", t(6, 7)[:, ::2])]
    return out


# ---- append ------------------------------------------------------------------------------------------------------------------------------
# (P, selection, repeat): P and n_sel * repeat on both sides of 256 and 2048; selections of 0, 1, all and the last row only
APPEND = ((0, "none", 1), (0, "none", 2), (1, "all", 1), (1, "all", 3), (255, "all", 1), (256, "last", 2), (257, "none", 3), (257, 128, 2),
          (300, 85, 3), (300, 86, 3), (300, 255, 1), (300, 257, 1), (2047, "all", 1), (2048, "first", 3), (2049, "last", 1), (2049, 1024, 2),
          (2049, 683, 3), (2049, 2047, 1), (2049, "all", 3))
APPEND_TENSORS = (("fp32 [P,1]", 1, F32, False), ("fp32 [P,15,3]", 45, F32, False), ("int32 [P]", 0, np.int32, False),
                  ("fp32 [P,3] zero_new", 3, F32, True), ("fp32 [P,15,3] zero_new", 45, F32, True), ("fp32 [P,1] zero_new", 1, F32, True))


def append_selection(P, sel):
    m = np.zeros(P, dtype=bool)
    if sel == "all":
        m[:] = True
    elif sel == "first":
        m[0] = True
    elif sel == "last":
        m[P - 1] = True
    elif sel != "none":
        m[np.random.default_rng(P + sel).choice(P, sel, replace=False)] = True
    return m


def append_tensors(P):
    out = []
    for i, (what, words, dtype, zero_new) in enumerate(APPEND_TENSORS):
        shape = (P,) + ((15, 3) if words == 45 else (words,) if words else ())
        out.append((what, (np.arange(P * max(words, 1), dtype=np.int64) + 1 + i).astype(dtype).reshape(shape), zero_new))
    return out


# ---- statistics --------------------------------------------------------------------------------------------------------------------------
# (P, stride of the viewspace gradient, weights given, filter)
STATS = tuple((P, s, w, "random") for P in (1, 255, 256, 257, 513) for s, w in ((2, True), (3, False), (4, True))) + \
    ((257, 3, True, "none"), (257, 3, False, "all"), (513, 2, False, "none"), (513, 4, True, "all"))


def stats_case(P, stride, weights, flt):
    rng = np.random.default_rng(1000 * P + 10 * stride + weights)
    c = dict(vgrad=(rng.standard_normal((P, stride)) * 10.0 ** rng.integers(-5, 1, (P, 1))).astype(F32),
             weights=rng.random((P, 1)).astype(F32) if weights else None,
             filter={"random": rng.random(P) < 0.5, "none": np.zeros(P, dtype=bool), "all": np.ones(P, dtype=bool)}[flt],
             accum=[rng.random((P, 1)).astype(F32) for _ in range(3)])       # weights_accum, xyz_gradient_accum, denom
    out = ~c["filter"]
    c["vgrad"][out & (rng.random(P) < 0.5)] = np.nan        # a filtered-out row's gradient is never read into its accumulator
    if P > 1:
        c["vgrad"][:, 2:] = np.nan                           # nor are the columns behind the first two
    return c


# ---- split transform ---------------------------------------------------------------------------------------------------------------------
# (selected rows, N): N * selected = 255, 256, 257 new rows (one workgroup, exactly one, one more thread), and the reference's N = 2 and 3
SPLIT = ((255, 1), (256, 1), (257, 1), (128, 2), (86, 3), (1, 2))
SPLIT_P = 300
SPLIT_SPEC = [("xyz", (3,), 1.6e-4), ("rotation", (4,), 1e-3), ("scaling", (3,), 5e-3), ("opacity", (1,), 5e-2), ("f_rest", (15, 3), 1.25e-4)]


def split_case(n_sel, N):
    """A small block whose selected rows hold, among ordinary ones: a zero quaternion (NaN position, as in the reference), a third
    log-scale already at -1e10, a NaN log-scale (get_scaling 1e-6) and an overflowing one (FLT_MAX; its draw is 0.5 or 2: clear of
    the overflow of the product on either side)."""
    rng = np.random.default_rng(77 * n_sel + N)
    P = SPLIT_P
    params = {n: (rng.integers(-64, 65, (P,) + shp) / 32.0).astype(F32) for n, shp, _ in SPLIT_SPEC}
    params["scaling"] = rng.uniform(-6.0, 1.0, (P, 3)).astype(F32)
    sel = np.zeros(P, dtype=bool)
    sel[rng.choice(P, n_sel, replace=False)] = True
    rows = np.flatnonzero(sel)
    z = (rng.integers(-16, 17, (n_sel * N, 3)) / 8.0).astype(F32)
    special = {}
    for j, what in enumerate(("zero_quat", "flat", "nan_scale", "huge_scale", "huge_scale_inf")):
        if j < n_sel:
            special[what] = r = rows[j * max(n_sel // 5, 1) % n_sel] if n_sel >= 5 else rows[0]
            if what == "zero_quat":
                params["rotation"][r] = 0.0
            elif what == "flat":
                params["scaling"][r, 2] = -1e10
            elif what == "nan_scale":
                params["scaling"][r, 1] = np.nan
            else:
                params["scaling"][r, 0] = 100.0
                params["rotation"][r] = (1.0, 0.0, 0.0, 0.0)
                k = int(np.flatnonzero(rows == r)[0])
                z[k::n_sel, 0] = 0.5 if what == "huge_scale" else 2.0
            if n_sel < 5:
                break
    return dict(params=params, sel=sel, z=z, N=N, special=special)


@functools.lru_cache(maxsize=None)
def split_expected(n_sel, N):
    c = split_case(n_sel, N)
    m = oo.Model(c["params"], {n: lr for n, _, lr in SPLIT_SPEC}, use_pbr=False, eps=EPS)
    g = np.where(c["sel"], 1.0, 0.0).astype(F32)
    # every selected row passes the size test whatever its scale: limit 0 (get_scaling > 0 always)
    sel = m.densify_and_split(g, np.zeros_like(g), 0.5, 0.5, 0.0, c["z"], N=c["N"])
    assert np.array_equal(sel, c["sel"])
    return snapshot(m)
