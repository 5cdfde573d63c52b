"""The case matrix of the image-space edge tests: one table for tests/test_image_edge_inputs.py (the fp64 oracle alone: every case holds
what it is named for, few pixels sit on a threshold, the reference arithmetic stays finite, and what the reference's own fp32 arithmetic
loses on the SSIM cases) and tests/test_gpu_image_edges.py (csrc/epilogue.hip and csrc/loss.hip against the fp64 oracle).

Every case is a seeded builder that returns fp32 arrays; nothing is read from a file.

Unpack cases (svgss train / eval, rgss).  GROUPS restates the plane layout of oracle/epilogue_oracle.py::unpack_svgss as a table (result
name, kind, source tensor, first source channel, channels); `probe` returns, per srgb evaluation, the argument of the knee compare and
the argument of the final clip (the unclipped sRGB value); the host test ties it to the oracle (the outputs rebuilt from the probe
equal the oracle's).

Threshold pixels.  An argument x of the sRGB knee compare (bound b = float32(0.0031308)) or of the 0 / 1 clip (b = 0, b = 1) is "on" its
bound when 0 < |x - b| <= 1e-4 max(|b|, 1e-1) in the fp64 oracle: fp32 may legitimately land on the other side.  An exact tie is NOT a
threshold: both precisions compute it exactly (the inputs are fp32 values; the knee is rounded to fp32 where the reference rounds
it).  A pixel with such an argument in any of its planes is a threshold pixel: it is held to finiteness only, and only in the
gradients (the values are continuous across every bound and stay compared); it gets zero upstream weight; a case may hold at most
MAX_THRESHOLD_SHARE of them.  The opacity against float32(1e-5) is never a threshold: the opacity is an input, exact in both precisions.

depth2normal cases.  Degenerate pixels (the summed cross product is EXACTLY zero under a non-zero mask: 1 / eps = 1e12 times rounding
noise in the adjoint, in the reference's autograd as in the kernel) and their 4-neighbours are excluded from the gradient comparison;
a run that checks gradients holds at most MAX_DEGENERATE_SHARE of excluded pixels.

SSIM cases.  E32 = |fp32 restatement - fp64 restatement| of oracle/epilogue_oracle.py::l1_ssim_torch, in the SSIM value and in its
gradient over max |gradient|: what the reference's own fp32 arithmetic loses.  SSIM_CEILING records it per content (asserted by the
host test); the GPU test allows max(existing tolerance, 4 x the run's E32).
"""
import numpy as np
import torch

from oracle import epilogue_oracle as eo

MAX_THRESHOLD_SHARE = 0.05
MAX_DEGENERATE_SHARE = 0.15
REL, REL_FLOOR = 1e-4, 1e-1
F32 = np.float32
OPMIN = F32(1e-5)
KNEE = F32(0.0031308)
BLOCK = 256                                     # threads per workgroup of the unpack / depth2normal kernels
UNPACK_SIZES = ((1, 1), (1, 257), (37, 29), (16, 16))   # one pixel; a workgroup + 1; 4 workgroups + 49 pixels; exactly one workgroup
BACKGROUNDS = {"black": (0.0, 0.0, 0.0), "white": (1.0, 1.0, 1.0), "colour": (0.2, 0.5, 0.9)}
PLANES = {"train": (4, 13), "eval": (7, 16)}    # (feature planes S, vfeature planes VS / 4)
SRGB_OF_OVER, PLAIN, OVER_SRGB, OVER_LIN, SRGB = "srgb_of_over", "plain", "over_srgb", "over_lin", "srgb"
GROUPS = {
    "train": (("pbr", SRGB_OF_OVER, "vfeature", 0, 3), ("normal", PLAIN, "vfeature", 6, 3), ("base_color", OVER_SRGB, "vfeature", 3, 3),
              ("roughness", OVER_LIN, "vfeature", 9, 1), ("diffuse", OVER_SRGB, "vfeature", 10, 3),
              ("local_lights", OVER_SRGB, "feature", 1, 3), ("visibility", OVER_LIN, "feature", 0, 1)),
    "eval": (("pbr", SRGB_OF_OVER, "vfeature", 0, 3), ("normal", PLAIN, "vfeature", 6, 3), ("base_color", OVER_SRGB, "vfeature", 3, 3),
             ("roughness", OVER_LIN, "vfeature", 9, 1), ("direct", SRGB, "vfeature", 10, 3), ("indirect", SRGB, "vfeature", 13, 3),
             ("lights", OVER_SRGB, "feature", 0, 3), ("local_lights", OVER_SRGB, "feature", 3, 3), ("visibility", OVER_LIN, "feature", 6, 1)),
}
RGSS_KEYS = ("feature_normal", "feature_depth", "depth_var")      # what svgir_harness.render_view.unpack_rgss exposes

# opacity_ends: 0, a clamped value, the three fp32 values around the clamp, a value just released, 0.5, the last value below 1, 1
# (pixel j of the scattered order takes OPACITY_ENDS[j % 9]: the 1 x 1 image is the tie)
OPACITY_ENDS = (OPMIN, F32(0), F32(1), np.nextafter(OPMIN, F32(0)), np.nextafter(OPMIN, F32(1)), F32(5e-6), F32(2e-5), F32(0.5),
                F32(1) - F32(2.0 ** -24))
NUM_CONTRIB = (1, 0, 7)
# srgb_knee_and_clips: values of x = plane / opacity that are NOT on a bound by the rule above (the knee itself is the exact tie) ...
LADDER_SAFE = (F32(-0.5), F32(0), F32(0.001), KNEE, F32(0.5), F32(4))
# ... and the ones that are: the fp32 neighbours of the knee, and of 1 (sRGB(1) = 1: the largest x whose sRGB is below 1 is the fp32
# value below 1; the unclipped sRGB of 1 itself is 1 - 1 ulp in fp64 and in fp32, within the window of the bound 1)
LADDER_THRESHOLD = (np.nextafter(KNEE, F32(0)), np.nextafter(KNEE, F32(1)), np.nextafter(F32(1), F32(0)), F32(1), np.nextafter(F32(1), F32(2)))
KNEE_OPACITIES = (F32(1), F32(0.5), F32(0.25))   # powers of two: x = raw * (1 / o) is exact in both precisions


def _runs_unpack():
    out = []
    for mode in ("train", "eval", "rgss"):
        for (H, W) in UNPACK_SIZES:
            out.append(dict(id=f"{mode}-opacity_ends-{H}x{W}", mode=mode, case="opacity_ends", H=H, W=W, bg="colour"))
            if H * W > 1:     # (5 % of one pixel is no pixel)
                out.append(dict(id=f"{mode}-nonfinite-{H}x{W}", mode=mode, case="nonfinite", H=H, W=W, bg="colour"))
            if mode != "rgss":
                for bg in BACKGROUNDS:
                    out.append(dict(id=f"{mode}-srgb_knee_and_clips-{bg}-{H}x{W}", mode=mode, case="srgb_knee_and_clips", H=H, W=W, bg=bg))
    return out


UNPACK_RUNS = _runs_unpack()


def _rng(run_id):
    return np.random.default_rng(sum((i + 1) * b for i, b in enumerate(run_id.encode())))


def srgb_unclipped(a):
    return eo.rgb_to_srgb(a, clip=False)


def probe(d, mode, bg):
    """{result name: dict(kind, x, arg, y)} from the fp64 oracle's arithmetic: x = plane / max(opacity, float32(1e-5)), arg = the argument
    of the knee compare (None without an sRGB), y = the argument of the clip to [0, 1] (the unclipped sRGB value)."""
    op = d["opacity"].astype(np.float64)
    den = np.maximum(op, float(OPMIN))
    bgc = np.asarray(bg, dtype=np.float64)[:, None, None]
    out = {}
    with np.errstate(invalid="ignore"):
        for name, kind, src, c0, n in GROUPS[mode]:
            x = d[src][c0:c0 + n].astype(np.float64) / den
            arg = x * op + (1 - op) * bgc if kind == SRGB_OF_OVER else (x if kind in (OVER_SRGB, SRGB) else None)
            out[name] = dict(kind=kind, x=x, arg=arg, y=None if arg is None else srgb_unclipped(arg))
    return out


def rebuild(p, d, bg):
    """The oracle's outputs from a probe (ties `probe` to oracle/epilogue_oracle.py::unpack_svgss)."""
    op = d["opacity"].astype(np.float64)
    bgc = np.asarray(bg, dtype=np.float64)[:, None, None]
    out = {}
    with np.errstate(invalid="ignore"):
        for name, q in p.items():
            s = None if q["y"] is None else np.clip(q["y"], 0.0, 1.0)
            out[name] = {SRGB_OF_OVER: s, PLAIN: q["x"], OVER_SRGB: None if s is None else s * op + (1 - op) * bgc,
                         OVER_LIN: q["x"] * op + (1 - op) * bgc, SRGB: s}[q["kind"]]
    return out


def near(x, b):
    """The threshold rule of the module docstring."""
    with np.errstate(invalid="ignore"):
        dist = np.abs(x - b)
        return (dist > 0) & (dist <= REL * max(abs(b), REL_FLOOR))


def threshold_pixels(p):
    """bool [H,W]: pixels with an argument of the knee compare or of the 0 / 1 clip on its bound, in any plane."""
    t = None
    for q in p.values():
        if q["arg"] is None:
            continue
        m = (near(q["arg"], float(KNEE)) | near(q["y"], 0.0) | near(q["y"], 1.0)).any(0)
        t = m if t is None else t | m
    return t


def nonfinite_pixels(d):
    """bool [H,W]: pixels with a non-finite value in any input plane."""
    bad = np.zeros(d["opacity"].shape[-2:], dtype=bool)
    for k in ("opacity", "feature", "vfeature", "depth"):
        if k in d:
            bad |= ~np.isfinite(d[k]).all(0)
    return bad


def _order(rng, N):
    """A scattered order of the pixels, pixel 0 first (so the 1 x 1 image takes the first recipe)."""
    return np.concatenate([[0], 1 + rng.permutation(N - 1)]).astype(np.int64)


def _raw(x, op):
    """The rasterizer's plane for a wanted x = plane / max(opacity, 1e-5): fp32 product (exact for a power-of-two opacity)."""
    return (x.astype(F32) * np.maximum(op, OPMIN)).astype(F32)


def build_unpack(run):
    """fp32 inputs of an UNPACK_RUNS entry: dict(opacity [1,H,W], feature, vfeature) -- rgss: dict(num_contrib [H,W] int32, opacity,
    depth [1,H,W], feature [5,H,W]) -- plus `special` [H,W] bool for `nonfinite` (the poisoned pixels)."""
    H, W, mode, case = run["H"], run["W"], run["mode"], run["case"]
    N = H * W
    rng = _rng(run["id"])
    order = _order(rng, N)
    S, VC = (5, 0) if mode == "rgss" else PLANES[mode]
    C = S + VC
    j = np.empty(N, dtype=np.int64)
    j[order] = np.arange(N)                                   # pixel -> its place in the scattered order
    x = rng.uniform(0.2, 0.95, size=(C, N))
    if mode == "rgss":
        x[0:3] = rng.uniform(-1, 1, size=(3, N))
        x[3] = rng.uniform(1, 5, size=N)
        x[4] = x[3] ** 2 + rng.uniform(0, 0.3, size=N)
    else:
        x[S + 6:S + 9] = rng.uniform(-1, 1, size=(3, N))      # the normal planes
    special = np.zeros(N, dtype=bool)
    if case == "opacity_ends":
        op = np.asarray(OPACITY_ENDS, dtype=F32)[j % 9]
        raw = _raw(x, op[None])
        zero_raw = (op == 0) & ((j // 9) % 2 == 0)            # o = 0: every other such pixel is the empty pixel, raw = 0 too
        raw[:, zero_raw] = 0
    elif case == "srgb_knee_and_clips":
        n_thr = int(0.04 * N)
        x = rng.uniform(0.01, 0.9, size=(C, N))
        op = np.asarray(KNEE_OPACITIES, dtype=F32)[j % 3]
        c = np.arange(C)[:, None]
        ladder = (j % 2 == 0) & (j >= n_thr)                  # every other ordinary pixel takes the ladder, one step per channel
        safe = np.asarray(LADDER_SAFE, dtype=np.float64)[(j[None] // 6 + c) % len(LADDER_SAFE)]
        x = np.where(ladder[None], safe, x)
        thr = j < n_thr                                       # the first pixels of the order: the values on a bound, at opacity 1
        x = np.where(thr[None], np.asarray(LADDER_THRESHOLD, dtype=np.float64)[(j[None] + c) % len(LADDER_THRESHOLD)], x)
        op = np.where(thr, F32(1), op).astype(F32)
        raw = _raw(x, op[None])
        # an ordinary pixel whose over() argument lands on a bound by coincidence (4 * 0.25 + 0.75 * 0 = 1) is re-drawn off the ladder
        d0 = dict(opacity=op.reshape(1, H, W), feature=raw[:S].reshape(S, H, W), vfeature=raw[S:].reshape(VC, H, W))
        hit = threshold_pixels(probe(d0, mode, BACKGROUNDS[run["bg"]])).reshape(N) & ~thr
        raw[:, hit] = _raw(rng.uniform(0.01, 0.9, size=(C, int(hit.sum()))), op[None, hit])
    elif case == "nonfinite":
        op = rng.uniform(0.1, 1.0, size=N).astype(F32)
        raw = _raw(x, op[None])
        n_bad = int(0.05 * N)
        special = j < n_bad
        vals = (F32("nan"), F32("inf"), F32("-inf"))
        for px in np.nonzero(special)[0]:
            t = int(j[px]) % 7
            if t == 6:
                op[px] = F32("nan")
            elif mode == "rgss":
                raw[(0, 3, 4)[int(j[px]) % 3], px] = vals[t % 3]
            elif t < 3:
                raw[1, px] = vals[t]
            else:
                raw[S + (0, 6, 9, 10)[int(j[px] // 7) % 4], px] = vals[t - 3]
    else:
        raise KeyError(case)
    if mode == "rgss":
        nc = np.asarray(NUM_CONTRIB, dtype=np.int32)[(j // 9) % 3] if case == "opacity_ends" else np.asarray(NUM_CONTRIB, dtype=np.int32)[j % 3]
        depth = rng.uniform(1, 5, size=N).astype(F32)
        return dict(num_contrib=nc.reshape(H, W), opacity=op.reshape(1, H, W), depth=depth.reshape(1, H, W),
                    feature=raw.reshape(5, H, W), special=special.reshape(H, W))
    return dict(opacity=op.reshape(1, H, W), feature=raw[:S].reshape(S, H, W), vfeature=raw[S:].reshape(VC, H, W),
                special=special.reshape(H, W))


def unpack_weights(run, shapes, keep):
    """Random fp64 upstream weights {result name: [n,H,W]}, zero outside `keep` [H,W]."""
    g = torch.Generator().manual_seed(len(run["id"]) + 17)
    return {k: torch.randn(shapes[k], generator=g, dtype=torch.float64) * torch.from_numpy(keep)[None] for k in shapes}


# ---- depth2normal ------------------------------------------------------------------------------------------------------------------
FOVX, FOVY = 0.9, 0.6
PRCP = ((0.5, 0.5), (0.37, 0.61))
D2N_SIZES = ((1, 1), (1, 19), (23, 1), (37, 29))
MASKS = ("ones", "zeros", "disc", "isolated", "border_holes", "checker")


def _runs_d2n():
    out = []

    def add(H, W, depth, mask, prcp=0, grad=True):
        out.append(dict(id=f"{H}x{W}-{depth}-{mask}-pp{prcp}", H=H, W=W, depth=depth, mask=mask, prcp=PRCP[prcp], grad=grad))

    for H, W in D2N_SIZES[:3]:                      # one pixel, one row, one column: every summed cross product is exactly zero
        add(H, W, "plane1", "ones", 0)
        add(H, W, "plane1", "zeros", 1)
        add(H, W, "holes", "ones", 1)
    H, W = D2N_SIZES[3]
    for i, mk in enumerate(MASKS):
        add(H, W, "plane1", mk, i % 2, grad=(mk != "checker"))   # the checkerboard leaves no pixel outside the excluded ones: forward only
    for depth in ("plane1e-3", "plane1e4"):
        add(H, W, depth, "ones", 1)
        add(H, W, depth, "disc", 0)
    for mk in ("ones", "disc", "border_holes"):
        add(H, W, "holes", mk, 1)
    return out


D2N_RUNS = _runs_d2n()


def build_d2n(run):
    """(depth [1,H,W] fp32, mask [1,H,W] fp32 of 0 / 1) of a D2N_RUNS entry."""
    H, W = run["H"], run["W"]
    rng = _rng(run["id"])
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = 2.0 + 0.021 * xs - 0.013 * ys + 0.002 * rng.standard_normal((H, W))       # a tilted, slightly rough plane
    if run["depth"].startswith("plane"):
        depth = depth * float(run["depth"][5:])
    else:                                            # depth-0 holes, as a render with empty pixels produces
        hole = np.zeros((H, W), dtype=bool)
        hole[H // 3:H // 3 + 3, W // 4:W // 4 + 4] = True
        hole[(2 * H) // 3, (2 * W) // 3] = True
        hole[0, W - 1] = True
        depth[hole] = 0.0
    m = np.ones((H, W), dtype=bool)
    mk = run["mask"]
    if mk == "zeros":
        m[:] = False
    elif mk == "disc":
        m = (ys - 0.45 * H) ** 2 + (xs - 0.55 * W) ** 2 <= (0.42 * min(H, W)) ** 2
    elif mk == "isolated":
        m[rng.integers(1, max(H - 1, 2), size=6) % H, rng.integers(1, max(W - 1, 2), size=6) % W] = False
    elif mk == "border_holes":                       # a hole on each border, in two corners, and beside the two other corners
        m[0, W // 2] = m[H - 1, W // 3] = m[H // 2, 0] = m[H // 3, W - 1] = False
        m[0, 0] = m[H - 1, W - 1] = False
        m[0, W - 2] = m[H - 2, 0] = False            # (the corner pixel next to it keeps no difference: an excluded degenerate pixel)
    elif mk == "checker":
        m = (ys + xs) % 2 == 0
    return depth.astype(F32)[None], m.astype(F32)[None]


def d2n_excluded(normal, mask):
    """(degenerate, excluded) bool [H,W]: the summed cross product is exactly zero under a non-zero mask; plus the 4-neighbours."""
    deg = (np.abs(np.asarray(normal)).sum(0) == 0) & (np.asarray(mask)[0] != 0)
    t = deg.copy()
    t[1:] |= deg[:-1]; t[:-1] |= deg[1:]; t[:, 1:] |= deg[:, :-1]; t[:, :-1] |= deg[:, 1:]
    return deg, t


def d2n_upstream(run):
    return torch.randn(3, run["H"], run["W"], generator=torch.Generator().manual_seed(run["H"] * 131 + run["W"]), dtype=torch.float64)


def d2n_reference(run):
    """(depth, mask, fp64 normal, fp64 depth gradient under d2n_upstream, excluded [H,W]) of a run."""
    depth, mask = build_d2n(run)
    d = torch.from_numpy(depth).double().requires_grad_(True)
    n = eo.depth2normal_torch(d, torch.from_numpy(mask), FOVX, FOVY, run["prcp"])
    (n * d2n_upstream(run)).sum().backward()
    n = n.detach().numpy()
    return depth, mask, n, d.grad.numpy(), d2n_excluded(n, mask)[1]


# ---- L1 + SSIM ---------------------------------------------------------------------------------------------------------------------
SSIM_SHAPES = ((3, 1, 1), (3, 5, 7), (3, 10, 11), (1, 15, 17), (3, 16, 16), (3, 17, 33), (2, 31, 32), (3, 150, 161))
SSIM_CONTENTS = ("rand", "flat", "sat", "equal", "nan")
UPSTREAMS = ((1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (-2.5, 0.3))       # (g_l1, g_ssim)
LAMBDAS = (0.0, 0.2, 1.0)
# E32 ceilings (value, gradient / max |gradient|) per content, over the table's shapes: the host test measures E32 and asserts it below
# these; DESIGN.md section 5 holds the measured figures.
SSIM_CEILING = {"rand": (4e-7, 1.2e-5), "equal": (4e-7, 1.2e-5), "flat": (8e-5, 7e-4), "sat": (1.5e-5, 1.5e-4)}


def _runs_ssim():
    out = [dict(id=f"rand-{C}x{H}x{W}", content="rand", C=C, H=H, W=W) for C, H, W in SSIM_SHAPES]
    for content in SSIM_CONTENTS[1:]:
        for C, H, W in ((1, 15, 17), (3, 17, 33)):
            out.append(dict(id=f"{content}-{C}x{H}x{W}", content=content, C=C, H=H, W=W))
    out.append(dict(id="flat-3x5x7", content="flat", C=3, H=5, W=7))
    out.append(dict(id="sat-2x31x32", content="sat", C=2, H=31, W=32))
    return out


SSIM_RUNS = _runs_ssim()


def partials(run):
    return run["C"] * ((run["H"] + 15) // 16) * ((run["W"] + 15) // 16)


def build_ssim(run):
    """(img, gt) fp32 [C,H,W] in [0, 1] of an SSIM_RUNS entry."""
    C, H, W = run["C"], run["H"], run["W"]
    g = torch.Generator().manual_seed(1000 * C + 10 * H + W)
    content = run["content"]
    if content in ("rand", "equal", "nan"):          # built like the recorded fixtures: a flat top third, Gaussian noise, clamped
        gt = torch.rand(C, H, W, generator=g)
        gt[:, : H // 3] = 0.25
        img = (gt + 0.15 * torch.randn(C, H, W, generator=g)).clamp(0, 1)
        if content == "equal":                       # equal on half the pixels: sign(0) = 0 in the L1 gradient
            same = torch.rand(H, W, generator=g) < 0.5
            img = torch.where(same[None], gt, img)
        if content == "nan":
            img[C - 1, H // 2, W // 3] = float("nan")
    elif content == "flat":                          # constant ground truth, two-level image: every window is flat or a single step
        gt = torch.full((C, H, W), 0.7)
        img = torch.full((C, H, W), 0.7)
        img[:, :, W // 2:] = 0.7 + 1.0 / 256
    elif content == "sat":                           # halves at exactly 0 and 1, noise on part of the image
        gt = torch.zeros(C, H, W)
        gt[:, H // 2:] = 1.0
        img = gt.clone()
        noisy = slice(W // 3, (2 * W) // 3)
        img[:, :, noisy] = (img[:, :, noisy] + 0.1 * torch.randn(C, H, len(range(W)[noisy]), generator=g)).clamp(0, 1)
    else:
        raise KeyError(content)
    return img.float().contiguous(), gt.float().contiguous()


def ssim_reference(run, dtype=torch.float64):
    """dict(l1, ssim, d_l1, d_ssim) of oracle/epilogue_oracle.py::l1_ssim_torch in `dtype` (fp32: the reference's own arithmetic)."""
    img, gt = build_ssim(run)
    a = img.to(dtype).requires_grad_(True)
    l1, s = eo.l1_ssim_torch(a, gt.to(dtype), keep_dtype=dtype != torch.float64)
    gs, = torch.autograd.grad(s, a, retain_graph=True)
    gl, = torch.autograd.grad(l1, a)
    return dict(l1=float(l1.detach()), ssim=float(s.detach()), d_l1=gl.double().numpy(), d_ssim=gs.double().numpy())


def ssim_e32(r64, r32):
    """(E32 of the SSIM value, E32 of its gradient over max |gradient|, the same two for L1)."""
    gm = max(np.abs(r64["d_ssim"]).max(), 1e-300)
    lm = max(np.abs(r64["d_l1"]).max(), 1e-300)
    return (abs(r32["ssim"] - r64["ssim"]), float(np.abs(r32["d_ssim"] - r64["d_ssim"]).max() / gm),
            abs(r32["l1"] - r64["l1"]), float(np.abs(r32["d_l1"] - r64["d_l1"]).max() / lm))
