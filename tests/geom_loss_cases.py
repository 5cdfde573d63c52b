"""The case table of the geometry-loss tests and its oracle: tests/test_geom_loss_edge_inputs.py (the fp64 oracle alone, against the recorded
reference results of tests/golden/geom_losses.npz) and tests/test_gpu_geom_loss.py (csrc/geom_loss.hip against the fp64 oracle).

The oracle is torch on top of oracle/epilogue_oracle.py::depth2normal_torch, in fp64; the same functions in fp32 are the restatement of the
reference's own arithmetic, so that E32 = |fp32 - fp64| of every loss is known per case (the GPU test allows 4 x E32 on the kernels'
sum / count in double, and holds the returned fp32 number to the exact rounding of that).

cos_loss (utils/loss_utils.py:119-121): cos = sum_c (output_c * gt_c) * weight, selected iff cos < 1, loss = sum_selected (1 - cos) / count.
The kernels' contract deviates from torch's autograd in one point, restated here: a pixel that is not selected gets ZERO gradient even when its
cos is NaN (torch: 0 * NaN) -- the oracle zeroes the unselected pixels' inputs before it multiplies.

Threshold pixels (surface form): the fp64 cos lies within 1e-5 of 1 without being exactly 1; the kernel's fp32 pseudo normal may put such a
pixel on either side of the compare.  `sure` = the selected pixels that are not threshold pixels: sure <= kernel count <= sure + threshold.
A case holds at most MAX_THRESHOLD_SHARE of them (rendered normal = normalize(d2n + 0.05 N(0, 1)): 0 ... 0.56 % over every 37 x 29 run of the
depth2normal table).  The `equal` case (rendered normal == the fp32 pseudo normal) is ill-conditioned on purpose: about half of its pixels
land on either side; only its count bounds and finiteness are checked.

Every case is a seeded builder that returns fp32 arrays; nothing is read from a file.
"""
import numpy as np
import torch

import image_cases as ic
from oracle import epilogue_oracle as eo

F32 = np.float32
MAX_THRESHOLD_SHARE = 0.02
MAX_DEGENERATE_SHARE = ic.MAX_DEGENERATE_SHARE                # 0.15, the depth2normal table's
THRESHOLD = 1e-5
ENT_LO, ENT_HI = float(F32(1e-6)), float(F32(1 - 1e-6))     # the reference clamps an fp32 tensor: the bounds are rounded to fp32
TILE = (8, 32)                                              # rows, columns of a workgroup's tile (csrc/geom_loss.hip)
SIZES = ((1, 1), (1, 19), (23, 1), (5, 7), (16, 16), (17, 33), (37, 29), (150, 161))
NOISE = 0.05


def _runs():
    out = []

    def add(H, W, depth="plane1", mask="ones", prcp=0, normal="noisy", opacity="rand", grad=True):
        out.append(dict(id=f"{H}x{W}-{depth}-{mask}-pp{prcp}-{normal}-{opacity}", H=H, W=W, depth=depth, mask=mask, prcp=ic.PRCP[prcp],
                        normal=normal, opacity=opacity, grad=grad))

    for H, W in SIZES[:3]:                          # one pixel, one row, one column: every pseudo normal is zero, every pixel selected
        add(H, W, "plane1", "ones", 0)
        add(H, W, "holes", "zeros", 1, opacity="ends")
    add(5, 7, "plane1", "ones", 1)                  # smaller than the 9 x 9 window
    add(5, 7, "plane1", "disc", 0, opacity="ends")
    add(16, 16, "plane1", "ones", 0)
    add(16, 16, "holes", "border_holes", 1)
    add(17, 33, "plane1", "tile_edges", 0)          # one column in the second tile
    add(17, 33, "holes", "disc", 1, opacity="ends")
    for i, mk in enumerate(ic.MASKS):               # every mask of the depth2normal table, several workgroups, both halos
        add(37, 29, "plane1", mk, i % 2, grad=(mk != "checker"))
    add(37, 29, "plane1", "tile_edges", 1)
    add(37, 29, "holes", "disc", 1, opacity="ends")
    add(37, 29, "holes", "ones", 0)
    for depth in ("plane1e-3", "plane1e4"):
        add(37, 29, depth, "disc", 0)
    add(37, 29, "plane1", "ones", 1, normal="equal", grad=False)      # the ill-conditioned case
    add(37, 29, "plane1", "disc", 0, opacity="nan", grad=False)       # a NaN opacity: the two opacity terms are NaN
    add(150, 161, "plane1", "tile_edges", 1)        # 19 x 6 workgroups: the multi-partial reduction
    return out


RUNS = _runs()
FUSED_RUNS = [r for r in RUNS if r["id"] in ("37x29-plane1-disc-pp0-noisy-rand", "17x33-plane1-tile_edges-pp0-noisy-rand", "1x1-plane1-ones-pp0-noisy-rand",
                                             "150x161-plane1-tile_edges-pp1-noisy-rand")]


def build_mask(run):
    """(depth, mask) [1,H,W] fp32: image_cases.build_d2n, plus the `tile_edges` mask (edges within 4 pixels of the image border and of the
    tile edges at multiples of 8 rows / 32 columns)."""
    H, W = run["H"], run["W"]
    if run["mask"] != "tile_edges":
        return ic.build_d2n(run)
    depth, _ = ic.build_d2n(dict(run, mask="ones"))
    m = np.zeros((H, W), dtype=bool)
    m[2:H - 3, 3:W - 1] = True                      # 2 / 3 pixels off the top / bottom border, 3 / 1 off the left / right one
    for y in range(8, H, 16):
        m[y - 1:y + 2, :] = False                   # a band across a row-tile edge
    for x in range(32, W, 64):
        m[:, x - 2:x + 1] = False                   # a band across a column-tile edge
    for y in range(4, H - 10, 32):
        m[y:y + 11, :] = False                      # 11 rows: the 9 x 9 pool leaves three rows of zeros, across a row-tile edge
    for x in range(17, W - 10, 64):
        m[:, x:x + 11] = False                      # 11 columns ending four pixels in front of a column-tile edge
    m[H // 2, W // 2] = False
    return depth, m.astype(F32)[None]


def build(run):
    """fp32 inputs of a RUNS entry: dict(normal [3,H,W], depth, mask, opacity [1,H,W])."""
    H, W = run["H"], run["W"]
    rng = ic._rng("geom-" + run["id"])
    depth, mask = build_mask(run)
    n32 = eo.depth2normal_torch(torch.from_numpy(depth), torch.from_numpy(mask), ic.FOVX, ic.FOVY, run["prcp"]).numpy()
    if run["normal"] == "equal":
        normal = n32.copy()
    else:
        v = n32.astype(np.float64) + NOISE * rng.standard_normal((3, H, W))
        normal = (v / np.maximum(np.linalg.norm(v, axis=0, keepdims=True), 1e-12)).astype(F32)
    op = rng.uniform(0.02, 0.98, size=(H, W)).astype(F32)
    if run["opacity"] == "ends":                    # on, below and above both bounds, 0 and 1
        ends = np.array([ENT_LO, ENT_HI, np.nextafter(F32(ENT_LO), F32(0)), np.nextafter(F32(ENT_HI), F32(1)), np.nextafter(F32(ENT_LO), F32(1)),
                         np.nextafter(F32(ENT_HI), F32(0)), 0.0, 1.0, 5e-7], dtype=F32)
        j = ic._order(rng, H * W).argsort()
        special = j % 3 == 0
        op = np.where(special.reshape(H, W), ends[(j // 3) % len(ends)].reshape(H, W), op).astype(F32)
    elif run["opacity"] == "nan":
        op[H // 2, W // 3] = np.nan
    return dict(normal=normal, depth=depth, mask=mask, opacity=op[None])


# ---- the oracle --------------------------------------------------------------------------------------------------------------------
def cos_map(output, gt, weight=None):
    """cos [H,W] in the kernels' order ((o0 g0) w + (o1 g1) w) + (o2 g2) w (what torch.sum(output * gt * weight, 0) evaluates)."""
    p = output * gt
    if weight is not None:
        p = p * weight
    return (p[0] + p[1]) + p[2]


def cos_loss_torch(output, gt, weight=None, count=None):
    """(loss, count, selected [H,W]) of cos_loss in the dtype of `output`; count=None: the number of selected pixels, else the given count
    divides (the GPU test passes the kernel's own, so that 1 / count is not charged to threshold pixels).  Unselected pixels get zero
    gradient (see the module docstring)."""
    with torch.no_grad():
        sel = cos_map(output, gt, weight) < 1
    zero = torch.zeros((), dtype=output.dtype)
    cos = cos_map(torch.where(sel[None], output, zero), torch.where(sel[None], gt, zero),
                  None if weight is None else torch.where(sel[None], weight.reshape(1, *sel.shape), zero))
    n = int(sel.sum())
    total = torch.where(sel, 1 - cos, zero).sum()
    return total / (n if count is None else count), n, sel


def surface_torch(normal, depth, mask, prcp, count=None, fovx=ic.FOVX, fovy=ic.FOVY):
    d2n = eo.depth2normal_torch(depth, mask, fovx, fovy, prcp)
    loss, n, sel = cos_loss_torch(normal, d2n, None, count)
    return loss, n, sel, d2n


def pool9(mask):
    return torch.nn.functional.max_pool2d(mask[None], 9, stride=1, padding=4)[0]


def mask_torch(opacity, mask):
    return (opacity * (1 - pool9(mask))).mean()


def entropy_torch(opacity, mask, lo=ENT_LO, hi=ENT_HI):
    o = opacity.clamp(lo, hi)
    return -(mask * torch.log(o) + (1 - mask) * torch.log(1 - o)).mean()


def reference(run, dtype=torch.float64, count=None):
    """The oracle on a run in `dtype` (fp32: the reference's own arithmetic): dict(surface, mask, entropy -- floats --, count, sel [H,W],
    cos [H,W], d2n [3,H,W], d_normal, d_depth, d_opacity_mask, d_opacity_entropy -- fp64 arrays, the gradients of the three losses)."""
    d = build(run)
    t = {k: torch.from_numpy(v).to(dtype) for k, v in d.items()}
    normal, depth, op = t["normal"].requires_grad_(True), t["depth"].requires_grad_(True), t["opacity"].requires_grad_(True)
    loss, n, sel, d2n = surface_torch(normal, depth, t["mask"], run["prcp"], count)
    gn, gd = torch.autograd.grad(loss, (normal, depth), allow_unused=True)
    lm = mask_torch(op, t["mask"])
    le = entropy_torch(op, t["mask"])
    gm, = torch.autograd.grad(lm, op)
    ge, = torch.autograd.grad(le, op)
    z = lambda g, like: (torch.zeros_like(like) if g is None else g).double().numpy()   # noqa: E731
    with torch.no_grad():
        cos = cos_map(normal, d2n)
    return dict(surface=float(loss.detach()), mask=float(lm.detach()), entropy=float(le.detach()), count=n, sel=sel.numpy(),
                cos=cos.double().numpy(), d2n=d2n.detach().double().numpy(), d_normal=z(gn, normal), d_depth=z(gd, depth),
                d_opacity_mask=gm.double().numpy(), d_opacity_entropy=ge.double().numpy())


def threshold_pixels(cos64):
    """bool [H,W]: the fp64 cos is within THRESHOLD of 1 without being exactly 1."""
    with np.errstate(invalid="ignore"):
        dist = np.abs(cos64 - 1.0)
        return (dist > 0) & (dist <= THRESHOLD)


def grow(t):
    """t and its 4-neighbours."""
    g = t.copy()
    g[1:] |= t[:-1]; g[:-1] |= t[1:]; g[:, 1:] |= t[:, :-1]; g[:, :-1] |= t[:, 1:]
    return g


# ---- the target form: exact cases ------------------------------------------------------------------------------------------------
TARGET_RUNS = ("unit_z", "zeros", "nan_pixel", "empty", "weights01", "weight_fractions", "random-1x1", "random-37x29", "random-17x33", "random-150x161")


def build_target(name):
    """dict(output, gt [3,H,W], weight [1,H,W] or None) fp32 of a TARGET_RUNS entry."""
    H, W = (37, 29)
    if name.startswith("random-"):
        H, W = (int(v) for v in name[7:].split("x"))
    rng = ic._rng("target-" + name)

    def unit(n=1.0):
        v = rng.standard_normal((3, H, W))
        return (n * v / np.linalg.norm(v, axis=0, keepdims=True)).astype(F32)

    z = np.zeros((3, H, W), dtype=F32)
    ez = z.copy()
    ez[2] = 1
    if name == "unit_z":            # output = gt = (0, 0, 1) on the lower half: cos == 1 exactly, not selected; random above
        out, gt = unit(), unit()
        out[:, H // 2:], gt[:, H // 2:] = ez[:, H // 2:], ez[:, H // 2:]
        return dict(output=out, gt=gt, weight=None)
    if name == "zeros":             # all selected, loss 1
        return dict(output=z, gt=z.copy(), weight=None)
    if name == "nan_pixel":
        out, gt = unit(), unit()
        out[1, 3, 5] = np.nan
        gt[0, H - 1, W - 1] = np.nan
        return dict(output=out, gt=gt, weight=None)
    if name == "empty":             # cos = 1 (exact) or 4 everywhere: nothing selected, NaN loss, zero gradients
        out, gt = ez.copy(), ez.copy()
        out[2, ::2] = 2; gt[2, ::2] = 2
        return dict(output=out, gt=gt, weight=None)
    if name == "weights01":
        return dict(output=unit(), gt=unit(), weight=(rng.uniform(size=(1, H, W)) < 0.6).astype(F32))
    if name == "weight_fractions":  # weights up to 3: part of the pixels reach cos >= 1
        return dict(output=unit(), gt=unit(1.2), weight=rng.uniform(0, 3, size=(1, H, W)).astype(F32))
    return dict(output=unit(), gt=unit(), weight=rng.uniform(0.25, 1.5, size=(1, H, W)).astype(F32) if H * W > 1 else None)


def target_reference(name, dtype=torch.float64):
    """dict(loss, count, sel, d_output) of the oracle on a TARGET_RUNS entry in `dtype`."""
    d = build_target(name)
    out = torch.from_numpy(d["output"]).to(dtype).requires_grad_(True)
    gt = torch.from_numpy(d["gt"]).to(dtype)
    w = None if d["weight"] is None else torch.from_numpy(d["weight"]).to(dtype)
    loss, n, sel = cos_loss_torch(out, gt, w)
    g = torch.autograd.grad(loss, out)[0].double().numpy() if n else np.zeros(out.shape)
    return dict(loss=float(loss.detach()), count=n, sel=sel.numpy(), d_output=g)
