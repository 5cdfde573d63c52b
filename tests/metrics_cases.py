"""The edge-case table of the eval view's tail (csrc/view_metrics.hip, svgir_harness/metrics.py) and its oracle, shared by
tests/test_metrics_edge_inputs.py (CPU: proves the table, pins the oracle by tests/golden/view_metrics.npz, measures E32 / E_SRGB) and
tests/test_gpu_view_metrics.py (the kernels against it).

The oracle forms every operand in fp32 in torch's operation order (the reference's planes are fp32 data: that is what it holds), then
evaluates the metrics
  * in fp64 (SSIM through oracle/epilogue_oracle.l1_ssim_torch; an sRGB operand through the fp64 rgb_to_srgb of the same fp32 argument),
  * in the reference's fp32 order (utils/image_utils.py:32-37, the fp32 stand-in of l1_ssim_torch; sRGB in fp32 as utils/graphics_utils.py
    writes it),
and E32 per column = what the reference's own fp32 arithmetic loses on the case, E_SRGB = max |srgb32 - srgb64| over the case.
Nothing here looks at a kernel's result."""
import functools
import zlib

import numpy as np
import torch

from oracle import epilogue_oracle as eo

F32 = np.float32
EPS32 = 2.0 ** -23
COLS = 10
KNEE = F32(0.0031308)
SIZES = ((1, 1), (5, 7), (16, 16), (17, 33), (31, 32), (150, 161))   # (H, W): one pixel; below a tile; one tile; tile + 1 / 2 tiles + 1; a partial tile row; 10 x 11 tiles
BACKGROUNDS = {"black": (0.0, 0.0, 0.0), "white": (1.0, 1.0, 1.0), "colour": (0.2, 0.5, 0.9)}


def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def op(src, mask=None, bg=None, fill=None, scale=1.0, offset=0.0, srgb=False):
    """An operand description: numpy fp32 arrays + host settings (the arguments of svgir_harness.metrics.plane)."""
    return dict(src=src, mask=mask, bg=bg, fill=fill, scale=scale, offset=offset, srgb=srgb)


def srgb32(x):
    """utils/graphics_utils.py:210-212 on an fp32 tensor, as written there."""
    y = torch.where(x > 0.0031308, torch.pow(torch.max(x, torch.tensor(0.0031308, device=x.device)), 1.0 / 2.4) * 1.055 - 0.055, 12.92 * x)
    return torch.clamp(y, 0.0, 1.0)


def compose(o, with_srgb=True):
    """The operand as torch forms it, fp32 [3,H,W]: src, (x * scale) + offset, (x * m) + ((1 - m) * f), srgb."""
    x = torch.from_numpy(o["src"])
    if o["scale"] != 1.0 or o["offset"] != 0.0:
        x = x * o["scale"] + o["offset"]
    if o["mask"] is not None:
        m = torch.from_numpy(o["mask"])
        f = torch.from_numpy(o["fill"]) if o["fill"] is not None else torch.tensor(_bg3(o["bg"]), dtype=torch.float32)[:, None, None]
        x = x * m + (1 - m) * f
    if o["srgb"] and with_srgb:
        x = srgb32(x)
    return x.contiguous()


def _bg3(bg):
    if bg is None:
        return (0.0, 0.0, 0.0)
    return tuple(bg) if isinstance(bg, (tuple, list)) else (float(bg),) * 3


def compose64(o):
    """The same operand for the fp64 evaluation: the fp32 value, sRGB (if any) in fp64 of the fp32 argument."""
    x = compose(o, with_srgb=False).numpy().astype(np.float64)
    return eo.rgb_to_srgb(x) if o["srgb"] else x


def e_srgb(o):
    if not o["srgb"]:
        return 0.0
    d = np.abs(compose(o).numpy().astype(np.float64) - compose64(o))
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


# ---- masks and contents --------------------------------------------------------------------------------------------------------------
def make_mask(kind, H, W, g):
    if kind == "binary":
        return (torch.rand(1, H, W, generator=g) < 0.6).float().numpy()
    if kind == "frac":
        m = torch.rand(1, H, W, generator=g)
        m[0, : max(H // 4, 1)] = 0.0
        m[0, H - max(H // 4, 1):] = 1.0
        return m.numpy()
    if kind == "edge16":     # the silhouette on the boundary between the first two tile columns
        m = torch.zeros(1, H, W)
        m[:, :, :16] = 1.0
        return m.numpy()
    raise KeyError(kind)


def srgb_ladder():
    k = KNEE
    return np.array([k, np.nextafter(k, F32(0)), np.nextafter(k, F32(1)), 0.0, -0.25, -1e-3, 1e-4, 0.002, 0.004, 0.05, 0.5, 1.0,
                     np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2)), 1.5, 4.0], dtype=F32)


def _pair(content, H, W, g):
    """(a, b) fp32 [3,H,W] sources."""
    if content in ("rand", "nan", "inf", "equal_all", "equal_ch1"):
        b = torch.rand(3, H, W, generator=g)
        b[:, : H // 3] = 0.25
        a = (b + 0.15 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
        if content == "equal_all":
            a = b.clone()
        if content == "equal_ch1":
            a[1] = b[1]
        if content == "nan":
            a[2, H // 2, W // 3] = float("nan")
        if content == "inf":
            a[0, H // 3, W // 2] = float("inf")
    elif content == "flat":
        b = torch.full((3, H, W), 0.7)
        a = torch.full((3, H, W), 0.7)
        a[:, :, W // 2:] = 0.7 + 1.0 / 256
    elif content == "sat":
        b = torch.zeros(3, H, W)
        b[:, H // 2:] = 1.0
        a = b.clone()
        noisy = slice(W // 3, (2 * W) // 3)
        a[:, :, noisy] = (a[:, :, noisy] + 0.1 * torch.randn(3, H, len(range(W)[noisy]), generator=g)).clamp(0, 1)
    elif content == "normal":     # unit-ish vectors in [-1, 1] against a [0, 1] encoded ground truth
        a = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
        b = (torch.nn.functional.normalize(a + 0.2 * torch.randn(3, H, W, generator=g), dim=0) * 0.5 + 0.5)
    elif content == "knee":       # b: linear values around the sRGB knee, below 0 and above 1, in every tile
        a = torch.rand(3, H, W, generator=g)
        b = 0.3 * torch.rand(3, H, W, generator=g) ** 3
        lad = torch.from_numpy(srgb_ladder())
        flat = b.reshape(-1)
        idx = torch.arange(0, flat.numel(), 3)
        flat[idx] = lad[torch.arange(idx.numel()) % lad.numel()]
        b = flat.reshape(3, H, W)
    else:
        raise KeyError(content)
    return a.float().contiguous().numpy(), b.float().contiguous().numpy()


def _case(id_, H, W, content, comp="none", ssim=True):
    return dict(id=f"{id_}-{H}x{W}", H=H, W=W, content=content, comp=comp, ssim=ssim)


def _metric_cases():
    out = [_case("rand", H, W, "rand") for H, W in SIZES]
    out += [_case("rand-nossim", 17, 33, "rand", ssim=False), _case("rand-nossim", 150, 161, "rand", ssim=False)]
    out += [_case("equal-all", 17, 33, "equal_all"), _case("equal-ch1", 17, 33, "equal_ch1"), _case("equal-all", 1, 1, "equal_all"),
            _case("equal-all-nossim", 31, 32, "equal_all", ssim=False)]
    out += [_case("flat", 5, 7, "flat"), _case("flat", 17, 33, "flat"), _case("sat", 31, 32, "sat")]
    out += [_case("nan", 17, 33, "nan"), _case("nan-nossim", 17, 33, "nan", ssim=False), _case("inf", 17, 33, "inf")]
    for comp in ("binary-black", "binary-white", "frac-colour", "edge16-white", "fill", "frac-colour-both"):
        out.append(_case(comp, 17, 33, "rand", comp))
    out += [_case("edge16-white", 31, 32, "rand", "edge16-white"), _case("fill", 150, 161, "rand", "fill"),
            _case("binary-white", 5, 7, "rand", "binary-white"), _case("frac-colour", 1, 1, "rand", "frac-colour")]
    out += [_case("affine", 17, 33, "normal", "affine", ssim=False), _case("affine", 31, 32, "normal", "affine")]
    out += [_case("srgb", H, W, "knee", "srgb") for H, W in ((5, 7), (17, 33), (150, 161))]
    out += [_case("srgb-masked", 17, 33, "knee", "srgb-masked"), _case("srgb-nossim", 16, 16, "knee", "srgb", ssim=False)]
    return out


METRIC_CASES = _metric_cases()
BY_ID = {c["id"]: c for c in METRIC_CASES}
# launches of several terms of one image size: 3 (the relighting frame's shape: two with SSIM, one without) and the maximum, 4
LAUNCHES = (("rand-17x33", "srgb-17x33", "affine-17x33"),
            ("nan-17x33", "rand-nossim-17x33", "fill-17x33", "srgb-masked-17x33"),
            ("rand-150x161", "fill-150x161", "rand-nossim-150x161"))
GOLDEN_CASES = ("rand-17x33", "equal-ch1-17x33", "nan-17x33", "srgb-17x33", "frac-colour-17x33")   # recorded from the reference


@functools.lru_cache(maxsize=None)
def _build(case_id):
    c = BY_ID[case_id]
    H, W = c["H"], c["W"]
    g = _gen(case_id)
    a, b = _pair(c["content"], H, W, g)
    comp = c["comp"]
    if comp == "none":
        return op(a), op(b)
    if comp == "srgb":
        return op(a), op(b, srgb=True)
    if comp == "srgb-masked":
        return op(a), op(b, mask=make_mask("frac", H, W, g), bg=BACKGROUNDS["white"], srgb=True)
    if comp == "affine":      # the captured normal: * 0.5 + 0.5, then over a white background; the ground truth over the same
        m = make_mask("binary", H, W, g)
        return op(a, mask=m, bg=1.0, scale=0.5, offset=0.5), op(b, mask=m, bg=1.0)
    if comp == "fill":
        return op(a, mask=make_mask("frac", H, W, g), fill=torch.rand(3, H, W, generator=g).numpy()), op(b)
    kind, bg = comp.split("-")[0], BACKGROUNDS[comp.split("-")[1]]
    m = make_mask(kind, H, W, g)
    if comp.endswith("-both") or kind in ("binary", "edge16"):
        return op(a, mask=m, bg=bg), op(b, mask=m, bg=bg)
    return op(a, mask=m, bg=bg), op(b)


def build(case):
    """(a, b) operand descriptions of a METRIC_CASES entry (cached: treat as read-only)."""
    return _build(case["id"])


# ---- the metrics oracle ----------------------------------------------------------------------------------------------------------------
def _rows(a, b, want_ssim, keep_dtype):
    """The row of 10 from operands of one dtype, in that dtype's arithmetic (fp32: the reference's own order)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        m = ((a - b) ** 2).view(3, -1).mean(1, keepdim=True)                    # utils/image_utils.py:32-33
        p = 20 * torch.log10(1.0 / torch.sqrt(m)) if keep_dtype else -10.0 * torch.log10(m)   # :36-37 (fp64: the same number, one rounding less)
        l1, s = eo.l1_ssim_torch(a, b, keep_dtype=keep_dtype)
    row = np.empty(COLS, dtype=np.float64)
    row[0:3], row[3:6] = m.double().numpy()[:, 0], p.double().numpy()[:, 0]
    row[6], row[7] = float(m.mean()), float(p.mean())
    row[8] = float(s) if want_ssim else np.nan
    row[9] = float(l1)
    return row


_REFERENCES = {}


def reference(case):
    """(row64, row32, E_SRGB) of a table case, or of an ad-hoc term dict(id, ssim, ops=(a, b)) (a frame's); computed once per id."""
    if case["id"] not in _REFERENCES:
        oa, ob = case["ops"] if "ops" in case else _build(case["id"])
        r64 = _rows(torch.from_numpy(compose64(oa)), torch.from_numpy(compose64(ob)), case["ssim"], False)
        r32 = _rows(compose(oa), compose(ob), case["ssim"], True)
        _REFERENCES[case["id"]] = (r64, r32, max(e_srgb(oa), e_srgb(ob)))
    return _REFERENCES[case["id"]]


def e32(case):
    """E32 per column: relative for the mse columns, absolute for the others; 0 where a row is not finite."""
    r64, r32, _ = reference(case)
    out = np.zeros(COLS)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs(r32 - r64)
        for j in range(COLS):
            if not (np.isfinite(r64[j]) and np.isfinite(r32[j])):
                continue
            out[j] = d[j] / r64[j] if j in (0, 1, 2, 6) and r64[j] > 0 else d[j]
    return out


def tolerances(case):
    """Absolute bounds per column for a kernel's row against row64 (tests/test_gpu_view_metrics.py's header has the derivation):
    mse_c 4 max(E32, eps32) mse_c [+ 2 l1 delta + delta^2, delta = 4 E_SRGB, for a term with sRGB]; psnr_c (10 / ln 10) tol_mse / mse_c;
    the means the mean of their parts' bounds; ssim max(1e-5, 4 E32); l1 max(1e-6, 4 E32)."""
    r64, _, es = reference(case)
    e = e32(case)
    tol = np.zeros(COLS)
    delta = 4.0 * es
    l1 = r64[9] if np.isfinite(r64[9]) else 0.0
    for c in range(3):
        if not np.isfinite(r64[c]):
            continue
        tol[c] = 4.0 * max(e[c], EPS32) * r64[c] + (2.0 * l1 * delta + delta * delta if es > 0 else 0.0)
        tol[3 + c] = (10.0 / np.log(10.0)) * tol[c] / r64[c] if r64[c] > 0 else 0.0
    tol[6], tol[7] = tol[0:3].mean(), tol[3:6].mean()
    tol[8] = max(1e-5, 4.0 * e[8])
    tol[9] = max(1e-6, 4.0 * e[9])
    return tol


def check_row(name, got, case, extra=None, cols=None):
    """The comparison rule: NaN and +-inf patterns equal the oracle's, finite entries within the bounds (+ `extra` per column); `cols`
    restricts the bound check to some columns."""
    r64 = reference(case)[0]
    tol = tolerances(case) + (0.0 if extra is None else extra)
    got = np.asarray(got, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(r64)), f"{name}: NaN pattern {got} vs {r64}"
    assert np.array_equal(np.isposinf(got), np.isposinf(r64)) and np.array_equal(np.isneginf(got), np.isneginf(r64)), f"{name}: inf pattern {got} vs {r64}"
    fin = np.isfinite(r64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - r64)
    print(f"{name}: err/tol " + " ".join(f"{err[j]:.1e}/{tol[j]:.1e}" if fin[j] else "-" for j in range(COLS)))
    bad = fin & (err > tol)
    if cols is not None:
        bad &= np.isin(np.arange(COLS), cols)
    assert not bad.any(), f"{name}: columns {np.nonzero(bad)[0].tolist()} off: got {got}, oracle {r64}, bounds {tol}"


# ---- the byte ladder ---------------------------------------------------------------------------------------------------------------------
BYTE_SIZES = ((1, 1), (5, 7), (1, 257), (16, 16), (17, 33))   # 1 x 257: 771 bytes per image, every image base and tail misaligned differently
BYTE_COUNTS = (1, 12, 16)


def byte_ladder():
    """k / 255 and both fp32 neighbours of (k + 0.5) / 255 (where the truncation flips), negatives, values above 1, NaN, +-inf."""
    k = np.arange(256, dtype=np.float64)
    half = ((k + 0.5) / 255.0).astype(F32)
    vals = [(k / 255.0).astype(F32), half, np.nextafter(half, F32(-1)), np.nextafter(half, F32(2)),
            np.array([-1.0, -0.002, -1e-9, -0.0, 1.0 + 1e-6, 1.002, 2.0, 300.0, -300.0, np.nan, np.inf, -np.inf, 3.4e38, -3.4e38], dtype=F32)]
    return np.concatenate(vals).astype(F32)


def _byte_cases():
    out = []
    for H, W in BYTE_SIZES:
        for n in BYTE_COUNTS:
            if n == 12 and (H, W) not in ((5, 7), (1, 257), (17, 33)):
                continue
            out.append(dict(id=f"{H}x{W}-n{n}", H=H, W=W, n=n))
    return out


BYTE_CASES = _byte_cases()


@functools.lru_cache(maxsize=None)
def _build_bytes(case_id):
    c = next(b for b in BYTE_CASES if b["id"] == case_id)
    H, W, n = c["H"], c["W"], c["n"]
    g = _gen("bytes" + case_id)
    lad = byte_ladder()
    ops = []
    for k in range(n):
        src = np.resize(np.roll(lad, -131 * k - 7 * W), 3 * H * W).reshape(3, H, W).astype(F32)   # every image starts elsewhere on the ladder
        kind = k % 4
        if kind == 0:
            ops.append(op(src))
        elif kind == 1:
            ops.append(op(src, mask=make_mask("binary", H, W, g), bg=BACKGROUNDS["colour"]))
        elif kind == 2:
            ops.append(op(src, mask=make_mask("frac", H, W, g), fill=np.resize(np.roll(lad, 17 * k), 3 * H * W).reshape(3, H, W).astype(F32)))
        else:
            ops.append(op((2.0 * torch.rand(3, H, W, generator=g) - 1.0).numpy(), mask=make_mask("binary", H, W, g), bg=1.0, scale=0.5, offset=0.5))
    return tuple(ops)


def build_bytes(case):
    return _build_bytes(case["id"])


def torch_quantise(x):
    """torchvision.utils.save_image's own line (through make_grid's 1 -> 3 channel repeat) on a torch tensor of any device."""
    if x.shape[0] == 1:
        x = torch.cat((x, x, x), 0)
    return x.clone().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)


def quantise(x):
    """numpy fp32 restatement of torchvision.utils.save_image's `mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8)` (restated from
    its source; unpinned by torchvision itself) for a composed fp32 [3,H,W] array -> uint8 [H,W,3]; NaN gives 0 (torch leaves it undefined)."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (x * F32(255)).astype(F32) + F32(0.5)
        v = np.where(v > 0, np.minimum(v, F32(255)), F32(0)).astype(F32)      # NaN > 0 is false
    return np.ascontiguousarray(v.astype(np.uint8).transpose(1, 2, 0))


def bytes_reference(case):
    return np.stack([quantise(compose(o).numpy()) for o in build_bytes(case)])


# ---- the albedo scale ----------------------------------------------------------------------------------------------------------------------
CLAMP_LO = float(F32(1e-6))


def _albedo_cases():
    out = []
    for H, W in ((5, 7), (17, 33), (40, 56)):       # 40 x 56 = 2240 pixels: three workgroups, the last partial
        for sel in ("partial", "all"):
            for srgb in (False, True):
                out.append(dict(id=f"{sel}-{H}x{W}" + ("-srgb" if srgb else ""), H=H, W=W, sel=sel, srgb=srgb, special=(H, W) != (5, 7)))
    out += [dict(id="empty-17x33", H=17, W=33, sel="empty", srgb=False, special=False),
            dict(id="one-1x1", H=1, W=1, sel="all", srgb=False, special=False),
            dict(id="zero-over-zero-17x33", H=17, W=33, sel="partial", srgb=True, special="nan")]
    return out


ALBEDO_CASES = _albedo_cases()
GOLDEN_ALBEDO = ("partial-17x33-srgb", "all-40x56", "zero-over-zero-17x33")   # recorded from the reference


@functools.lru_cache(maxsize=None)
def _build_albedo(case_id):
    c = next(a for a in ALBEDO_CASES if a["id"] == case_id)
    H, W = c["H"], c["W"]
    g = _gen("albedo" + case_id)
    render = 0.05 + 0.9 * torch.rand(3, H, W, generator=g)
    gt = (render * (0.4 + 0.5 * torch.rand(3, H, W, generator=g))).clamp(0, 1)
    if c["sel"] == "partial":      # background: exactly zero; a few pixels with a clearly negative sum
        off = torch.rand(H, W, generator=g) < 0.4
        render[:, off] = 0.0
        neg = torch.rand(H, W, generator=g) < 0.05
        render[:, neg] = -0.25
    elif c["sel"] == "empty":
        render = torch.zeros(3, H, W)
        render[:, ::2] = -0.5
    if c["special"]:
        flat_r, flat_g = render.reshape(3, -1), gt.reshape(3, -1)
        pos = torch.nonzero(flat_r.sum(0) > 1.6)[:, 0]   # the sum stays clearly positive after the edits below
        assert pos.numel() >= 4, case_id
        p0, p1, p2, p3 = (int(pos[i]) for i in (0, pos.numel() // 3, pos.numel() // 2, pos.numel() - 1))
        flat_r[0, p0], flat_g[0, p0] = 0.0, 0.5          # gt / 0 = inf -> 1
        flat_g[1, p1] = 1e-9                              # ratio below 1e-6 -> 1e-6
        flat_g[2, p2] = 1.0                               # ratio above 1 -> 1
        flat_r[1, p3] = -0.3                              # a negative channel inside a positive sum: ratio < 0 -> 1e-6
        if c["special"] == "nan":
            flat_r[0, p2], flat_g[0, p2] = 0.0, 0.0       # 0 / 0 -> NaN in channel 0
    return render.float().contiguous().numpy(), gt.float().contiguous().numpy()


def build_albedo(case):
    return _build_albedo(case["id"])


def albedo_lines(render_albedo, gt_albedo, srgb, rgb_to_srgb):
    """eval_relighting_tensoIR.py:285-294, literally, on torch tensors of one dtype."""
    img_mask = render_albedo.mean(dim=0) > 0
    if srgb:
        gt_albedo = rgb_to_srgb(gt_albedo)
    render_albedo = render_albedo.permute(1, 2, 0)[img_mask]
    gt_albedo = gt_albedo.permute(1, 2, 0)[img_mask]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        albedo_scale = (gt_albedo / render_albedo).clamp(CLAMP_LO, 1).mean(dim=0)
    return albedo_scale, img_mask


def albedo_reference(case):
    """(scale64 [3], scale32 [3], count, mask32, mask64)."""
    r, g = build_albedo(case)
    s32, m32 = albedo_lines(torch.from_numpy(r), torch.from_numpy(g), case["srgb"], srgb32)
    s64, m64 = albedo_lines(torch.from_numpy(r).double(), torch.from_numpy(g).double(), case["srgb"],
                            lambda x: torch.from_numpy(eo.rgb_to_srgb(x.numpy())))
    return s64.numpy(), s32.double().numpy(), int(m64.sum()), m32.numpy(), m64.numpy()


# ---- one relighting frame ------------------------------------------------------------------------------------------------------------------
FRAME_SIZES = ((17, 33), (150, 161))
FRAME_CAPTURES = ("pbr", "base_color", "normal", "roughness", "diffuse", "specular", "lights", "local_lights", "global_lights", "visibility",
                  "direct", "pbr_env")      # 12: every branch of the reference's capture loop; "pbr" in front of "pbr_env"
FRAME_BG = 1.0                              # dataset.white_background


@functools.lru_cache(maxsize=None)
def build_frame(H, W):
    """dict(render_pkg={name: fp32 array}, gt_image, gt_albedo, gt_normal, mask): what one frame of eval_relighting_tensoIR.py holds after
    `render_fn` and its image loads; a BINARY mask (the alpha of the ground truth), values in [0, 1] (normals in [-1, 1]), no NaN."""
    g = _gen(f"frame{H}x{W}")
    r = lambda c: torch.rand(c, H, W, generator=g)  # noqa: E731
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    mask = ((((yy - H / 2.0) / (0.45 * H)) ** 2 + ((xx - W / 2.0) / (0.4 * W)) ** 2) < 1).float()[None]
    pkg = {k: r(3) for k in ("pbr", "base_color", "diffuse", "specular", "lights", "local_lights", "global_lights", "direct", "env_only")}
    pkg["pbr"] = 1.2 * pkg["pbr"]          # (HDR: some values above 1 reach the clamp of the quantisation)
    pkg["roughness"], pkg["visibility"] = r(1), r(1)
    pkg["normal"] = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
    gt_image = (pkg["pbr"] + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    gt_albedo = (0.6 * pkg["base_color"] ** 2.2 + 0.02 * torch.randn(3, H, W, generator=g)).clamp(0, 1)   # linear: the eval applies srgb
    gt_normal = (torch.nn.functional.normalize(pkg["normal"] + 0.2 * torch.randn(3, H, W, generator=g), dim=0) * 0.5 + 0.5)
    f = lambda t: t.float().contiguous().numpy()  # noqa: E731
    return dict(render_pkg={k: f(v) for k, v in pkg.items()}, gt_image=f(gt_image), gt_albedo=f(gt_albedo), gt_normal=f(gt_normal), mask=f(mask))


def frame_terms(H, W):
    """The three metric terms of the frame with FRAME_CAPTURES (pbr and normal were captured: composited, the normal after * 0.5 + 0.5)."""
    fr = build_frame(H, W)
    pkg, m = fr["render_pkg"], fr["mask"]
    return (dict(id=f"frame-pbr-{H}x{W}", ssim=True, ops=(op(pkg["pbr"], mask=m, bg=FRAME_BG), op(fr["gt_image"], mask=m, bg=FRAME_BG))),
            dict(id=f"frame-albedo-{H}x{W}", ssim=True, ops=(op(pkg["base_color"]), op(fr["gt_albedo"], mask=m, bg=FRAME_BG, srgb=True))),
            dict(id=f"frame-normal-{H}x{W}", ssim=False,
                 ops=(op(pkg["normal"], mask=m, bg=FRAME_BG, scale=0.5, offset=0.5), op(fr["gt_normal"], mask=m, bg=FRAME_BG))))


def eager_relighting_frame(render_pkg, gt_image, gt_albedo, gt_normal, mask, bg, capture_list, save, rgb_to_srgb, psnr, ssim, mse):
    """The eager restatement of eval_relighting_tensoIR.py:333-378 on torch tensors of any device: the capture loop, the ground-truth
    composites and the metric calls in the reference's order (LPIPS apart); `save(name, image)` stands where save_image is called.
    Returns {pbr, albedo, normal: {psnr, ssim, mse}} as the tensors the reference accumulates."""
    render_pkg = dict(render_pkg)
    for capture_type in capture_list:
        if capture_type == "normal":
            render_pkg[capture_type] = render_pkg[capture_type] * 0.5 + 0.5
            render_pkg[capture_type] = render_pkg[capture_type] * mask + (1 - mask) * bg
        elif capture_type in ["roughness", "diffuse", "specular", "lights", "local_lights", "global_lights", "visibility", "direct"]:
            render_pkg[capture_type] = render_pkg[capture_type] * mask + (1 - mask) * bg
        elif capture_type in ["base_color"]:
            render_pkg[capture_type] = render_pkg[capture_type]
        elif capture_type in ["pbr"]:
            render_pkg[capture_type] = render_pkg["pbr"] * mask + (1 - mask) * bg
        elif capture_type in ["pbr_env"]:
            render_pkg[capture_type] = render_pkg["pbr"] * mask + (1 - mask) * render_pkg["env_only"]
        save(capture_type, render_pkg[capture_type])
    gt_image = gt_image * mask + bg * (1 - mask)
    save("gt", gt_image)
    gt_albedo = gt_albedo * mask + bg * (1 - mask)
    gt_albedo = rgb_to_srgb(gt_albedo)
    gt_normal = gt_normal * mask + bg * (1 - mask)
    return dict(pbr=dict(psnr=psnr(render_pkg["pbr"], gt_image).mean(), ssim=ssim(render_pkg["pbr"], gt_image).mean(),
                         mse=mse(render_pkg["pbr"], gt_image).mean()),
                albedo=dict(psnr=psnr(render_pkg["base_color"], gt_albedo).mean(), ssim=ssim(render_pkg["base_color"], gt_albedo).mean(),
                            mse=mse(render_pkg["base_color"], gt_albedo).mean()),
                normal=dict(mse=mse(render_pkg["normal"], gt_normal).mean()))


def torch_mse(img1, img2):
    return ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)


def torch_psnr(img1, img2):
    return 20 * torch.log10(1.0 / torch.sqrt(torch_mse(img1, img2)))


def torch_ssim(img1, img2):
    """utils/loss_utils.py:33-64 in the dtype of img1 (oracle/epilogue_oracle.l1_ssim_torch's fp32 stand-in), evaluated on the CPU."""
    return eo.l1_ssim_torch(img1.cpu(), img2.cpu(), keep_dtype=True)[1]
