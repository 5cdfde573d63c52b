"""The case table of LPIPS (csrc/lpips.hip, svgir_harness/metrics.py `LPIPS` / `lpips_terms`, the drop-in lpipsPyTorch) and its oracle, shared
by tests/test_lpips_edge_inputs.py (CPU: pins the oracle by tests/golden/lpips.npz, proves the table, measures E32 / EM) and
tests/test_gpu_lpips.py (the kernels against it).

WEIGHTS.  The pretrained VGG16 and the LPIPS linear layers are not available to this project (58.9 MB; unpinned by the published weights),
so the network is filled with seeded weights of the same shapes: numpy default_rng, He-normal convolutions (std sqrt(2 / (9 Cin))), biases
0.05 N, linear weights |N| / C.  The fixture holds an fp64 checksum of them, so the builder cannot drift.  Variants: "dead5" sets the
conv5_3 bias to -1e3 (every relu5_3 vector is zero: the `+ 1e-10` case), "signed" gives the linear weights mixed signs.

ORACLE.  `evaluate` restates lpipsPyTorch/modules/{lpips,networks,utils}.py with torch on the CPU: (x - mean) / std with the reference's
fp32 constants, vgg16.features up to relu5_3, x / (sqrt(sum_c x^2) + 1e-10) at the five tapped layers, (fx - fy)^2 through the 1 x 1 layers,
the mean over the pixels, the sum of the five.  dtype float64 is the oracle; float32 in torch's contiguous order and in channels_last are
the two fp32 orders whose deviation from it (E32 per tap, EM per tap map) the GPU bounds are derived from.  Operands are composed in fp32
as torch forms them (tests/metrics_cases.compose).  Nothing here looks at a kernel's result."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import metrics_cases as mc

F32 = np.float32
EPS32 = 2.0 ** -23
SEED = 20240611
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_SHAPE = ((64, 3), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256), (512, 512), (512, 512), (512, 512),
              (512, 512), (512, 512))
POOL_INDEX = (4, 9, 16, 23)            # (the fifth pool, features.30, never runs)
TAP_INDEX = (3, 8, 15, 22, 29)         # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3: the reference's 1-based target_layers 4, 9, 16, 23, 30
TAP_C = (64, 128, 256, 512, 512)
MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)


# ---- weights ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base_arrays():
    rng = np.random.default_rng(SEED)
    conv_w, conv_b, lin = [], [], []
    for co, ci in CONV_SHAPE:
        conv_w.append((rng.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))).astype(F32))
        conv_b.append((0.05 * rng.standard_normal(co)).astype(F32))
    for c in TAP_C:
        lin.append((np.abs(rng.standard_normal(c)) / c).astype(F32))
    return conv_w, conv_b, lin


@functools.lru_cache(maxsize=None)
def weights(variant="base"):
    """(vgg_state, lin_state): torch fp32 CPU tensors under torchvision's keys (`features.N.weight` / `.bias`) and the published LPIPS keys
    (`linK.model.1.weight`, [1,C,1,1])."""
    conv_w, conv_b, lin = _base_arrays()
    conv_b, lin = list(conv_b), list(lin)
    if variant == "dead5":
        conv_b[12] = np.full(512, -1e3, F32)
    elif variant == "signed":
        sign = np.random.default_rng(SEED + 1)
        lin = [(w * np.where(sign.random(w.size) < 0.5, -1.0, 1.0)).astype(F32) for w in lin]
    elif variant != "base":
        raise KeyError(variant)
    vgg = {}
    for i, w, b in zip(CONV_INDEX, conv_w, conv_b):
        vgg[f"features.{i}.weight"] = torch.from_numpy(w)
        vgg[f"features.{i}.bias"] = torch.from_numpy(b)
    lin_state = {f"lin{k}.model.1.weight": torch.from_numpy(w).reshape(1, -1, 1, 1) for k, w in enumerate(lin)}
    return vgg, lin_state


def weight_checksum(variant="base"):
    """fp64 (sum, sum of squares) over every weight, in state-dict order."""
    vgg, lin = weights(variant)
    s = q = 0.0
    for t in list(vgg.values()) + list(lin.values()):
        a = t.numpy().astype(np.float64).ravel()
        s += float(a.sum()); q += float((a * a).sum())
    return np.array([s, q], np.float64)


# ---- oracle ----------------------------------------------------------------------------------------------------------------------------
def features(x, vgg, dtype=torch.float64, channels_last=False):
    """The five tapped maps (before normalisation) of a [3,H,W] fp32 image, as [1,C_k,H_k,W_k] tensors of `dtype`."""
    mean = torch.tensor(MEAN, dtype=torch.float32)[None, :, None, None].to(dtype)   # (the reference's buffers are fp32 tensors)
    std = torch.tensor(STD, dtype=torch.float32)[None, :, None, None].to(dtype)
    h = (x[None].to(dtype) - mean) / std
    if channels_last:
        h = h.contiguous(memory_format=torch.channels_last)
    taps = []
    for i in range(TAP_INDEX[-1] + 1):
        if i in CONV_INDEX:
            w, b = vgg[f"features.{i}.weight"].to(dtype), vgg[f"features.{i}.bias"].to(dtype)
            if channels_last:
                w = w.contiguous(memory_format=torch.channels_last)
            h = F.conv2d(h, w, b, padding=1)
        elif i in POOL_INDEX:
            h = F.max_pool2d(h, 2, 2)
        else:
            h = torch.relu(h)
            if i in TAP_INDEX:
                taps.append(h)
    return taps


def _normalize(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


@torch.no_grad()
def evaluate(x, y, variant="base", dtype=torch.float64, channels_last=False):
    """x, y: torch fp32 [3,H,W] (composed operands).  Returns dict(taps [5], score (), maps: five [2,C_k,H_k,W_k] arrays (x, then y)),
    numpy arrays of `dtype`."""
    vgg, lin = weights(variant)
    fx, fy = features(x, vgg, dtype, channels_last), features(y, vgg, dtype, channels_last)
    res = []
    for k, (a, b) in enumerate(zip(fx, fy)):
        d = (_normalize(a) - _normalize(b)) ** 2
        res.append(F.conv2d(d, lin[f"lin{k}.model.1.weight"].to(dtype)).mean((2, 3), True))
    score = torch.sum(torch.cat(res, 0), 0, True)
    return dict(taps=torch.cat(res, 0).reshape(5).numpy(), score=score.reshape(()).numpy(),
                maps=[torch.cat([a, b], 0).contiguous().numpy() for a, b in zip(fx, fy)])


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def _rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


def _rand(key, H, W, lo=0.0, hi=1.0):
    return (lo + (hi - lo) * _rng(key).random((3, H, W))).astype(F32)


def _const(v, H, W):
    return np.full((3, H, W), v, F32)


def _pair(cid, H, W):
    """Two correlated images in [0, 1], as a render and its ground truth are."""
    x = _rand(cid + "/x", H, W)
    y = np.clip(x + 0.2 * (_rand(cid + "/n", H, W) - 0.5), 0.0, 1.0).astype(F32)
    return x, y


def _case(cid, a, b, variant="base", expect=None):
    """a, b: operand descriptions (metrics_cases.op).  expect: None, "zero" (every tap exactly 0), "zero5" (tap 5 exactly 0), "nan"."""
    H, W = a["src"].shape[1:]
    return dict(id=cid, H=H, W=W, a=a, b=b, variant=variant, expect=expect)


def _build_cases():
    cases = []
    # 1-4: the sizes.  16: every level down to 1 x 1; floors in every pool; strips; partial tiles on both axes at every level
    for H, W in ((16, 16), (17, 19), (31, 31), (32, 32), (33, 47), (16, 150), (150, 16), (150, 161)):
        x, y = _pair(f"size{H}x{W}", H, W)
        cases.append(_case(f"size_{H}x{W}", mc.op(x), mc.op(y)))
    # 5: equal operands (the GPU test also passes the SAME tensor twice)
    x, y = _pair("equal", 33, 47)
    cases.append(_case("equal_copy_33x47", mc.op(x), mc.op(x.copy()), expect="zero"))
    # 6: (y, x) of a case above: the same bits as (x, y)
    x, y = _pair("size33x47", 33, 47)
    cases.append(_case("swapped_33x47", mc.op(y), mc.op(x)))
    # 7: constants
    cases.append(_case("const_0_vs_1_17x19", mc.op(_const(0.0, 17, 19)), mc.op(_const(1.0, 17, 19))))
    cases.append(_case("const_vs_itself_17x19", mc.op(_const(0.25, 17, 19)), mc.op(_const(0.25, 17, 19)), expect="zero"))
    # 8: values outside [0, 1]
    cases.append(_case("range_-2_3_31x31", mc.op(_rand("range/x", 31, 31, -2.0, 3.0)), mc.op(_rand("range/y", 31, 31, -2.0, 3.0))))
    # 9, 10: weight variants
    x, y = _pair("dead5", 32, 32)
    cases.append(_case("dead_relu5_3_32x32", mc.op(x), mc.op(y), variant="dead5", expect="zero5"))
    x, y = _pair("signed", 33, 47)
    cases.append(_case("signed_lin_33x47", mc.op(x), mc.op(y), variant="signed"))
    # 11: non-finite pixels
    for name, v in (("nan", np.nan), ("inf", np.inf)):
        x, y = _pair(name, 33, 47)
        x[1, 20, 31] = v
        cases.append(_case(f"{name}_pixel_33x47", mc.op(x), mc.op(y), expect="nan"))
    # 12: plane operands
    H, W = 33, 47
    x, y = _pair("plane", H, W)
    mask = (_rng("plane/m").random((1, H, W)) < 0.6).astype(F32)
    mask[0, :, 10:14] = _rng("plane/soft").random((H, 4)).astype(F32)   # a soft edge
    fill = _rand("plane/fill", H, W)
    nrm = _rand("plane/nrm", H, W, -1.0, 1.0)
    cases.append(_case("plane_mask_bg_33x47", mc.op(x, mask=mask, bg=(0.2, 0.5, 0.9)), mc.op(y, mask=mask, bg=(0.2, 0.5, 0.9))))
    cases.append(_case("plane_mask_fill_33x47", mc.op(x, mask=mask, fill=fill), mc.op(y)))
    cases.append(_case("plane_affine_33x47", mc.op(nrm, scale=0.5, offset=0.5), mc.op(y, mask=mask, bg=1.0)))
    cases.append(_case("plane_srgb_33x47", mc.op(x), mc.op(y, mask=mask, bg=0.0, srgb=True)))
    return cases


CASES = _build_cases()
BY_ID = {c["id"]: c for c in CASES}
SRGB_CASES = tuple(c["id"] for c in CASES if c["a"]["srgb"] or c["b"]["srgb"])
FINITE_CASES = tuple(c["id"] for c in CASES if c["expect"] != "nan")
# 13: pairs per call (one image size each); the first entry of each is also evaluated alone
BATCHES = (("size_33x47",), ("size_33x47", "swapped_33x47"), ("plane_mask_bg_33x47", "size_33x47", "signed_base_33x47", "equal_copy_33x47"))
GOLDEN_CASES = ("size_16x16", "size_17x19", "size_33x47", "const_0_vs_1_17x19", "range_-2_3_31x31", "dead_relu5_3_32x32", "signed_lin_33x47")

# "signed_base_33x47": the inputs of the signed case with the base weights (a batch shares one network)
CASES.append(_case("signed_base_33x47", BY_ID["signed_lin_33x47"]["a"], BY_ID["signed_lin_33x47"]["b"]))
BY_ID["signed_base_33x47"] = CASES[-1]
FINITE_CASES += ("signed_base_33x47",)


def operands(case):
    """The two composed fp32 [3,H,W] torch tensors of a case."""
    return mc.compose(case["a"]), mc.compose(case["b"])


@functools.lru_cache(maxsize=None)
def oracle(cid, kind="f64"):
    """The case evaluated in fp64 ("f64"), in fp32 contiguous ("f32") or fp32 channels_last ("f32cl"); computed once, shared, never written."""
    c = BY_ID[cid]
    x, y = operands(c)
    dtype = torch.float64 if kind == "f64" else torch.float32
    return evaluate(x, y, c["variant"], dtype, channels_last=(kind == "f32cl"))


@functools.lru_cache(maxsize=None)
def measured_errors():
    """(E32 [5], EM [5]): per tap k the largest relative deviation of the two fp32 orders from fp64 over the finite cases of the table, and
    the same for the tap maps, normalised by each map's largest magnitude.  Cases whose fp64 tap is exactly 0 contribute nothing to E32
    (their fp32 taps are exactly 0 too: test_lpips_edge_inputs.py)."""
    e32, em = np.zeros(5), np.zeros(5)
    for cid in FINITE_CASES:
        ref = oracle(cid)
        for kind in ("f32", "f32cl"):
            got = oracle(cid, kind)
            for k in range(5):
                if ref["taps"][k] != 0.0:
                    e32[k] = max(e32[k], abs(float(got["taps"][k]) - ref["taps"][k]) / abs(ref["taps"][k]))
                top = np.abs(ref["maps"][k]).max()
                if top > 0.0:
                    em[k] = max(em[k], float(np.abs(got["maps"][k].astype(np.float64) - ref["maps"][k]).max() / top))
    return e32, em


def tap_bounds(cid):
    """4 max(E32_k, 8 eps32) |oracle tap_k| per tap, and their sum for the score."""
    e32, _ = measured_errors()
    tol = 4.0 * np.maximum(e32, 8 * EPS32) * np.abs(oracle(cid)["taps"])
    return tol, float(tol.sum())


def map_bounds(cid):
    """4 max(EM_k, 8 eps32) max|map_k| per element."""
    _, em = measured_errors()
    return [4.0 * max(em[k], 8 * EPS32) * float(np.abs(oracle(cid)["maps"][k]).max()) for k in range(5)]
