"""The case table of the smoothness-loss tests and its oracle: tests/test_smooth_edge_inputs.py (the oracle alone: against the recorded
reference results of tests/golden/smooth_losses.npz, against a second construction in numpy, against finite differences) and
tests/test_gpu_smooth_loss.py (csrc/smooth_loss.hip against the fp64 oracle).

The image derivative is kornia's spatial_gradient(x[None], 'sobel', order, normalized=True)[0], restated (kornia is not installed where this
project is built): per channel the cross-correlation (F.conv2d) of the REPLICATE-padded plane with
    order 1, pad 1: Kx = [[-1,0,1],[-2,0,2],[-1,0,1]] / 8, Ky = Kx^T                      -> [C,2,H,W] in (x, y) order
    order 2, pad 2: Kxx = [[-1,0,2,0,-1],[-4,0,8,0,-4],[-6,0,12,0,-6],[-4,0,8,0,-4],[-1,0,2,0,-1]] / 64, Kyy = Kxx^T   (the reference takes
                    [:, [0, 2]] of (xx, xy, yy): the mixed derivative is never built)
Every derivative goes through abs, so neither the overall sign of a kernel nor kornia's kernel flip can change a value defined here.

Terms (utils/loss_utils.py:101-117), D = data * data_mask, I = img * img_mask in fp32, Cb = max(C, Ci):
    first : sum |d_k D| exp(-|d_k I|) / (Cb H W);   second: sum |d_kk D| exp(-10 |d_k I|) / (Cb H W);   tv: the two means of squared differences.

Two evaluations per term:
    torch_eval(term, dtype) -- the reference's own operation order: torch pad + conv2d + abs / exp + .sum(1).mean() + autograd, in fp64 or
        in fp32 (the latter is what the reference's arithmetic loses: E32 = |fp32 - fp64| per loss, G32 for the gradients, below);
    oracle(term)            -- fp64 with the kernels' conventions written out: sign(0) = 0, an element (cb, k, p) whose value is NaN puts NaN
        into the loss and contributes to NO gradient (torch's autograd would spread 0 * NaN), the adjoint of pad + conv2d applied to the
        explicit per-element derivatives.  It also returns A (the sum of the absolute contributions to the loss), Aabs (the same per
        gradient element) and the threshold elements.  On finite inputs oracle == torch_eval(fp64) (asserted by the CPU test).

Bounds (the GPU test): loss   |kernel sum / count - oracle| <= 4 E32 + n 2^-53 A   (n elements summed in another order);
                       grads  |kernel - oracle| <= 4 G32 eps32 max(Aabs, AABS_FLOOR) per element that is not a threshold element.
G32 = the largest |torch_eval(fp32) gradient - oracle| / (eps32 max(Aabs, AABS_FLOOR)) over the non-threshold elements of the whole table,
measured by tests/test_smooth_edge_inputs.py::test_e32_g32_and_threshold_caps, which fails if the constant below is smaller than what it
measures.  Measured: 330.3 (case `strong`, the second-order term: 10 x the fp32 error of an img derivative of 20 ... 100 goes into the
exponent); without that case 4.2.  The constant leaves room for a conv2d that sums in another order on another CPU.
AABS_FLOOR = FLT_MIN / eps32: where every contribution to a gradient element is below fp32's normal range -- the `strong` case, whose weights
exp(-200) are 0 in fp32 -- Aabs is 1e-90 and a relative bound would ask fp32 for numbers it does not have; the floor makes the bound there
4 G32 FLT_MIN = 2.4e-35 absolute, and changes nothing for an element above the normal range.

Threshold elements: a derivative whose fp64 magnitude is non-zero but below 2^-20 sum |K| |x| over its window can take either sign in fp32;
the gradient elements inside the stencil of such a derivative (of `data` for d_data, of `img` for d_img) are held to finiteness only.  At most
MAX_THRESHOLD_SHARE of a term's gradient elements (the radiance table's cap).  Exact zeros are not threshold elements.

Every case is a seeded builder that returns fp32 arrays; nothing is read from a file."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
AABS_FLOOR = float(np.finfo(np.float32).tiny) / EPS32
G32 = 512.0                    # measured 330.3 (see the module docstring)
MAX_THRESHOLD_SHARE = 0.01
THRESHOLD = 2.0 ** -20
TILE = (8, 32)                 # rows, columns of a workgroup's tile (csrc/smooth_loss.hip)
SIZES = ((1, 1), (1, 7), (5, 1), (2, 2), (3, 3), (5, 5), (8, 32), (7, 31), (9, 33), (21, 70), (150, 161))
PAIRS = ((1, 1), (1, 3), (3, 1), (3, 3))
KINDS = {"first": 1, "second": 2, "tv": 3}
SHARP = {"first": 1.0, "second": 10.0}

KX = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=np.float64) / 8
KXX = np.array([[-1, 0, 2, 0, -1], [-4, 0, 8, 0, -4], [-6, 0, 12, 0, -6], [-4, 0, 8, 0, -4], [-1, 0, 2, 0, -1]], dtype=np.float64) / 64


def kernels(order, dtype=torch.float64, absolute=False):
    """[2,1,k,k]: (d_x, d_y) of order 1, (d_xx, d_yy) of order 2."""
    k = torch.from_numpy(KX if order == 1 else KXX)
    k = torch.stack([k, k.t()])[:, None].to(dtype)
    return k.abs() if absolute else k


def spatial_gradient(x, order, absolute=False):
    """[C,H,W] -> [C,2,H,W]: the contract's derivative in the dtype of x (absolute: |K| on |x|, the magnitude sum |K| |x| of a window)."""
    if absolute:
        x = x.abs()
    xp = F.pad(x[:, None], (order,) * 4, mode="replicate")
    return F.conv2d(xp, kernels(order, x.dtype, absolute))


def adjoint(G, order, absolute=False):
    """The adjoint of spatial_gradient applied to G [C,2,H,W] (fp64): [C,H,W].  The operator is linear, so autograd through it at 0 IS the
    adjoint -- the replicate padding's folds included."""
    x0 = torch.zeros(G.shape[0], G.shape[2], G.shape[3], dtype=torch.float64, requires_grad=True)
    xp = F.pad(x0[:, None], (order,) * 4, mode="replicate")
    y = F.conv2d(xp, kernels(order, torch.float64, absolute))
    return torch.autograd.grad(y, x0, G)[0]


def _rng(name):
    return np.random.default_rng(zlib.crc32(("smooth-" + name).encode()))


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def _mask(name, H, W, rng):
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "ones":
        m = np.ones((H, W))
    elif name == "zeros":
        m = np.zeros((H, W))
    elif name == "disc":
        m = ((yy - 0.5 * H) ** 2 + (xx - 0.45 * W) ** 2 <= (0.42 * min(H, W)) ** 2).astype(np.float64)
    elif name == "fractions":
        m = rng.uniform(0, 1, size=(H, W))
    elif name == "border_edge":          # zero on the outermost pixel of the top / left border and the two outermost of the bottom / right one
        m = np.zeros((H, W))
        m[1:H - 2, 1:W - 2] = 1
    else:
        raise KeyError(name)
    return m.astype(F32)[None]


def _plane(name, C, H, W, rng):
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "rand":
        return rng.uniform(-1, 1, size=(C, H, W)).astype(F32)
    if name == "rand64":                 # multiples of 1 / 64: a derivative that is exactly 0 in fp64 (one row, one column) is 0 in fp32 too
        return (np.round(64 * rng.uniform(-1, 1, size=(C, H, W))) / 64).astype(F32)
    if name == "flat":
        return np.full((C, H, W), 0.75, dtype=F32)
    if name == "step":                   # a vertical step edge on the tile border at x = 32
        return np.broadcast_to((xx >= TILE[1]).astype(F32) * F32(0.5) + F32(0.25), (C, H, W)).copy()
    if name == "plane":                  # a x + b y, dyadic: every second derivative of the interior is exactly 0
        return np.stack([(F32(0.25) * (c + 1)) * xx.astype(F32) - F32(0.5) * yy.astype(F32) for c in range(C)]).astype(F32)
    if name == "strong":                 # derivatives around 20: exp(-10 |g|) underflows in fp32
        return (160.0 * rng.uniform(-1, 1, size=(C, H, W))).astype(F32)
    raise KeyError(name)


def _term(kind, C, Ci=0, data="rand", img="rand", data_mask=None, img_mask=None, img_grad=False, share=None, poke=None):
    return dict(kind=kind, C=C, Ci=Ci, data=data, img=img, data_mask=data_mask, img_mask=img_mask, img_grad=img_grad, share=share, poke=poke)


def _cases():
    out = []

    def add(name, H, W, *terms):
        out.append(dict(id=f"{name}-{H}x{W}", H=H, W=W, terms=list(terms)))

    for i, (H, W) in enumerate(SIZES):   # every kind at every size, the channel pairs in turn, a differentiable img in each
        (c1, ci1), (c2, ci2) = PAIRS[i % 4], PAIRS[(i + 1) % 4]
        rnd = "rand64" if min(H, W) == 1 else "rand"
        add("sizes", H, W, _term("first", c1, ci1, data=rnd, img=rnd, img_grad=True), _term("second", c2, ci2, data=rnd, img=rnd, img_grad=bool(i % 2)),
            _term("tv", 1 + i % 3))
    add("four", 7, 31, _term("first", 4, 4, img_grad=True), _term("second", 4, 4, img_grad=True), _term("tv", 4))
    add("flat", 21, 70, _term("first", 3, 3, data="flat", img_grad=True), _term("second", 3, 1, data="flat"), _term("tv", 3, data="flat"),
        _term("first", 1, 3, img="flat", img_grad=True))
    add("step", 21, 70, _term("first", 3, 3, data="step", img_grad=True), _term("second", 1, 3, data="step"), _term("first", 3, 1, img="step", img_grad=True),
        _term("tv", 2, data="step"))
    add("plane", 21, 70, _term("second", 3, 3, data="plane"), _term("first", 3, 3, data="plane", img_grad=True), _term("second", 3, 1, img="plane", img_grad=True))
    add("masks", 21, 70, *[_term("first", 3, 3, data_mask=m, img_mask=m, img_grad=True) for m in ("ones", "zeros", "disc", "fractions")])
    add("mask_border", 21, 70, _term("first", 3, 3, data_mask="border_edge", img_mask="border_edge", img_grad=True),
        _term("second", 3, 3, data_mask="border_edge", img_mask="fractions", img_grad=True), _term("second", 1, 3, data_mask="disc"))
    add("shared", 9, 33, _term("first", 3, 3), _term("second", 1, 3, share=0))
    # the stage-2 launch (svgss.py:366-387): base colour and roughness against the masked ground truth, diffuse light against the rendered normal
    add("stage2", 21, 70, _term("first", 3, 3, data_mask="disc", img_mask="disc"), _term("first", 1, 3, data_mask="disc", img_mask="disc", share=0),
        _term("first", 3, 3, data_mask="disc", img_grad=True))
    add("light", 9, 33, _term("first", 3, 3, data_mask="disc", img_grad=True), _term("first", 1, 3, img_grad=True), _term("first", 3, 1, img_grad=True))
    add("strong", 21, 70, _term("second", 3, 3, img="strong", img_grad=True), _term("first", 3, 3, img="strong", img_grad=True))
    add("nan_data", 9, 33, _term("first", 3, 3, img_grad=True, poke=("data", np.nan)), _term("second", 3, 1, img_grad=True, poke=("data", np.nan)))
    add("nan_img", 9, 33, _term("first", 3, 3, img_grad=True, poke=("img", np.nan)), _term("second", 1, 3, img_grad=True, poke=("img", np.nan)))
    add("inf_img", 9, 33, _term("first", 3, 3, img_grad=True, poke=("img", np.inf)), _term("second", 3, 3, img_grad=True, poke=("img", np.inf)))
    add("envmap", 16, 32, _term("tv", 3))
    return out


CASES = _cases()
NONFINITE = ("nan_data", "nan_img", "inf_img")
POKE_AT = (4, 31)                       # row, column of the non-finite pixel (channel 1 where there is one): beside the tile border at x = 32


def build(case):
    """The terms of a CASES entry as fp32 arrays: a list of dict(kind, data [C,H,W], img [Ci,H,W] or None, data_mask, img_mask [1,H,W] or
    None, img_grad).  Terms that share an img hold the SAME array object."""
    H, W = case["H"], case["W"]
    out = []
    for k, t in enumerate(case["terms"]):
        rng = _rng(f"{case['id']}-{k}")
        d = dict(kind=t["kind"], img_grad=t["img_grad"], data=_plane(t["data"], t["C"], H, W, rng), img=None, data_mask=None, img_mask=None)
        if t["kind"] != "tv":
            d["img"] = out[t["share"]]["img"] if t["share"] is not None else _plane(t["img"], t["Ci"], H, W, rng)
            for m in ("data_mask", "img_mask"):
                if t[m] is not None:
                    d[m] = _mask(t[m], H, W, rng)
        if t["poke"] is not None:
            a = d[t["poke"][0]]
            a[min(1, a.shape[0] - 1), POKE_AT[0], POKE_AT[1]] = t["poke"][1]
        out.append(d)
    return out


# ---- the two evaluations -------------------------------------------------------------------------------------------------------------
def _tensors(term, dtype):
    return {k: None if term[k] is None else torch.from_numpy(term[k]).to(dtype) for k in ("data", "img", "data_mask", "img_mask")}


def counts(term):
    """(count_a, count_b) of the kernels' stats."""
    C, H, W = term["data"].shape
    if term["kind"] == "tv":
        return C * (H - 1) * W, C * H * (W - 1)
    return max(C, term["img"].shape[0]) * H * W, 0


def torch_eval(term, dtype=torch.float64):
    """The reference's own operation order in `dtype` with autograd: dict(loss, d_data, d_img (None without img)) -- floats / fp64 arrays.
    The mask products are formed in fp32 first, as the reference forms them on its fp32 tensors."""
    t = _tensors(term, torch.float32)
    data = t["data"].to(dtype).requires_grad_(True)
    if term["kind"] == "tv":
        loss = torch.square(data[..., 1:, :] - data[..., :-1, :]).mean() + torch.square(data[..., :, 1:] - data[..., :, :-1]).mean()
        g, = torch.autograd.grad(loss, data)     # (an empty mean, H or W = 1, is NaN and passes nothing back; the other mean's gradient flows)
        return dict(loss=float(loss.detach()), d_data=g.double().numpy(), d_img=None)
    img = t["img"].to(dtype).requires_grad_(True)
    D = data if t["data_mask"] is None else _masked(data, t["data_mask"])
    I = img if t["img_mask"] is None else _masked(img, t["img_mask"])   # noqa: E741
    order = 1 if term["kind"] == "first" else 2
    loss = (spatial_gradient(D, order).abs() * torch.exp(-SHARP[term["kind"]] * spatial_gradient(I, 1).abs())).sum(1).mean()
    gd, gi = torch.autograd.grad(loss, (data, img))
    return dict(loss=float(loss.detach()), d_data=gd.double().numpy(), d_img=gi.double().numpy())


class _MaskedProduct(torch.autograd.Function):
    """x * mask with the VALUE rounded once in fp32 (what the reference's fp32 product gives) whatever the dtype of x; gradient g * mask."""

    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return (x.float() * mask).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0].to(g.dtype), None


def _masked(x, mask):
    return _MaskedProduct.apply(x, mask)


def _dilate(b, h):
    """bool [C,H,W] -> the elements within h pixels (Chebyshev) of a set one."""
    return F.max_pool2d(b.double()[None], 2 * h + 1, stride=1, padding=h)[0] > 0


def oracle(term):
    """fp64 with the kernels' conventions: dict(loss, A, n, d_data, d_img, aabs_data, aabs_img, thr_data, thr_img, gd, gi) -- gradients for
    an upstream of 1 (they are linear in it); d_img / aabs_img / thr_img None for tv; thr_* bool arrays of the gradient's shape."""
    t = _tensors(term, torch.float32)
    data = t["data"]
    ca, cb = counts(term)
    if term["kind"] == "tv":
        x = data.double()
        ev, eh = x[:, 1:, :] - x[:, :-1, :], x[:, :, 1:] - x[:, :, :-1]
        sa, sb = float((ev * ev).sum()), float((eh * eh).sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            loss = float(np.float64(sa) / np.float64(ca) + np.float64(sb) / np.float64(cb))
        g, ab = torch.zeros_like(x), torch.zeros_like(x)
        for e, cnt, lo, hi in ((ev, ca, (slice(None), slice(0, -1)), (slice(None), slice(1, None))),
                               (eh, cb, (slice(None), slice(None), slice(0, -1)), (slice(None), slice(None), slice(1, None)))):
            if cnt > 0:
                e = torch.nan_to_num(e, nan=0.0) if torch.isnan(e).any() else e
                g[hi] += 2 * e / cnt; g[lo] -= 2 * e / cnt
                ab[hi] += 2 * e.abs() / cnt; ab[lo] += 2 * e.abs() / cnt
        return dict(loss=loss, A=abs(loss) if np.isfinite(loss) else np.nan, n=ca + cb, d_data=g.numpy(), d_img=None, aabs_data=ab.numpy(), aabs_img=None,
                    thr_data=np.zeros(x.shape, dtype=bool), thr_img=None, gd=None, gi=None)
    order, s = (1, 1.0) if term["kind"] == "first" else (2, 10.0)
    dm = t["data_mask"].double() if t["data_mask"] is not None else None
    im = t["img_mask"].double() if t["img_mask"] is not None else None
    D = (data if dm is None else data * t["data_mask"]).double()
    I = (t["img"] if im is None else t["img"] * t["img_mask"]).double()   # noqa: E741
    C, Ci = D.shape[0], I.shape[0]
    gd, gi = spatial_gradient(D, order), spatial_gradient(I, 1)
    w = torch.exp(-s * gi.abs())
    v = gd.abs() * w                                                       # [Cb,2,H,W]
    loss = float(v.sum() / ca)
    ok = ~torch.isnan(v)
    zero = torch.zeros((), dtype=torch.float64)
    on_c = lambda e: e if C == e.shape[0] else e.sum(0, keepdim=True)      # noqa: E731   the broadcast dimension folds back onto C = 1
    on_ci = lambda e: e if Ci == e.shape[0] else e.sum(0, keepdim=True)    # noqa: E731
    ew = torch.where(ok, w.expand_as(v), zero)
    eb = torch.where(ok, (s * v).expand_as(v), zero)
    sgn = lambda e: torch.nan_to_num(torch.sign(e), nan=0.0)          # noqa: E731
    d_data = adjoint(on_c(sgn(gd) * ew), order) / ca
    aabs_data = adjoint(on_c(sgn(gd).abs() * ew), order, absolute=True) / ca
    d_img = adjoint(on_ci(-sgn(gi) * eb), 1) / ca
    aabs_img = adjoint(on_ci(sgn(gi).abs() * eb), 1, absolute=True) / ca
    if dm is not None:
        d_data, aabs_data = d_data * dm, aabs_data * dm.abs()
    if im is not None:
        d_img, aabs_img = d_img * im, aabs_img * im.abs()
    thr_d = (gd.abs() > 0) & (gd.abs() < THRESHOLD * spatial_gradient(D, order, absolute=True))
    thr_i = (gi.abs() > 0) & (gi.abs() < THRESHOLD * spatial_gradient(I, 1, absolute=True))
    return dict(loss=loss, A=float(torch.where(ok, v, zero).sum() / ca), n=2 * ca, d_data=d_data.numpy(), d_img=d_img.numpy(),
                aabs_data=aabs_data.numpy(), aabs_img=aabs_img.numpy(), thr_data=_dilate(thr_d.any(1), order).numpy(),
                thr_img=_dilate(thr_i.any(1), 1).numpy(), gd=gd.numpy(), gi=gi.numpy(), thr_gd=thr_d.numpy(), thr_gi=thr_i.numpy())


def loss_bound(o64, e32):
    """4 E32 + n 2^-53 A."""
    return 4 * e32 + o64["n"] * 2.0 ** -53 * o64["A"]


def grad_bound(aabs, upstream=1.0):
    """4 G32 eps32 max(Aabs, AABS_FLOOR) per element, for an upstream gradient `upstream`."""
    return 4 * G32 * EPS32 * np.maximum(abs(upstream) * aabs, AABS_FLOOR)
