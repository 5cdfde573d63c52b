"""The tail of an eval view, fused (csrc/view_metrics.hip): MSE / PSNR / SSIM / L1 rows of composed image pairs (`view_metrics`, the
drop-ins `mse` and `psnr` for utils/image_utils.py:32-37), the 8-bit arrays that get written as images (`captures_u8`: what torchvision's
save_image hands to PIL), the albedo scale of the relighting eval (`albedo_scale`: eval_relighting_tensoIR.py:285-294, the variant the
reference never uses; `albedo_scale_median`: :227-237, the one it applies, on the exact median of csrc/select.hip, which `column_median`
exposes as a drop-in for torch.median(x, dim=0)) and the whole tail of one relighting frame (`relighting_frame`: :333-378).  Nothing here waits for the device: every result is a device tensor, a metrics row
can be written straight into row v of the [views, terms, 10] table that `view_parallel.run_views` gathers at the end."""
import ctypes as C

import torch

from gaussian_renderer import _native as N

MAX_TERMS = 4       # SVGIR_METRIC_MAX_TERMS
CAPTURE_MAX = 16    # SVGIR_CAPTURE_MAX
COLS = ("mse_0", "mse_1", "mse_2", "psnr_0", "psnr_1", "psnr_2", "mse", "psnr", "ssim", "l1")   # SVGIR_METRIC_COLS = 10
# what the reference's capture loop composites over the background (eval_relighting_tensoIR.py:337); every other name is saved as it is
MASKED_CAPTURES = ("roughness", "diffuse", "specular", "lights", "local_lights", "global_lights", "visibility", "direct")


class Plane:
    """A plane operand (svgir_plane_op): how a [3,H,W] image is formed per pixel from the tensors the caller holds; see `plane`."""
    __slots__ = ("src", "mask", "fill", "bg", "scale", "offset", "srgb")

    def __init__(self, src, mask, fill, bg, scale, offset, srgb):
        self.src, self.mask, self.fill, self.bg, self.scale, self.offset, self.srgb = src, mask, fill, bg, scale, offset, srgb

    @property
    def size(self):
        return int(self.src.shape[-2]), int(self.src.shape[-1])


def _gpu(t, what):
    if not torch.is_tensor(t):
        raise TypeError(f"metrics: {what} must be a tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"metrics: {what} must live on the GPU (libsvgir_raster.so has no CPU path)")
    return t


def _bg3(bg):
    """Three host floats from a number, a sequence of three, or a CPU tensor ([3], [3,1,1] or one element)."""
    if bg is None:
        return (0.0, 0.0, 0.0)
    if torch.is_tensor(bg):
        if bg.device.type != "cpu":
            raise RuntimeError("metrics: bg is read on the host: pass numbers or a CPU tensor (a device tensor would need a host wait); "
                               "a per-pixel background goes into fill")
        bg = bg.reshape(-1).tolist()
    elif not isinstance(bg, (tuple, list)):
        bg = [float(bg)]
    bg = [float(v) for v in bg]
    if len(bg) == 1:
        bg = bg * 3
    if len(bg) != 3:
        raise ValueError(f"metrics: bg must be one number or three, got {len(bg)}")
    return tuple(bg)


def plane(src, mask=None, bg=None, fill=None, scale=1.0, offset=0.0, srgb=False):
    """The operand  srgb?( (src * scale + offset) * mask + (1 - mask) * (fill | bg) ), formed in fp32 in torch's operation order inside
    the kernels (never stored).  src [3,H,W] (a [1,H,W] plane is repeated to three channels, as torchvision's make_grid does before
    an image is saved); mask [1,H,W] or [H,W]; fill [3,H,W] or bg (a number, three numbers, a CPU tensor: host values); the affine is
    skipped when scale == 1 and offset == 0; srgb: utils/graphics_utils.py `rgb_to_srgb` last."""
    src = _gpu(src, "src")
    if src.dim() != 3 or src.shape[0] not in (1, 3):
        raise ValueError(f"metrics: src must be [3,H,W] (or [1,H,W]), got {tuple(src.shape)}")
    dev = src.device
    H, W = int(src.shape[1]), int(src.shape[2])
    if src.shape[0] == 1:
        src = src.expand(3, H, W)
    src = N.f32c(src.detach(), dev)
    if mask is not None:
        mask = _gpu(mask, "mask")
        if tuple(mask.shape) not in ((1, H, W), (H, W)):
            raise ValueError(f"metrics: mask must be [1,{H},{W}], got {tuple(mask.shape)}")
        mask = N.f32c(mask.detach(), dev)
    if fill is not None:
        fill = _gpu(fill, "fill")
        if tuple(fill.shape) != (3, H, W):
            raise ValueError(f"metrics: fill must be [3,{H},{W}], got {tuple(fill.shape)}")
        fill = N.f32c(fill.detach(), dev)
    return Plane(src, mask, fill, _bg3(bg), float(scale), float(offset), bool(srgb))


def _as_plane(p):
    return p if isinstance(p, Plane) else plane(p)


def _fill_op(op, p):
    op.src, op.mask, op.fill = p.src.data_ptr(), N.ptr(p.mask), N.ptr(p.fill)
    op.bg[0], op.bg[1], op.bg[2] = p.bg
    op.scale, op.offset, op.srgb = p.scale, p.offset, int(p.srgb)


def _same_size(planes, what):
    size, dev = planes[0].size, planes[0].src.device
    for p in planes:
        if p.size != size or p.src.device != dev:
            raise ValueError(f"{what}: every operand of a launch must have one image size and one device, got {p.size} and {size}")
    return size[0], size[1], dev


def view_metrics(terms, out=None):
    """Rows of COLS = (mse_0, mse_1, mse_2, psnr_0, psnr_1, psnr_2, mean mse, mean psnr, ssim, l1) for up to 4 terms of one image size
    from one call (one launch for the terms with SSIM, one for those without, one small reduction).  terms: [(a, b, want_ssim)] or
    [(a, b)] (SSIM wanted), a / b a `plane(...)` or a plain [3,H,W] tensor.  Returns float64 [n,10] on the device; `out`: a contiguous
    float64 [n,10] device view to write instead (a row of a caller's table; nothing else of the table is touched).  mse_c, psnr_c are
    utils/image_utils.py:32-37 per channel, evaluated in double from the fp32 differences; psnr is +inf where the mse is exactly 0;
    ssim is NaN where it was not wanted."""
    terms = [tuple(t) for t in terms]
    n = len(terms)
    pairs = [(_as_plane(t[0]), _as_plane(t[1])) for t in terms]
    if not pairs:
        raise ValueError("view_metrics: no term given")
    H, W, dev = _same_size([p for pair in pairs for p in pair], "view_metrics")
    arr = (N.MetricTerm * n)()
    for k, (t, (a, b)) in enumerate(zip(terms, pairs)):
        _fill_op(arr[k].a, a)
        _fill_op(arr[k].b, b)
        arr[k].want_ssim = int(bool(t[2])) if len(t) > 2 else 1
    with torch.cuda.device(dev):
        if out is None:
            out = N.out_tensor((n, len(COLS)), torch.float64, dev)
        elif (out.dtype != torch.float64 or out.device != dev or tuple(out.shape) != (n, len(COLS)) or not out.is_contiguous()):
            raise ValueError(f"view_metrics: out must be a contiguous float64 [{n},{len(COLS)}] tensor on {dev}")
        partial = torch.empty(max(N.lib.svgir_view_metrics_partials(W, H, n), 1), dtype=torch.float64, device=dev)
        N.check(N.lib.svgir_view_metrics(W, H, n, arr, partial.data_ptr(), out.data_ptr(), N.stream_ptr(dev)), "view_metrics")
    return out


def _pair3(img1, img2, what):
    for t in (img1, img2):
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[0] != 3:
            raise ValueError(f"{what}: only [3,H,W] images are implemented, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    return view_metrics([(img1, img2, False)])


def mse(img1, img2):
    """Drop-in for utils/image_utils.py:32: the per-channel mean squared error, [3,1] fp32 on the device."""
    return _pair3(img1, img2, "mse")[0, 0:3].to(torch.float32).reshape(3, 1)


def psnr(img1, img2):
    """Drop-in for utils/image_utils.py:36: 20 log10(1 / sqrt(mse)) per channel, [3,1] fp32 on the device (no host wait: the
    reference's callers take `.mean()` of it)."""
    return _pair3(img1, img2, "psnr")[0, 3:6].to(torch.float32).reshape(3, 1)


def captures_u8(planes):
    """uint8 [n,H,W,3]: for each of up to 16 operands the array torchvision's save_image hands to PIL,
    (x * 255 + 0.5).clamp(0, 255).to(uint8) in HWC order (restated from torchvision's source; unpinned by torchvision itself), in one
    launch.  NaN gives 0.  Operands with srgb are refused by the library (no byte contract holds against torch's pow)."""
    planes = [_as_plane(p) for p in planes]
    if not planes:
        raise ValueError("captures_u8: no operand given")
    H, W, dev = _same_size(planes, "captures_u8")
    n = len(planes)
    arr = (N.PlaneOp * n)()
    for k, p in enumerate(planes):
        _fill_op(arr[k], p)
    with torch.cuda.device(dev):
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        if N.POISON:
            out.fill_(0xA5)
        N.check(N.lib.svgir_capture_u8(W, H, n, arr, out.data_ptr(), N.stream_ptr(dev)), "capture_u8")
    return out


def albedo_scale(render_albedo, gt_albedo, gt_srgb=False):
    """eval_relighting_tensoIR.py:285-294: over the pixels where render_albedo.mean(dim=0) > 0, the per-channel mean of
    (gt / render).clamp(1e-6, 1); gt_srgb=True applies rgb_to_srgb to gt_albedo first (:289).  Returns (scale [3] fp32, count [1] int32),
    both on the device: the scale goes into `activations.activate(..., base_color_scale=)` as it is.  An empty selection gives NaN and 0."""
    r, g = _gpu(render_albedo, "render_albedo"), _gpu(gt_albedo, "gt_albedo")
    if r.dim() != 3 or r.shape[0] != 3 or tuple(g.shape) != tuple(r.shape):
        raise ValueError(f"albedo_scale: both images must be [3,H,W] of one size, got {tuple(r.shape)} and {tuple(g.shape)}")
    dev = r.device
    r, g = N.f32c(r.detach(), dev), N.f32c(g.detach(), dev)
    H, W = int(r.shape[1]), int(r.shape[2])
    with torch.cuda.device(dev):
        partial = torch.empty(max(N.lib.svgir_albedo_scale_partials(W, H), 1), dtype=torch.float64, device=dev)
        scale = N.out_tensor((3,), torch.float32, dev)
        count = N.out_tensor((1,), torch.int32, dev)
        N.check(N.lib.svgir_albedo_scale(W, H, r.data_ptr(), g.data_ptr(), int(bool(gt_srgb)), partial.data_ptr(), scale.data_ptr(),
                                         count.data_ptr(), N.stream_ptr(dev)), "albedo_scale")
    return scale, count


SELECT_ROWS = 2048    # rows per workgroup of csrc/select.hip (SEL_ROWS = BLOCK * SEL_PER_THREAD): the tests put their sizes around it
MEDIAN_MAX_COLUMNS = 4


def column_median(x, with_counts=False):
    """Drop-in for `torch.median(x, dim=0)` on a 2-D fp32 device tensor [n, C] of ANY strides, C = 1 ... 4 (a planar [C, n] goes in as
    `planes.t()`): (values [C] fp32, indices [C] int64), both on the device, from csrc/select.hip's radix select -- no sort, no host wait.
    The value is the lower median, bit for bit an element of the column; -0 and +0 are one value and come out as +0; a NaN in a column
    gives NaN; the index is the SMALLEST row holding the value (torch leaves ties open), in a NaN column the first NaN row; n == 0 gives
    NaN and -1 (torch raises).  with_counts=True adds (n_less [C], n_greater [C]) int32: the rows strictly below / above the value."""
    x = _gpu(x, "x")
    if x.dim() != 2 or x.dtype != torch.float32 or not 1 <= x.shape[1] <= MEDIAN_MAX_COLUMNS:
        raise ValueError(f"column_median: x must be a 2-D float32 tensor [n, 1 ... {MEDIAN_MAX_COLUMNS}], got "
                         f"{x.dtype} {tuple(x.shape)}")
    dev = x.device
    x = x.detach()
    n, Cn = int(x.shape[0]), int(x.shape[1])
    with torch.cuda.device(dev):
        scratch = N.out_tensor((max(N.lib.svgir_column_median_scratch_bytes(n, Cn) // 4, 1),), torch.int32, dev)
        values = N.out_tensor((Cn,), torch.float32, dev)
        idx, less, greater = (N.out_tensor((Cn,), torch.int32, dev) for _ in range(3))
        N.check(N.lib.svgir_column_median(N.ptr(x), n, Cn, x.stride(0), x.stride(1), scratch.data_ptr(), values.data_ptr(), idx.data_ptr(),
                                          less.data_ptr(), greater.data_ptr(), N.stream_ptr(dev)), "column_median")
    res = (values, idx.to(torch.int64))
    return res + (less, greater) if with_counts else res


def albedo_scale_median(render_albedo, gt_albedo, lo=1e-6, hi=10.0, render_srgb=True):
    """eval_relighting_tensoIR.py:227-237, the albedo scale the relighting eval applies: over the pixels where
    srgb_to_rgb(render_albedo).mean(dim=0) > 0, the per-channel MEDIAN of (gt_albedo / srgb_to_rgb(render_albedo)).clamp(lo, hi);
    render_srgb=False takes render_albedo as it is.  Returns (scale [3] fp32, count [1] int32), both on the device: the scale goes into
    `activations.activate(..., base_color_scale=)` as it is.  An empty selection gives NaN and 0.  (`albedo_scale` is the mean variant
    of :285-294, which the reference computes and never uses.)"""
    r, g = _gpu(render_albedo, "render_albedo"), _gpu(gt_albedo, "gt_albedo")
    if r.dim() != 3 or r.shape[0] != 3 or tuple(g.shape) != tuple(r.shape):
        raise ValueError(f"albedo_scale_median: both images must be [3,H,W] of one size, got {tuple(r.shape)} and {tuple(g.shape)}")
    dev = r.device
    r, g = N.f32c(r.detach(), dev), N.f32c(g.detach(), dev)
    H, W = int(r.shape[1]), int(r.shape[2])
    with torch.cuda.device(dev):
        scratch = N.out_tensor((max(N.lib.svgir_albedo_scale_median_scratch_bytes(W, H) // 4, 1),), torch.int32, dev)
        scale = N.out_tensor((3,), torch.float32, dev)
        count = N.out_tensor((1,), torch.int32, dev)
        N.check(N.lib.svgir_albedo_scale_median(W, H, r.data_ptr(), g.data_ptr(), int(bool(render_srgb)), float(lo), float(hi),
                                                scratch.data_ptr(), scale.data_ptr(), count.data_ptr(), N.stream_ptr(dev)), "albedo_scale_median")
    return scale, count


def _captured(render_pkg, name, mask, bg):
    """The operand the reference's capture loop saves for `name` (eval_relighting_tensoIR.py:333-346)."""
    if name == "normal":
        return plane(render_pkg["normal"], mask=mask, bg=bg, scale=0.5, offset=0.5)
    if name in MASKED_CAPTURES or name == "pbr":
        return plane(render_pkg[name], mask=mask, bg=bg)
    if name == "pbr_env":   # (the raw pbr: see relighting_frame)
        return plane(render_pkg["pbr"], mask=mask, fill=render_pkg["env_only"])
    return plane(render_pkg[name])


def relighting_frame(render_pkg, gt_image, gt_albedo, gt_normal, mask, bg, capture_list):
    """The tail of one frame of eval_relighting_tensoIR.py:333-378: ONE captures_u8 launch and ONE view_metrics call with three terms.
    Returns ({name: uint8 [H,W,3]}, rows float64 [3,10]): the images of `capture_list` plus "gt" (gt_image over the background, :348-349),
    and the metric rows of  pbr vs gt,  base_color vs srgb(gt_albedo over the background),  normal vs gt_normal over the background
    (SSIM for the first two).  The metrics see the planes as the reference's loop leaves them in render_pkg: composited over the
    background when they were captured, the normal after `* 0.5 + 0.5`.  render_pkg itself is not modified.
    One deviation: "pbr_env" composites the RAW pbr over env_only; the reference composites the pbr its loop has already composited
    over bg when "pbr" comes first in the list -- equal for a binary mask.  bg: a number or three (host values)."""
    names = list(capture_list)
    ops = [_captured(render_pkg, k, mask, bg) for k in names]
    gt = plane(gt_image, mask=mask, bg=bg)
    u8 = captures_u8(ops + [gt])
    images = {k: u8[i] for i, k in enumerate(names)}
    images["gt"] = u8[len(names)]
    seen = lambda k: _captured(render_pkg, k, mask, bg) if k in names else plane(render_pkg[k])   # noqa: E731
    rows = view_metrics([(seen("pbr"), gt, True),
                         (plane(render_pkg["base_color"]), plane(gt_albedo, mask=mask, bg=bg, srgb=True), True),
                         (seen("normal"), plane(gt_normal, mask=mask, bg=bg), False)])
    return images, rows


# ---- LPIPS (csrc/lpips.hip) ------------------------------------------------------------------------------------------------------------
VGG_CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)   # the convolutions of torchvision's vgg16().features up to relu5_3
VGG_CONV_SHAPE = ((64, 3), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256), (512, 512), (512, 512),
                  (512, 512), (512, 512), (512, 512))               # (Cout, Cin)
LPIPS_TAP_CHANNELS = (64, 128, 256, 512, 512)                       # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
LPIPS_MIN_SIZE = 16


def _state(s, what):
    if isinstance(s, (str, bytes)) or hasattr(s, "__fspath__"):
        s = torch.load(s, map_location="cpu", weights_only=True)
    if not hasattr(s, "keys"):
        raise TypeError(f"LPIPS: {what} must be a state dict or a path to one, got {type(s).__name__}")
    return s


def _pick(state, names, shape, what, squeeze=False):
    """state[first of `names` present], which must have exactly `shape` (squeeze: after dropping dimensions of size 1)."""
    for k in names:
        if k in state:
            t = state[k].detach()
            got = tuple(d for d in t.shape if d != 1) if squeeze else tuple(t.shape)
            if got != tuple(shape):
                raise ValueError(f"LPIPS: {what} '{k}' has shape {tuple(t.shape)}, expected {tuple(shape)}")
            return t.reshape(shape)
    raise KeyError(f"LPIPS: {what} has none of the keys {names}")


class LPIPS:
    """lpipsPyTorch's `LPIPS('vgg')` on the HIP kernels.  vgg_state: the state dict of torchvision's vgg16 (keys `features.N.weight` /
    `.bias`) or of its `.features` (`N.weight`), or a path to one; lin_state: the LPIPS linear layers as published (`linK.model.1.weight`)
    or as lpipsPyTorch renames them (`K.1.weight`), or a path.  Nothing is downloaded.  The weights are packed once per device, on first
    use there.  `net(x, y)`: x, y [3,H,W] or [1,3,H,W] device tensors in [0, 1] -> the reference's [1,1,1,1] fp32 device tensor."""

    def __init__(self, vgg_state, lin_state):
        vgg, lin = _state(vgg_state, "vgg_state"), _state(lin_state, "lin_state")
        self._w, self._b, self._lin = [], [], []
        for i, (co, ci) in zip(VGG_CONV_INDEX, VGG_CONV_SHAPE):
            self._w.append(_pick(vgg, (f"features.{i}.weight", f"{i}.weight"), (co, ci, 3, 3), "vgg_state").to("cpu", torch.float32))
            self._b.append(_pick(vgg, (f"features.{i}.bias", f"{i}.bias"), (co,), "vgg_state").to("cpu", torch.float32))
        for k, c in enumerate(LPIPS_TAP_CHANNELS):
            self._lin.append(_pick(lin, (f"lin{k}.model.1.weight", f"{k}.1.weight"), (c,), "lin_state", squeeze=True).to("cpu", torch.float32))
        self._packed = {}

    def packed(self, dev):
        """The kernels' weight block on `dev` (packed on first use)."""
        dev = torch.device(dev)
        if dev.type != "cuda":
            raise RuntimeError("LPIPS: the kernels run on the GPU only (libsvgir_raster.so has no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._packed:
            with torch.cuda.device(dev):
                src = [t.to(dev).contiguous() for t in self._w + self._b + self._lin]
                arrs = []
                for part in (src[:13], src[13:26], src[26:]):
                    arrs.append((C.c_void_p * len(part))(*[t.data_ptr() for t in part]))
                out = N.out_tensor((N.lib.svgir_lpips_packed_floats(),), torch.float32, dev)
                N.check(N.lib.svgir_lpips_pack(arrs[0], arrs[1], arrs[2], out.data_ptr(), N.stream_ptr(dev)), "lpips_pack")
                for t in src:   # the pack kernels read them on this stream after we return
                    t.record_stream(torch.cuda.current_stream(dev))
            self._packed[dev] = out
        return self._packed[dev]

    def __call__(self, x, y):
        return lpips_terms(self, [(_image3(x, "x"), _image3(y, "y"))]).reshape(1, 1, 1, 1)


def _image3(t, what):
    """[3,H,W] from a [3,H,W] or [1,3,H,W] device tensor."""
    if not torch.is_tensor(t):
        raise TypeError(f"lpips: {what} must be a tensor, got {type(t).__name__}")
    if t.dim() == 4:
        if t.shape[0] != 1:
            raise ValueError(f"lpips: {what} has a batch of {t.shape[0]}; one image per call (the reference sums a batch into one number, "
                             f"which is not reproduced) -- use metrics.lpips_terms for several pairs")
        t = t[0]
    if t.dim() != 3 or t.shape[0] != 3:
        raise ValueError(f"lpips: {what} must be [3,H,W] or [1,3,H,W], got {tuple(t.shape)}")
    _gpu(t, what)
    return t


def lpips_terms(net, pairs, out=None, with_taps=False, tap_maps=False):
    """LPIPS scores of up to 4 pairs of one image size from one batched pass (23 launches whatever the count).  pairs: [(a, b)], a / b a
    `plane(...)` operand or a plain [3,H,W] device tensor, values as the reference passes them (in [0, 1]).  Returns float32 [n] on the
    device (`out`: a contiguous float32 [n] device view to write instead); with_taps=True: (scores, taps [n,5]), the per-layer terms whose
    sum the score is; tap_maps=True (tests): additionally the five tapped feature maps, [2 n, C_k, H_k, W_k] each, image 2 p = a of pair p.
    A pair's bits do not depend on the other pairs of the call."""
    pairs = list(pairs)
    n = len(pairs)
    if not 1 <= n <= MAX_TERMS:
        raise ValueError(f"lpips_terms: {n} pairs given, 1 ... {MAX_TERMS} per call")
    ops = [(_as_plane(a), _as_plane(b)) for a, b in pairs]
    H, W, dev = _same_size([p for pair in ops for p in pair], "lpips_terms")
    if H < LPIPS_MIN_SIZE or W < LPIPS_MIN_SIZE:
        raise ValueError(f"lpips_terms: image {H} x {W} is smaller than {LPIPS_MIN_SIZE} x {LPIPS_MIN_SIZE}: relu5_3 would be empty")
    arr = (N.LpipsPair * n)()
    for k, (a, b) in enumerate(ops):
        _fill_op(arr[k].a, a)
        _fill_op(arr[k].b, b)
    packed = net.packed(dev)
    with torch.cuda.device(dev):
        if out is None:
            out = N.out_tensor((n,), torch.float32, dev)
        elif out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (n,) or not out.is_contiguous():
            raise ValueError(f"lpips_terms: out must be a contiguous float32 [{n}] tensor on {dev}")
        taps = N.out_tensor((n, 5), torch.float32, dev)
        work = N.out_tensor((N.lib.svgir_lpips_work_bytes(W, H, n) // 4,), torch.float32, dev)
        maps, mp = None, None
        if tap_maps:
            maps = [N.out_tensor((2 * n, c, H >> k, W >> k), torch.float32, dev) for k, c in enumerate(LPIPS_TAP_CHANNELS)]
            mp = (C.c_void_p * 5)(*[m.data_ptr() for m in maps])
        N.check(N.lib.svgir_lpips(W, H, n, arr, packed.data_ptr(), work.data_ptr(), taps.data_ptr(), out.data_ptr(), mp,
                                  N.stream_ptr(dev)), "lpips")
    res = (out,)
    if with_taps:
        res += (taps,)
    if tap_maps:
        res += (maps,)
    return res[0] if len(res) == 1 else res
