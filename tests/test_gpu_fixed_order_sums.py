"""The fixed order of the image-space record reductions (csrc/wave.hpp: block_reduce_records / block_sum_ordered), pinned bit for bit.

Each of the six `*_reduce_kernel`s is one 256-thread workgroup: thread t adds columns of records t, t + 256, ... sequentially in double, every
wave runs the xor butterfly v = v + v[lane ^ d] for d = 32, 16, ..., 1, and the four wave totals combine as (w0 + w1) + (w2 + w3); then the
kernel's own epilogue.  The tests call the C entry points through ctypes as svgir_harness does, read the caller-owned `partial` buffer back,
redo exactly that in numpy and compare the final scalars as bit patterns -- at 1, 256 and more than 512 records.  psnr goes through the
device's log10 and stays with the tolerance tests of tests/test_gpu_view_metrics.py.  The last test holds csrc/ssim_tile.hpp: on a plain term
the per-tile SSIM record of svgir_view_metrics is svgir_l1_ssim_forward's per-tile SSIM partial, widened to double.  Inputs are finite (a
NaN's payload is not part of the contract)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RECORDS = (1, 256, 600)          # one record, exactly one per thread, more than two per thread


def _dev():
    return torch.device("cuda:0")


def _native():
    """The ctypes binding with every prototype set (svgir_harness.losses declares those of the l1_ssim and geometry-loss entry points)."""
    from gaussian_renderer import _native as N
    from svgir_harness import losses  # noqa: F401
    return N


def _rand(seed, *shape, lo=0.0, hi=1.0):
    return torch.from_numpy(np.random.default_rng(seed).uniform(lo, hi, size=shape).astype(np.float32)).to(_dev())


def _nan(shape, dtype=torch.float64):
    return torch.full(shape, float("nan"), dtype=dtype, device=_dev())


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same_bits(name, got, want):
    got, want = np.asarray(got), np.asarray(want, dtype=np.asarray(got).dtype)
    print(f"{name}: kernel {got.ravel()!r}, documented order {want.ravel()!r}")
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), name


def ordered_sum(records):
    """[n, N] records (float32 or float64) -> [N] float64: the documented order of one 256-thread workgroup."""
    rec = np.asarray(records).astype(np.float64)
    acc = np.zeros((256, rec.shape[1]))
    for base in range(0, rec.shape[0], 256):              # thread t: records t, t + 256, ... one after the other
        chunk = rec[base:base + 256]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    v = acc.reshape(4, 64, -1)                            # [wave, lane, column]
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ d]
    w = v[:, 0]
    return (w[0] + w[1]) + (w[2] + w[3])


@pytest.mark.parametrize("n", RECORDS)
def test_l1_ssim_means(built, n):
    N = _native()
    Cc, H, W = 1, 16, 16 * n
    a, b = _rand(1, Cc, H, W), _rand(2, Cc, H, W)
    nblk = N.lib.svgir_l1_ssim_partials(Cc, H, W)
    assert nblk == n
    partial, means = _nan((nblk, 2), torch.float32), _nan((2,), torch.float32)
    N.check(N.lib.svgir_l1_ssim_forward(a.data_ptr(), b.data_ptr(), Cc, H, W, partial.data_ptr(), None, means.data_ptr(), N.stream_ptr(_dev())),
            "l1_ssim_forward")
    s = ordered_sum(partial.cpu().numpy())
    inv = 1.0 / (float(Cc) * float(H) * float(W))
    _same_bits("ssim and l1 means", means.cpu().numpy(), np.float32(s * inv))


@pytest.mark.parametrize("P", (200, 256 * 256, 256 * 256 + 1, 256 * 600 - 17))
def test_activation_sum_and_mean(built, P):
    N = _native()
    normal = _rand(3, P, 12, lo=-1.0)
    nblk = N.lib.svgir_activate_partials(P)
    assert nblk == (P + 255) // 256
    partial, total, mean = _nan((nblk,)), _nan((1,)), _nan((1,), torch.float32)
    a = N.Activation()
    a.P, a.normal = P, normal.data_ptr()
    a.partial, a.normal_reg_sum, a.normal_reg = partial.data_ptr(), total.data_ptr(), mean.data_ptr()
    N.check(N.lib.svgir_activate_forward(C.byref(a), N.stream_ptr(_dev())), "activate_forward")
    s = ordered_sum(partial.cpu().numpy()[:, None])
    _same_bits("normal_reg_sum", total.cpu().numpy(), s)
    _same_bits("normal_reg", mean.cpu().numpy(), np.float32(s / (12.0 * float(P))))


@pytest.mark.parametrize("n", RECORDS)
def test_geometry_stats_and_losses(built, n):
    N = _native()
    import image_cases as ic
    H, W = 8, 32 * n                                       # 32 x 8 pixel tiles
    v = np.random.default_rng(4).standard_normal((2, 3, H, W))
    unit = torch.from_numpy((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)).to(_dev())
    depth, opacity = _rand(5, 1, H, W, lo=1.0, hi=2.0), _rand(7, 1, H, W, lo=0.02, hi=0.98)
    mask = ((_rand(6, 1, H, W) < 0.7) & (torch.arange(W, device=_dev()) % 32 >= 16)).float()   # (bands of zeros wider than the 9 x 9 pool)
    nblk = N.lib.svgir_geometry_loss_partials(W, H)
    assert nblk == n
    partial, stats, losses = _nan((nblk, 8)), _nan((4, 2)), _nan((4,), torch.float32)
    N.check(N.lib.svgir_geometry_loss_forward(W, H, 15, unit[0].data_ptr(), depth.data_ptr(), mask.data_ptr(), opacity.data_ptr(),
                                              unit[1].data_ptr(), None, ic.FOVX, ic.FOVY, 0.5, 0.5, partial.data_ptr(), stats.data_ptr(),
                                              losses.data_ptr(), N.stream_ptr(_dev())), "geometry_loss_forward")
    p = partial.cpu().numpy()
    assert not p[:, 5].any() and not p[:, 7].any()
    s = ordered_sum(p)
    want = np.array([[s[0], s[1]], [s[2], s[3]], [s[4], float(W) * float(H)], [s[6], float(W) * float(H)]])
    _same_bits("geometry stats", stats.cpu().numpy(), want)
    _same_bits("geometry losses", losses.cpu().numpy(), np.float32(want[:, 0] / want[:, 1]))


@pytest.mark.parametrize("n", RECORDS)
def test_smoothness_stats_and_losses(built, n):
    N = _native()
    H, W = 8, 32 * n                                       # 32 x 8 pixel tiles
    data, img = _rand(8, 3, H, W), _rand(9, 3, H, W)
    arr = (N.SmoothTerm * 2)()
    arr[0].kind, arr[0].C, arr[0].Ci, arr[0].data, arr[0].img = 1, 3, 3, data.data_ptr(), img.data_ptr()   # first order, edge aware
    arr[1].kind, arr[1].C, arr[1].Ci, arr[1].data = 3, 3, 0, data.data_ptr()                                 # tv
    assert N.lib.svgir_smooth_loss_partials(W, H, 2) == 2 * n
    partial, stats, losses = _nan((2, n, 2)), _nan((2, 4)), _nan((2,), torch.float32)
    N.check(N.lib.svgir_smooth_loss_forward(W, H, 2, arr, partial.data_ptr(), stats.data_ptr(), losses.data_ptr(), N.stream_ptr(_dev())),
            "smooth_loss_forward")
    p = partial.cpu().numpy()
    first, tv = ordered_sum(p[0]), ordered_sum(p[1])
    ca, ra, rb = 3.0 * H * W, 3.0 * (H - 1.0) * W, 3.0 * H * (W - 1.0)
    _same_bits("smoothness stats", stats.cpu().numpy(), np.array([[first[0], ca, 0.0, 0.0], [tv[0], ra, tv[1], rb]]))
    _same_bits("smoothness losses", losses.cpu().numpy(), np.array([np.float32(first[0] / ca), np.float32(tv[0] / ra + tv[1] / rb)]))


@pytest.mark.parametrize("W", (63, 256 * 64, 600 * 64 - 1))
def test_albedo_scale_and_count(built, W):
    N = _native()
    H = 16                                                 # 1024 pixels per workgroup
    render, gt = _rand(10, 3, H, W, lo=-0.3), _rand(11, 3, H, W)
    nblk = N.lib.svgir_albedo_scale_partials(W, H) // 4
    assert nblk == (H * W + 1023) // 1024
    partial, scale, count = _nan((nblk, 4)), _nan((3,), torch.float32), torch.full((1,), -7, dtype=torch.int32, device=_dev())
    N.check(N.lib.svgir_albedo_scale(W, H, render.data_ptr(), gt.data_ptr(), 0, partial.data_ptr(), scale.data_ptr(), count.data_ptr(),
                                     N.stream_ptr(_dev())), "albedo_scale")
    s = ordered_sum(partial.cpu().numpy())
    _same_bits("albedo scale", scale.cpu().numpy(), np.float32(s[:3] / s[3]))
    assert int(count.cpu()[0]) == int(s[3]) > 0


def _metrics(N, terms, H, W):
    """svgir_view_metrics on plain [3,H,W] operand pairs [(a, b, want_ssim)]: (partial [n,3,tiles,3], rows [n,10])."""
    n = len(terms)
    arr = (N.MetricTerm * n)()
    for k, (a, b, want) in enumerate(terms):
        for op, t in ((arr[k].a, a), (arr[k].b, b)):
            op.src, op.scale, op.offset = t.data_ptr(), 1.0, 0.0
        arr[k].want_ssim = int(want)
    tiles = ((H + 15) // 16) * ((W + 15) // 16)
    assert N.lib.svgir_view_metrics_partials(W, H, n) == n * 3 * tiles * 3
    partial, rows = _nan((n, 3, tiles, 3)), _nan((n, 10))
    N.check(N.lib.svgir_view_metrics(W, H, n, arr, partial.data_ptr(), rows.data_ptr(), N.stream_ptr(_dev())), "view_metrics")
    return partial.cpu().numpy(), rows.cpu().numpy()


@pytest.mark.parametrize("n", RECORDS)
def test_metrics_row(built, n):
    N = _native()
    H, W = 16, 16 * n
    a, b = _rand(12, 3, H, W), _rand(13, 3, H, W)
    partial, rows = _metrics(N, [(a, b, True), (b, a, False)], H, W)
    HW = float(W) * float(H)
    for k, want_ssim in enumerate((True, False)):
        s = np.stack([ordered_sum(partial[k, c]) for c in range(3)])    # [channel, (d^2, |d|, ssim)]
        mse = s[:, 0] / HW
        _same_bits(f"term {k} mse", rows[k, 0:3], mse)
        _same_bits(f"term {k} mean mse", rows[k, 6], ((mse[0] + mse[1]) + mse[2]) / 3.0)
        _same_bits(f"term {k} l1", rows[k, 9], ((s[0, 1] + s[1, 1]) + s[2, 1]) / (3.0 * HW))
        if want_ssim:
            _same_bits(f"term {k} ssim", rows[k, 8], ((s[0, 2] + s[1, 2]) + s[2, 2]) / (3.0 * HW))
        else:
            assert np.isnan(rows[k, 8]) and not partial[k, :, :, 2].any()


@pytest.mark.parametrize("H,W", ((21, 37), (16, 16)))
def test_plain_metric_tile_is_the_loss_tile(built, H, W):
    N = _native()
    a, b = _rand(14, 3, H, W), _rand(15, 3, H, W)
    partial, _ = _metrics(N, [(a, b, True)], H, W)
    nblk = N.lib.svgir_l1_ssim_partials(3, H, W)
    lp = _nan((nblk, 2), torch.float32)
    N.check(N.lib.svgir_l1_ssim_forward(a.data_ptr(), b.data_ptr(), 3, H, W, lp.data_ptr(), None, None, N.stream_ptr(_dev())), "l1_ssim_forward")
    _same_bits("per-tile SSIM sums", partial[0, :, :, 2].reshape(-1), lp.cpu().numpy()[:, 0].astype(np.float64))
