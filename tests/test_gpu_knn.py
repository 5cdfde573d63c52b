"""GPU tests of the exact nearest-neighbour search (csrc/knn.hip) through the two drop-in modules, `simple_knn._C.distCUDA2` and
`custom_knn._C.topKdistCUDA2`, on every case of tests/knn_cases.py.

No tolerance: the result is a pure function of the input (include/svgir_raster.h), the oracle is the same fp32 operations in numpy, so
the mean and the distances are compared as int32 views (that compares the +inf / FLT_MAX padding as well) and the indices exactly."""
import numpy as np
import pytest
import torch

from tests import knn_cases as kc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = sorted(kc.CASES)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _dev(name):
    return torch.from_numpy(kc.cloud(name).copy()).to(DEV)


def _run(pts):
    from custom_knn._C import topKdistCUDA2
    from simple_knn._C import distCUDA2
    mean = distCUDA2(pts)
    dist, idx = topKdistCUDA2(pts)
    return mean, dist, idx


def _check(got, name):
    mean, dist, idx = (t.cpu().numpy() for t in got)
    P = len(kc.cloud(name))
    omean, odist, oidx = kc.oracle(name)
    assert mean.shape == (P,) and mean.dtype == np.float32
    assert dist.shape == (P, 8) and dist.dtype == np.float32 and idx.shape == (P, 8) and idx.dtype == np.int32
    # (the poison: NaN in float outputs, -7 in integer outputs -- neither is a value of the contract)
    assert not np.isnan(mean).any() and not np.isnan(dist).any() and not (idx == -7).any()
    bad = np.flatnonzero(_bits(mean) != _bits(omean))
    assert bad.size == 0, f"{name}: mean differs at {bad[:5]}: {mean[bad[:5]]} vs {omean[bad[:5]]}"
    bad = np.flatnonzero((_bits(dist) != _bits(odist)).any(1) | (idx != oidx).any(1))
    assert bad.size == 0, f"{name}: row {bad[0]}: {dist[bad[0]]} {idx[bad[0]]} vs {odist[bad[0]]} {oidx[bad[0]]} ({bad.size} rows)"


@pytest.mark.parametrize("name", NAMES)
def test_case_is_bit_identical_to_the_oracle(built, name):
    pts = _dev(name)
    first = _run(pts)
    _check(first, name)
    second = _run(pts)   # same input, fresh scratch: same bits
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_empty_cloud(built):
    mean, dist, idx = _run(torch.zeros(0, 3, device=DEV))
    assert mean.shape == (0,) and dist.shape == (0, 8) and idx.shape == (0, 8)
    assert mean.dtype == torch.float32 and dist.dtype == torch.float32 and idx.dtype == torch.int32


@pytest.mark.parametrize("name", ["uniform_257", "lattice_16"])
def test_strided_fp64_input_equals_its_contiguous_fp32_copy(built, name):
    p = kc.cloud(name)
    wide = torch.zeros(len(p), 2, 5, dtype=torch.float64, device=DEV)
    view = wide[:, 1, 1:4]
    view.copy_(torch.from_numpy(p.copy()).to(DEV).double())
    assert not view.is_contiguous() and view.dtype == torch.float64
    _check(_run(view), name)


def test_cpu_tensor_raises(built):
    from custom_knn._C import topKdistCUDA2
    from simple_knn._C import distCUDA2
    p = torch.from_numpy(kc.cloud("uniform_64").copy())
    with pytest.raises(RuntimeError, match="no CPU path"):
        distCUDA2(p)
    with pytest.raises(RuntimeError, match="no CPU path"):
        topKdistCUDA2(p)


def test_knn_loss_arithmetic_stays_finite_with_padding(built):
    """get_knn_loss (scene/gaussian_model.py:577-592) on P = 4: five of the eight slots are padding, whose index is the row's own."""
    from custom_knn._C import topKdistCUDA2
    pts = _dev("uniform_4")
    dist2d, idx = topKdistCUDA2(pts)
    dist2d, idx = dist2d.reshape(-1, 8), idx.reshape(-1, 8)
    assert int(idx.min()) >= 0 and int(idx.max()) < 4
    assert torch.equal(idx[:, 3:].cpu(), torch.arange(4, dtype=torch.int32)[:, None].expand(4, 5))
    assert torch.isinf(dist2d[:, 3:]).all() and torch.isfinite(dist2d[:, :3]).all()
    g = torch.Generator().manual_seed(3)
    albedo, roughness = torch.rand(4, 3, generator=g).to(DEV), torch.rand(4, 1, generator=g).to(DEV)
    albedo_loss = torch.var(albedo[idx.long()], dim=1).mean()
    roughness_loss = torch.var(roughness[idx.long()], dim=1).mean()
    assert torch.isfinite(albedo_loss) and torch.isfinite(roughness_loss)


def test_side_stream_without_synchronisation(built):
    """Both calls on a non-default stream, consumed by the next kernel of that stream with no synchronisation in between."""
    name = "uniform_4097"
    pts = _dev(name)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        mean, dist, idx = _run(pts)
        mean2, dist2, idx2 = mean.clone(), dist.clone(), idx.clone()   # the next kernels of the stream
    side.synchronize()
    _check((mean2, dist2, idx2), name)
