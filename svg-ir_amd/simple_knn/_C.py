"""Drop-in replacement of the reference's CUDA / cub / thrust extension `simple_knn._C` (submodules/simple-knn/ext.cpp,
spatial.cu, simple_knn.cu): `distCUDA2(points)` -- for every point the mean squared distance to its 3 nearest neighbours,
from which GaussianModel.create_from_pcd takes the initial scales (scene/gaussian_model.py:706).

The search is the HIP kernel behind the C ABI (`svgir_knn_mean_dist`, include/svgir_raster.h -> svg-ir_amd/csrc/knn.hip): exact,
a pure function of the input, launched on the current stream without a host wait (the reference copies the whole box to the
host twice).  No CPU / PyTorch fallback."""
import ctypes as C

import torch

from gaussian_renderer import _native

_lib = _native.lib
_lib.svgir_knn_bytes.restype = C.c_size_t
_lib.svgir_knn_bytes.argtypes = [C.c_int32]
_lib.svgir_knn_mean_dist.restype = C.c_int
_lib.svgir_knn_mean_dist.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


@torch.no_grad()
def distCUDA2(points):
    """points [P,3] (any float dtype, any stride) -> [P] float32."""
    if not points.is_cuda:
        raise RuntimeError("distCUDA2 needs a CUDA/HIP tensor (there is no CPU path)")
    dev = points.device
    P = int(points.shape[0])
    with torch.cuda.device(dev):
        pts = _native.f32c(points.detach().reshape(P, 3), dev)
        mean = _native.out_tensor((P,), torch.float32, dev)
        work = torch.empty(int(_lib.svgir_knn_bytes(P)), dtype=torch.uint8, device=dev)
        _native.check(_lib.svgir_knn_mean_dist(P, _native.ptr(pts), _native.ptr(mean), work.data_ptr(), _native.stream_ptr(dev)),
                      "knn_mean_dist")
    return mean
