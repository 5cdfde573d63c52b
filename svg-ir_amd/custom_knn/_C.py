"""Drop-in replacement of the extension `custom_knn._C` the reference imports (scene/gaussian_model.py:14) but does not ship:
`topKdistCUDA2(points)` -- for every point its 8 nearest neighbours' squared distances and indices, the input of
GaussianModel.get_knn_loss (scene/gaussian_model.py:577-592).

With no upstream source, two things are this project's decisions: a point is never its own neighbour (as in
simple_knn), and the outputs are `dist [P,8]` float32, `idx [P,8]` int32, nearest first, so that the caller's `.reshape(-1, 8)`
changes nothing.  A slot without a neighbour (P < 9, non-finite points) holds dist = +inf and idx = the row's own index: the
caller indexes parameter tensors with idx, so it stays in range.

The search is the HIP kernel behind the C ABI (`svgir_knn_topk`, include/svgir_raster.h -> svg-ir_amd/csrc/knn.hip), launched on
the current stream without a host wait.  No CPU / PyTorch fallback."""
import ctypes as C

import torch

from gaussian_renderer import _native

K = 8

_lib = _native.lib
_lib.svgir_knn_bytes.restype = C.c_size_t
_lib.svgir_knn_bytes.argtypes = [C.c_int32]
_lib.svgir_knn_topk.restype = C.c_int
_lib.svgir_knn_topk.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


@torch.no_grad()
def topKdistCUDA2(points):
    """points [P,3] (any float dtype, any stride) -> (dist [P,8] float32, idx [P,8] int32)."""
    if not points.is_cuda:
        raise RuntimeError("topKdistCUDA2 needs a CUDA/HIP tensor (there is no CPU path)")
    dev = points.device
    P = int(points.shape[0])
    with torch.cuda.device(dev):
        pts = _native.f32c(points.detach().reshape(P, 3), dev)
        dist = _native.out_tensor((P, K), torch.float32, dev)
        idx = _native.out_tensor((P, K), torch.int32, dev)
        work = torch.empty(int(_lib.svgir_knn_bytes(P)), dtype=torch.uint8, device=dev)
        _native.check(_lib.svgir_knn_topk(P, _native.ptr(pts), _native.ptr(dist), _native.ptr(idx), work.data_ptr(),
                                          _native.stream_ptr(dev)), "knn_topk")
    return dist, idx
