"""Drop-in for the reference's `lpipsPyTorch` package: `lpips(x, y, net_type='vgg')` on the HIP kernels of csrc/lpips.hip
(svgir_harness/metrics.py).  Only the VGG16 variant exists -- the one every call site of the reference uses (train.py:398, eval_nvs.py:81,
eval_relighting_tensoIR.py:370/375).  The weights are never downloaded: give them with `set_weights(vgg=..., lin=...)` (state dicts or
paths), or name the files in SVGIR_LPIPS_VGG_WEIGHTS (torchvision's vgg16 state dict) and SVGIR_LPIPS_LIN_WEIGHTS (the LPIPS v0.1
`vgg.pth`).  The packed network is built once and kept per device; the reference rebuilds it on every call."""
import os

import torch

ENV_VGG, ENV_LIN = "SVGIR_LPIPS_VGG_WEIGHTS", "SVGIR_LPIPS_LIN_WEIGHTS"
_source = None   # (vgg, lin) as given to set_weights
_net = None


def set_weights(vgg=None, lin=None):
    """vgg: torchvision's vgg16 state dict (or of its `.features`) or a path; lin: the LPIPS linear layers' state dict or a path.
    `set_weights()` forgets them (the environment variables are consulted again)."""
    global _source, _net
    if (vgg is None) != (lin is None):
        raise ValueError("lpipsPyTorch.set_weights: give both vgg and lin, or neither")
    _source = None if vgg is None else (vgg, lin)
    _net = None


def _network():
    global _net
    if _net is None:
        src = _source
        if src is None:
            paths = os.environ.get(ENV_VGG), os.environ.get(ENV_LIN)
            if not all(paths):
                raise RuntimeError(
                    f"lpipsPyTorch: no weights given and nothing is downloaded. Call lpipsPyTorch.set_weights(vgg=..., lin=...) or set "
                    f"{ENV_VGG} to torchvision's vgg16 state dict (vgg16-397923af.pth) and {ENV_LIN} to the LPIPS v0.1 linear layers "
                    f"(lpips/weights/v0.1/vgg.pth of richzhang/PerceptualSimilarity)")
            src = paths
        from svgir_harness import metrics
        _net = metrics.LPIPS(*src)
    return _net


def lpips(x: torch.Tensor, y: torch.Tensor, net_type: str = 'alex', version: str = '0.1'):
    """The reference's signature; x, y [3,H,W] or [1,3,H,W] on the GPU -> [1,1,1,1] fp32 on the GPU."""
    if version != '0.1':
        raise NotImplementedError("lpipsPyTorch: v0.1 is only supported now")
    if net_type != 'vgg':
        raise NotImplementedError(f"lpipsPyTorch: net_type '{net_type}' is not implemented here, only 'vgg' (the one the reference's call "
                                  f"sites use)")
    return _network()(x, y)
