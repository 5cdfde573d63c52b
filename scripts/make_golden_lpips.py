"""Reference-run fixture for LPIPS (tests/golden/lpips.npz).  Runs only in the authoring container: the REFERENCE's own `lpipsPyTorch`
package is imported and executed on the CPU, unmodified -- `LPIPS('vgg')` of lpipsPyTorch/modules/lpips.py with its BaseNet / VGG16 /
LinLayers (modules/networks.py) and normalize_activation / get_state_dict (modules/utils.py).  The two things it fetches from outside are
stood in for: a stub `torchvision` whose `models.vgg16(...).features` is the standard configuration-D stack filled with the seeded
weights of tests/lpips_cases.py, and `torch.hub.load_state_dict_from_url`, patched to return that module's seeded `lin{k}.model.1.weight`
tensors.  The committed fixture is data: the reference's taps and scores on inputs that lpips_cases rebuilds from its seeds, the fp64
(sum, sum of squares) of the generated weights, and three small inputs themselves; no reference source.

    python scripts/make_golden_lpips.py
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (REF: where the reference lies)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

CFG_D = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")
_variant = ["base"]


def _vgg16(*args, **kwargs):
    """torchvision.models.vgg16: configuration D, conv3x3 + ReLU(inplace) and MaxPool2d(2, 2); weights from lpips_cases."""
    import lpips_cases as lc
    layers, cin = [], 3
    for v in CFG_D:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    net = types.SimpleNamespace(features=nn.Sequential(*layers))
    vgg, _ = lc.weights(_variant[0])
    net.features.load_state_dict({k[len("features."):]: v for k, v in vgg.items()})
    return net


def _stub_torchvision():
    tv = types.ModuleType("torchvision")
    models = types.ModuleType("torchvision.models")
    models.vgg16 = _vgg16
    models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1="IMAGENET1K_V1")
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models


def _lin_state(url, *args, **kwargs):
    import lpips_cases as lc
    assert url.endswith("v0.1/vgg.pth"), url
    return dict(lc.weights(_variant[0])[1])


def lpips_fixtures():
    import lpips_cases as lc
    _stub_torchvision()
    torch.hub.load_state_dict_from_url = _lin_state
    if mg.REF not in sys.path:
        sys.path.insert(0, mg.REF)
    from lpipsPyTorch.modules.lpips import LPIPS
    assert os.path.abspath(sys.modules["lpipsPyTorch"].__file__).startswith(os.path.abspath(mg.REF))
    out = {}
    for variant in ("base", "dead5", "signed"):
        out[f"weights_{variant}"] = lc.weight_checksum(variant)
    nets = {}
    with torch.no_grad():
        for cid in lc.GOLDEN_CASES:
            c = lc.BY_ID[cid]
            if c["variant"] not in nets:
                _variant[0] = c["variant"]
                nets[c["variant"]] = LPIPS("vgg").eval()
            net = nets[c["variant"]]
            x, y = lc.operands(c)
            # the class as the reference calls it: [1,1,1,1]; and its parts, for the taps
            score = net(x[None], y[None])
            fx, fy = net.net(x[None]), net.net(y[None])
            taps = torch.cat([l((a - b) ** 2).mean((2, 3), True) for a, b, l in zip(fx, fy, net.lin)], 0).reshape(5)
            assert tuple(score.shape) == (1, 1, 1, 1)
            out[f"{cid}/score"] = score.reshape(()).numpy()
            out[f"{cid}/taps"] = taps.numpy()
    for cid in ("size_16x16", "size_17x19", "const_0_vs_1_17x19"):   # small inputs, so the case builder cannot drift either
        x, y = lc.operands(lc.BY_ID[cid])
        out[f"{cid}/x"], out[f"{cid}/y"] = x.numpy(), y.numpy()
    return out


def main():
    out = lpips_fixtures()
    path = os.path.join(ROOT, "tests", "golden", "lpips.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")
    for k in sorted(out):
        if k.endswith("/score") or k.startswith("weights_"):
            print(f"  {k}: {out[k]}")


if __name__ == "__main__":
    main()
