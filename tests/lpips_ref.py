"""Independent restatement of LPIPS (VGG-16, net-lin) in plain torch, fp64 by default: the reference of the LPIPS tests where the original
implementation is not available.

    y = ((2 x - 1) - shift_c) / scale_c;  thirteen zero-padded 3x3 convs + ReLU with a 2x2 max-pool in front of slices 2..5;
    level_k = mean_pixels sum_c w_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2;   value = sum_k level_k
"""
import torch
import torch.nn.functional as F

from lpips_util import SCALE, SHIFT, VGG16_D


def scale_ref(x, normalize=True, dtype=torch.float64):
    x = x.to(dtype)
    if normalize:
        x = 2 * x - 1
    sh = torch.tensor(SHIFT, dtype=torch.float32).to(device=x.device, dtype=dtype).view(1, 3, 1, 1)      # the module keeps them as fp32 buffers
    sc = torch.tensor(SCALE, dtype=torch.float32).to(device=x.device, dtype=dtype).view(1, 3, 1, 1)
    return (x - sh) / sc


def layer_ref(f0, f1, w, dtype=torch.float64):
    """[N] level term of two feature maps [N,C,h,w] under the head w [C]."""
    f0, f1, w = f0.to(dtype), f1.to(dtype), w.to(dtype).view(1, -1, 1, 1)
    n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return (w * (n0 - n1).pow(2)).sum(1).mean((1, 2))


def backbone_ref(x, sd, dtype=torch.float64):
    """The five tapped feature maps (the ReLU in front of every pool but the last of torchvision's layout, which LPIPS does not reach)."""
    feats, idx = [], 0
    for v in VGG16_D[:-1]:
        if v == 'M':
            feats.append(x)
            x = F.max_pool2d(x, 2, 2)
            idx += 1
        else:
            x = F.relu(F.conv2d(x, sd[f'features.{idx}.weight'].to(dtype), sd[f'features.{idx}.bias'].to(dtype), padding=1))
            idx += 2
    feats.append(x)
    return feats


def lpips_ref(pred, target, sd, heads, normalize=True, dtype=torch.float64):
    """(value [N], levels [5, N]) in ``dtype``; ``heads``: five [C] tensors."""
    with torch.no_grad():
        f0 = backbone_ref(scale_ref(target, normalize, dtype), sd, dtype)
        f1 = backbone_ref(scale_ref(pred, normalize, dtype), sd, dtype)
        levels = torch.stack([layer_ref(a, b, w.reshape(-1), dtype) for a, b, w in zip(f0, f1, heads)])
    return levels.sum(0), levels
