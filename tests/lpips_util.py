"""Shared by the LPIPS golden script and the LPIPS tests: the seeded synthetic VGG-16 backbone (never committed: regenerated from the seed), the
real linear heads and the recorded cases of tests/golden/lpips.npz."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'lpips.npz')
BACKBONE_SEED = 20261017
# VGG-16 configuration D in torchvision's ``features`` numbering: a conv takes two indices (conv, ReLU), a pool one
VGG16_D = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M')
CHNS = (64, 128, 256, 512, 512)
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
CASES = ('a', 'b', 'c', 'd', 'f', 'g', 'h')           # see tests/golden/make_golden_lpips.py
RANDOM_OF_SIZE = {'c': 'f', 'h': 'f', 'd': None}      # small-valued cases -> the independent-random case of the same size (absolute bar)


def vgg16_conv_indices():
    """[(features index, cin, cout)] of the thirteen convs."""
    out, idx, cin = [], 0, 3
    for v in VGG16_D:
        if v == 'M':
            idx += 1
        else:
            out.append((idx, cin, v))
            cin, idx = v, idx + 2
    return out


def backbone_state_dict(seed: int = BACKBONE_SEED) -> dict:
    """He-initialised conv weights, bias 0.1 * randn, under torchvision's keys ('features.N.weight' / '.bias'), fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, cin, cout in vgg16_conv_indices():
        std = (2.0 / (cin * 9)) ** 0.5                 # kaiming_normal_, fan_in, ReLU gain
        sd[f'features.{idx}.weight'] = torch.randn(cout, cin, 3, 3, generator=g) * std
        sd[f'features.{idx}.bias'] = 0.1 * torch.randn(cout, generator=g)
    return sd


def features_sequential(sd: dict) -> torch.nn.Sequential:
    """A plain-torch ``features`` Sequential of the standard layout holding ``sd`` (what the golden script hands the reference as torchvision's)."""
    layers, cin = [], 3
    for v in VGG16_D:
        if v == 'M':
            layers.append(torch.nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [torch.nn.Conv2d(cin, v, kernel_size=3, padding=1), torch.nn.ReLU(inplace=True)]
            cin = v
    seq = torch.nn.Sequential(*layers)
    seq.load_state_dict({k[len('features.'):]: v for k, v in sd.items()}, strict=True)
    return seq


def heads_state_dict(gold) -> dict:
    """The real linear heads recorded in lpips.npz, in the format of the reference's vgg.pth."""
    return {f'lin{k}.model.1.weight': torch.from_numpy(gold[f'lin{k}']).view(1, -1, 1, 1) for k in range(5)}


def case_inputs(gold, tag):
    """(pred, target, normalize) of a recorded case: the images are stored as uint8, [0, 1] = u8 / 255, [-1, 1] = u8 / 127.5 - 1."""
    normalize = bool(gold[f'{tag}_normalize'])
    conv = (lambda u: torch.from_numpy(u).float() / 255.0) if normalize else (lambda u: torch.from_numpy(u).float() / 127.5 - 1.0)
    return conv(gold[f'{tag}_pred']), conv(gold[f'{tag}_target']), normalize
