"""Shared by the FID golden script and the FID tests: a plain-torch restatement of the FID Inception-v3 (torchvision's module names; the golden
script hands it to the reference as its ``torchvision.models``, the tests use its ``.double()`` as the fp64 reference), the seeded synthetic
state dict (conv weights regenerated from the seed, BatchNorm statistics from tests/golden/fid.npz) and the recorded cases."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'fid.npz')
SEED = 20261019
BN_BIAS = 0.25                      # every BatchNorm: weight 1, bias 0.25 -> about 60 % of a layer's outputs survive the ReLU
CASES = ('a', 'b', 'c', 'd')       # see tests/golden/make_golden_fid.py; d runs with resize_input=False


class BasicConv2d(nn.Module):
    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, bias=False, **kwargs)
        self.bn = nn.BatchNorm2d(out_channels, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)


def _avg(x):                        # the FID variant: the padding is left out of the divisor
    return F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)


class InceptionA(nn.Module):
    def __init__(self, in_channels, pool_features, conv_block=None):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(in_channels, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(in_channels, pool_features, kernel_size=1)

    def forward(self, x):
        return torch.cat([self.branch1x1(x), self.branch5x5_2(self.branch5x5_1(x)),
                          self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))), self.branch_pool(_avg(x))], 1)


class InceptionB(nn.Module):
    def __init__(self, in_channels, conv_block=None):
        super().__init__()
        self.branch3x3 = BasicConv2d(in_channels, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        return torch.cat([self.branch3x3(x), self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionC(nn.Module):
    def __init__(self, in_channels, channels_7x7, conv_block=None):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)

    def forward(self, x):
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = self.branch7x7dbl_5(self.branch7x7dbl_4(self.branch7x7dbl_3(self.branch7x7dbl_2(self.branch7x7dbl_1(x)))))
        return torch.cat([self.branch1x1(x), b7, bd, self.branch_pool(_avg(x))], 1)


class InceptionD(nn.Module):
    def __init__(self, in_channels, conv_block=None):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([self.branch3x3_2(self.branch3x3_1(x)), b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionE(nn.Module):
    def __init__(self, in_channels, conv_block=None, pool='avg'):
        super().__init__()
        self.pool = pool
        self.branch1x1 = BasicConv2d(in_channels, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(in_channels, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)

    def forward(self, x):
        b3 = self.branch3x3_1(x)
        bd = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        # Mixed_7c of the FID network pools with a MAXIMUM (a quirk of the original TensorFlow graph)
        pooled = _avg(x) if self.pool == 'avg' else F.max_pool2d(x, kernel_size=3, stride=1, padding=1)
        return torch.cat([self.branch1x1(x), self.branch3x3_2a(b3), self.branch3x3_2b(b3), self.branch3x3dbl_3a(bd), self.branch3x3dbl_3b(bd),
                          self.branch_pool(pooled)], 1)


class Inception3(nn.Module):
    """The FID Inception-v3 under torchvision's module names (``fc`` included: a real weights file carries it, the feature extractor ignores it)."""

    def __init__(self, num_classes=1008, aux_logits=False, **kwargs):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, pool_features=32)
        self.Mixed_5c = InceptionA(256, pool_features=64)
        self.Mixed_5d = InceptionA(288, pool_features=64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, channels_7x7=128)
        self.Mixed_6c = InceptionC(768, channels_7x7=160)
        self.Mixed_6d = InceptionC(768, channels_7x7=160)
        self.Mixed_6e = InceptionC(768, channels_7x7=192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280, pool='avg')
        self.Mixed_7c = InceptionE(2048, pool='max')
        self.fc = nn.Linear(2048, num_classes)

    def features(self, x):
        """pool3: [N, 2048, 1, 1] of an input already in [-1, 1]."""
        x = self.Conv2d_2b_3x3(self.Conv2d_2a_3x3(self.Conv2d_1a_3x3(x)))
        x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = self.Conv2d_4a_3x3(self.Conv2d_3b_1x1(x))
        x = F.max_pool2d(x, kernel_size=3, stride=2)
        for name in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e', 'Mixed_7a', 'Mixed_7b', 'Mixed_7c'):
            x = getattr(self, name)(x)
        return F.adaptive_avg_pool2d(x, (1, 1))


def inception_v3(pretrained=False, **kwargs):
    return Inception3(**kwargs)


def basic_convs(net):
    """The 94 BasicConv2d of a network in module order."""
    return [m for m in net.modules() if isinstance(m, BasicConv2d)]


def seeded_network(seed: int = SEED) -> Inception3:
    """He-scaled conv weights from a CPU generator (bit-reproducible); BatchNorm weight 1, bias BN_BIAS, statistics still at their defaults."""
    g = torch.Generator().manual_seed(seed)
    net = Inception3().eval()
    with torch.no_grad():
        for m in basic_convs(net):
            w = m.conv.weight
            w.copy_(torch.randn(w.shape, generator=g) * (2.0 / (w.shape[1] * w.shape[2] * w.shape[3])) ** 0.5)
            m.bn.weight.fill_(1.0)
            m.bn.bias.fill_(BN_BIAS)
        net.fc.weight.zero_()
        net.fc.bias.zero_()
    return net


def synthetic_state_dict(gold, seed: int = SEED) -> dict:
    """The seeded synthetic FID Inception under torchvision's keys: the BatchNorm statistics are the recorded ones (a calibration pass on another
    CPU would differ in the last bits), everything else comes from the seed."""
    net = seeded_network(seed)
    mean, var, o = torch.from_numpy(gold['bn_mean']), torch.from_numpy(gold['bn_var']), 0
    with torch.no_grad():
        for m in basic_convs(net):
            c = m.bn.num_features
            m.bn.running_mean.copy_(mean[o:o + c])
            m.bn.running_var.copy_(var[o:o + c])
            o += c
    assert o == mean.numel() == var.numel()
    return {k: v.clone() for k, v in net.state_dict().items()}


def restated_features(sd: dict, images01: torch.Tensor, resize_input: bool = True) -> torch.Tensor:
    """[N, 2048] fp64 pool3 features of images in [0, 1]: inception.py:151-168 on the restated network in double precision."""
    net = Inception3().eval()
    net.load_state_dict(sd, strict=True)
    net = net.double()
    x = images01.double()
    with torch.no_grad():
        if resize_input:
            x = F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False)
        return net.features(2 * x - 1).flatten(1)


def case_inputs(gold, tag):
    """(pred, target) of a recorded case, [0, 1] = u8 / 255 in fp32."""
    return torch.from_numpy(gold[f'{tag}_pred']).float() / 255.0, torch.from_numpy(gold[f'{tag}_target']).float() / 255.0
