"""Quality evaluators on the HIP path.

SSIM: ``saicinpainting/evaluation/losses/ssim.py`` ``SSIM`` as one launch pair (``lama_ssim_fwd``, csrc/metrics.hip), same constructor, same
``forward(img1, img2)``.  Around the scores, with the reference's names, constructor arguments and result dicts: ``get_groupings``,
``PairwiseScore``, ``SSIMScore``, ``LPIPSScore`` (``losses/base_loss.py``), ``InpaintingEvaluator`` / ``InpaintingEvaluatorOnline``
(``evaluator.py``), ``make_evaluator`` (``evaluation/__init__.py``) and ``PrecomputedInpaintingResultsDataset`` (``data.py``), which yields the
u8 arrays that are on disk: ``InpaintingEvaluator.evaluate()`` then runs the device loop of ``lama_amd/evaluate.py`` (the counterpart of
``bin/evaluate_predicts.py``; one ``lama_eval_ingest_u8_fwd`` launch per batch).  A reference user may still switch ONE import --
``from lama_amd.evaluation import SSIM`` in ``losses/base_loss.py`` -- and keep the reference's own evaluator code.

LPIPS: ``losses/lpips.py`` ``PerceptualLoss(model='net-lin', net='vgg')`` and ``base_loss.LPIPSScore``.  Pred and target go through the VGG-16
backbone as ONE batch of 2N images: ``lama_lpips_scale_fwd`` writes both scaled inputs into one tensor, the thirteen zero-padded 3x3 convs + ReLU
are ``lama_conv2d_fwd`` / ``lama_winograd_conv3x3_fwd`` launches, and one ``lama_lpips_layer_fwd`` per feature level forms the distance term AND
the 2x2 max-pool that feeds the next slice (csrc/metrics.hip).  Module tree and state-dict keys are the reference's.  Nothing is downloaded: the
linear heads (``model_path``, the reference's ``models/lpips_models/vgg.pth``) and the backbone (``backbone``, e.g. torchvision's
``vgg16-397923af.pth``) are files or state dicts the caller supplies.  The other nets / models / ``spatial`` / ``Lab`` raise NotImplementedError.

FID: ``losses/fid/inception.py`` ``InceptionV3`` (the FID variant of torchvision's Inception-v3 up to pool3) and ``base_loss.FIDScore`` /
``calculate_frechet_distance``.  Pred and target go through the network as ONE batch of 2N images: ``lama_fid_input_fwd`` resizes both to 299 x 299
and applies 2x - 1 into one tensor, the 94 convolutions (BatchNorm folded, ReLU in the epilogue) are ``lama_conv2d_rect_fwd`` launches that store
straight into their block's concatenation buffer, the poolings ``lama_pool3x3_fwd`` and ``lama_global_avgpool_fwd`` (csrc/inception.hip).  The
architecture is restated below (torchvision is not a dependency); module tree and keys are the reference's ``blocks.K.J.*``, torchvision's keys
(the format of ``pt_inception-2015-12-05-6726825d.pth``) load as well.  Nothing is downloaded: ``weights`` is a state dict or a path the caller
supplies.  The Frechet distance is numpy only (two ``eigh`` in fp64 instead of scipy's ``sqrtm``).

The segmentation-aware scores need a pretrained ADE20k segmenter: out of scope.
"""
from __future__ import annotations

import collections
import glob
import math
import os
import warnings
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from ._lib import LamaError, LamaRangeError
from .ffc import _Exec, _HipModule, _bn_fold
from .pix2pixhd import Conv2dBN


# ----------------------------------------------------------------------------------------------------
# losses/ssim.py
# ----------------------------------------------------------------------------------------------------

class SSIM(nn.Module):
    """ssim.py:7-74.  ``forward(img1, img2)`` on device tensors [B, C, H, W] fp32: the mean SSIM (``size_average``) or one value per
    image; the five depthwise window convolutions and the map never reach HBM (csrc/metrics.hip)."""

    def __init__(self, window_size: int = 11, size_average: bool = True):
        super().__init__()
        self.window_size = window_size
        self.size_average = size_average
        self.channel = 1
        self.register_buffer('window', self._create_window(window_size, self.channel))
        self._lib: Optional[L.LamaLib] = None

    def _gaussian(self, window_size: int, sigma: float) -> torch.Tensor:                 # ssim.py:36-40
        gauss = torch.Tensor([np.exp(-(x - (window_size // 2)) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)])
        return gauss / gauss.sum()

    def _create_window(self, window_size: int, channel: int) -> torch.Tensor:            # ssim.py:42-45 (kept for state-dict shape)
        w1 = self._gaussian(window_size, 1.5).unsqueeze(1)
        w2 = w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0)
        return w2.expand(channel, 1, window_size, window_size).contiguous()

    def forward(self, img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
        assert len(img1.shape) == 4
        if img1.shape != img2.shape:
            raise LamaError(f'SSIM: shapes differ {tuple(img1.shape)} vs {tuple(img2.shape)}')
        lib = self._lib or L.get_lib()
        if not lib.host_emulated and not img1.is_cuda:
            raise LamaError('SSIM runs on the GPU: move the images to the device (there is no CPU path)')
        a, b = img1.contiguous().float(), img2.contiguous().float()
        B, Cn, H, W = a.shape
        out = torch.empty(B, dtype=torch.float32, device=a.device)
        ws = torch.empty(max(1, lib.ssim_workspace_bytes(B, Cn, H, W) // 4), dtype=torch.float32, device=a.device)
        g = self._gaussian(self.window_size, 1.5).tolist()
        lib.ssim(L.view(a), L.view(b), B, g, out, ws, stream=L.LamaLib.stream_of(a))
        return out.mean() if self.size_average else out

    def _load_from_state_dict(self, *args, **kwargs):                                     # ssim.py:73-74: the window is never loaded
        return


# ----------------------------------------------------------------------------------------------------
# losses/lpips.py
# ----------------------------------------------------------------------------------------------------

# VGG-16 (Simonyan & Zisserman, configuration D) as torchvision's ``features`` lays it out: a 3x3 conv takes two indices (conv, ReLU), a
# max-pool ('M') one.  LPIPS taps the ReLU in front of every pool and the last one, so slice k = the layers from the (k-1)-th pool up to that ReLU.
_VGG16_D = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512)
_VGG16_FILE = 'vgg16-397923af.pth'           # torchvision's file name of the ImageNet weights


def _vgg16_slices():
    """[(slice number 1..5, [(features index, cin, cout), ...])]"""
    out, idx, cin, cur = [], 0, 3, []
    for v in _VGG16_D:
        if v == 'M':
            out.append(cur)
            cur, idx = [], idx + 1
        else:
            cur.append((idx, cin, v))
            cin, idx = v, idx + 2
    out.append(cur)
    return list(enumerate(out, 1))


class _Slice(nn.Module):
    """Parameter container of one backbone slice: children named by their torchvision ``features`` index (the convs only)."""

    def convs(self):
        return list(self.children())


class _VGG16(nn.Module):                      # lpips.py:808-846: slice1 .. slice5
    def __init__(self):
        super().__init__()
        self.chns = []
        for k, convs in _vgg16_slices():
            sl = _Slice()
            for idx, cin, cout in convs:
                sl.add_module(str(idx), Conv2dBN(cin, cout, 3, padding=1))
            self.add_module(f'slice{k}', sl)
            self.chns.append(convs[-1][2])
        for p in self.parameters():
            p.requires_grad = False

    def slices(self):
        return [getattr(self, f'slice{k}') for k in range(1, 6)]

    def features_key_map(self) -> dict:
        """torchvision key 'features.N.weight' -> this module's key 'sliceK.N.weight'."""
        return {f'features.{idx}.{n}': f'slice{k}.{idx}.{n}' for k, convs in _vgg16_slices() for idx, _, _ in convs for n in ('weight', 'bias')}


class _ScalingLayer(nn.Module):               # lpips.py:603-610
    def __init__(self):
        super().__init__()
        self.register_buffer('shift', torch.Tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer('scale', torch.Tensor([.458, .448, .450])[None, :, None, None])


class _NetLinLayer(nn.Module):                # lpips.py:613-621: model.1 is the 1x1 head (model.0 a Dropout, identity in eval)
    def __init__(self, chn_in: int):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(chn_in, 1, 1, stride=1, padding=0, bias=False))


class _PNetLin(nn.Module):                    # lpips.py:533-600 with pnet_type='vgg', lpips=True, spatial=False, version '0.1'
    def __init__(self):
        super().__init__()
        self.scaling_layer = _ScalingLayer()
        self.net = _VGG16()
        self.chns = self.net.chns
        self.L = len(self.chns)
        for k, c in enumerate(self.chns):
            self.add_module(f'lin{k}', _NetLinLayer(c))

    def heads(self):
        return [getattr(self, f'lin{k}').model[1].weight for k in range(self.L)]


def _load_file(path: str, what: str) -> dict:
    if not os.path.exists(path):
        raise LamaError(f'LPIPS: {what} {path!r} not found (lama_amd downloads nothing)')
    sd = torch.load(path, map_location='cpu', weights_only=True)
    if not isinstance(sd, dict):
        raise LamaError(f'LPIPS: {path!r} does not hold a state dict')
    return sd


class _DistModel(_HipModule):
    """lpips.py:248-338 (model='net-lin', net='vgg', test mode): ``forward(in0, in1, retPerLayer=False)`` on images in [-1, 1].  Owns the per-shape
    buffers and the launch sequence."""

    _PREFIX = 'model.net.net.'

    def __init__(self, model_path=None, backbone=None):
        super().__init__()
        self.model, self.model_name, self.spatial, self.is_train = 'net-lin', 'net-lin [vgg]', False, False
        self.net = _PNetLin()
        self.use_graph = False            # capture the launch sequence of a shape into a hipGraph and replay it (inputs are then copied into static buffers)
        self.auto_fallback = True         # an activation beyond the fp16 split's range: repeat with the 3-term bf16 split and stay on it
        self.max_plans = 4
        self._plans = collections.OrderedDict()
        self._load_heads(model_path)
        self._load_backbone(backbone)
        super().train(False)

    # -- weights ---------------------------------------------------------------------------------
    def _load_heads(self, model_path):
        if isinstance(model_path, dict):
            sd = model_path
        else:
            if model_path is None:
                model_path = os.path.abspath(os.path.join(os.path.dirname(__file__), '..', 'models', 'lpips_models', 'vgg.pth'))
                if not os.path.exists(model_path):
                    raise LamaError(f"LPIPS: no linear heads at {model_path!r}: pass model_path= the reference's models/lpips_models/vgg.pth "
                                    '(keys lin{0..4}.model.1.weight)')
            sd = _load_file(model_path, 'heads file')
        res = self.net.load_state_dict(sd, strict=False)                  # lpips.py:294
        missing = [k for k in res.missing_keys if k.startswith('lin')]
        if missing:
            raise LamaError(f'LPIPS: the heads state dict lacks {missing} (the format of models/lpips_models/vgg.pth is lin{{k}}.model.1.weight)')

    def _load_backbone(self, backbone):
        if backbone is None:
            path = os.path.join(torch.hub.get_dir(), 'checkpoints', _VGG16_FILE)
            if not os.path.exists(path):
                raise LamaError(f"LPIPS: no VGG-16 backbone: pass backbone= a state dict or a path to one (torchvision's {_VGG16_FILE} with "
                                f"'features.N.*' keys, or the reference's '{self._PREFIX}slice*' keys); {path!r} does not exist and nothing is downloaded")
            backbone = path
        sd = backbone if isinstance(backbone, dict) else _load_file(os.fspath(backbone), 'backbone')
        kmap = self.net.net.features_key_map()
        own = {}
        for k, v in sd.items():
            if k in kmap:
                own[kmap[k]] = v
            elif k.startswith(self._PREFIX):
                own[k[len(self._PREFIX):]] = v
        want = set(self.net.net.state_dict().keys())
        if set(own) != want:
            raise LamaError(f'LPIPS: the backbone state dict lacks {sorted(want - set(own))[:4]} ... / has unknown {sorted(set(own) - want)[:4]}: '
                            f"expected the 26 conv tensors under 'features.N.*' or '{self._PREFIX}sliceK.N.*'")
        self.net.net.load_state_dict(own, strict=True)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError('lama_amd.evaluation LPIPS is inference-only')
        return nn.Module.train(self, False)

    def _invalidate(self):
        super()._invalidate()
        self._packed = None
        self._plans = collections.OrderedDict()

    # -- execution -------------------------------------------------------------------------------
    def _consts(self, device) -> dict:
        """Per-precision constants outside the conv layers' own packed weights: the heads as [C] device vectors, shift / scale as host floats."""
        if self._packed is None:
            sl = self.net.scaling_layer
            self._packed = dict(heads=[w.detach().float().reshape(-1).contiguous() for w in self.net.heads()],
                                shift=sl.shift.detach().float().reshape(-1).tolist(), scale=sl.scale.detach().float().reshape(-1).tolist())
        return self._packed

    def _build_plan(self, shape, device) -> dict:
        B, _, H, W = shape
        lib, prec = self._exec.lib, self.precision
        bufs = dict(x=torch.empty((2 * B, 3, H, W), device=device, dtype=torch.float32))
        steps, wino_bytes, ws_bytes = [], 0, 0
        src, h, w = 'x', H, W
        for k, sl in enumerate(self.net.net.slices()):
            convs = sl.convs()
            for j, cv in enumerate(convs):
                dst = f'a{k}' if src != f'a{k}' else f'b{k}'
                if dst not in bufs:
                    bufs[dst] = torch.empty((2 * B, cv.out_channels, h, w), device=device, dtype=torch.float32)
                wino = lib.winograd_preferred(2 * B, cv.out_channels, cv.in_channels, h, w, prec) and cv.wino_ok(None)
                if wino:
                    wino_bytes = max(wino_bytes, lib.winograd_workspace_bytes(2 * B, cv.out_channels, h, w))
                steps.append(('conv', cv, src, dst, wino))
                src = dst
            C = convs[-1].out_channels
            ws_bytes = max(ws_bytes, lib.lpips_layer_workspace_bytes(B, C, h, w))
            pool = None
            if k + 1 < self.net.L:
                pool = f'p{k}'
                bufs[pool] = torch.empty((2 * B, C, h // 2, w // 2), device=device, dtype=torch.float32)
            steps.append(('layer', k, src, pool))
            src, h, w = pool, h // 2, w // 2
        bufs['levels'] = torch.zeros((self.net.L, B), device=device, dtype=torch.float32)
        bufs['ws'] = torch.empty(max(1, ws_bytes // 8), device=device, dtype=torch.float64)
        bufs['wino'] = torch.empty(max(1, wino_bytes // 4), device=device, dtype=torch.float32) if wino_bytes else None
        return dict(bufs=bufs, steps=steps, B=B, graph=None, static=None)

    def conv_paths(self, shape, device):
        """'wino' / 'direct' per conv of the plan of this input shape (tests, tools)."""
        return ['wino' if st[4] else 'direct' for st in self._plan_for(shape, torch.device(device))['steps'] if st[0] == 'conv']

    def _plan_for(self, shape, device) -> dict:
        key = (tuple(int(v) for v in shape), _Exec._dev_key(device), self.precision)
        plan = self._plans.get(key)
        if plan is None:
            while len(self._plans) >= max(1, self.max_plans):
                self._plans.popitem(last=False)
            plan = self._plans[key] = self._build_plan(shape, device)
        else:
            self._plans.move_to_end(key)
        return plan

    @staticmethod
    def _half(t: torch.Tensor, i: int, B: int) -> L.Tensor4:
        """lama_tensor view of images [i B, (i + 1) B) of a contiguous fp32 [2B, C, H, W] buffer."""
        _, C, H, W = t.shape
        return L.Tensor4(t.data_ptr() + 4 * i * B * C * H * W, C * H * W, C, H, W, L.DT_F32)

    def _run_plan(self, plan, in0: torch.Tensor, in1: torch.Tensor, normalize: bool) -> torch.Tensor:
        ex, lib, B, bufs = self._exec, self._exec.lib, plan['B'], plan['bufs']
        k = self._consts(in0.device)
        st = ex.stream(in0)
        lib.lpips_scale(L.view(in0), L.view(in1), L.view(bufs['x']), B, k['shift'], k['scale'], normalize=normalize, stream=st)
        levels = bufs['levels']
        levels.zero_()
        for step in plan['steps']:
            if step[0] == 'conv':
                _, cv, src, dst, wino = step
                cv.run(bufs[src], bufs[dst], None, L.ACT_RELU, 1, L.PAD_ZERO, None, bufs['wino'] if wino else None)
            else:
                _, lvl, src, pool = step
                f, p = bufs[src], (bufs[pool] if pool else None)
                lib.lpips_layer(self._half(f, 0, B), self._half(f, 1, B), B, k['heads'][lvl], levels[lvl], bufs['ws'],
                                None if p is None else self._half(p, 0, B), None if p is None else self._half(p, 1, B), stream=st)
        return levels

    def _levels(self, in0: torch.Tensor, in1: torch.Tensor, normalize: bool) -> torch.Tensor:
        plan = self._plan_for(in0.shape, in0.device)
        if not (self.use_graph and in0.is_cuda):
            return self._run_plan(plan, in0, in1, normalize)
        if plan['graph'] is None or plan['static'][2] != normalize:
            s0, s1 = torch.empty_like(in0), torch.empty_like(in1)
            s0.copy_(in0)
            s1.copy_(in1)
            side = torch.cuda.Stream(device=in0.device)
            side.wait_stream(torch.cuda.current_stream(in0.device))
            with torch.cuda.stream(side):                # warm-up outside capture: packs the weights
                self._run_plan(plan, s0, s1, normalize)
            torch.cuda.current_stream(in0.device).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._run_plan(plan, s0, s1, normalize)
            plan['graph'], plan['static'] = g, (s0, s1, normalize)
        plan['static'][0].copy_(in0)
        plan['static'][1].copy_(in1)
        plan['graph'].replay()
        return plan['bufs']['levels']

    def _check(self, in0: torch.Tensor, in1: torch.Tensor):
        for t in (in0, in1):
            if not self._exec.injected and not t.is_cuda:
                raise LamaError('LPIPS runs on the GPU: move the images to the device (there is no CPU path)')
        if in0.dim() != 4 or in0.shape != in1.shape or in0.shape[1] != 3:
            raise LamaError(f'LPIPS: two [N,3,H,W] batches of one shape expected, got {tuple(in0.shape)} and {tuple(in1.shape)}')
        if min(in0.shape[2:]) < 16:
            raise LamaError(f'LPIPS (VGG-16): planes of at least 16 x 16 survive the four 2x2 pools, got {tuple(in0.shape[2:])}')
        if in0.shape[0] < 1:
            raise LamaError('LPIPS: empty batch')
        if next(self.net.net.parameters()).device != in0.device and not self._exec.injected:
            raise LamaError(f'LPIPS: the weights are on {next(self.net.net.parameters()).device}, the images on {in0.device}: move the module (.to(device))')

    def forward(self, in0: torch.Tensor, in1: torch.Tensor, retPerLayer: bool = False, normalize: bool = False):
        """``in0``, ``in1``: [N,3,H,W] in [-1, 1] (``normalize``: in [0, 1], the 2x - 1 then runs inside the scaling launch).  Returns [N,1,1,1], with
        ``retPerLayer`` (value, [the five per-level terms, each [N,1,1,1]])."""
        self._check(in0, in1)
        a, b = in0.contiguous().float(), in1.contiguous().float()
        try:
            with self._exec.range_scope(a, self.precision):
                levels = self._levels(a, b, bool(normalize)).clone()
        except LamaRangeError as e:
            if not (self.auto_fallback and self.precision == L.PREC_F16X3):
                raise
            warnings.warn(f'lama_amd: {e}; switching LPIPS to the 3-term bf16 split (PREC_BF16X3)')
            self.set_precision(L.PREC_BF16X3)
            return self.forward(in0, in1, retPerLayer, normalize)
        val = levels[0].clone()
        for l in range(1, levels.shape[0]):        # lpips.py:593-595: the levels are added in order
            val += levels[l]
        val = val.view(-1, 1, 1, 1)
        if retPerLayer:
            return val, [levels[l].view(-1, 1, 1, 1) for l in range(levels.shape[0])]
        return val


class PerceptualLoss(nn.Module):
    """lpips.py:18-42.  ``forward(pred, target, normalize=True) -> [N,1,1,1]`` fp32 on the device.  ``backbone``: the VGG-16 conv weights as a state
    dict or a path to one (torchvision ``features.N.*`` keys or the reference's ``model.net.net.sliceK.N.*``); None looks for torchvision's file in the
    torch hub cache directory.  ``model_path``: the linear heads (the reference's ``models/lpips_models/vgg.pth``).  Nothing is downloaded.
    ``set_precision('f16x3' | 'bf16x3' | 'f32')`` selects the convolution arithmetic (default f16x3 with the range fallback to bf16x3)."""

    def __init__(self, model='net-lin', net='vgg', colorspace='rgb', model_path=None, spatial=False, use_gpu=True, backbone=None):
        super().__init__()
        if model != 'net-lin':
            raise NotImplementedError(f"LPIPS on the HIP path is model='net-lin' only (the linearly calibrated metric), not {model!r}")
        if net not in ('vgg', 'vgg16'):
            raise NotImplementedError(f"LPIPS on the HIP path is net='vgg' only (what LPIPSScore uses), not {net!r}")
        if spatial:
            raise NotImplementedError('LPIPS on the HIP path: spatial=True (upsampled distance maps) is not served')
        if str(colorspace).lower() != 'rgb':
            raise NotImplementedError(f'LPIPS on the HIP path: colorspace {colorspace!r} is not served (rgb only)')
        self.use_gpu = use_gpu
        self.spatial = spatial
        self.model = _DistModel(model_path=model_path, backbone=backbone)

    def set_precision(self, precision):
        self.model.set_precision(L.PREC_NAMES[precision] if isinstance(precision, str) else int(precision))
        return self

    def set_exec(self, ex):
        self.model.set_exec(ex)
        return self

    def forward(self, pred, target, normalize=True):
        return self.model(target, pred, normalize=bool(normalize))          # lpips.py:42: the model sees (target, pred)

    def forward_per_layer(self, pred, target, normalize=True):
        """(value, the five per-level terms): ``DistModel.forward(..., retPerLayer=True)`` of the reference."""
        return self.model(target, pred, retPerLayer=True, normalize=bool(normalize))


# ----------------------------------------------------------------------------------------------------
# losses/base_loss.py: get_groupings, PairwiseScore, SSIMScore, LPIPSScore
# ----------------------------------------------------------------------------------------------------

def _mean_std(v: np.ndarray) -> dict:
    return {'mean': v.mean(), 'std': v.std()}


def get_groupings(groups) -> dict:
    """{group label: the indices of its elements}; inside a group the indices come in the order ``np.argsort(groups)`` leaves them, as in the
    reference's function of this name (losses/base_loss.py)."""
    groups = np.asarray(groups)
    order = np.argsort(groups)
    labels, first = np.unique(groups[order], return_index=True)        # groups[order] is sorted: one run per label
    return dict(zip(labels, np.split(order, first[1:])))


class PairwiseScore(nn.Module):
    """What every per-image score of the evaluator keeps (the reference's class of this name): ``individual_values``, the float64 vector of the
    values seen since ``reset()``; ``get_value(groups, states)`` -> ({'mean', 'std'}, {label: {'mean', 'std'}} or None), over
    ``individual_values`` or, when given, over the concatenated ``states`` (the batches' returned tensors).  A subclass sets ``self.score`` (the
    module that maps (prediction, target) to one value per image) and returns ``self._keep(values)`` from ``forward``."""

    def __init__(self):
        super().__init__()
        self.individual_values = None

    def _keep(self, batch_values: torch.Tensor) -> torch.Tensor:
        self.individual_values = np.hstack([self.individual_values, batch_values.detach().cpu().numpy()])
        return batch_values

    def get_value(self, groups=None, states=None):
        values = self.individual_values if states is None else torch.cat(states, dim=-1).reshape(-1).cpu().numpy()
        total = _mean_std(values)
        if groups is None:
            return total, None
        groups = np.asarray(groups)
        return total, {label: _mean_std(values[np.flatnonzero(groups == label)]) for label in np.unique(groups)}

    def reset(self):
        self.individual_values = []


class SSIMScore(PairwiseScore):
    """The reference's SSIMScore: per-image SSIM (``SSIM(window_size, size_average=False)``) of (prediction, target); the mask is not used."""

    def __init__(self, window_size: int = 11):
        super().__init__()
        self.score = SSIM(window_size=window_size, size_average=False).eval()
        self.reset()

    def forward(self, pred_batch, target_batch, mask=None):
        return self._keep(self.score(pred_batch, target_batch))


class LPIPSScore(PairwiseScore):
    """The reference's LPIPSScore: ``forward`` returns the batch's values flattened to [N] and appends them to ``individual_values``."""

    def __init__(self, model='net-lin', net='vgg', model_path=None, use_gpu=True, backbone=None):
        super().__init__()
        self.score = PerceptualLoss(model=model, net=net, model_path=model_path, use_gpu=use_gpu, spatial=False, backbone=backbone).eval()
        self.reset()

    def forward(self, pred_batch, target_batch, mask=None):
        return self._keep(self.score(pred_batch, target_batch).flatten())


# ----------------------------------------------------------------------------------------------------
# losses/fid/inception.py: InceptionV3 (use_fid_inception=True), restated from the published architecture (Szegedy et al. 2015, as
# torchvision lays it out; the FID variant's three differences: average pools that leave the padding out of the divisor, a max pool in
# Mixed_7c's pool branch, 1008 classes -- the classifier is not part of the feature extractor)
# ----------------------------------------------------------------------------------------------------

def _pair2(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _c(name, cout, k=1, s=1, p=0):
    return ('conv', name, cout, _pair2(k), s, _pair2(p))


def _fork(*branches):
    return ('fork', branches)


_AVG = ('pool', L.POOL_AVG_EXCLUDE_PAD, 1, 1)
_MAX1 = ('pool', L.POOL_MAX, 1, 1)
_MAX2 = ('pool', L.POOL_MAX, 2, 0)
_GAP = ('gap',)


def _inc_a(pf):
    return [[_c('branch1x1', 64)], [_c('branch5x5_1', 48), _c('branch5x5_2', 64, 5, 1, 2)],
            [_c('branch3x3dbl_1', 64), _c('branch3x3dbl_2', 96, 3, 1, 1), _c('branch3x3dbl_3', 96, 3, 1, 1)], [_AVG, _c('branch_pool', pf)]]


def _inc_b():
    return [[_c('branch3x3', 384, 3, 2)], [_c('branch3x3dbl_1', 64), _c('branch3x3dbl_2', 96, 3, 1, 1), _c('branch3x3dbl_3', 96, 3, 2)], [_MAX2]]


def _inc_c(c7):
    return [[_c('branch1x1', 192)],
            [_c('branch7x7_1', c7), _c('branch7x7_2', c7, (1, 7), 1, (0, 3)), _c('branch7x7_3', 192, (7, 1), 1, (3, 0))],
            [_c('branch7x7dbl_1', c7), _c('branch7x7dbl_2', c7, (7, 1), 1, (3, 0)), _c('branch7x7dbl_3', c7, (1, 7), 1, (0, 3)),
             _c('branch7x7dbl_4', c7, (7, 1), 1, (3, 0)), _c('branch7x7dbl_5', 192, (1, 7), 1, (0, 3))],
            [_AVG, _c('branch_pool', 192)]]


def _inc_d():
    return [[_c('branch3x3_1', 192), _c('branch3x3_2', 320, 3, 2)],
            [_c('branch7x7x3_1', 192), _c('branch7x7x3_2', 192, (1, 7), 1, (0, 3)), _c('branch7x7x3_3', 192, (7, 1), 1, (3, 0)),
             _c('branch7x7x3_4', 192, 3, 2)], [_MAX2]]


def _inc_e(pool):
    return [[_c('branch1x1', 320)],
            [_c('branch3x3_1', 384), _fork([_c('branch3x3_2a', 384, (1, 3), 1, (0, 1))], [_c('branch3x3_2b', 384, (3, 1), 1, (1, 0))])],
            [_c('branch3x3dbl_1', 448), _c('branch3x3dbl_2', 384, 3, 1, 1),
             _fork([_c('branch3x3dbl_3a', 384, (1, 3), 1, (0, 1))], [_c('branch3x3dbl_3b', 384, (3, 1), 1, (1, 0))])],
            [pool, _c('branch_pool', 192)]]


# the four blocks of inception.py:89-129: (torchvision name or None, op | list of branches)
_INCEPTION = (
    (('Conv2d_1a_3x3', _c(None, 32, 3, 2)), ('Conv2d_2a_3x3', _c(None, 32, 3)), ('Conv2d_2b_3x3', _c(None, 64, 3, 1, 1)), (None, _MAX2)),
    (('Conv2d_3b_1x1', _c(None, 80)), ('Conv2d_4a_3x3', _c(None, 192, 3)), (None, _MAX2)),
    (('Mixed_5b', _inc_a(32)), ('Mixed_5c', _inc_a(64)), ('Mixed_5d', _inc_a(64)), ('Mixed_6a', _inc_b()), ('Mixed_6b', _inc_c(128)),
     ('Mixed_6c', _inc_c(160)), ('Mixed_6d', _inc_c(160)), ('Mixed_6e', _inc_c(192))),
    (('Mixed_7a', _inc_d()), ('Mixed_7b', _inc_e(_AVG)), ('Mixed_7c', _inc_e(_MAX1)), (None, _GAP)),
)


def _out_hw(h, w, k, s, p):
    return (h + 2 * p[0] - k[0]) // s + 1, (w + 2 * p[1] - k[1]) // s + 1


class _BasicConv2d(_HipModule):
    """torchvision's BasicConv2d: conv without bias, BatchNorm(eps=0.001), ReLU -- one ``lama_conv2d_rect_fwd`` launch (scale folded into the
    packed weights, shift = the epilogue's bias)."""

    def __init__(self, cin, cout, k, s, p):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size=k, stride=s, padding=p, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)

    def pack(self):
        if self._packed is None or self._packed['key'] != self.precision:
            scale, shift = _bn_fold(self.bn)
            self._packed = dict(key=self.precision, b=shift.contiguous(),
                                w=self._exec.lib.pack_conv_rect_weight(self.conv.weight.detach(), scale, self.precision))
        return self._packed

    def run(self, x: L.Tensor4, y: L.Tensor4, batch: int, stream: int):
        pk, ex = self.pack(), self._exec
        flag = ex._cur_flag if self.precision == L.PREC_F16X3 else None
        k, p = self.conv.kernel_size, self.conv.padding
        ex.lib.conv2d_rect(x, pk['w'], y, batch, k[0], k[1], self.conv.stride[0], p[0], p[1], bias=pk['b'], act=L.ACT_RELU,
                           precision=self.precision, stream=stream, range_flag=flag)


class _Mixed(nn.Module):
    """Parameter container of one Inception block: its BasicConv2d children under torchvision's names."""


def _mixed_module(spec, cin):
    """(module, output channels) of a block spec fed ``cin`` channels."""
    m, total = _Mixed(), 0

    def walk(ops, c):
        nonlocal total
        for op in ops:
            if op[0] == 'fork':
                for br in op[1]:
                    walk(br, c)
                return
            if op[0] == 'conv':
                m.add_module(op[1], _BasicConv2d(c, op[2], op[3], op[4], op[5]))
                c = op[2]
        total += c

    for br in spec:
        walk(br, cin)
    return m, total


class InceptionV3(_HipModule):
    """inception.py:21-168.  ``forward(inp) -> [features]`` for images [N,3,H,W] in [0, 1]; ``pair(pred, target)`` runs both as one batch and
    returns the two halves of the last requested block's output (what ``FIDScore`` calls).  ``weights``: the FID Inception state dict or a path to
    it (torchvision keys -- ``pt_inception-2015-12-05-6726825d.pth`` -- or this module's own ``blocks.K.J.*``); nothing is downloaded.  Only
    ``use_fid_inception=True`` and ``normalize_input=True`` are served."""

    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input=True, normalize_input=True, requires_grad=False, use_fid_inception=True,
                 weights=None):
        super().__init__()
        if not use_fid_inception:
            raise NotImplementedError("InceptionV3 on the HIP path serves use_fid_inception=True only (torchvision's own Inception-v3 differs in "
                                      'its pools and weights and is not what FID is defined on)')
        if not normalize_input:
            raise NotImplementedError('InceptionV3 on the HIP path: normalize_input=False is not served (the 2x - 1 runs inside the input launch)')
        if requires_grad:
            raise NotImplementedError('InceptionV3 on the HIP path is inference-only')
        self.resize_input, self.normalize_input = resize_input, normalize_input
        self.output_blocks = sorted(output_blocks)
        self.last_needed_block = max(output_blocks)
        assert self.last_needed_block <= 3, 'Last possible output block index is 3'
        self.blocks = nn.ModuleList()
        self._names = {}                                     # torchvision name -> 'blocks.K.J'
        cin = 3
        for bi, block in enumerate(_INCEPTION[:self.last_needed_block + 1]):
            mods = []
            for j, (name, spec) in enumerate(block):
                if isinstance(spec, list):
                    m, cin = _mixed_module(spec, cin)
                elif spec[0] == 'conv':
                    m, cin = _BasicConv2d(cin, spec[2], spec[3], spec[4], spec[5]), spec[2]
                elif spec[0] == 'pool':
                    m = nn.MaxPool2d(kernel_size=3, stride=2)
                else:
                    m = nn.AdaptiveAvgPool2d(output_size=(1, 1))
                if name is not None:
                    self._names[name] = f'blocks.{bi}.{j}'
                mods.append(m)
            self.blocks.append(nn.Sequential(*mods))
        for p in self.parameters():
            p.requires_grad = False
        self.use_graph = False            # capture the launch sequence of a shape into a hipGraph and replay it (inputs are then copied into static buffers)
        self.auto_fallback = True         # an activation beyond the fp16 split's range: repeat with the 3-term bf16 split and stay on it
        self.max_plans = 4
        self._plans = collections.OrderedDict()
        self._load(weights)
        nn.Module.train(self, False)

    # -- weights ---------------------------------------------------------------------------------
    def _load(self, weights):
        if weights is None:
            raise LamaError("FID: no Inception weights: pass weights= the FID Inception state dict or a path to it (torchvision keys, the format of "
                            "'pt_inception-2015-12-05-6726825d.pth', or 'blocks.K.J.*'); nothing is downloaded")
        if not isinstance(weights, dict):
            path = os.fspath(weights)
            if not os.path.exists(path):
                raise LamaError(f'FID: weights file {path!r} not found (lama_amd downloads nothing)')
            weights = torch.load(path, map_location='cpu', weights_only=True)
            if not isinstance(weights, dict):
                raise LamaError(f'FID: {path!r} does not hold a state dict')
        own = {}
        for k, v in weights.items():
            head, _, rest = k.partition('.')
            if head == 'blocks':
                own[k] = v
            elif head in self._names:
                own[f'{self._names[head]}.{rest}'] = v
            # fc.*, AuxLogits.* and blocks past the last needed one: not part of the feature extractor
        mine = nn.Module.state_dict(self)
        want = {k for k in mine if not k.endswith('num_batches_tracked')}
        own = {k: v for k, v in own.items() if k in mine}
        missing = sorted(want - set(own))
        bad = sorted(k for k, v in own.items() if tuple(v.shape) != tuple(mine[k].shape))
        if missing or bad:
            raise LamaError(f'FID: the Inception state dict lacks {missing[:4]}{" ..." if len(missing) > 4 else ""} ({len(missing)} tensors) / has '
                            f'wrongly shaped {[(k, tuple(own[k].shape), tuple(mine[k].shape)) for k in bad[:4]]} ({len(bad)}): expected '
                            "torchvision's Inception3 keys ('Conv2d_1a_3x3.conv.weight', 'Mixed_6c.branch7x7dbl_3.bn.running_var', ...) or 'blocks.K.J.*'")
        nn.Module.load_state_dict(self, own, strict=False)
        self._invalidate()

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError('lama_amd.evaluation InceptionV3 is inference-only')
        return nn.Module.train(self, False)

    def _invalidate(self):
        super()._invalidate()
        self._plans = collections.OrderedDict()

    # -- execution -------------------------------------------------------------------------------
    def _build_plan(self, shape, device) -> dict:
        """``shape``: (B, 3, H, W) of ONE of the two inputs; every buffer holds 2B images."""
        B, _, H, W = shape
        n = 2 * B
        h, w = (299, 299) if self.resize_input else (H, W)
        bufs, steps, outs = {}, [], {}

        def new(name, C, hh, ww):
            if hh < 1 or ww < 1:
                raise LamaError(f'InceptionV3: a {H} x {W} input is too small for the network (layer {name} would be {hh} x {ww})')
            bufs[name] = torch.empty((n, C, hh, ww), device=device, dtype=torch.float32)
            return name

        new('x', 3, h, w)
        cur = ('x', 0, 3)                                                # (buffer, first channel, channels)

        def op_out(op, C, hh, ww):
            if op[0] == 'conv':
                return (op[2],) + _out_hw(hh, ww, op[3], op[4], op[5])
            return (C,) + _out_hw(hh, ww, (3, 3), op[2], (op[3], op[3]))

        def emit(op, mod, src, dst):
            steps.append(('conv', mod, src, dst) if op[0] == 'conv' else ('pool', op[1], op[2], op[3], src, dst))

        for bi, block in enumerate(_INCEPTION[:self.last_needed_block + 1]):
            for j, (name, spec) in enumerate(block):
                mod, tag = self.blocks[bi][j], f'{bi}.{j}'
                if not isinstance(spec, list):
                    if spec[0] == 'gap':
                        bufs[tag] = torch.empty((n, cur[2]), device=device, dtype=torch.float32)
                        steps.append(('gap', cur, tag))
                        cur, h, w = (tag, 0, cur[2]), 1, 1
                        continue
                    C, ho, wo = op_out(spec, cur[2], h, w)
                    dst = (new(tag, C, ho, wo), 0, C)
                    emit(spec, mod, cur, dst)
                    cur, h, w = dst, ho, wo
                    continue
                # a Mixed block: every branch ends in a channel slice of the block's concatenation buffer
                leaves = []

                def shape_walk(ops, C, hh, ww):
                    for op in ops:
                        if op[0] == 'fork':
                            for br in op[1]:
                                shape_walk(br, C, hh, ww)
                            return
                        C, hh, ww = op_out(op, C, hh, ww)
                    leaves.append((C, hh, ww))

                for br in spec:
                    shape_walk(br, cur[2], h, w)
                ho, wo = leaves[0][1:]
                assert all(l[1:] == (ho, wo) for l in leaves)
                cat = new(tag, sum(l[0] for l in leaves), ho, wo)
                c_off, tmp = [0], [0]

                def walk(ops, src, hh, ww):
                    for i, op in enumerate(ops):
                        if op[0] == 'fork':
                            for br in op[1]:
                                walk(br, src, hh, ww)
                            return
                        C, h2, w2 = op_out(op, src[2], hh, ww)
                        if i == len(ops) - 1:
                            dst = (cat, c_off[0], C)
                            c_off[0] += C
                        else:
                            tmp[0] += 1
                            dst = (new(f'{tag}.t{tmp[0]}', C, h2, w2), 0, C)
                        emit(op, getattr(mod, op[1]) if op[0] == 'conv' else None, src, dst)
                        src, hh, ww = dst, h2, w2

                for br in spec:
                    walk(br, cur, h, w)
                cur, h, w = (cat, 0, bufs[cat].shape[1]), ho, wo
            outs[bi] = cur[0]
        return dict(bufs=bufs, steps=steps, outs=outs, B=B, graph=None, static=None)

    def conv_paths(self, shape, device):
        """The entry every conv of the plan of this input shape takes (tests, tools): all 94 run on ``lama_conv2d_rect_fwd``."""
        return ['rect' for st in self._plan_for(shape, torch.device(device))['steps'] if st[0] == 'conv']

    def _plan_for(self, shape, device) -> dict:
        key = (tuple(int(v) for v in shape), _Exec._dev_key(device), self.precision)
        plan = self._plans.get(key)
        if plan is None:
            while len(self._plans) >= max(1, self.max_plans):
                self._plans.popitem(last=False)
            plan = self._plans[key] = self._build_plan(shape, device)
        else:
            self._plans.move_to_end(key)
        return plan

    def _run_plan(self, plan, a: torch.Tensor, b: torch.Tensor):
        ex, lib, bufs, n = self._exec, self._exec.lib, plan['bufs'], 2 * plan['B']
        st = ex.stream(a)
        lib.fid_input(L.view(a), L.view(b), L.view(bufs['x']), plan['B'], resize=self.resize_input, stream=st)

        def v(ref):
            return L.view(bufs[ref[0]], ref[1], ref[2])

        for step in plan['steps']:
            if step[0] == 'conv':
                step[1].run(v(step[2]), v(step[3]), n, st)
            elif step[0] == 'pool':
                lib.pool3x3(v(step[4]), v(step[5]), n, step[1], step[2], step[3], stream=st)
            else:
                lib.global_avgpool(v(step[1]), bufs[step[2]], n, stream=st)

    def _launch(self, a: torch.Tensor, b: torch.Tensor) -> dict:
        plan = self._plan_for(a.shape, a.device)
        if not (self.use_graph and a.is_cuda):
            self._run_plan(plan, a, b)
            return plan
        if plan['graph'] is None:
            s0, s1 = torch.empty_like(a), torch.empty_like(b)
            s0.copy_(a)
            s1.copy_(b)
            side = torch.cuda.Stream(device=a.device)
            side.wait_stream(torch.cuda.current_stream(a.device))
            with torch.cuda.stream(side):                # warm-up outside capture: packs the weights
                self._run_plan(plan, s0, s1)
            torch.cuda.current_stream(a.device).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._run_plan(plan, s0, s1)
            plan['graph'], plan['static'] = g, (s0, s1)
        plan['static'][0].copy_(a)
        plan['static'][1].copy_(b)
        plan['graph'].replay()
        return plan

    def _check(self, a: torch.Tensor, b: torch.Tensor):
        for t in (a, b):
            if not self._exec.injected and not t.is_cuda:
                raise LamaError('InceptionV3 runs on the GPU: move the images to the device (there is no CPU path)')
        if a.dim() != 4 or a.shape != b.shape or a.shape[1] != 3 or a.shape[0] < 1:
            raise LamaError(f'InceptionV3: [N,3,H,W] batches of one shape expected, got {tuple(a.shape)} and {tuple(b.shape)}')
        dev = next(self.parameters()).device
        if dev != a.device and not self._exec.injected:
            raise LamaError(f'InceptionV3: the weights are on {dev}, the images on {a.device}: move the module (.to(device))')

    def _blocks_of(self, a: torch.Tensor, b: torch.Tensor) -> list:
        """The requested blocks' outputs for the 2B images (a, then b), cloned out of the plan's buffers."""
        self._check(a, b)
        a, b = a.contiguous().float(), b.contiguous().float()
        try:
            with self._exec.range_scope(a, self.precision):
                plan = self._launch(a, b)
                outs = [plan['bufs'][plan['outs'][i]].clone() for i in self.output_blocks]
        except LamaRangeError as e:
            if not (self.auto_fallback and self.precision == L.PREC_F16X3):
                raise
            warnings.warn(f'lama_amd: {e}; switching the FID Inception to the 3-term bf16 split (PREC_BF16X3)')
            self.set_precision(L.PREC_BF16X3)
            return self._blocks_of(a, b)
        return [o.view(o.shape[0], o.shape[1], 1, 1) if o.dim() == 2 else o for o in outs]

    def pair(self, pred: torch.Tensor, target: torch.Tensor):
        """(features of pred, features of target) of the LAST requested block, both from one pass over 2N images."""
        out = self._blocks_of(pred, target)[-1]
        n = pred.shape[0]
        return out[:n], out[n:]

    def forward(self, inp: torch.Tensor):
        n = inp.shape[0]
        if n % 2 == 0 and n > 0:                           # the plan's two inputs: the two halves of the batch
            outs = self._blocks_of(inp[:n // 2], inp[n // 2:])
        else:
            outs = [o[:n] for o in self._blocks_of(inp, inp)]
        return outs


# ----------------------------------------------------------------------------------------------------
# losses/base_loss.py: fid_calculate_activation_statistics, calculate_frechet_distance, FIDScore
# ----------------------------------------------------------------------------------------------------

def fid_calculate_activation_statistics(act):
    """base_loss.py:121-124, in the dtypes numpy gives the reference: the mean of fp32 activations is fp32, their covariance fp64."""
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def _psd_eigenvalues(lam: np.ndarray) -> np.ndarray:
    """Eigenvalues of a positive semi-definite matrix as ``eigh`` returns them, with its noise cut: ``eigh`` is accurate to eps x lambda_max
    ABSOLUTELY, so everything below D eps lambda_max (numpy's ``matrix_rank`` threshold) is indistinguishable from 0.  Without the cut the
    D - N null eigenvalues of a rank-deficient covariance (N images, D = 2048) each add sqrt(noise) to the trace below: 1e-6 relative for an
    identical pair, whose FID is 0."""
    top = lam.max(initial=0.0)
    return np.where(lam > lam.size * np.finfo(np.float64).eps * top, lam, 0.0)


def _psd_sqrt(sigma: np.ndarray) -> np.ndarray:
    lam, vec = np.linalg.eigh(sigma)
    return (vec * np.sqrt(_psd_eigenvalues(lam))) @ vec.T


def calculate_frechet_distance(activations_pred, activations_target, eps=1e-6):
    """base_loss.py:127-153: |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2).  The reference takes scipy's ``sqrtm`` of the (non-symmetric)
    product; S1 S2 is similar to the symmetric positive semi-definite S1^1/2 S2 S1^1/2, so tr sqrt(S1 S2) = sum_i sqrt(max(lambda_i, 0)) over
    that matrix's eigenvalues: two ``eigh`` in fp64, numpy only.  Nothing can come out non-finite or complex, so ``eps`` (the reference's
    diagonal offset for a singular product) is accepted and not needed."""
    mu1, sigma1 = fid_calculate_activation_statistics(activations_pred)
    mu2, sigma2 = fid_calculate_activation_statistics(activations_target)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    diff = mu1 - mu2
    root1 = _psd_sqrt(sigma1)
    mid = root1 @ sigma2 @ root1
    lam = _psd_eigenvalues(np.linalg.eigvalsh((mid + mid.T) * 0.5))
    tr_covmean = np.sqrt(lam).sum()
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr_covmean


class FIDScore(nn.Module):
    """The reference's FIDScore: ``forward`` appends the two [N, dims] activation batches (on the CPU) to ``activations_pred`` /
    ``activations_target`` and returns them; ``get_value(groups, states)`` -> ({'mean': FID}, {label: {'mean': FID of the group}} or None) and
    resets.  A group of one element has no covariance: nan.  ``weights``: see ``InceptionV3`` (one network per score; nothing is downloaded)."""

    def __init__(self, dims=2048, eps=1e-6, weights=None):
        super().__init__()
        self.model = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]], weights=weights).eval()
        self.eps = eps
        self.reset()

    def activations(self, pred_batch, target_batch):
        """The two [N, dims] activation batches on the device (the device loop keeps them there until a bucket is done)."""
        ap, at = self.model.pair(pred_batch, target_batch)
        if ap.shape[2] != 1 or ap.shape[3] != 1:
            ap, at = ap.mean(dim=(2, 3), keepdim=True), at.mean(dim=(2, 3), keepdim=True)
        return ap.flatten(1), at.flatten(1)

    def forward(self, pred_batch, target_batch, mask=None):
        ap, at = self.activations(pred_batch, target_batch)
        self.activations_pred.append(ap.detach().cpu())
        self.activations_target.append(at.detach().cpu())
        return ap, at

    def get_value(self, groups=None, states=None):
        ap, at = zip(*states) if states is not None else (self.activations_pred, self.activations_target)
        ap, at = torch.cat(list(ap)).cpu().numpy(), torch.cat(list(at)).cpu().numpy()
        total = dict(mean=calculate_frechet_distance(ap, at, eps=self.eps))
        per_group = None
        if groups is not None:
            per_group = {}
            for label, index in get_groupings(groups).items():
                per_group[label] = dict(mean=calculate_frechet_distance(ap[index], at[index], eps=self.eps) if len(index) > 1 else float('nan'))
        self.reset()
        return total, per_group

    def reset(self):
        self.activations_pred = []
        self.activations_target = []


# ----------------------------------------------------------------------------------------------------
# evaluation/evaluator.py, evaluation/__init__.py, evaluation/data.py: the bookkeeping around the scores
# ----------------------------------------------------------------------------------------------------

def _interval_names(bins: int, bin_edges: np.ndarray) -> list:
    """The rows of the report: '0-10%' ... '90-100%' for 10 bins, one more decimal per further power of ten of ``bins``."""
    digits = max(0, math.ceil(math.log10(bins)) - 1)
    percent = ['%.*f' % (digits, round(100 * edge, digits)) for edge in bin_edges]
    return [f'{lo}-{hi}%' for lo, hi in zip(percent, percent[1:])]


def mask_area(mask_sums, plane) -> np.ndarray:
    """The mask area of the device path, BY DEFINITION: ``sum of the padded u8 mask / (255 * Hp * Wp)`` in fp64, from the exact integer sums
    ``lama_eval_ingest_u8_fwd`` leaves.  (The reference's fp32 ``mask.mean()`` depends on the reduction order in its last ulp; this does not.)"""
    sums = mask_sums.detach().cpu().numpy() if torch.is_tensor(mask_sums) else np.asarray(mask_sums)
    return sums.astype(np.float64) / (255.0 * np.asarray(plane, dtype=np.float64))      # plane: Hp * Wp, one number or one per image


def _result_table(scores, groups, interval_names, states=None, integral=(None, None)) -> dict:
    """{(score name, 'total' | interval name): {'mean', 'std'}}: per score its total, then its non-empty groups in label order; ``states`` =
    the per-batch dicts an online evaluator returned; ``integral`` = (title, function of this table) adds one more 'total' row."""
    table = {}
    for name, score in scores.items():
        own = None if states is None else [batch[name] for batch in states]
        total, per_group = score.get_value(groups=groups, states=own)
        table[(name, 'total')] = total
        for label, stats in (per_group or {}).items():
            table[(name, interval_names[label])] = stats
    title, func = integral
    if func is not None:
        table[(title, 'total')] = dict(mean=func(table))
    return table


class InpaintingEvaluator:
    """evaluator.py:16-109.  ``evaluate()`` returns {(score name, 'total' | 'a-b%'): {'mean', 'std'}}.  A dataset of u8 items
    (``PrecomputedInpaintingResultsDataset`` below) is scored by the device loop of ``lama_amd.evaluate`` -- u8 upload, one ingest launch per
    batch, every score on the same tensors; any other dataset (float ``image`` / ``mask`` / ``inpainted`` items of one size, as the reference's
    loaders yield them) by the reference's loop: one pass over the dataset for the groups and one per score."""

    def __init__(self, dataset, scores, area_grouping=True, bins=10, batch_size=32, device='cuda', integral_func=None, integral_title=None,
                 clamp_image_range=None):
        self.dataset, self.scores = dataset, scores
        self.area_grouping, self.bins = area_grouping, bins
        self.batch_size, self.device = batch_size, torch.device(device)
        self.integral_func, self.integral_title = integral_func, integral_title
        self.clamp_image_range = clamp_image_range

    def _dataloader(self):
        return torch.utils.data.DataLoader(self.dataset, shuffle=False, batch_size=self.batch_size)

    def bin_edges(self):
        bin_edges = np.linspace(0, 1, self.bins + 1)
        return bin_edges, _interval_names(self.bins, bin_edges)

    def bins_of_area(self, area: np.ndarray) -> np.ndarray:
        """evaluator.py:59-61: ``searchsorted(side='right') - 1``; an area of exactly 1 belongs to the last bin."""
        bin_indices = np.searchsorted(self.bin_edges()[0], area, side='right') - 1
        bin_indices[bin_indices == self.bins] = self.bins - 1
        return bin_indices

    def bins_of_mask_sums(self, mask_sums, plane) -> np.ndarray:
        return self.bins_of_area(mask_area(mask_sums, plane))

    def _get_bin_edges(self):
        _, interval_names = self.bin_edges()
        groups = []
        for batch in self._dataloader():
            mask = batch['mask']
            area = mask.to(self.device).reshape(mask.shape[0], -1).mean(dim=-1)
            groups.append(self.bins_of_area(area.detach().cpu().numpy()))
        return np.hstack(groups), interval_names

    def results_of(self, groups, interval_names) -> dict:
        """The result dict of scores that hold their values."""
        return _result_table(self.scores, groups, interval_names, integral=(self.integral_title, self.integral_func))

    def _float_batches(self):
        """(image, mask, prediction or None) of every batch of a float dataset, on the device, the image clamped."""
        for batch in self._dataloader():
            image, mask, inpainted = (None if batch.get(k) is None else batch[k].to(self.device) for k in ('image', 'mask', 'inpainted'))
            if self.clamp_image_range is not None:
                image = image.clamp(*self.clamp_image_range)
            yield image, mask, inpainted

    def evaluate(self, model=None):
        if getattr(self.dataset, 'u8_items', False):
            if model is not None:
                raise NotImplementedError('InpaintingEvaluator on u8 items scores precomputed predictions (model=None); run lama_amd.predict first')
            from . import evaluate as _loop                      # the device loop lives beside its CLI
            groups, interval_names = _loop.score_dataset(self.dataset, self.scores, batch_size=self.batch_size, device=self.device,
                                                         clamp_image_range=self.clamp_image_range, evaluator=self)
            return self.results_of(groups if self.area_grouping else None, interval_names)
        groups, interval_names = self._get_bin_edges() if self.area_grouping else (None, None)
        with torch.no_grad():
            for score in self.scores.values():               # as the reference: one pass over the dataset per score
                score.to(self.device)
                score.reset()
                for image, mask, inpainted in self._float_batches():
                    if model is not None:
                        inpainted = model(image, mask)
                    elif inpainted is None:
                        raise LamaError("InpaintingEvaluator.evaluate(model=None) scores precomputed predictions: the items need an 'inpainted' entry")
                    score(inpainted, image, mask)
        return self.results_of(groups, interval_names)


def _fid_absent(what: str):
    return NotImplementedError(f'{what}: FID needs the pretrained FID Inception-v3 weights, which lama_amd neither ships nor downloads: pass '
                               "fid_kwargs=dict(weights=<state dict or path to pt_inception-2015-12-05-6726825d.pth>), or score ssim / lpips only")


def _fid_rel(metrics, fid_scale):
    return max(0, fid_scale - metrics[('fid', 'total')]['mean']) / fid_scale


def ssim_fid100_f1(metrics, fid_scale=100):          # evaluator.py:112-117
    ssim, fid_rel = metrics[('ssim', 'total')]['mean'], _fid_rel(metrics, fid_scale)
    return 2 * ssim * fid_rel / (ssim + fid_rel + 1e-3)


def lpips_fid100_f1(metrics, fid_scale=100):         # evaluator.py:120-125
    neg_lpips, fid_rel = 1 - metrics[('lpips', 'total')]['mean'], _fid_rel(metrics, fid_scale)       # inverted, so bigger is better
    return 2 * neg_lpips * fid_rel / (neg_lpips + fid_rel + 1e-3)


class InpaintingEvaluatorOnline(nn.Module):
    """evaluator.py:129-220: ``forward(batch)`` scores one batch and records its groups, ``evaluation_end(states)`` returns the result dict and
    resets.  ``batch['mask']`` is the float mask as in the reference; a batch of the device loop carries ``batch['mask_sum']`` (int64 [B], from
    ``lama_eval_ingest_u8_fwd``) instead and the area is ``mask_area`` of it over the image plane."""

    def __init__(self, scores, bins=10, image_key='image', inpainted_key='inpainted', integral_func=None, integral_title=None,
                 clamp_image_range=None):
        super().__init__()
        self.scores = nn.ModuleDict(scores)
        self.image_key, self.inpainted_key = image_key, inpainted_key
        self.integral_func, self.integral_title = integral_func, integral_title
        self.clamp_image_range = clamp_image_range
        self.bins_num, self.bin_edges = bins, np.linspace(0, 1, bins + 1)
        self.interval_names = _interval_names(bins, self.bin_edges)
        self.groups = []                                     # the bin of every image seen since the last evaluation_end

    def bins_of_area(self, area: np.ndarray) -> np.ndarray:
        """evaluator.py:165: ``clip(searchsorted - 1, 0, bins - 1)`` (side='left': an area ON an edge belongs to the bin below)."""
        return np.clip(np.searchsorted(self.bin_edges, area) - 1, 0, self.bins_num - 1)

    def _get_bins(self, mask_batch):
        area = mask_batch.view(mask_batch.shape[0], -1).mean(dim=-1).detach().cpu().numpy()
        return self.bins_of_area(area)

    def forward(self, batch):
        image, inpainted, mask = batch[self.image_key], batch[self.inpainted_key], batch.get('mask')
        with torch.no_grad():
            if self.clamp_image_range is not None:
                image = image.clamp(*self.clamp_image_range)
            if mask is not None:
                bins = self._get_bins(mask)
            else:
                bins = self.bins_of_area(mask_area(batch['mask_sum'], image.shape[-2] * image.shape[-1]))
            self.groups.extend(bins)
            return {name: score(inpainted, image, mask) for name, score in self.scores.items()}

    def process_batch(self, batch):
        return self(batch)

    def evaluation_end(self, states=None):
        """The result dict over everything seen since the last call (``states``: the dicts ``forward`` returned, when the caller gathered them
        itself); forgets the groups and resets the scores."""
        results = _result_table(self.scores, np.array(self.groups), self.interval_names, states=states,
                                integral=(self.integral_title, self.integral_func))
        self.groups = []
        for score in self.scores.values():
            score.reset()
        return results


def make_evaluator(kind='default', ssim=True, lpips=True, fid=False, integral_kind=None, **kwargs):
    """evaluation/__init__.py:9-33.  ``fid`` defaults to False here, because FID needs weights the caller must supply:
    ``fid_kwargs`` = dict(weights=...) reaches ``FIDScore``, ``lpips_kwargs`` = dict(model_path=..., backbone=...) ``LPIPSScore`` (nothing is
    downloaded).  ``fid=True`` without weights, or an integral kind (both are built on FID) while ``fid`` is off, raises NotImplementedError."""
    lpips_kwargs = kwargs.pop('lpips_kwargs', None) or {}
    fid_kwargs = kwargs.pop('fid_kwargs', None) or {}
    if fid and fid_kwargs.get('weights') is None:
        raise _fid_absent('make_evaluator(fid=True)')
    integral_func = None
    if integral_kind is not None:
        if integral_kind not in ('ssim_fid100_f1', 'lpips_fid100_f1'):
            raise ValueError(f'Unexpected integral_kind={integral_kind}')
        if not fid:
            raise _fid_absent(f'make_evaluator(integral_kind={integral_kind!r}) with fid off')
        integral_func = ssim_fid100_f1 if integral_kind == 'ssim_fid100_f1' else lpips_fid100_f1
    metrics = {}
    if ssim:
        metrics['ssim'] = SSIMScore()
    if lpips:
        metrics['lpips'] = LPIPSScore(**lpips_kwargs)
    if fid:
        metrics['fid'] = FIDScore(**fid_kwargs)
    if kind == 'default':
        return InpaintingEvaluatorOnline(scores=metrics, integral_func=integral_func, integral_title=integral_kind, **kwargs)


class PrecomputedInpaintingResultsDataset:
    """data.py:58-67,110-124: the (image, mask, prediction) triples of a dataset directory and a prediction directory, paired as the reference
    pairs them.  Items are what is on disk: ``image`` / ``inpainted`` u8 [h, w, 3] (RGB), ``mask`` u8 [h, w] (PIL decode) -- the / 255, the padding
    to ``pad_out_to_modulo`` and the layout change happen on the device (``lama_eval_ingest_u8_fwd``)."""

    u8_items = True

    def __init__(self, datadir, predictdir, inpainted_suffix='_inpainted.jpg', img_suffix='.jpg', pad_out_to_modulo=None, scale_factor=None):
        if scale_factor is not None:
            raise NotImplementedError('PrecomputedInpaintingResultsDataset: scale_factor is not served by the evaluator (score predictions at '
                                      'the size they were made: lama_amd.predict applies dataset.scale_factor itself)')
        self.datadir, self.predictdir = datadir, predictdir
        self.pad_out_to_modulo, self.scale_factor = pad_out_to_modulo, None
        # <name>_mask<anything>.png anywhere under datadir belongs to <name><img_suffix> beside it and to the prediction at the same relative
        # path under predictdir, its '.png' replaced by inpainted_suffix
        root = os.path.join(datadir, '')                      # (with its trailing separator)
        self.mask_filenames = sorted(glob.glob(os.path.join(datadir, '**', '*mask*.png'), recursive=True))
        self.img_filenames = [(m.rpartition('_mask')[0] or m) + img_suffix for m in self.mask_filenames]
        self.pred_filenames = [os.path.join(predictdir, os.path.splitext(m[len(root):])[0] + inpainted_suffix) for m in self.mask_filenames]

    @property
    def pad_mod(self) -> int:
        return int(self.pad_out_to_modulo) if self.pad_out_to_modulo is not None and self.pad_out_to_modulo > 1 else 1

    def __len__(self):
        return len(self.mask_filenames)

    @staticmethod
    def _load(fname, mode):
        from PIL import Image
        return np.array(Image.open(fname).convert(mode))

    def size(self, i):
        """(h, w) of item i from the mask file's header (no decode)."""
        from PIL import Image
        with Image.open(self.mask_filenames[i]) as im:
            return im.size[1], im.size[0]

    def __getitem__(self, i):
        result = dict(image=self._load(self.img_filenames[i], 'RGB'), mask=self._load(self.mask_filenames[i], 'L'),
                      inpainted=self._load(self.pred_filenames[i], 'RGB'))
        if result['image'].shape[:2] != result['mask'].shape or result['inpainted'].shape != result['image'].shape:
            raise LamaError(f"{self.mask_filenames[i]}: image {result['image'].shape}, mask {result['mask'].shape} and prediction "
                            f"{result['inpainted'].shape} differ in size")
        if self.pad_mod > 1:
            result['unpad_to_size'] = result['image'].shape[:2]
        return result
