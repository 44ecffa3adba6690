#!/usr/bin/env python3
"""Throughput of the pix2pixhd_global generators (big-lama-regular, lama-regular) and of the pix2pixhd_multidilated one (lama-dilated) on one
GPU, and the conv path of their bottleneck.

    python tools/regular_bench.py [--steps 20] [--warmup 5] [--precision f16x3] [--no-torch] [--conv-probe] [--models lama-dilated,...]

One JSON line per (model, batch) at 512^2: the HIP plan replayed from its hipGraph (ms / step, images/s), the same forward in
PyTorch-ROCm eager fp32 (the restatement of tests/regular_util.py: F.conv2d / conv_transpose2d / batch_norm), and the conv path
('winograd' / 'direct') of every bottleneck launch.  ``--conv-probe``: one line per plane shape with the 512 -> 512 3x3 conv timed
as Winograd (GEMM + output transform) and as the direct kernel, next to what ``lama_winograd_preferred`` answers for it.
lama-dilated's eager comparator is ``EagerDilated`` below, an nn.Module of the same layers (nn.Conv2d with dilation and reflect padding, summed per
group); its probe lines time the multi-dilated launch (lama_multidilated_conv3x3_fwd, four dilations) beside the plain direct 512 -> 512 conv
at the same plane shapes: the same MACs, the ratio is the price of the dilated staging.
Synthetic seeded weights: the arithmetic does not depend on their values."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lama_amd import _lib as L                      # noqa: E402
from lama_amd.modules import make_generator        # noqa: E402
from tests import multidilated_util as M           # noqa: E402
from tests import regular_util as R                # noqa: E402

MODELS = ('big-lama-regular', 'lama-regular', 'lama-dilated')


class EagerDilated(torch.nn.Module):
    """The lama-dilated generator (pix2pixhd_multidilated, cat_in, 4 dilations) from torch layers, loadable from the same state dict."""

    class MDConv(torch.nn.Module):
        def __init__(self, dim, G):
            super().__init__()
            self.convs = torch.nn.ModuleList([torch.nn.Conv2d(dim // G, dim, 3, padding=2 ** j, dilation=2 ** j, padding_mode='reflect') for j in range(G)])

        def forward(self, x):
            return sum(c(xj) for c, xj in zip(self.convs, x.chunk(len(self.convs), dim=1)))

    class Block(torch.nn.Module):
        def __init__(self, dim, G):
            super().__init__()
            nn = torch.nn
            self.conv_block = nn.Sequential(EagerDilated.MDConv(dim, G), nn.BatchNorm2d(dim), nn.ReLU(True), EagerDilated.MDConv(dim, G), nn.BatchNorm2d(dim))

        def forward(self, x):
            return x + self.conv_block(x)

    def __init__(self, cfg):
        super().__init__()
        nn, ngf, nd, G = torch.nn, cfg['ngf'], cfg['n_downsampling'], cfg['multidilation_kwargs']['dilation_num']
        m = [nn.ReflectionPad2d(3), nn.Conv2d(cfg['input_nc'], ngf, 7), nn.BatchNorm2d(ngf), nn.ReLU(True)]
        for i in range(nd):
            m += [nn.Conv2d(ngf * 2 ** i, ngf * 2 ** (i + 1), 3, stride=2, padding=1), nn.BatchNorm2d(ngf * 2 ** (i + 1)), nn.ReLU(True)]
        m += [EagerDilated.Block(ngf * 2 ** nd, G) for _ in range(cfg['n_blocks'])]
        for i in range(nd):
            c = ngf * 2 ** (nd - i)
            m += [nn.ConvTranspose2d(c, c // 2, 3, stride=2, padding=1, output_padding=1), nn.BatchNorm2d(c // 2), nn.ReLU(True)]
        m += [nn.ReflectionPad2d(3), nn.Conv2d(ngf, cfg['output_nc'], 7), nn.Sigmoid()]
        self.model = nn.Sequential(*m)

    def forward(self, x):
        return self.model(x)


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def bench_models(a):
    for name in a.models:
        dilated = name == 'lama-dilated'
        cfg = M.LAMA_DILATED if dilated else (R.BIG_LAMA_REGULAR if name == 'big-lama-regular' else R.LAMA_REGULAR)
        sd = M.make_state_dict(cfg, seed=11) if dilated else R.make_state_dict(cfg, seed=11, calib_hw=32)
        gen = make_generator(None, kind='pix2pixhd_multidilated' if dilated else 'pix2pixhd_global', **cfg)
        gen.load_state_dict(sd, strict=True)
        gen.cuda().set_precision(L.PREC_NAMES[a.precision])
        gen.use_graph, gen.clone_output, gen.defer_range_check = True, False, True
        sdc = {k: v.cuda() for k, v in sd.items()}
        if dilated:
            eager = EagerDilated(cfg).eval()
            eager.load_state_dict(sd, strict=True)
            eager.cuda()
            torch_fwd = eager
        else:
            torch_fwd = lambda t: R.forward(sdc, cfg, t)       # noqa: E731
        for B in (8, 1):
            x = R.calib_input(B, 512, 512, seed=3).cuda()
            ms = _time(lambda: gen(x), a.steps, a.warmup)
            assert gen.check_range(), 'fp16 split range exceeded on the benchmark input'
            rec = dict(model=name, batch=B, hw=512, precision=a.precision, hip_graph_ms=round(ms, 3), hip_images_per_s=round(B * 1000.0 / ms, 1),
                       bottleneck_paths=sorted(set(gen.conv_paths(x.shape, x.device))), bottleneck_launches=len(gen.conv_paths(x.shape, x.device)))
            if not a.no_torch:
                with torch.no_grad():
                    if dilated:
                        rec['max_abs_vs_eager'] = float((gen(x) - torch_fwd(x)).abs().max())
                    tms = _time(lambda: torch_fwd(x), max(3, a.steps // 4), 2)
                rec.update(torch_eager_fp32_ms=round(tms, 3), torch_images_per_s=round(B * 1000.0 / tms, 1), speedup=round(tms / ms, 2),
                           torch_allow_tf32=bool(torch.backends.cudnn.allow_tf32))
            print(json.dumps(rec), flush=True)
            gen.drop_plan(x.shape, x.device)


def dilated_probe(a):
    """The multi-dilated launch (G = 4, dilations 1, 2, 4, 8) beside the plain direct 512 -> 512 3x3 launch on the same operands."""
    lib = L.get_lib()
    p = L.PREC_NAMES[a.precision]
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(512, 512, 3, 3, generator=g) / 68.0).cuda()
    bias = torch.zeros(512, device='cuda')
    wd = lib.pack_conv_weight(w, None, precision=p)
    for B, H, W in ((8, 64, 64), (1, 64, 64), (1, 135, 240), (2, 125, 188), (8, 125, 188), (1, 16, 24)):
        x = torch.rand(B, 512, H, W, device='cuda')
        y = torch.empty_like(x)
        rec = dict(probe='mdconv512', batch=B, H=H, W=W, precision=a.precision)
        for G in (4, 1):
            t = _time(lambda: lib.multidilated_conv3x3(L.view(x), wd, L.view(y), B, G, 1, bias, L.ACT_NONE, L.view(y), precision=p), 20, 3) * 1000
            rec['multidilated_us' if G == 4 else 'multidilated_g1_us'] = round(t, 1)
        td = _time(lambda: lib.conv2d(L.view(x), wd, L.view(y), B, 3, 1, 1, L.PAD_REFLECT, False, bias, L.ACT_NONE, L.view(y), precision=p), 20, 3) * 1000
        rec.update(direct_us=round(td, 1), ratio=round(rec['multidilated_us'] / td, 2),
                   tflops_multidilated=round(2 * B * H * W * 512 * 512 * 9 / rec['multidilated_us'] / 1e6, 1))
        print(json.dumps(rec), flush=True)


def conv_probe(a):
    lib = L.get_lib()
    p = L.PREC_NAMES[a.precision]
    if p not in (L.PREC_F16X3, L.PREC_BF16X3):
        raise SystemExit('--conv-probe: the Winograd form exists at the split precisions only (f16x3, bf16x3)')
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(512, 512, 3, 3, generator=g) / 68.0).cuda()
    bias = torch.zeros(512, device='cuda')
    wp, wd = lib.pack_winograd_weight(w, None, p), lib.pack_conv_weight(w, None, precision=p)
    for B, H, W in ((8, 64, 64), (1, 64, 64), (1, 32, 32), (8, 32, 32), (1, 135, 240), (2, 135, 240), (8, 135, 240), (1, 125, 188), (2, 125, 188),
                    (8, 125, 188), (1, 168, 168), (4, 100, 100), (1, 135, 94), (3, 168, 32), (4, 168, 40), (8, 17, 94), (2, 67, 94)):
        x = torch.rand(B, 512, H, W, device='cuda')
        y = torch.empty_like(x)
        ws = torch.empty(lib.winograd_workspace_bytes(B, 512, H, W) // 4, device='cuda')
        tw = _time(lambda: lib.winograd_conv3x3(L.view(x), wp, L.view(y), B, ws, bias, L.ACT_NONE, L.view(y), precision=p), 20, 3) * 1000
        td = _time(lambda: lib.conv2d(L.view(x), wd, L.view(y), B, 3, 1, 1, L.PAD_REFLECT, False, bias, L.ACT_NONE, L.view(y), precision=p), 20, 3) * 1000
        print(json.dumps(dict(probe='conv512', batch=B, H=H, W=W, precision=a.precision, winograd_us=round(tw, 1), direct_us=round(td, 1),
                              faster='winograd' if tw < td else 'direct', model_prefers_winograd=bool(lib.winograd_preferred(B, 512, 512, H, W, p)),
                              tflops_winograd_algorithmic=round(2 * B * H * W * 512 * 512 * 9 / tw / 1e6, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--precision', default='f16x3', choices=['f16x3', 'bf16x3', 'f32'])
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--conv-probe', action='store_true', help='time the 512 -> 512 conv as Winograd and direct per plane shape')
    ap.add_argument('--no-models', action='store_true')
    ap.add_argument('--models', default=','.join(MODELS), help='comma-separated subset of ' + ', '.join(MODELS))
    a = ap.parse_args()
    a.models = [m for m in a.models.split(',') if m]
    if any(m not in MODELS for m in a.models):
        ap.error(f'--models: choose from {MODELS}')
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False     # the eager baseline in true fp32
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    if a.conv_probe:
        if any(m != 'lama-dilated' for m in a.models):
            conv_probe(a)
        if 'lama-dilated' in a.models:
            dilated_probe(a)
    if not a.no_models:
        bench_models(a)


if __name__ == '__main__':
    main()
