#!/usr/bin/env python3
"""Throughput of the pix2pixhd_global generators (big-lama-regular, lama-regular) on one GPU, and the conv path of their bottleneck.

    python tools/regular_bench.py [--steps 20] [--warmup 5] [--precision f16x3] [--no-torch] [--conv-probe]

One JSON line per (model, batch) at 512^2: the HIP plan replayed from its hipGraph (ms / step, images/s), the same forward in
PyTorch-ROCm eager fp32 (the restatement of tests/regular_util.py: F.conv2d / conv_transpose2d / batch_norm), and the conv path
('winograd' / 'direct') of every bottleneck launch.  ``--conv-probe``: one line per plane shape with the 512 -> 512 3x3 conv timed
as Winograd (GEMM + output transform) and as the direct kernel, next to what ``lama_winograd_preferred`` answers for it.
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
from tests import regular_util as R                # noqa: E402


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
    for name, cfg in (('big-lama-regular', R.BIG_LAMA_REGULAR), ('lama-regular', R.LAMA_REGULAR)):
        sd = R.make_state_dict(cfg, seed=11, calib_hw=32)
        gen = make_generator(None, kind='pix2pixhd_global', **cfg)
        gen.load_state_dict(sd, strict=True)
        gen.cuda().set_precision(L.PREC_NAMES[a.precision])
        gen.use_graph, gen.clone_output, gen.defer_range_check = True, False, True
        sdc = {k: v.cuda() for k, v in sd.items()}
        for B in (8, 1):
            x = R.calib_input(B, 512, 512, seed=3).cuda()
            ms = _time(lambda: gen(x), a.steps, a.warmup)
            assert gen.check_range(), 'fp16 split range exceeded on the benchmark input'
            rec = dict(model=name, batch=B, hw=512, precision=a.precision, hip_graph_ms=round(ms, 3), hip_images_per_s=round(B * 1000.0 / ms, 1),
                       bottleneck_paths=sorted(set(gen.conv_paths(x.shape, x.device))), bottleneck_launches=len(gen.conv_paths(x.shape, x.device)))
            if not a.no_torch:
                with torch.no_grad():
                    tms = _time(lambda: R.forward(sdc, cfg, x), max(3, a.steps // 4), 2)
                rec.update(torch_eager_fp32_ms=round(tms, 3), torch_images_per_s=round(B * 1000.0 / tms, 1), speedup=round(tms / ms, 2),
                           torch_allow_tf32=bool(torch.backends.cudnn.allow_tf32))
            print(json.dumps(rec), flush=True)
            gen.drop_plan(x.shape, x.device)


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
    a = ap.parse_args()
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False     # the eager baseline in true fp32
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    if a.conv_probe:
        conv_probe(a)
    if not a.no_models:
        bench_models(a)


if __name__ == '__main__':
    main()
