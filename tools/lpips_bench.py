#!/usr/bin/env python3
"""LPIPS (VGG-16, net-lin) throughput on one GPU: lama_amd.evaluation.PerceptualLoss against PyTorch-ROCm eager fp32 of the same network on the
same box, and the two memory-bound kernels of the path on their own.

    python tools/lpips_bench.py [--batch 8] [--hw 512] [--steps 10] [--warmup 3] [--repeats 5] [--precision f16x3] [--no-torch]

JSON lines: the whole metric (8 x 3 x 512^2 pairs by default; hipGraph replay when capture works, plain launches otherwise; median of ``--repeats``
timed runs of ``--steps`` batches each), the eager comparator (F.conv2d / max_pool2d and the distance formula in fp32, TF32 off), and per launch of
lama_lpips_scale_fwd / lama_lpips_layer_fwd at every level: microseconds and achieved GB/s against the compulsory bytes (each input element read
once, each pooled / scaled element written once).  Synthetic seeded backbone (tests/lpips_util.py): the arithmetic does not depend on the values."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import lpips_ref as R                                # noqa: E402
import lpips_util as U                               # noqa: E402
from lama_amd import _lib as L                       # noqa: E402
from lama_amd import evaluation as EV                # noqa: E402


def _time(fn, steps, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / steps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--hw', type=int, default=512)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--precision', default='f16x3', choices=['f16x3', 'bf16x3', 'f32'])
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    gold = np.load(U.GOLDEN)
    sd = U.backbone_state_dict()
    B, S = a.batch, a.hw
    g = torch.Generator().manual_seed(1)
    target = torch.rand(B, 3, S, S, generator=g).cuda()
    pred = (target + 0.1 * torch.randn(B, 3, S, S, generator=g).cuda()).clamp(0, 1)
    m = EV.PerceptualLoss(model_path=U.heads_state_dict(gold), backbone=sd).cuda().set_precision(a.precision)
    plain = m(pred, target).flatten()
    mode = 'graph'
    try:
        m.model.use_graph = True
        replay = m(pred, target).flatten()
        assert torch.equal(plain, replay), 'graph replay differs from plain launches'
    except Exception as e:                           # capture is not available: plain launches
        m.model.use_graph, mode = False, f'plain ({type(e).__name__})'
        m.model._invalidate()
    ms = _time(lambda: m(pred, target), a.steps, a.warmup, a.repeats)
    rec = dict(what='lpips', batch=B, hw=S, precision=a.precision, mode=mode, hip_ms=round(ms, 3), hip_pairs_per_s=round(B * 1000 / ms, 1),
               conv_paths=m.model.conv_paths(pred.shape, 'cuda'), precision_after=m.model.precision)
    if not a.no_torch:
        sdc = {k: v.cuda() for k, v in sd.items()}
        heads = [torch.from_numpy(gold[f'lin{k}']).cuda() for k in range(5)]
        eager = lambda: R.lpips_ref(pred, target, sdc, heads, True, torch.float32)       # noqa: E731
        ref64 = R.lpips_ref(pred[:1].cpu(), target[:1].cpu(), sd, [h.cpu() for h in heads])[0] if S <= 256 else None
        tms = _time(eager, max(2, a.steps // 2), 2, a.repeats)
        ev = eager()[0]
        rec.update(torch_eager_fp32_ms=round(tms, 3), torch_pairs_per_s=round(B * 1000 / tms, 1), ratio_to_eager=round(tms / ms, 2),
                   max_rel_hip_vs_eager=float(((plain - ev).abs() / ev).max()))
        if ref64 is not None:
            rec['rel_hip_vs_fp64_image0'] = float(abs(float(plain[0]) - float(ref64)) / float(ref64))
    print(json.dumps(rec), flush=True)
    del m
    torch.cuda.empty_cache()
    # the two kernels on their own
    lib = L.get_lib()
    x0, y = torch.rand(B, 3, S, S, device='cuda'), torch.empty(2 * B, 3, S, S, device='cuda')
    us = _time(lambda: lib.lpips_scale(L.view(x0), L.view(x0), L.view(y), B, U.SHIFT, U.SCALE), 20, 3, a.repeats) * 1000
    nbytes = 2 * y.numel() * 4
    print(json.dumps(dict(kernel='lama_lpips_scale_fwd', shape=list(y.shape), us=round(us, 1), compulsory_mb=round(nbytes / 1e6, 1),
                          gb_per_s=round(nbytes / us / 1e3, 1))), flush=True)
    del x0, y
    h = S
    for k, C in enumerate(U.CHNS):
        f = torch.relu(torch.randn(2 * B, C, h, h, device='cuda'))
        pool = k + 1 < len(U.CHNS)
        p = torch.empty(2 * B, C, h // 2, h // 2, device='cuda') if pool else None
        w, acc = torch.rand(C, device='cuda'), torch.zeros(B, device='cuda')
        ws = torch.empty(max(1, lib.lpips_layer_workspace_bytes(B, C, h, h) // 8), dtype=torch.float64, device='cuda')
        hv = EV._DistModel._half
        fn = lambda: lib.lpips_layer(hv(f, 0, B), hv(f, 1, B), B, w, acc, ws, hv(p, 0, B) if pool else None, hv(p, 1, B) if pool else None)   # noqa: E731
        us = _time(fn, 20, 3, a.repeats) * 1000
        nbytes = 4 * (f.numel() + (p.numel() if pool else 0))
        print(json.dumps(dict(kernel='lama_lpips_layer_fwd (+ its reduction launch)', level=k, shape=[B, C, h, h], pool=pool, us=round(us, 1),
                              compulsory_mb=round(nbytes / 1e6, 1), gb_per_s=round(nbytes / us / 1e3, 1))), flush=True)
        del f, p
        h //= 2


if __name__ == '__main__':
    main()
