#!/usr/bin/env python3
"""FID feature pass (Inception-v3 to pool3) on one GPU: lama_amd.evaluation.InceptionV3 against PyTorch-ROCm eager fp32 of the same network (the
restatement of tests/inception_util.py) on the same box, per-layer times, and the evaluator CLI with and without fid_weights=.

    python tools/fid_bench.py [--batch 8] [--steps 10] [--warmup 3] [--repeats 5] [--precision f16x3] [--no-torch] [--no-cli] [--out profiles/fid.txt]

JSON lines (also appended to ``--out``): the feature pass for ``--batch`` pairs (2 x batch images at 299^2; hipGraph replay when capture works),
its multiply-add count summed from the plan's layer table and the resulting TF/s (2 FLOP per multiply-add; a whole-pass rate, not a kernel's share
of peak), the eager comparator (fp32 against a three-term 16-bit split: the same accuracy class, not the same arithmetic), the ten slowest
layers by device time, and ``lama_amd.evaluate`` over the 256-triple set of tools/evaluate_bench.py with and without the FID column.
Synthetic seeded network (tests/inception_util.py): the arithmetic does not depend on the values."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import inception_util as U                           # noqa: E402
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


def layer_table(model, shape):
    """[(name, multiply-adds for the 2B images, step)] of the convs of the plan of this input shape."""
    plan = model._plan_for(shape, torch.device('cuda'))
    names = {id(m): n for n, m in model.named_modules()}
    rows = []
    for st in plan['steps']:
        if st[0] != 'conv':
            continue
        conv, dst = st[1].conv, plan['bufs'][st[3][0]]
        n, _, ho, wo = dst.shape
        rows.append((names[id(st[1])], n * ho * wo * conv.out_channels * conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1], st))
    return plan, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--precision', default='f16x3', choices=['f16x3', 'bf16x3'])
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--no-cli', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fid.txt'))
    a = ap.parse_args()
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    emit(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__))
    sd = U.synthetic_state_dict(np.load(U.GOLDEN))
    B = a.batch
    g = torch.Generator().manual_seed(1)
    target = torch.rand(B, 3, 512, 512, generator=g).cuda()
    pred = (target + 0.1 * torch.randn(B, 3, 512, 512, generator=g).cuda()).clamp(0, 1)
    m = EV.InceptionV3([3], weights=sd).cuda().set_precision(L.PREC_NAMES[a.precision])
    plain = torch.cat(m.pair(pred, target)).flatten(1)
    mode = 'graph'
    try:
        m.use_graph = True
        assert torch.equal(torch.cat(m.pair(pred, target)).flatten(1), plain), 'graph replay differs from plain launches'
    except Exception as e:                           # capture is not available: plain launches
        m.use_graph, mode = False, f'plain ({type(e).__name__})'
        m._invalidate()
    ms = _time(lambda: m.pair(pred, target), a.steps, a.warmup, a.repeats)
    plan, rows = layer_table(m, pred.shape)
    macs = sum(r[1] for r in rows)
    rec = dict(what='fid feature pass', pairs=B, images=2 * B, source_hw=512, precision=a.precision, mode=mode, hip_ms=round(ms, 3),
               hip_pairs_per_s=round(B * 1000 / ms, 1), gmacs=round(macs / 1e9, 2), tflops=round(2 * macs / ms / 1e9, 1),
               precision_after=m.precision)
    if not a.no_torch:
        net = U.Inception3().eval()
        net.load_state_dict(sd)
        net = net.cuda()

        def eager():
            with torch.no_grad():
                x = torch.nn.functional.interpolate(torch.cat([pred, target]), size=(299, 299), mode='bilinear', align_corners=False)
                return net.features(2 * x - 1).flatten(1)
        tms = _time(eager, max(2, a.steps // 2), 2, a.repeats)
        ev = eager()
        rec.update(torch_eager_fp32_ms=round(tms, 3), ratio_to_eager=round(tms / ms, 2),
                   max_abs_hip_vs_eager_over_max=float((plain - ev).abs().max() / ev.abs().max()))
        del net
    emit(rec)
    # per layer: the launch of each conv on its own, on the plan's buffers
    m.use_graph = False
    n = 2 * B
    per = []
    for name, mac, st in rows:
        def v(ref):
            return L.view(plan['bufs'][ref[0]], ref[1], ref[2])
        us = _time(lambda: st[1].run(v(st[2]), v(st[3]), n, torch.cuda.current_stream().cuda_stream), 20, 3, 3) * 1000
        per.append((us, name, mac))
    total = sum(p[0] for p in per)
    emit(dict(what='conv launches on their own', layers=len(per), sum_us=round(total, 1)))
    for us, name, mac in sorted(per, reverse=True)[:10]:
        emit(dict(layer=name, us=round(us, 1), share=round(us / total, 3), gmacs=round(mac / 1e9, 3), tflops=round(2 * mac / us / 1e6, 1)))
    del m
    torch.cuda.empty_cache()
    if not a.no_cli:
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        import evaluate_bench as EB
        from lama_amd import evaluate as EVL
        with tempfile.TemporaryDirectory() as td:
            datadir, preddir = EB.write_pairs(td, 256, 512)
            ds = EV.PrecomputedInpaintingResultsDataset(datadir, preddir, inpainted_suffix='_inpainted.png', img_suffix='.png', pad_out_to_modulo=8)
            for label, scores in (('ssim', {'ssim': EV.SSIMScore()}),
                                  ('ssim + fid', {'ssim': EV.SSIMScore(), 'fid': EV.FIDScore(weights=sd)})):
                if 'fid' in scores:
                    scores['fid'].model.set_precision(L.PREC_NAMES[a.precision])
                for rnd in range(2):                  # round 0 warms (page cache, code objects, packed weights, plans); round 1 is reported
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    EVL.score_dataset(ds, scores, batch_size=8, io_threads=8)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                emit(dict(what='lama_amd.evaluate device loop, 256 PNG triples of 512^2, batch 8, decode included', scores=label,
                          seconds=round(dt, 3), images_per_s=round(256 / dt, 1)))
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
