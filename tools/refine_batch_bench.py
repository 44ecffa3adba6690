#!/usr/bin/env python3
"""Seconds per image of batched refinement (refine_predict_batch at B = 2, 4, 8) against refine_predict one image at a time (B = 1), on
bench.py's synthetic big-lama weights (f16x3 forward, bf16x3 reverse pass, 15 iterations, max_scales 3), for three workloads of 8 images:

  (a) 8 x 2048^2     at the default px_budget 1800000 (iterating scale ~1341^2, bottleneck planes 168 x 168)
  (b) 8 x 1080x1920  at the default px_budget          (iterating scale ~1006 x 1789, planes 126 x 224)
  (c) 8 x 1024^2     at px_budget 4194304              (scales 512 / 1024: 128 x 128 planes at the iterating one)

Every image has its own random content and mask.  Per (workload, B): one untimed warm-up pass over the 8 images (plans, weight packs,
allocator), then ``--reps`` timed passes (host clock around work that ends in a device synchronise); the median is reported, with the
spread, and torch.cuda.max_memory_allocated over the timed passes.  usage: refine_batch_bench.py [--reps 3] [--out FILE] [--workloads abc]"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _toollib  # noqa: E402,F401
import bench  # noqa: E402
from lama_amd import _lib as L  # noqa: E402
from lama_amd import refinement as RF  # noqa: E402

WORKLOADS = {'a': ('8 x 2048x2048, px_budget 1800000', 2048, 2048, 1800000),
             'b': ('8 x 1080x1920, px_budget 1800000', 1080, 1920, 1800000),
             'c': ('8 x 1024x1024, px_budget 4194304', 1024, 1024, 4194304)}
N_IMAGES = 8
BATCHES = (1, 2, 4, 8)


def make_images(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    imgs, masks = [], []
    for i in range(N_IMAGES):
        imgs.append(torch.rand(1, 3, h, w, generator=g))
        m = torch.zeros(1, 1, h, w)
        y0, x0 = int(h * (0.1 + 0.05 * i)), int(w * (0.1 + 0.04 * i))
        m[:, :, y0:y0 + h // (3 + i % 3), x0:x0 + w // (2 + i % 4)] = 1.0
        masks.append(m)
    return torch.cat(imgs), torch.cat(masks)


def one_pass(model, imgs, masks, h, w, B, px_budget, dev):
    kw = dict(gpu_ids='0,', modulo=8, n_iters=15, lr=0.002, min_side=512, max_scales=3, px_budget=px_budget)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(0, N_IMAGES, B):
        n = min(B, N_IMAGES - i)
        batch = dict(image=imgs[i:i + n].to(dev), mask=masks[i:i + n].to(dev), unpad_to_size=[torch.tensor([h] * n), torch.tensor([w] * n)])
        with contextlib.redirect_stdout(io.StringIO()):          # the pyramid's "Original image too large" notice, once per call
            if B == 1:
                RF.refine_predict(batch, model, **kw)
            else:
                RF.refine_predict_batch(batch, model, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--workloads', default='abc')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('refine_batch_bench.py measures on an MI355X: no GPU visible')
    dev = torch.device('cuda')
    model = bench.build_model(dev, L.PREC_F16X3)
    lines = [f'# refine_batch_bench.py: {torch.cuda.get_device_name(0)}, big-lama synthetic weights (bench.build_model), f16x3 forward / bf16x3 '
             f'reverse pass, n_iters 15, {N_IMAGES} images per pass, median of {a.reps} timed passes after one warm-up pass per (workload, B)',
             f'{"workload":<36} {"B":>2} {"s/image":>8} {"min":>7} {"max":>7} {"speed-up":>8} {"peak GiB":>9}']
    print('\n'.join(lines), flush=True)
    for key in a.workloads:
        name, h, w, budget = WORKLOADS[key]
        imgs, masks = make_images(h, w, seed=100 + ord(key))
        base = None
        for B in BATCHES:
            one_pass(model, imgs, masks, h, w, B, budget, dev)                       # warm-up
            torch.cuda.reset_peak_memory_stats()
            ts = [one_pass(model, imgs, masks, h, w, B, budget, dev) / N_IMAGES for _ in range(a.reps)]
            peak = torch.cuda.max_memory_allocated() / 2 ** 30
            med = statistics.median(ts)
            base = med if B == 1 else base
            ln = f'({key}) {name:<32} {B:>2} {med:8.4f} {min(ts):7.4f} {max(ts):7.4f} {base / med:7.2f}x {peak:9.1f}'
            print(ln, flush=True)
            lines.append(ln)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
