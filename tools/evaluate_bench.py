"""A/B of the evaluation loop's input form on one box: the device ingest (u8 upload + lama_eval_ingest_u8_fwd) against the host float conversion
(astype / 255, np.pad symmetric, CHW, fp32 upload -- what the reference's loader does), same PNG files, same scores, same loop.

    python tools/evaluate_bench.py [--n 256] [--size 512] [--batch 8] [--io-threads 8] [--model-path heads.pth --backbone vgg16.pth]

Writes both rates (images / s over the loop's wall time, decode included) and the ingest kernel's time per batch (50 launches captured in one hipGraph, hipEvents
around its replay)
to profiles/evaluate.txt.  SSIM only unless the LPIPS files are given.  No threshold: this reports."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lama_amd import _lib as L  # noqa: E402
from lama_amd import evaluate as EVL  # noqa: E402
from lama_amd import evaluation as EV  # noqa: E402


class HostIngest(EVL.DeviceIngest):
    """The comparator: fp32 CHW batches built on the host (data.py:12-33), uploaded from pinned memory; the clamp as the reference does it."""

    def __init__(self, lib, bucket, batch_size, device, pad_mod, clamp):
        (Hp, Wp) = bucket['shape']
        self.pad_mod, self.clamp, self.device = pad_mod, clamp, device
        self.hostf = [dict(image=torch.zeros(batch_size, 3, Hp, Wp, pin_memory=True), inpainted=torch.zeros(batch_size, 3, Hp, Wp, pin_memory=True),
                           mask=torch.zeros(batch_size, 1, Hp, Wp, pin_memory=True)) for _ in range(2)]
        self.free = [None, None]
        self.devf = {k: torch.empty_like(v, device=device) for k, v in self.hostf[0].items()}

    def _item(self, a):
        a = a[None] if a.ndim == 2 else np.transpose(a, (2, 0, 1))
        a = a.astype('float32') / 255
        _, h, w = a.shape
        return np.pad(a, ((0, 0), (0, EVL.ceil_modulo(h, self.pad_mod) - h), (0, EVL.ceil_modulo(w, self.pad_mod) - w)), mode='symmetric')

    def fill(self, k, items):
        if self.free[k] is not None:
            self.free[k].synchronize()
            self.free[k] = None
        for j, it in enumerate(items):
            for key in ('image', 'inpainted', 'mask'):
                self.hostf[k][key][j] = torch.from_numpy(self._item(it[key]))
        return [it['mask'].shape for it in items]

    def run(self, k, sizes):
        n = len(sizes)
        for key in self.devf:
            self.devf[key][:n].copy_(self.hostf[k][key][:n], non_blocking=True)
        self.free[k] = torch.cuda.Event()
        self.free[k].record(torch.cuda.current_stream(self.device))
        image = self.devf['image'][:n]
        if self.clamp is not None:
            image = torch.clamp(image, min=self.clamp[0], max=self.clamp[1])
        Hp, Wp = image.shape[-2:]
        sums = torch.round(self.devf['mask'][:n].double().sum(dim=(1, 2, 3)) * 255.0).long()     # (exact: every term is k / 255 in fp32, the sum in fp64)
        return image, self.devf['inpainted'][:n], sums


def write_pairs(root, n, size, seed=0):
    from PIL import Image
    g = np.random.default_rng(seed)
    data, pred = os.path.join(root, 'data'), os.path.join(root, 'pred')
    os.makedirs(data), os.makedirs(pred)
    for i in range(n):
        img = g.integers(0, 256, (size, size, 3), dtype=np.uint8)
        mask = np.zeros((size, size), np.uint8)
        y, x, s = (int(v) for v in g.integers(0, size // 2, 3))
        mask[y:y + s + 8, x:x + s + 8] = 255
        out = img.copy()
        out[mask > 0] = g.integers(0, 256, (int((mask > 0).sum()), 3), dtype=np.uint8)
        Image.fromarray(img).save(os.path.join(data, f'im{i:05d}.png'), compress_level=1)
        Image.fromarray(mask).save(os.path.join(data, f'im{i:05d}_mask000.png'), compress_level=1)
        Image.fromarray(out).save(os.path.join(pred, f'im{i:05d}_mask000_inpainted.png'), compress_level=1)
    return data, pred


def kernel_us(batch, size, reps=50, rounds=7):
    """Device time of one ingest launch: ``reps`` launches captured into ONE hipGraph (so the host's call rate through the Python binding is not
    in the figure), hipEvents around a replay, the median of ``rounds`` replays divided by ``reps``."""
    lib = L.get_lib()
    gt = torch.randint(0, 256, (batch, size, size, 3), dtype=torch.uint8, device='cuda')
    pr = torch.randint(0, 256, (batch, size, size, 3), dtype=torch.uint8, device='cuda')
    mk = torch.randint(0, 256, (batch, size, size), dtype=torch.uint8, device='cuda')
    oi, op = torch.empty(batch, 3, size, size, device='cuda'), torch.empty(batch, 3, size, size, device='cuda')
    sums = torch.empty(batch, dtype=torch.int64, device='cuda')
    for _ in range(5):
        lib.eval_ingest_u8(gt, pr, mk, None, 8, oi, op, sums, batch, stream=L.LamaLib.stream_of(oi))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            lib.eval_ingest_u8(gt, pr, mk, None, 8, oi, op, sums, batch, stream=L.LamaLib.stream_of(oi))
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1000.0 / reps)
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=256)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--io-threads', type=int, default=8)
    ap.add_argument('--model-path', default=None)
    ap.add_argument('--backbone', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'evaluate.txt'))
    a = ap.parse_args()
    lines = [f'evaluate_bench: {a.n} PNG triples of {a.size}x{a.size}, batch {a.batch}, io_threads {a.io_threads}, '
             f'scores: {"ssim + lpips" if a.model_path or a.backbone else "ssim"}, {torch.cuda.get_device_name(0)}']
    with tempfile.TemporaryDirectory() as td:
        data, pred = write_pairs(td, a.n, a.size)
        ds = EV.PrecomputedInpaintingResultsDataset(data, pred, inpainted_suffix='_inpainted.png', img_suffix='.png', pad_out_to_modulo=8)
        scores = {'ssim': EV.SSIMScore()}
        if a.model_path or a.backbone:
            scores['lpips'] = EV.LPIPSScore(model_path=a.model_path, backbone=a.backbone)
        vals = {}
        for rnd in range(2):                          # round 0 warms both forms (page cache, plans); round 1 is reported
            for name, ing in (('device ingest (u8 upload)', EVL.DeviceIngest), ('host float conversion (fp32 upload)', HostIngest)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                EVL.score_dataset(ds, scores, batch_size=a.batch, io_threads=a.io_threads, ingest=ing)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                vals[name] = {k: s.individual_values.copy() for k, s in scores.items()}
                if rnd:
                    lines.append(f'{name}: {a.n / dt:.1f} images/s ({dt:.3f} s)')
        (n0, v0), (n1, v1) = vals.items()
        lines.append('per-image values of the two forms identical: ' + str(all(np.array_equal(v0[k], v1[k]) for k in v0)))
    lines.append(f'lama_eval_ingest_u8_fwd, {a.batch} x {a.size}^2: {kernel_us(a.batch, a.size):.1f} us per launch (replay of 50 captured launches) '
                 f'{a.batch * a.size * a.size * 31 / 1e6:.1f} MB moved')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
