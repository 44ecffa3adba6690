#!/usr/bin/env python3
"""``python -m lama_amd.predict ... dataset.scale_factor=F batch_size=8`` on N synthetic PNG pairs (tmpfs), big-lama shape, synthetic weights:
images/s of the CLI's own loop (median of the runs), a digest of the PNGs it wrote, the unscaled rate on images of the same OUTPUT size, and
the resize kernel's own time from HIP events.
usage: scale_probe.py [--n 256] [--side 1024] [--factor 0.5] [--runs 3] [--roots DIR[,DIR...]]
``--roots``: checkouts (with built libraries) to run the CLI from, alternating run by run -- this tree when omitted; a second checkout of an
earlier commit gives the A/B of one session."""
import argparse
import hashlib
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lama_amd import _lib as L  # noqa: E402
from lama_amd.predict import encode_png, scaled_size  # noqa: E402


def write_pairs(indir, n, side):
    os.makedirs(indir)
    base = np.random.RandomState(7).randint(0, 256, (side + 64, side + 64, 3)).astype('uint8')
    m = np.zeros((side, side), 'uint8')
    m[side // 4: 3 * side // 4, side // 4: 3 * side // 4] = 255
    mpng = encode_png(m)
    for i in range(n):
        oy, ox = (i * 7) % 64, (i * 13) % 64
        with open(os.path.join(indir, f'im{i:05d}.png'), 'wb') as f:
            f.write(encode_png(base[oy:oy + side, ox:ox + side]))
        with open(os.path.join(indir, f'im{i:05d}_mask001.png'), 'wb') as f:
            f.write(mpng)


def digest(outdir):
    h = hashlib.sha256()
    for dp, _, fs in sorted(os.walk(outdir)):
        for fn in sorted(fs):
            h.update(fn.encode())
            with open(os.path.join(dp, fn), 'rb') as f:
                h.update(f.read())
    return h.hexdigest()[:16]


def run_cli(root, mdir, indir, outdir, extra):
    r = subprocess.run([sys.executable, '-m', 'lama_amd.predict', f'model.path={mdir}', f'indir={indir}', f'outdir={outdir}', 'batch_size=8'] + extra,
                       cwd=root, capture_output=True, text=True, timeout=900)
    m = re.search(r'wrote (\d+) images .*\(([\d.]+) images/s', r.stdout)
    if r.returncode != 0 or not m:
        raise RuntimeError(f'predict failed in {root}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
    d = digest(outdir)
    shutil.rmtree(outdir, ignore_errors=True)
    return int(m.group(1)), float(m.group(2)), d


def kernel_time(side, factor, batch=8, reps=50):
    lib = L.get_lib()
    dh, dw = scaled_size(side, side, factor)
    Hp, Wp = (dh + 7) // 8 * 8, (dw + 7) // 8 * 8
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (batch, side, side, 3), generator=g, dtype=torch.uint8).cuda()
    msk = torch.randint(0, 2, (batch, side, side), generator=g, dtype=torch.uint8).cuda()
    ssz = torch.tensor([[side, side]] * batch, dtype=torch.int32).cuda()
    dsz = torch.tensor([[dh, dw]] * batch, dtype=torch.int32).cuda()
    oi, om = torch.empty(batch, 3, Hp, Wp, device='cuda'), torch.empty(batch, 1, Hp, Wp, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(5):
        lib.resize_u8(img, msk, ssz, dsz, factor, L.view(oi), L.view(om), batch, stream=st)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        lib.resize_u8(img, msk, ssz, dsz, factor, L.view(oi), L.view(om), batch, stream=st)
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / reps
    moved = img.numel() + msk.numel() + 4 * (oi.numel() + om.numel())
    print(f'lama_resize_u8_fwd {batch} x {side}^2 -> {Hp} x {Wp} at factor {factor}: {ms * 1e3:.1f} us per launch (HIP events, {reps} launches back to back), '
          f'{moved / ms / 1e6:.0f} GB/s of the {moved / 1e6:.1f} MB it reads and writes', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=256)
    ap.add_argument('--side', type=int, default=1024)
    ap.add_argument('--factor', type=float, default=0.5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--roots', default=ROOT)
    a = ap.parse_args()
    roots = [os.path.abspath(r) for r in a.roots.split(',')]
    model = bench.build_model(torch.device('cuda', 0), L.PREC_F16X3)
    tmp = tempfile.mkdtemp(prefix='lama_scale_', dir='/dev/shm')
    try:
        mdir = os.path.join(tmp, 'model')
        os.makedirs(os.path.join(mdir, 'models'))
        with open(os.path.join(mdir, 'config.yaml'), 'w') as f:
            yaml.safe_dump(dict(training_model=dict(kind='default', concat_mask=True), generator=dict(bench.BIG_LAMA)), f)
        torch.save({'state_dict': {k: v.detach().cpu() for k, v in model.state_dict().items()}}, os.path.join(mdir, 'models', 'best.ckpt'))
        del model
        torch.cuda.empty_cache()
        kernel_time(a.side, a.factor)
        out_side = scaled_size(a.side, a.side, a.factor)[0]
        big, small = os.path.join(tmp, 'in_big'), os.path.join(tmp, 'in_small')
        write_pairs(big, a.n, a.side)
        write_pairs(small, a.n, out_side)
        rates = {r: [] for r in roots}
        digests = {r: set() for r in roots}
        for k in range(a.runs):
            for r in roots:                                                     # alternating: the box's drift hits every tree alike
                n, ips, d = run_cli(r, mdir, big, os.path.join(tmp, 'out'), [f'dataset.scale_factor={a.factor}'])
                rates[r].append(ips)
                digests[r].add(d)
                print(f'run {k} {r}: {n} images of {a.side}^2 at scale_factor={a.factor}: {ips:.1f} images/s, PNG digest {d}', flush=True)
        plain = []
        for k in range(a.runs):
            n, ips, d = run_cli(roots[0], mdir, small, os.path.join(tmp, 'out'), [])
            plain.append(ips)
            print(f'run {k} {roots[0]}: {n} images of {out_side}^2, unscaled: {ips:.1f} images/s', flush=True)
        for r in roots:
            print(f'MEDIAN scaled   {r}: {statistics.median(rates[r]):.1f} images/s  (runs {rates[r]}; digests {sorted(digests[r])})')
        print(f'MEDIAN unscaled {roots[0]}: {statistics.median(plain):.1f} images/s  (runs {plain})')
        if len(roots) > 1:
            print(f'ratio {roots[0]} / {roots[1]}: {statistics.median(rates[roots[0]]) / statistics.median(rates[roots[1]]):.2f}x; '
                  f'same PNG bytes: {digests[roots[0]] == digests[roots[1]] and len(digests[roots[0]]) == 1}')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
