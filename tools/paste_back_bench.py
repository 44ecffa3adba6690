#!/usr/bin/env python3
"""Measure ``paste_back`` (lama_paste_back_u8_fwd; python -m lama_amd.predict ... dataset.scale_factor=F paste_back=true).

    python tools/paste_back_bench.py [--launches 20] [--warmup 5] [--n 48] [--runs 2] [--no-cli] > profiles/paste_back.txt

JSON lines.  Nothing here is a gate: the numbers are recorded in profiles/paste_back.txt and quoted in the README.

Kernel part, per case (8 x 2048^2 -> 512^2 at factor 0.25 and 8 x 1024^2 -> 512^2 at factor 0.5; a sparse mask = a centred box of a quarter of
the area, and a full mask), microseconds as the median of ``--launches`` launches timed one by one with events after ``--warmup`` launches, in
the same process and on the same data:
  paste      lama_paste_back_u8_fwd, one launch for the batch: 7 bytes per source pixel (1 mask + 3 in + 3 out) + the low-resolution tensor;
  d2d_copy   a device-to-device copy of those 7 bytes per pixel (3.5 read + 3.5 written: the floor of moving them once);
  chain      what the kernel replaces -- per image lama_bilinear_fwd to an fp32 [1,3,h,w] tensor, then lama_blend_quantize_u8_fwd on it: two
             launches per image, 24 bytes per source pixel more (the fp32 tensor written and read back).  The chain is not held to the
             restatement (its kernels are compiled with floating-point contraction): the tool reports how many bytes differ, and by how much.
CLI part: images/s of the CLI's own loop over the same ``--n`` PNG pairs of 2048^2 (tmpfs), big-lama shape, synthetic weights, three ways,
alternating, ``--runs`` runs each (the spread of the runs of one way is the A/A spread of the session):
  paste      dataset.scale_factor=0.25 paste_back=true   (source-size PNGs)
  scaled     dataset.scale_factor=0.25                   (512^2 PNGs: what the tool wrote before; the difference is the larger download and encode)
  full       no scale factor, batch_size=1               (the only way to a source-size result before: the generator at 2048^2, one image per
                                                         step -- the batch the refinement leg of bench.py runs at this size)
A way that fails ends the CLI part there: nothing more is started on the GPU after a failed run."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

import _toollib  # noqa: F401
from lama_amd import _lib as L
from lama_amd.predict import encode_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _each(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1) * 1e3)
    return round(statistics.median(ts), 1), round(min(ts), 1)


def kernel_case(lib, side, low, mask_kind, launches, warmup, batch=8):
    g = torch.Generator().manual_seed(side + low)
    img = torch.randint(0, 256, (batch, side, side, 3), generator=g, dtype=torch.uint8).cuda()
    msk = torch.zeros(batch, side, side, dtype=torch.uint8)
    if mask_kind == 'full':
        msk[:] = 255
    else:
        msk[:, side // 4:3 * side // 4, side // 4:3 * side // 4] = 255
    msk = msk.cuda()
    ssz = torch.tensor([[side, side]] * batch, dtype=torch.int32).cuda()
    dsz = torch.tensor([[low, low]] * batch, dtype=torch.int32).cuda()
    lowres = torch.rand(batch, 3, low, low, generator=g).cuda()
    out = torch.empty_like(img)
    st = torch.cuda.current_stream().cuda_stream
    v_low = L.view(lowres)
    paste = _each(lambda: lib.paste_back_u8(img, msk, ssz, dsz, v_low, out, batch, stream=st), launches, warmup)
    # the floor: the same 7 bytes per pixel moved once, device to device
    src = torch.empty(batch * side * side * 7 // 2, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    copy = _each(lambda: dst.copy_(src), launches, warmup)
    del src, dst
    # the two-launch chain per image
    up = torch.empty(1, 3, side, side, device='cuda')
    out2 = torch.empty_like(img)
    v_up = L.view(up)
    lows = [L.view(lowres[b:b + 1]) for b in range(batch)]

    def chain():
        for b in range(batch):
            lib.bilinear(lows[b], v_up, 1, stream=st)
            lib.blend_quantize_u8(img[b:b + 1], msk[b:b + 1], None, v_up, out2[b:b + 1], 1, stream=st)
    ch = _each(chain, launches, warmup)
    px = batch * side * side
    mb = (7 * px + lowres.numel() * 4) / 1e6
    print(json.dumps(dict(what='kernel', case=f'{batch} x {side}^2 <- {low}^2', mask=mask_kind, masked_share=round(float((msk != 0).float().mean()), 3),
                          paste_us=paste[0], paste_us_min=paste[1], mb_moved=round(mb, 1), paste_gb_per_s=round(mb / paste[0] * 1e3, 1),
                          d2d_copy_7B_per_px_us=copy[0], d2d_copy_us_min=copy[1], ratio_to_copy=round(paste[0] / copy[0], 3),
                          chain_us=ch[0], chain_us_min=ch[1], chain_launches=2 * batch, chain_over_paste=round(ch[0] / paste[0], 2),
                          bytes_differing_from_chain=int((out != out2).sum()),
                          max_level_difference=int((out.to(torch.int16) - out2.to(torch.int16)).abs().max()))), flush=True)


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


def run_cli(mdir, indir, outdir, extra):
    r = subprocess.run([sys.executable, '-m', 'lama_amd.predict', f'model.path={mdir}', f'indir={indir}', f'outdir={outdir}'] + extra,
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    m = re.search(r'wrote (\d+) images .*\(([\d.]+) images/s', r.stdout)
    if r.returncode != 0 or not m:
        raise RuntimeError(f'predict failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
    from PIL import Image
    first = sorted(os.listdir(outdir))[0]
    with Image.open(os.path.join(outdir, first)) as im:
        size = im.size
    shutil.rmtree(outdir, ignore_errors=True)
    return int(m.group(1)), float(m.group(2)), size


def cli_part(n, runs, side=2048, factor=0.25):
    import yaml
    import bench
    model = bench.build_model(torch.device('cuda', 0), L.PREC_F16X3)
    tmp = tempfile.mkdtemp(prefix='lama_paste_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
    try:
        mdir = os.path.join(tmp, 'model')
        os.makedirs(os.path.join(mdir, 'models'))
        with open(os.path.join(mdir, 'config.yaml'), 'w') as f:
            yaml.safe_dump(dict(training_model=dict(kind='default', concat_mask=True), generator=dict(bench.BIG_LAMA)), f)
        torch.save({'state_dict': {k: v.detach().cpu() for k, v in model.state_dict().items()}}, os.path.join(mdir, 'models', 'best.ckpt'))
        del model
        torch.cuda.empty_cache()
        indir = os.path.join(tmp, 'in')
        write_pairs(indir, n, side)
        ways = dict(paste=['batch_size=8', f'dataset.scale_factor={factor}', 'paste_back=true'], scaled=['batch_size=8', f'dataset.scale_factor={factor}'],
                    full=['batch_size=1'])
        rates = {k: [] for k in ways}
        for k in range(runs):
            for way, extra in ways.items():                      # alternating: the box's drift hits every way alike
                cnt, ips, size = run_cli(mdir, indir, os.path.join(tmp, 'out'), extra)
                rates[way].append(ips)
                print(json.dumps(dict(what='cli_run', way=way, run=k, images=cnt, source=f'{side}^2', png_size=list(size), images_per_s=ips)), flush=True)
        print(json.dumps(dict(what='cli', images=n, source=f'{side}^2', factor=factor,
                              **{f'{w}_images_per_s_median': round(statistics.median(v), 2) for w, v in rates.items()},
                              **{f'{w}_runs': v for w, v in rates.items()},
                              aa_spread_percent={w: round(100 * (max(v) - min(v)) / statistics.median(v), 1) for w, v in rates.items()})), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--n', type=int, default=48)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--no-cli', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('paste_back_bench needs an MI355X: a CPU run measures nothing')
    lib = L.get_lib()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, host_cpus=os.cpu_count())), flush=True)
    for side, low in ((2048, 512), (1024, 512)):
        for mask_kind in ('sparse', 'full'):
            kernel_case(lib, side, low, mask_kind, a.launches, a.warmup)
    if not a.no_cli:
        cli_part(a.n, a.runs)


if __name__ == '__main__':
    main()
