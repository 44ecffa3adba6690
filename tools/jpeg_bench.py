#!/usr/bin/env python3
"""Measure the device JPEG encoder (lama_jpeg_scan_u8_fwd; python -m lama_amd.predict ... out_ext=.jpg device_jpeg=true).

    python tools/jpeg_bench.py [--launches 20] [--warmup 5] [--runs 3] [--n512 512] [--n2048 48] [--no-cli] > profiles/jpeg_encode.txt

JSON lines.  Nothing here is a gate: the numbers are recorded in profiles/jpeg_encode.txt and quoted in DESIGN 4.22 and the README.

Kernel part, per case (8 x 512^2 and 8 x 2048^2, full crops, quality 95, 4:2:0 and 4:4:4; the photo-like input of tools/png_bench.py), microseconds as
the median of ``--launches`` calls timed one by one with events after ``--warmup`` calls, in the same process and on the same data:
  encode     lama_jpeg_scan_u8_fwd: its three launches together, and each launch's own time from the profiler's kernel records where it gives any;
  d2d_copy   a device-to-device copy of the same u8 bytes (the floor of reading them once and writing as many).
Host part: milliseconds per image of PIL.Image.save(quality=95) into memory on one thread against predict.jpeg_from_scan (the headers and one copy)
on the same images, and the file sizes of both.  ``condition``: the call's device time per image plus the host's share, against PIL's time.
CLI part: images/s of the CLI's own loop with out_ext=.jpg, device_jpeg off (PIL at its defaults, the parent commit's path) and on, alternating,
``--runs`` runs each way (the spread of one way's runs is the A/A spread of the session), at io_threads 4 and 16: ``--n512`` PNG pairs of 512^2, and
``--n2048`` pairs of 2048^2 with dataset.scale_factor=0.25 paste_back=true.  Big-lama shape, synthetic weights, files on tmpfs.  A run that fails
ends the CLI part there: nothing more is started on the GPU."""
import argparse
import io
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

import _toollib  # noqa: F401
from lama_amd import _lib as L
from lama_amd.predict import jpeg_from_scan
from png_bench import _each, photo, write_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _per_kernel(fn, launches):
    """Median microseconds per kernel over ``launches`` calls, from the profiler's device records ({} where it has none)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(launches):
                fn()
            torch.cuda.synchronize()
        per = {}
        for ev in prof.events():
            if 'jpeg_' in ev.name:
                key = 'offsets' if 'offsets' in ev.name else ('emit' if 'ELb1' in ev.name or 'true' in ev.name else 'count')
                per.setdefault(key, []).append(ev.device_time)
        return {k: round(statistics.median(v), 1) for k, v in per.items()}
    except Exception as e:      # noqa: BLE001 -- the profiler is optional here
        return dict(profiler_error=str(e)[:200])


def kernel_case(lib, side, ss_name, launches, warmup, batch=8, quality=95):
    from PIL import Image
    ss = L.JPEG_420 if ss_name == '420' else L.JPEG_444
    imgs = np.stack([photo(side, side, b) for b in range(batch)])
    img = torch.from_numpy(imgs).cuda()
    sizes = torch.tensor([[side, side]] * batch, dtype=torch.int32).cuda()
    stride = side * side * 3
    out = torch.empty(batch * stride, dtype=torch.uint8, device='cuda')
    n_out = torch.zeros(batch, dtype=torch.int32, device='cuda')
    ws = torch.empty(lib.jpeg_scan_workspace_bytes(batch, side, side, ss), dtype=torch.uint8, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def call():
        lib.jpeg_scan_u8(img, sizes, out, stride, n_out, ws, batch, quality=quality, subsampling=ss, stream=st)
    enc = _each(call, launches, warmup)
    per = _per_kernel(call, launches)
    dst = torch.empty_like(img)
    copy = _each(lambda: dst.copy_(img), launches, warmup)
    lens = n_out.cpu().numpy()
    assert (lens > 0).all(), lens
    host = out.cpu().numpy()
    scans = [host[j * stride:j * stride + int(lens[j])].tobytes() for j in range(batch)]
    t0 = time.perf_counter()
    files_pil = []
    for j in range(batch):
        b = io.BytesIO()
        Image.fromarray(imgs[j]).save(b, 'JPEG', quality=quality, subsampling=2 if ss else 0)
        files_pil.append(b.getvalue())
    t1 = time.perf_counter()
    files_dev = [jpeg_from_scan(side, side, quality, ss, s) for s in scans]
    t2 = time.perf_counter()

    def psnr(data, j):
        d = np.array(Image.open(io.BytesIO(data))).astype(np.float64) - imgs[j]
        return 10 * np.log10(255.0 ** 2 / np.mean(d * d))
    pil_ms, host_ms = (t1 - t0) / batch * 1e3, (t2 - t1) / batch * 1e3
    dev_ms = enc[0] / batch * 1e-3
    print(json.dumps(dict(what='kernel', case=f'{batch} x {side}^2', quality=quality, subsampling=ss_name, encode_call_us=enc[0], encode_call_us_min=enc[1],
                          per_launch_us=per, d2d_copy_us=copy[0], d2d_copy_us_min=copy[1], ratio_to_copy=round(enc[0] / copy[0], 2),
                          u8_mb=round(img.numel() / 1e6, 2), host_pil_save_ms_per_image=round(pil_ms, 3),
                          host_jpeg_from_scan_ms_per_image=round(host_ms, 3),
                          condition=dict(device_ms_per_image=round(dev_ms, 4), plus_host_ms=round(dev_ms + host_ms, 3), pil_ms=round(pil_ms, 3),
                                         holds=bool(dev_ms + host_ms < pil_ms)),
                          file_bytes_pil=sum(map(len, files_pil)), file_bytes_device=sum(map(len, files_dev)),
                          device_over_pil=round(sum(map(len, files_dev)) / sum(map(len, files_pil)), 4),
                          psnr_db_device=round(psnr(files_dev[0], 0), 3), psnr_db_pil=round(psnr(files_pil[0], 0), 3),
                          scan_share_of_raw=round(sum(map(len, scans)) / img.numel(), 4))), flush=True)


def run_cli(mdir, indir, outdir, extra):
    r = subprocess.run([sys.executable, '-m', 'lama_amd.predict', f'model.path={mdir}', f'indir={indir}', f'outdir={outdir}'] + extra,
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    m = re.search(r'wrote (\d+) images .*\(([\d.]+) images/s', r.stdout)
    if r.returncode != 0 or not m:
        raise RuntimeError(f'predict failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
    size = sum(os.path.getsize(os.path.join(outdir, f)) for f in os.listdir(outdir))
    shutil.rmtree(outdir, ignore_errors=True)
    return int(m.group(1)), float(m.group(2)), size


def cli_part(runs, n512, n2048):
    import yaml
    import bench
    model = bench.build_model(torch.device('cuda', 0), L.PREC_F16X3)
    tmp = tempfile.mkdtemp(prefix='lama_jpeg_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
    try:
        mdir = os.path.join(tmp, 'model')
        os.makedirs(os.path.join(mdir, 'models'))
        with open(os.path.join(mdir, 'config.yaml'), 'w') as f:
            yaml.safe_dump(dict(training_model=dict(kind='default', concat_mask=True), generator=dict(bench.BIG_LAMA)), f)
        torch.save({'state_dict': {k: v.detach().cpu() for k, v in model.state_dict().items()}}, os.path.join(mdir, 'models', 'best.ckpt'))
        del model
        torch.cuda.empty_cache()
        for name, n, side, extra in (('512^2', n512, 512, []), ('2048^2 scale 0.25 paste_back', n2048, 2048, ['dataset.scale_factor=0.25', 'paste_back=true'])):
            if n <= 0:
                continue
            indir = os.path.join(tmp, f'in{side}')
            write_pairs(indir, n, side)
            for io_threads in (4, 16):
                rates, sizes = dict(off=[], on=[]), {}
                for k in range(runs):
                    for way in ('off', 'on'):                     # alternating: the box's drift hits both ways alike
                        cnt, ips, size = run_cli(mdir, indir, os.path.join(tmp, 'out'),
                                                 ['batch_size=8', f'io_threads={io_threads}', 'out_ext=.jpg'] + (['device_jpeg=true'] if way == 'on' else []) + extra)
                        rates[way].append(ips)
                        sizes[way] = size
                print(json.dumps(dict(what='cli', dataset=name, images=n, io_threads=io_threads, host_cpus=os.cpu_count(),
                                      off='PIL quality 75', on='device quality 95 4:2:0',
                                      off_images_per_s_median=statistics.median(rates['off']), on_images_per_s_median=statistics.median(rates['on']),
                                      off_runs=rates['off'], on_runs=rates['on'],
                                      spread_percent={w: round(100 * (max(v) - min(v)) / statistics.median(v), 1) for w, v in rates.items()},
                                      on_over_off=round(statistics.median(rates['on']) / statistics.median(rates['off']), 3),
                                      output_bytes=sizes)), flush=True)
            shutil.rmtree(indir, ignore_errors=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--n512', type=int, default=512)
    ap.add_argument('--n2048', type=int, default=48)
    ap.add_argument('--no-cli', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_bench needs an MI355X: a CPU run measures nothing')
    lib = L.get_lib()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, host_cpus=os.cpu_count(),
                          cpus_usable=len(os.sched_getaffinity(0)))), flush=True)
    for side in (512, 2048):
        for ss in ('420', '444'):
            kernel_case(lib, side, ss, a.launches, a.warmup)
    if not a.no_cli:
        cli_part(a.runs, a.n512, a.n2048)


if __name__ == '__main__':
    main()
