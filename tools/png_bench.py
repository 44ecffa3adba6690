#!/usr/bin/env python3
"""Measure the device PNG encoder (lama_png_deflate_u8_fwd; python -m lama_amd.predict ... device_png=true).

    python tools/png_bench.py [--launches 20] [--warmup 5] [--runs 3] [--n512 512] [--n2048 48] [--no-cli] > profiles/png_encode.txt

JSON lines.  Nothing here is a gate: the numbers are recorded in profiles/png_encode.txt and quoted in DESIGN 4.21 and the README.

Kernel part, per case (8 x 512^2 and 8 x 2048^2, full crops, default chunk; a photo-like and a uniformly random input), microseconds as the median
of ``--launches`` calls timed one by one with events after ``--warmup`` calls, in the same process and on the same data:
  encode     lama_png_deflate_u8_fwd: its two launches together, and each launch's own time from the profiler's kernel records where it gives any;
  d2d_copy   a device-to-device copy of the same u8 bytes (the floor of reading them once and writing as many);
  merge      the serial table build: the profiling build with LAMA_PNG_MERGE_REPS=2 runs the (idempotent) two-queue merge twice, the time added is its own.
Host part: milliseconds per image of predict.encode_png (filter + zlib level 1 Z_RLE + container) against predict.png_from_zlib (one CRC + the
container) on the same images, and the file sizes of both.
CLI part: images/s of the CLI's own loop, device_png off and on, alternating, ``--runs`` runs each way (the spread of one way's runs is the A/A
spread of the session), at io_threads 4 and 16: ``--n512`` PNG pairs of 512^2, and ``--n2048`` pairs of 2048^2 with dataset.scale_factor=0.25
paste_back=true.  Big-lama shape, synthetic weights, files on tmpfs.  A run that fails ends the CLI part there: nothing more is started on the GPU."""
import argparse
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
from lama_amd import build as B
from lama_amd.predict import encode_png, png_from_zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def photo(h, w, seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[:h, :w].astype(np.float32)
    base = (128 + 60 * np.sin(x / 9.0) + 50 * np.cos(y / 7.0))[..., None] + np.arange(3, dtype=np.float32) * 10
    return np.clip(base + rs.randn(h, w, 3).astype(np.float32) * 6, 0, 255).astype(np.uint8)


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


def _per_kernel(fn, launches):
    """Median microseconds per kernel name over ``launches`` calls, from the profiler's device records ({} where it has none)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(launches):
                fn()
            torch.cuda.synchronize()
        per = {}
        for ev in prof.events():
            if 'png_' in ev.name:
                per.setdefault('encode' if 'encode' in ev.name else 'assemble', []).append(ev.device_time)
        return {k: round(statistics.median(v), 1) for k, v in per.items()}
    except Exception as e:      # noqa: BLE001 -- the profiler is optional here
        return dict(profiler_error=str(e)[:200])


def kernel_case(lib, prof_lib, side, kind, launches, warmup, batch=8):
    imgs = np.stack([photo(side, side, b) if kind == 'photo' else np.random.RandomState(b).randint(0, 256, (side, side, 3)).astype(np.uint8)
                     for b in range(batch)])
    img = torch.from_numpy(imgs).cuda()
    sizes = torch.tensor([[side, side]] * batch, dtype=torch.int32).cuda()
    stride = (lib.png_deflate_bound(side, side, 3, 0) + 15) & ~15
    out = torch.empty(batch * stride, dtype=torch.uint8, device='cuda')
    n_out = torch.zeros(batch, dtype=torch.int32, device='cuda')
    ws = torch.empty(lib.png_deflate_workspace_bytes(batch, side, side, 3, 0), dtype=torch.uint8, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def call(which=lib):
        which.png_deflate_u8(img, sizes, out, stride, n_out, ws, batch, stream=st)
    enc = _each(call, launches, warmup)
    per = _per_kernel(call, launches)
    dst = torch.empty_like(img)
    copy = _each(lambda: dst.copy_(img), launches, warmup)
    merge = {}
    if prof_lib is not None:
        os.environ['LAMA_PNG_MERGE_REPS'] = '1'
        one = _each(lambda: call(prof_lib), launches, warmup)
        os.environ['LAMA_PNG_MERGE_REPS'] = '2'
        two = _each(lambda: call(prof_lib), launches, warmup)
        os.environ['LAMA_PNG_MERGE_REPS'] = '1'
        merge = dict(prof_build_us=one[0], prof_build_merge_twice_us=two[0], serial_merge_us=round(two[0] - one[0], 1),
                     serial_merge_share_of_call=round((two[0] - one[0]) / one[0], 3))
    lens = n_out.cpu().numpy()
    host = out.cpu().numpy()
    streams = [host[j * stride:j * stride + int(lens[j])].tobytes() for j in range(batch)]
    # the host's share, and the sizes
    t0 = time.perf_counter()
    files_host = [encode_png(imgs[j]) for j in range(batch)]
    t1 = time.perf_counter()
    files_dev = [png_from_zlib(side, side, 3, s) for s in streams]
    t2 = time.perf_counter()
    from PIL import Image
    import io
    assert all(np.array_equal(np.array(Image.open(io.BytesIO(f))), imgs[j]) for j, f in enumerate(files_dev))
    raw = batch * side * (1 + 3 * side)
    print(json.dumps(dict(what='kernel', case=f'{batch} x {side}^2', input=kind, chunks_per_image=-(-side // max(1, 24576 // (1 + 3 * side))),
                          encode_call_us=enc[0], encode_call_us_min=enc[1], per_launch_us=per, d2d_copy_us=copy[0], d2d_copy_us_min=copy[1],
                          ratio_to_copy=round(enc[0] / copy[0], 2), u8_mb=round(img.numel() / 1e6, 2), **merge,
                          host_encode_png_ms_per_image=round((t1 - t0) / batch * 1e3, 3), host_png_from_zlib_ms_per_image=round((t2 - t1) / batch * 1e3, 3),
                          file_bytes_encode_png=sum(map(len, files_host)), file_bytes_device=sum(map(len, files_dev)),
                          device_over_encode_png=round(sum(map(len, files_dev)) / sum(map(len, files_host)), 4),
                          device_share_of_raw=round(sum(map(len, streams)) / raw, 4))), flush=True)


def write_pairs(indir, n, side):
    os.makedirs(indir)
    base = photo(side + 64, side + 64, 7)
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
    size = sum(os.path.getsize(os.path.join(outdir, f)) for f in os.listdir(outdir))
    shutil.rmtree(outdir, ignore_errors=True)
    return int(m.group(1)), float(m.group(2)), size


def cli_part(runs, n512, n2048):
    import yaml
    import bench
    model = bench.build_model(torch.device('cuda', 0), L.PREC_F16X3)
    tmp = tempfile.mkdtemp(prefix='lama_png_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
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
                                                 ['batch_size=8', f'io_threads={io_threads}', f'device_png={"true" if way == "on" else "false"}'] + extra)
                        rates[way].append(ips)
                        sizes[way] = size
                print(json.dumps(dict(what='cli', dataset=name, images=n, io_threads=io_threads, host_cpus=os.cpu_count(),
                                      off_images_per_s_median=statistics.median(rates['off']), on_images_per_s_median=statistics.median(rates['on']),
                                      off_runs=rates['off'], on_runs=rates['on'],
                                      spread_percent={w: round(100 * (max(v) - min(v)) / statistics.median(v), 1) for w, v in rates.items()},
                                      on_over_off=round(statistics.median(rates['on']) / statistics.median(rates['off']), 3),
                                      output_bytes=sizes, on_over_off_bytes=round(sizes['on'] / sizes['off'], 4))), flush=True)
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
        raise SystemExit('png_bench needs an MI355X: a CPU run measures nothing')
    lib = L.get_lib()
    prof_lib = L.LamaLib(B.LIB_PROF) if os.path.exists(B.LIB_PROF) else None
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, host_cpus=os.cpu_count(),
                          cpus_usable=len(os.sched_getaffinity(0)))), flush=True)
    for side in (512, 2048):
        for kind in ('photo', 'random'):
            kernel_case(lib, prof_lib, side, kind, a.launches, a.warmup)
    if not a.no_cli:
        cli_part(a.runs, a.n512, a.n2048)


if __name__ == '__main__':
    main()
