#!/usr/bin/env python3
"""Measure ``crop_to_mask`` (lama_crop_compose_u8_fwd / lama_crop_paste_u8_fwd; python -m lama_amd.predict ... crop_to_mask=true).

    python tools/crop_bench.py [--launches 20] [--warmup 5] [--n 48] [--runs 3] [--io-threads 4 16] [--no-cli] > profiles/crop_to_mask.txt

JSON lines.  Nothing here is a gate: the numbers are recorded in profiles/crop_to_mask.txt and quoted in the README.

Kernel part, per case (8 x 2048^2 sources with 512^2 windows, 8 x 1024^2 with 384^2 windows; the mask a centred box of a quarter of the window;
the windows at x0 % 4 == 0 and at x0 % 4 == 1), microseconds as the median of ``--launches`` launches timed one by one with events after
``--warmup`` launches, in the same process and on the same data:
  compose    lama_crop_compose_u8_fwd, one launch for the batch: 4 bytes read and 16 written per window pixel;
  paste      lama_crop_paste_u8_fwd, one launch for the batch: 7 bytes per SOURCE pixel (1 mask + 3 in + 3 out) + the prediction under the mask;
  d2d_copy   a device-to-device copy of the bytes each of them moves (half read, half written: the floor of moving them once);
  compose_u8 lama_mask_compose_u8_fwd on a slot batch of the window's size: what the compose does when the crop has been made on the host.
CLI part: images/s of the CLI's own loop over the same ``--n`` PNG pairs of 2048^2 (tmpfs) with box masks of about 5 % of the area at varying
positions, big-lama shape, synthetic weights, three ways, alternating, ``--runs`` runs each (the spread of the runs of one way is the A/A spread
of the session), each with device_png off and on and at every ``--io-threads`` value:
  crop       crop_to_mask=true, batch_size=8            (the generator on a 768^2 window)
  full       no option, batch_size=1                    (the generator at 2048^2, one image per step)
  scaled     dataset.scale_factor=0.25 paste_back=true  (the generator at 512^2, the hole resampled bilinearly)
and, from the first run of ``crop`` and of ``full``, the largest u8 difference under the mask between the two results: a description of the
definition (a crop sees less context; synthetic weights), not a parity claim.  The crop runs print the pre-pass's wall time (the CLI's own line).
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


def _copy_us(nbytes, launches, warmup):
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    return _each(lambda: dst.copy_(src), launches, warmup)


def kernel_case(lib, side, win, x0_off, launches, warmup, batch=8):
    g = torch.Generator().manual_seed(side + win)
    img = torch.randint(0, 256, (batch, side, side, 3), generator=g, dtype=torch.uint8).cuda()
    y0, x0 = (side - win) // 2, (side - win) // 2 // 4 * 4 + x0_off
    msk = torch.zeros(batch, side, side, dtype=torch.uint8)
    msk[:, y0 + win // 4:y0 + 3 * win // 4, x0 + win // 4:x0 + 3 * win // 4] = 255
    msk = msk.cuda()
    ssz = torch.tensor([[side, side]] * batch, dtype=torch.int32).cuda()
    rects = torch.tensor([[y0, x0, win, win]] * batch, dtype=torch.int32).cuda()
    masked = torch.empty(batch, 4, win, win, device='cuda')
    pred = torch.rand(batch, 3, win, win, generator=g).cuda()
    out = torch.empty_like(img)
    st = torch.cuda.current_stream().cuda_stream
    v_masked, v_pred = L.view(masked), L.view(pred)
    compose = _each(lambda: lib.crop_compose_u8(img, msk, ssz, rects, v_masked, batch, stream=st), launches, warmup)
    paste = _each(lambda: lib.crop_paste_u8(img, msk, ssz, rects, v_pred, out, batch, stream=st), launches, warmup)
    wpx, spx = batch * win * win, batch * side * side
    compose_mb, paste_mb = 20 * wpx / 1e6, (7 * spx + 12 * int((msk != 0).sum())) / 1e6
    compose_copy, paste_copy = _copy_us(20 * wpx, launches, warmup), _copy_us(7 * spx, launches, warmup)
    # the existing compose on host-cropped slots of the window's size
    c_img = img[:, y0:y0 + win, x0:x0 + win].contiguous()
    c_msk = msk[:, y0:y0 + win, x0:x0 + win].contiguous()
    c_sz = torch.tensor([[win, win]] * batch, dtype=torch.int32).cuda()
    masked2 = torch.empty_like(masked)
    v_masked2 = L.view(masked2)
    compose_u8 = _each(lambda: lib.mask_compose_u8(c_img, c_msk, c_sz, v_masked2, batch, True, st), launches, warmup)
    blend = torch.empty(batch, win, win, 3, dtype=torch.uint8, device='cuda')
    lib.blend_quantize_u8(c_img, c_msk, c_sz, v_pred, blend, batch, True, st)
    torch.cuda.synchronize()
    want = img.clone()
    want[:, y0:y0 + win, x0:x0 + win] = blend
    print(json.dumps(dict(what='kernel', case=f'{batch} x {side}^2, windows {win}^2', x0=x0, masked_share_of_source=round(float((msk != 0).float().mean()), 4),
                          compose_us=compose[0], compose_us_min=compose[1], compose_mb=round(compose_mb, 1), compose_gb_per_s=round(compose_mb / compose[0] * 1e3, 1),
                          compose_d2d_copy_us=compose_copy[0], compose_ratio_to_copy=round(compose[0] / compose_copy[0], 2),
                          mask_compose_u8_on_cropped_slots_us=compose_u8[0], mask_compose_u8_us_min=compose_u8[1],
                          paste_us=paste[0], paste_us_min=paste[1], paste_mb=round(paste_mb, 1), paste_gb_per_s=round(paste_mb / paste[0] * 1e3, 1),
                          paste_d2d_copy_us=paste_copy[0], paste_ratio_to_copy=round(paste[0] / paste_copy[0], 2),
                          compose_bits_equal_mask_compose_u8=bool(torch.equal(masked.view(torch.int32), masked2.view(torch.int32))),
                          paste_bytes_equal_blend_pasted_by_slicing=bool(torch.equal(out, want)))), flush=True)


def write_pairs(indir, n, side, share=0.05):
    os.makedirs(indir)
    base = np.random.RandomState(7).randint(0, 256, (side + 64, side + 64, 3)).astype('uint8')
    box = int(round((share * side * side) ** 0.5))
    for i in range(n):
        oy, ox = (i * 7) % 64, (i * 13) % 64
        m = np.zeros((side, side), 'uint8')
        by, bx = (i * 211) % (side - box), (i * 397) % (side - box)          # the boxes move over the image, the corners included
        m[by:by + box, bx:bx + box] = 255
        with open(os.path.join(indir, f'im{i:05d}.png'), 'wb') as f:
            f.write(encode_png(base[oy:oy + side, ox:ox + side]))
        with open(os.path.join(indir, f'im{i:05d}_mask001.png'), 'wb') as f:
            f.write(encode_png(m))
    return box


def run_cli(mdir, indir, outdir, extra, keep=False):
    r = subprocess.run([sys.executable, '-m', 'lama_amd.predict', f'model.path={mdir}', f'indir={indir}', f'outdir={outdir}'] + extra,
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    m = re.search(r'wrote (\d+) images to \S+ in ([\d.]+) s \(([\d.]+) images/s', r.stdout)
    if r.returncode != 0 or not m:
        raise RuntimeError(f'predict failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
    pre = re.search(r'crop_to_mask pre-pass: ([\d.]+) s', r.stdout)
    from PIL import Image
    first = sorted(os.listdir(outdir))[0]
    with Image.open(os.path.join(outdir, first)) as im:
        size = im.size
    if not keep:
        shutil.rmtree(outdir, ignore_errors=True)
    return int(m.group(1)), float(m.group(3)), size, float(m.group(2)), (float(pre.group(1)) if pre else None)


def difference_under_the_mask(indir, crop_dir, full_dir, count=8):
    from PIL import Image
    worst, per_image = 0, []
    for name in sorted(os.listdir(crop_dir))[:count]:
        a = np.array(Image.open(os.path.join(crop_dir, name))).astype(np.int16)
        b = np.array(Image.open(os.path.join(full_dir, name))).astype(np.int16)
        mask = np.array(Image.open(os.path.join(indir, name)).convert('L')) != 0
        assert np.array_equal(a[~mask], b[~mask])            # both give the source pixels back outside the mask
        d = np.abs(a[mask] - b[mask])
        per_image.append(dict(max=int(d.max()), mean=round(float(d.mean()), 2)))
        worst = max(worst, int(d.max()))
    print(json.dumps(dict(what='crop_vs_full_under_the_mask', images=len(per_image), max_abs_u8=worst, per_image=per_image)), flush=True)


def cli_part(n, runs, io_threads, side=2048, factor=0.25):
    import yaml
    import bench
    model = bench.build_model(torch.device('cuda', 0), L.PREC_F16X3)
    tmp = tempfile.mkdtemp(prefix='lama_crop_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
    try:
        mdir = os.path.join(tmp, 'model')
        os.makedirs(os.path.join(mdir, 'models'))
        with open(os.path.join(mdir, 'config.yaml'), 'w') as f:
            yaml.safe_dump(dict(training_model=dict(kind='default', concat_mask=True), generator=dict(bench.BIG_LAMA)), f)
        torch.save({'state_dict': {k: v.detach().cpu() for k, v in model.state_dict().items()}}, os.path.join(mdir, 'models', 'best.ckpt'))
        del model
        torch.cuda.empty_cache()
        indir = os.path.join(tmp, 'in')
        box = write_pairs(indir, n, side)
        ways = dict(crop=['batch_size=8', 'crop_to_mask=true'], full=['batch_size=1'],
                    scaled=['batch_size=8', f'dataset.scale_factor={factor}', 'paste_back=true'])
        compared = False
        for threads in io_threads:
            for device_png in (False, True):
                rates = {k: [] for k in ways}
                shares = []
                for k in range(runs):
                    for way, extra in ways.items():                      # alternating: the box's drift hits every way alike
                        keep = not compared and k == 0 and way in ('crop', 'full')
                        out = os.path.join(tmp, 'out_' + way if keep else 'out')
                        cnt, ips, size, wall, pre = run_cli(mdir, indir, out, extra + [f'io_threads={threads}'] + (['device_png=true'] if device_png else []), keep)
                        rates[way].append(ips)
                        if pre is not None:
                            shares.append(round(100 * pre / wall, 1))
                        print(json.dumps(dict(what='cli_run', way=way, run=k, io_threads=threads, device_png=device_png, images=cnt, source=f'{side}^2',
                                              png_size=list(size), images_per_s=ips, wall_s=wall, prepass_s=pre)), flush=True)
                    if not compared:
                        difference_under_the_mask(indir, os.path.join(tmp, 'out_crop'), os.path.join(tmp, 'out_full'))
                        shutil.rmtree(os.path.join(tmp, 'out_crop'), ignore_errors=True)
                        shutil.rmtree(os.path.join(tmp, 'out_full'), ignore_errors=True)
                        compared = True
                print(json.dumps(dict(what='cli', images=n, source=f'{side}^2', box=f'{box}^2', io_threads=threads, device_png=device_png,
                                      **{f'{w}_images_per_s_median': round(statistics.median(v), 2) for w, v in rates.items()},
                                      **{f'{w}_runs': v for w, v in rates.items()},
                                      aa_spread_percent={w: round(100 * (max(v) - min(v)) / statistics.median(v), 1) for w, v in rates.items()},
                                      crop_beats_full_by_more_than_the_spread=min(rates['crop']) > max(rates['full']),
                                      crop_over_full=round(statistics.median(rates['crop']) / statistics.median(rates['full']), 2),
                                      crop_over_scaled=round(statistics.median(rates['crop']) / statistics.median(rates['scaled']), 2),
                                      prepass_percent_of_wall=shares)), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--n', type=int, default=48)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--io-threads', type=int, nargs='+', default=[4, 16])
    ap.add_argument('--no-cli', action='store_true')
    ap.add_argument('--no-kernels', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('crop_bench needs an MI355X: a CPU run measures nothing')
    lib = L.get_lib()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, host_cpus=os.cpu_count())), flush=True)
    if not a.no_kernels:
        for side, win in ((2048, 512), (1024, 384)):
            for x0_off in (0, 1):
                kernel_case(lib, side, win, x0_off, a.launches, a.warmup)
    if not a.no_cli:
        cli_part(a.n, a.runs, a.io_threads)


if __name__ == '__main__':
    main()
