#!/usr/bin/env python3
"""Measure ``crop_max_side`` (lama_crop_shrink_compose_u8_fwd / lama_crop_shrink_paste_u8_fwd; python -m lama_amd.predict ... crop_to_mask=true
crop_max_side=512).

    python tools/crop_shrink_bench.py [--launches 20] [--warmup 5] [--n 48] [--runs 3] [--io-threads 4 16] [--no-cli] > profiles/crop_shrink.txt

JSON lines, in the manner of tools/crop_bench.py.  Nothing here is a gate: the numbers are recorded in profiles/crop_shrink.txt and quoted in the
README.

Kernel part, per case (8 source slots of 2048^2; windows of 1024^2 and of 2048^2, each with k = 2 and k = 4; the mask a centred box of a quarter
of the window), microseconds as the median of ``--launches`` launches timed one by one with events after ``--warmup`` launches, in the same
process and on the same data:
  compose        lama_crop_shrink_compose_u8_fwd, one launch: 4 bytes read per window pixel, 16 written per low-resolution pixel;
  compose_copy   a device-to-device copy of those bytes (half read, half written);
  parent_route   what the parent commit offers for the same image planes: lama_resize_u8_fwd (factor 1 / k) + lama_mask_compose_fwd on slots
                 the host has cropped already (the crop itself is not timed; its mask is INTER_NEAREST, not the max);
  paste          lama_crop_shrink_paste_u8_fwd, one launch: 7 bytes per SOURCE pixel + the gather under the mask;
  paste_copy     a copy of 7 bytes per source pixel;
  crop_paste_k1  lama_crop_paste_u8_fwd with the same window at k = 1 (a prediction of the window's size).
CLI part: images/s of the CLI's own loop over ``--n`` PNG pairs of 2048^2 (tmpfs), big-lama shape, synthetic weights, batch_size=8, for box masks of
25 % of the area (windows that need k >= 2) and of 5 % (k = 1: the option must cost nothing), three ways, alternating, ``--runs`` runs each (the
spread of the runs of one way is the A/A spread of the session), at every ``--io-threads`` value:
  crop           crop_to_mask=true
  crop_limited   crop_to_mask=true crop_max_side=512
  scaled         dataset.scale_factor=0.25 paste_back=true
A way that fails ends the CLI part there: nothing more is started on the GPU after a failed run."""
import argparse
import json
import os
import shutil
import statistics
import tempfile

import torch

import _toollib  # noqa: F401
import crop_bench as CB
from lama_amd import _lib as L


def kernel_case(lib, side, win, k, launches, warmup, batch=8):
    g = torch.Generator().manual_seed(side + win + k)
    img = torch.randint(0, 256, (batch, side, side, 3), generator=g, dtype=torch.uint8).cuda()
    y0 = x0 = (side - win) // 2 // 4 * 4
    msk = torch.zeros(batch, side, side, dtype=torch.uint8)
    msk[:, y0 + win // 4:y0 + 3 * win // 4, x0 + win // 4:x0 + 3 * win // 4] = 255
    msk = msk.cuda()
    low = win // k
    i32 = lambda rows: torch.tensor(rows, dtype=torch.int32).cuda()
    ssz, rects, ks = i32([[side, side]] * batch), i32([[y0, x0, win, win]] * batch), i32([k] * batch)
    masked = torch.empty(batch, 4, low, low, device='cuda')
    pred = torch.rand(batch, 3, low, low, generator=g).cuda()
    out = torch.empty_like(img)
    st = torch.cuda.current_stream().cuda_stream
    v_masked, v_pred = L.view(masked), L.view(pred)
    compose = CB._each(lambda: lib.crop_shrink_compose_u8(img, msk, ssz, rects, ks, v_masked, batch, stream=st), launches, warmup)
    paste = CB._each(lambda: lib.crop_shrink_paste_u8(img, msk, ssz, rects, ks, v_pred, out, batch, stream=st), launches, warmup)
    wpx, lpx, spx = batch * win * win, batch * low * low, batch * side * side
    compose_bytes = 4 * wpx + 16 * lpx
    compose_copy, paste_copy = CB._copy_us(compose_bytes, launches, warmup), CB._copy_us(7 * spx, launches, warmup)
    # the parent's route on host-cropped slots: resize_u8 + mask_compose through fp32 image / mask tensors
    c_img = img[:, y0:y0 + win, x0:x0 + win].contiguous()
    c_msk = msk[:, y0:y0 + win, x0:x0 + win].contiguous()
    c_sz, d_sz = i32([[win, win]] * batch), i32([[low, low]] * batch)
    f_img, f_msk = torch.empty(batch, 3, low, low, device='cuda'), torch.empty(batch, 1, low, low, device='cuda')
    masked2 = torch.empty_like(masked)
    v_img, v_msk, v_masked2 = L.view(f_img), L.view(f_msk), L.view(masked2)

    def parent():
        lib.resize_u8(c_img, c_msk, c_sz, d_sz, 1.0 / k, v_img, v_msk, batch, True, st)
        lib.mask_compose(v_img, v_msk, v_masked2, batch, st)
    route = CB._each(parent, launches, warmup)
    # the crop paste at k = 1 on the same window
    pred1 = torch.rand(batch, 3, win, win, generator=g).cuda()
    v_pred1 = L.view(pred1)
    out1 = torch.empty_like(img)
    paste1 = CB._each(lambda: lib.crop_paste_u8(img, msk, ssz, rects, v_pred1, out1, batch, stream=st), launches, warmup)
    torch.cuda.synchronize()
    hole = masked[:, 3] != 0
    same_planes = bool(torch.equal((masked[:, :3] * ~hole[:, None]).view(torch.int32), (masked2[:, :3] * ~hole[:, None]).view(torch.int32)))
    print(json.dumps(dict(what='kernel', case=f'{batch} x {side}^2, windows {win}^2, k = {k}', low=f'{low}^2',
                          compose_us=compose[0], compose_us_min=compose[1], compose_mb=round(compose_bytes / 1e6, 1),
                          compose_gb_per_s=round(compose_bytes / compose[0] / 1e3, 1), compose_copy_us=compose_copy[0],
                          compose_ratio_to_copy=round(compose[0] / compose_copy[0], 2),
                          parent_route_us=route[0], parent_route_us_min=route[1], compose_over_parent_route=round(compose[0] / route[0], 2),
                          image_planes_outside_the_hole_equal_the_parent_routes=same_planes,
                          paste_us=paste[0], paste_us_min=paste[1], paste_mb=round(7 * spx / 1e6, 1), paste_gb_per_s=round(7 * spx / paste[0] / 1e3, 1),
                          paste_copy_us=paste_copy[0], paste_ratio_to_copy=round(paste[0] / paste_copy[0], 2),
                          crop_paste_k1_us=paste1[0], crop_paste_k1_us_min=paste1[1], paste_over_crop_paste_k1=round(paste[0] / paste1[0], 2))), flush=True)


def cli_part(n, runs, io_threads, side=2048, factor=0.25):
    import yaml
    import bench
    model = bench.build_model(torch.device('cuda', 0), L.PREC_F16X3)
    tmp = tempfile.mkdtemp(prefix='lama_crop_shrink_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
    try:
        mdir = os.path.join(tmp, 'model')
        os.makedirs(os.path.join(mdir, 'models'))
        with open(os.path.join(mdir, 'config.yaml'), 'w') as f:
            yaml.safe_dump(dict(training_model=dict(kind='default', concat_mask=True), generator=dict(bench.BIG_LAMA)), f)
        torch.save({'state_dict': {k: v.detach().cpu() for k, v in model.state_dict().items()}}, os.path.join(mdir, 'models', 'best.ckpt'))
        del model
        torch.cuda.empty_cache()
        ways = dict(crop=['crop_to_mask=true'], crop_limited=['crop_to_mask=true', 'crop_max_side=512'],
                    scaled=[f'dataset.scale_factor={factor}', 'paste_back=true'])
        for share in (0.25, 0.05):
            indir = os.path.join(tmp, f'in{int(share * 100)}')
            box = CB.write_pairs(indir, n, side, share)
            for threads in io_threads:
                rates = {w: [] for w in ways}
                for k in range(runs):
                    for way, extra in ways.items():                      # alternating: the box's drift hits every way alike
                        cnt, ips, size, wall, pre = CB.run_cli(mdir, indir, os.path.join(tmp, 'out'), ['batch_size=8', f'io_threads={threads}'] + extra)
                        rates[way].append(ips)
                        print(json.dumps(dict(what='cli_run', way=way, run=k, mask_share=share, io_threads=threads, images=cnt, source=f'{side}^2',
                                              png_size=list(size), images_per_s=ips, wall_s=wall, prepass_s=pre)), flush=True)
                print(json.dumps(dict(what='cli', images=n, source=f'{side}^2', box=f'{box}^2', mask_share=share, io_threads=threads,
                                      **{f'{w}_images_per_s_median': round(statistics.median(v), 2) for w, v in rates.items()},
                                      **{f'{w}_runs': v for w, v in rates.items()},
                                      aa_spread_percent={w: round(100 * (max(v) - min(v)) / statistics.median(v), 1) for w, v in rates.items()},
                                      crop_limited_over_crop=round(statistics.median(rates['crop_limited']) / statistics.median(rates['crop']), 2),
                                      crop_limited_over_scaled=round(statistics.median(rates['crop_limited']) / statistics.median(rates['scaled']), 2))),
                      flush=True)
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
        raise SystemExit('crop_shrink_bench needs an MI355X: a CPU run measures nothing')
    lib = L.get_lib()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, host_cpus=os.cpu_count())), flush=True)
    if not a.no_kernels:
        for win in (1024, 2048):
            for k in (2, 4):
                kernel_case(lib, 2048, win, k, a.launches, a.warmup)
    if not a.no_cli:
        cli_part(a.n, a.runs, a.io_threads)


if __name__ == '__main__':
    main()
