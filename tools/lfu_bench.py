#!/usr/bin/env python3
"""What the local Fourier unit (enable_lfu=True) costs: its two kernels and its FourierUnit beside device-to-device copies of the same bytes,
and the step of a big-lama-shaped generator with the LFU against the same generator without it.

    python tools/lfu_bench.py [--batches 8,1] [--launches 20] [--group 20] [--repeats 9] [--no-step]

JSON lines.  Per batch B of 512 x 512 inputs (bottleneck x1 [B, 192, 64, 64], fp32):
  * lama_lfu_gather_fwd, lama_lfu_tile_add_fwd (in place, as SpectralTransformLFU runs it) and the LFU's FourierUnit(192, 192) on
    [B, 192, 32, 32]: device microseconds per call -- ``--group`` calls captured into one hipGraph, its replay timed with events, divided, the
    median of ``--launches`` replays -- each beside ``dst.copy_(src)`` of a tensor with the same number of bytes read plus written, timed the same way in the same process;
  * the A/A spread of that copy: the measurement repeated ``--repeats`` times, (max - min) / median of the medians.  A kernel is "within" when
    its time is at most the copy's median times (1 + spread);
  * the generator's step (graph replay of ``generator(x)``, LFU on and off alternating, median of ``--repeats`` replays timed one by one),
    the difference, and the share of it that 36 x (gather + tile-add) account for.
The comparison of the LFU-off generator with the commit before is bench.py's, run from both trees."""
import argparse
import copy
import json
import statistics

import torch

import _toollib  # noqa: F401
from lama_amd import _lib as L
from lama_amd import ffc as F
from lama_amd.modules import make_generator


def _time(fn, launches, group):
    """Device microseconds per call of ``fn(stream)``: ``group`` calls captured into one hipGraph (no host call between the launches), the
    graph replayed ``launches`` times between two events each, the median divided by ``group``."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(group):
            fn(torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        g.replay()
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1) * 1e3 / group)
    return statistics.median(ts)


def _beside_copy(name, shape, fn, nbytes, a):
    """``fn`` against a copy that reads + writes ``nbytes`` in all (a tensor of nbytes / 2)."""
    src = torch.randn(nbytes // 8, device='cuda')
    dst = torch.empty_like(src)
    copies = [_time(lambda st: dst.copy_(src), a.launches, a.group) for _ in range(a.repeats)]
    k = _time(fn, a.launches, a.group)
    c = statistics.median(copies)
    spread = (max(copies) - min(copies)) / c
    rec = dict(kernel=name, shape=list(shape), mb_read_plus_written=round(nbytes / 1e6, 2), us=round(k, 2), gb_per_s=round(nbytes / k / 1e3, 1),
               d2d_copy_us=round(c, 2), copy_aa_spread=round(spread, 3), ratio_to_copy=round(k / c, 3), within_copy_margin=bool(k <= c * (1 + spread)))
    print(json.dumps(rec), flush=True)
    return k


def kernels(B, a):
    lib = L.get_lib()
    C, h = 192, 64
    s, q = h // 2, C // 4
    x1 = torch.randn(B, C, h, h, device='cuda')
    xs_in = torch.empty(B, C, s, s, device='cuda')
    xs = torch.randn(B, C, s, s, device='cuda')
    n_q = B * q * h * h * 4
    tg = _beside_copy('lama_lfu_gather_fwd', x1.shape, lambda st: lib.lfu_gather(L.view(x1, 0, q), L.view(xs_in), B, st), 2 * n_q, a)
    n_a = x1.numel() * 4
    tt = _beside_copy('lama_lfu_tile_add_fwd (in place)', x1.shape, lambda st: lib.lfu_tile_add(L.view(x1), L.view(xs), L.view(x1), B, st),
                      2 * n_a + n_a // 4, a)
    fu = F.FourierUnit(C, C).cuda()
    ws = fu.workspace(xs_in)
    n_x, n_s = xs_in.numel() * 4, B * 2 * C * s * (s // 2 + 1) * 4           # rfft2: x -> S; spectral 1x1: S -> S; irfft2: S -> x
    _beside_copy('FourierUnit(192, 192) of the LFU (3 launches)', xs_in.shape,
                 lambda st: fu.run(L.view(xs_in), L.view(xs), B, False, ws, st), 2 * n_x + 4 * n_s, a)
    return tg, tt


_SD = {}


def step(B, a, tg, tt):
    from oracle import lama_oracle as O
    if 'sd' not in _SD:
        _SD['sd'] = O.make_synthetic_state_dict(O.BIG_LAMA, seed=0, calib_hw=64)        # calibrated: activations stay inside the fp16 split's range
    sd = _SD['sd']
    gens = {}
    for lfu in (False, True):
        cfg = copy.deepcopy(O.BIG_LAMA)
        cfg['resnet_conv_kwargs']['enable_lfu'] = lfu
        torch.manual_seed(1)
        g = make_generator(None, kind='ffc_resnet', **cfg)
        g.load_state_dict(sd, strict=not lfu)                                # (the lfu.* entries keep their seeded default initialisation)
        g.cuda()
        g.use_graph = True
        gens[lfu] = g
    batch = O.make_synthetic_batch(B, 512, 512, seed=3)
    x = torch.cat([batch['image'] * (1 - batch['mask']), batch['mask']], 1).cuda()
    with torch.no_grad():
        for g in gens.values():
            for _ in range(3):
                g(x)
        torch.cuda.synchronize()
        ts = {False: [], True: []}
        for _ in range(a.repeats):
            for lfu in (False, True):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                gens[lfu](x)
                t1.record()
                torch.cuda.synchronize()
                ts[lfu].append(t0.elapsed_time(t1))
    off, on = statistics.median(ts[False]), statistics.median(ts[True])
    kern = 36 * (tg + tt) / 1e3
    print(json.dumps(dict(what='generator step, graph replay', shape=[B, 4, 512, 512], ms_lfu_off=round(off, 3), ms_lfu_on=round(on, 3),
                          off_spread=round((max(ts[False]) - min(ts[False])) / off, 3), added_ms=round(on - off, 3),
                          two_kernels_ms=round(kern, 3), two_kernels_share_of_added=round(kern / (on - off), 3) if on > off else None,
                          precision_off=gens[False].precision, precision_on=gens[True].precision,
                          parts_off=gens[False].split_decisions and [d['kept'] for d in gens[False].split_decisions.values()],
                          parts_on=gens[True].split_decisions and [d['kept'] for d in gens[True].split_decisions.values()])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='8,1')
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--group', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    for B in (int(v) for v in a.batches.split(',')):
        tg, tt = kernels(B, a)
        if not a.no_step:
            step(B, a, tg, tt)


if __name__ == '__main__':
    main()
