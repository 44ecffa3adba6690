#!/usr/bin/env python3
"""Time lama_range_stats_fwd (both launches) against a device-to-device copy of the same bytes, and a whole probe_ranges of the big-lama shape.

    python tools/range_stats_bench.py [--launches 20] [--warmup 5] [--no-probe]

JSON lines.  Per shape ([8,512,64,64], [8,384,64,33], [8,64,512,512] fp32): microseconds per call as the median of ``--launches`` calls timed one
by one with events after ``--warmup`` calls, the same for ``dst.copy_(src)`` of the tensor in the same process -- the floor of reading it once
(the copy also WRITES those bytes; the kernel only reads) -- and the ratio.  Then one ``probe_ranges`` at 1 x 4 x 512 x 512 on a synthetic
big-lama generator: wall milliseconds against a plain eager forward and a graph replay (a diagnostic, not a serving path: no bar)."""
import argparse
import json
import statistics
import time

import torch

import _toollib  # noqa: F401
from lama_amd import _lib as L
from lama_amd.modules import make_generator
from lama_amd.probe import probe_ranges


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
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-probe', action='store_true')
    a = ap.parse_args()
    lib = L.get_lib()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    for shape in ((8, 512, 64, 64), (8, 384, 64, 33), (8, 64, 512, 512)):
        x = torch.randn(shape, device='cuda')
        y = torch.empty_like(x)
        out = torch.empty(shape[1], 4, dtype=torch.int32, device='cuda')
        ws = torch.empty(lib.range_stats_workspace_bytes(*shape) // 4, dtype=torch.int32, device='cuda')
        v, st = L.view(x), torch.cuda.current_stream().cuda_stream
        k_med, k_min = _each(lambda: lib.range_stats(v, shape[0], L.F16_MAX, stream=st, out=out, ws=ws), a.launches, a.warmup)
        c_med, c_min = _each(lambda: y.copy_(x), a.launches, a.warmup)
        mb = x.numel() * 4 / 1e6
        print(json.dumps(dict(kernel='lama_range_stats_fwd (partial + fold)', shape=list(shape), mb_read=round(mb, 1), us=round(k_med, 1), us_min=round(k_min, 1),
                              gb_per_s=round(mb / k_med * 1e3, 1), d2d_copy_us=round(c_med, 1), d2d_copy_us_min=round(c_min, 1),
                              ratio_to_copy=round(k_med / c_med, 3))), flush=True)
        del x, y
    if a.no_probe:
        return
    from oracle import lama_oracle as O
    torch.manual_seed(0)
    gen = make_generator(None, kind='ffc_resnet', **O.BIG_LAMA).cuda()       # seeded random weights: the timing does not depend on the values
    x = torch.rand(1, 4, 512, 512, device='cuda')
    with torch.no_grad():
        gen(x)
        rep = probe_ranges(gen, x)                                            # warm-up: packs the stand-alone layers' weights
        torch.cuda.synchronize()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            rep = probe_ranges(gen, x)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        f = []
        for _ in range(3):
            t0 = time.perf_counter()
            gen(x)
            torch.cuda.synchronize()
            f.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(what='probe_ranges', shape=[1, 4, 512, 512], rows=len(rep.rows), channels=int(sum(r.shape[1] for r in rep.rows if r.shape)),
                          probe_ms=round(statistics.median(t), 2), eager_forward_ms=round(statistics.median(f), 2),
                          winograd_rows=sum(r.bound is not None for r in rep.rows), precision=gen.precision)), flush=True)


if __name__ == '__main__':
    main()
