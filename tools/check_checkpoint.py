#!/usr/bin/env python3
"""Does this checkpoint stay inside the range of the default arithmetic (the 3-term fp16 split, |x| <= 65504) -- and if not, WHERE does it leave?

    python tools/check_checkpoint.py model.path=<dir> indir=<dir> [model.checkpoint=best.ckpt] [n=8] [oracle=false] [out=<report.json>]

``model.path`` holds config.yaml and models/<checkpoint> (the layout bin/predict.py reads); ``indir`` holds <name>.png + <name>_mask*.png pairs.
For each of the first ``n`` images (default dataset, pad_out_to_modulo 8):
  1. ``lama_amd.probe.probe_ranges`` at f16x3: the five rows closest to the limit and, if there is one, the first row out of range with its channel;
  2. a plain forward at f16x3 with ``auto_fallback=False``: did the range watch raise?
  3. forwards at bf16x3 and f32; for each pair of precisions the max-abs difference of ``inpainted`` and the number of u8 values that differ after
     the predict CLI's quantisation (clip(x * 255, 0, 255) truncated);
  4. ``oracle=true``: the CPU oracle (oracle/lama_oracle.py, ffc_resnet only) on the same input and its max-abs difference to each precision.
Everything goes to ``out=`` as JSON (one record per image + a summary); one verdict line per precision is printed.
Exit status: 1 if the f16x3 probe found a row out of range or the f16x3 forward ended with LamaRangeError (the watch raised, or a weight was
refused at pack time), 2 on usage errors, 3 on any other failure (no GPU, an unreadable checkpoint, an exception), 0 otherwise.  All GPU work happens in this
process.  The probe's forward is the un-fused one-stream order (lama_amd/probe.py): its tensors agree with the serving plan's to fp32 rounding."""
import json
import os
import sys

import numpy as np
import torch

import _toollib  # noqa: F401
from lama_amd import _lib as L
from lama_amd import config as lcfg
from lama_amd import ffc
from lama_amd import predict as P
from lama_amd import trainers
from lama_amd.probe import probe_ranges

KEYS = {'model.path': str, 'indir': str, 'model.checkpoint': str, 'n': int, 'oracle': bool, 'out': str}
PRECS = ('f16x3', 'bf16x3', 'f32')


class Usage(Exception):
    pass


def parse(argv):
    cfg = {'model.checkpoint': 'best.ckpt', 'n': 8, 'oracle': False, 'out': None}
    for a in argv:
        if '=' not in a:
            raise Usage(f'expected key=value, got {a!r}')
        k, v = a.split('=', 1)
        if k not in KEYS:
            raise Usage(f'unknown option {k!r}; known: {sorted(KEYS)}')
        if KEYS[k] is bool:
            if v.lower() not in ('true', 'false'):
                raise Usage(f'{k}={v!r}: expected true or false')
            cfg[k] = v.lower() == 'true'
        elif KEYS[k] is int:
            try:
                cfg[k] = int(v)
            except ValueError:
                raise Usage(f'{k}={v!r}: expected an integer')
        else:
            cfg[k] = v
    for need in ('model.path', 'indir'):
        if need not in cfg:
            raise Usage(f'missing {need}=...')
    if cfg['n'] < 1:
        raise Usage('n: at least one image')
    for path in (os.path.join(cfg['model.path'], 'config.yaml'), os.path.join(cfg['model.path'], 'models', cfg['model.checkpoint']), cfg['indir']):
        if not os.path.exists(path):
            raise Usage(f'{path} does not exist')
    return cfg


def quantise(inpainted: torch.Tensor, hw) -> torch.Tensor:
    """bin/predict.py:86-92: crop to the unpadded size, clip(x * 255, 0, 255), truncate to u8."""
    cur = inpainted[0, :, :hw[0], :hw[1]]
    return (cur * 255).clamp(0, 255).to(torch.uint8)


def check_image(gen, image: np.ndarray, mask: np.ndarray, hw, oracle=None) -> dict:
    dev = next(gen.parameters()).device
    img = torch.from_numpy(image)[None].to(dev)
    msk = (torch.from_numpy(mask)[None] > 0).float().to(dev)                    # bin/predict.py:84
    masked = torch.cat([img * (1 - msk), msk], 1).contiguous()                   # trainers/default.py:59,67-68
    rec = dict(shape=list(masked.shape), unpadded=list(hw))
    # 1. the probe at the default arithmetic
    gen.set_precision(L.PREC_F16X3)
    rep = probe_ranges(gen, masked)
    first = rep.first_over()
    rec['rows'] = [r.as_dict() for r in rep.rows]
    rec['worst'] = [r.name for r in rep.worst(5)]
    rec['first_over'] = None if first is None else dict(first.as_dict(), bad_channel=first.bad_channel)
    print(rep.format(rep.worst(5)))
    if first is not None:
        print(f'  first out of range: {first.name} channel {first.bad_channel if first.bad_channel is not None else "-"} '
              f'(refused {first.refused}, n_over {first.n_over}, n_nan {first.n_nan}, n_inf {first.n_inf}, max |x| {first.abs_max:.6g}){first.note}')
    # 2. / 3. plain forwards
    out, keep = {}, gen.auto_fallback
    gen.auto_fallback = False
    try:
        for name in PRECS:
            gen.set_precision(L.PREC_NAMES[name])
            err = None
            try:
                pred = gen(masked)
            except L.LamaRangeError as e:
                pred, err = None, str(e)
            if name == 'f16x3':
                # the watch raised = an ACTIVATION left the range in a launch; a folded WEIGHT beyond the range is refused at pack time, before
                # any launch (both end the f16x3 forward with LamaRangeError)
                rec['watch_raised'] = err is not None and err == ffc._RANGE_MSG
                rec['pack_refused'] = err is not None and err != ffc._RANGE_MSG
                rec['range_error'] = err
            out[name] = None if pred is None else msk * pred + (1 - msk) * img          # trainers/default.py:71
    finally:
        gen.auto_fallback = keep
        gen.set_precision(L.PREC_F16X3)
    rec['diff'] = {}
    for i, a in enumerate(PRECS):
        for b in PRECS[i + 1:]:
            if out[a] is None or out[b] is None:
                rec['diff'][f'{a}_vs_{b}'] = None
                continue
            qa, qb = quantise(out[a], hw), quantise(out[b], hw)
            rec['diff'][f'{a}_vs_{b}'] = dict(max_abs=float((out[a] - out[b]).abs().max()), u8_levels_differ=int((qa != qb).sum()))
    if oracle is not None:
        O, sd, cfg = oracle
        with torch.no_grad():
            ref = O.training_module_forward(dict(image=img.cpu(), mask=msk.cpu()), sd, cfg)['inpainted']
        rec['oracle'] = {p: (None if out[p] is None else float((out[p].cpu() - ref).abs().max())) for p in PRECS}
    return rec


def main(argv=None) -> int:
    try:
        cfg = parse(sys.argv[1:] if argv is None else argv)
    except Usage as e:
        print(f'check_checkpoint: {e}\n{__doc__.split("For each")[0]}', file=sys.stderr)
        return 2
    if not torch.cuda.is_available():
        raise L.LamaError('check_checkpoint needs an MI355X: no GPU is visible (there is no CPU fallback)')
    device = torch.device('cuda', 0)
    train_config = lcfg.load_train_config(os.path.join(cfg['model.path'], 'config.yaml'))
    ckpt = os.path.join(cfg['model.path'], 'models', cfg['model.checkpoint'])
    model = trainers.load_checkpoint(train_config, ckpt, strict=False, map_location=device)
    model.freeze()
    gen = model.generator
    oracle = None
    if cfg['oracle']:
        gcfg = dict(train_config['generator'])
        if gcfg.pop('kind', None) != 'ffc_resnet':
            print('check_checkpoint: oracle=true: the CPU oracle covers the ffc_resnet generator only', file=sys.stderr)
            return 2
        from oracle import lama_oracle as O
        sd = {k: v for k, v in torch.load(ckpt, map_location='cpu', weights_only=False)['state_dict'].items() if k.startswith('generator.')}
        oracle = (O, sd, gcfg)
    indir = cfg['indir'] if cfg['indir'].endswith(os.sep) else cfg['indir'] + os.sep
    items = P.list_dataset(indir, '.png')[:cfg['n']]
    if not items:
        print(f'check_checkpoint: no *mask*.png under {indir}', file=sys.stderr)
        return 2
    records = []
    for mask_path, img_path in items:
        image, mask, hw = P.load_item(mask_path, img_path, 8)
        print(f'== {os.path.relpath(img_path, indir)}  {image.shape[1]} x {image.shape[2]}')
        rec = check_image(gen, image, mask, hw, oracle)
        rec['image'] = os.path.relpath(img_path, indir)
        records.append(rec)
    over = [r for r in records if r['first_over'] is not None]
    raised = [r for r in records if r['watch_raised']]
    refused = [r for r in records if r['pack_refused']]

    def worst_pair(key):
        vals = [r['diff'][key] for r in records if r['diff'].get(key)]
        return (max(v['max_abs'] for v in vals), max(v['u8_levels_differ'] for v in vals)) if vals else None

    peak = max((row['abs_max'] for r in records for row in r['rows'] if row['abs_max'] is not None), default=0.0)
    summary = dict(images=len(records), out_of_range_images=len(over), watch_raised_images=len(raised), pack_refused_images=len(refused), peak_abs_max=peak, limit=L.F16_MAX,
                   first_over=None if not over else dict(image=over[0]['image'], **over[0]['first_over']),
                   diff={k: (None if worst_pair(k) is None else dict(max_abs=worst_pair(k)[0], u8_levels_differ=worst_pair(k)[1]))
                         for k in ('f16x3_vs_bf16x3', 'f16x3_vs_f32', 'bf16x3_vs_f32')})
    if oracle is not None:
        summary['oracle'] = {p: max((r['oracle'][p] for r in records if r['oracle'][p] is not None), default=None) for p in PRECS}
    bad = bool(over or raised or refused)
    summary['exit_status'] = 1 if bad else 0
    if cfg['out']:
        with open(cfg['out'], 'w') as f:
            json.dump(dict(images=records, summary=summary), f, indent=1)

    def pair_text(key):
        d = summary['diff'][key]
        return 'n/a (the f16x3 forward raised)' if d is None else f'max-abs {d["max_abs"]:.3g}, {d["u8_levels_differ"]} u8 values differ'

    if bad:
        fo = summary['first_over']
        where = ('the probe found no row (the watch raised in a fused launch)' if fo is None else
                 f'first out of range: {fo["name"]} channel {fo["bad_channel"] if fo["bad_channel"] is not None else "-"} in {fo["image"]} '
                 + ('(a folded weight beyond the range)' if fo["abs_max"] is None else f'(max |x| {fo["abs_max"]:.6g})'))
        print(f'f16x3: OUT OF RANGE in {len(over)} of {len(records)} images, watch raised in {len(raised)}, a weight refused at pack time in {len(refused)}; {where} -- serve this checkpoint with bf16x3')
    else:
        print(f'f16x3: in range on {len(records)} images (peak |x| {peak:.6g}, {L.F16_MAX / max(peak, 1e-30):.3g}x headroom); vs f32: {pair_text("f16x3_vs_f32")}')
    print(f'bf16x3: vs f32: {pair_text("bf16x3_vs_f32")}; vs f16x3: {pair_text("f16x3_vs_bf16x3")}')
    print('f32: the reference of the two lines above' + ('' if oracle is None else f'; vs the CPU oracle: max-abs {summary["oracle"]["f32"]:.3g}'))
    return 1 if bad else 0


def run(argv=None) -> int:
    """``main`` with every failure that is not a verdict mapped to exit status 3 (a crash must not read as 'out of range')."""
    try:
        return main(argv)
    except Exception as e:        # noqa: BLE001
        import traceback
        traceback.print_exc()
        print(f'check_checkpoint: failed: {type(e).__name__}: {e}', file=sys.stderr)
        return 3


if __name__ == '__main__':
    sys.exit(run())
