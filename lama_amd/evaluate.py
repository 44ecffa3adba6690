"""Score precomputed predictions on the device: the counterpart of the reference's ``bin/evaluate_predicts.py``.

    python -m lama_amd.evaluate <config.yaml> <datadir> <predictdir> <outpath> [model_path=<heads .pth>] [backbone=<vgg16 .pth>]
                                [fid_weights=<inception .pth>] [batch_size=N] [io_threads=8] [precision=f16x3|bf16x3|f32]

``config.yaml`` is one of the reference's ``configs/eval*.yaml``: ``evaluator_kwargs`` (batch_size, device, ...) and ``dataset_kwargs``
(img_suffix, inpainted_suffix, pad_out_to_modulo) are honoured, ``segmentation.enable: true`` raises (the segmentation-aware scores need an
ADE20k segmenter).  ``outpath`` receives the table ``evaluate_predicts.py:41-43`` writes with pandas -- rows ``total`` and the non-empty
mask-area bins, columns (ssim | lpips) x (mean | std), with ``fid_weights=`` also fid x mean and (when LPIPS is on) lpips_fid100_f1 x mean,
tab-separated, ``%.4f`` -- written here without pandas.

What differs from the reference's loop (one pass over the dataset per score, fp32 batches built on the host): the items are bucketed by padded
size as ``lama_amd.predict`` buckets them, decoded on ``io_threads`` host threads (at most 16) into pinned u8 slots, uploaded as u8 (7 bytes per
pixel instead of 28), and ONE pass serves everything: per batch the ingest launch (``lama_eval_ingest_u8_fwd``: / 255, symmetric padding, NCHW,
clamp, the mask's integer sum), then SSIM, then LPIPS, then the FID Inception on the same two tensors, all on the current stream.  Nothing is
read back per batch: the values of a bucket (for FID: its [n, 2048] activation rows) stay on the device until the bucket is done and are then
put back in dataset order.

LPIPS needs the linear heads (``model_path``: the reference's ``models/lpips_models/vgg.pth``) and the VGG-16 backbone (``backbone``:
torchvision's ``vgg16-397923af.pth``); nothing is downloaded.  With neither given the run scores SSIM only and says so.  FID needs the FID
Inception-v3 weights (``fid_weights``: ``pt_inception-2015-12-05-6726825d.pth``); without them the run says so and has no fid column."""
from __future__ import annotations

import math
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import evaluation as EV
from .predict import ceil_modulo

MAX_IO_THREADS = 16


# ---- the device loop ---------------------------------------------------------------------------------------------------------------------

def plan_buckets(sizes: Sequence[Tuple[int, int]], pad_mod: int, batch_size: int) -> List[dict]:
    """Item indices bucketed by padded size (largest first, as ``predict.plan_rounds`` orders them), each bucket cut into batches in dataset
    order.  A bucket's upload slots hold its largest image."""
    buckets: Dict[Tuple[int, int], List[int]] = {}
    for i, (h, w) in enumerate(sizes):
        buckets.setdefault((ceil_modulo(h, pad_mod), ceil_modulo(w, pad_mod)), []).append(i)
    out = []
    for shape in sorted(buckets, key=lambda hw: (-hw[0] * hw[1], hw)):
        idx = buckets[shape]
        out.append(dict(shape=shape, slot=(max(sizes[i][0] for i in idx), max(sizes[i][1] for i in idx)), items=idx,
                        batches=[idx[k:k + batch_size] for k in range(0, len(idx), batch_size)]))
    return out


class DeviceIngest:
    """The upload side of one bucket: two sets of pinned u8 slots (the host fills one while the copy of the other is in flight), one set of
    device slots and the two fp32 outputs of the ingest launch."""

    def __init__(self, lib: L.LamaLib, bucket: dict, batch_size: int, device: torch.device, pad_mod: int, clamp):
        (Hs, Ws), (Hp, Wp) = bucket['slot'], bucket['shape']
        self.lib, self.pad_mod, self.clamp, self.device = lib, pad_mod, clamp, device
        self.on_gpu = device.type == 'cuda'
        pin = dict(pin_memory=True) if self.on_gpu else {}
        self.host = [dict(image=torch.zeros(batch_size, Hs, Ws, 3, dtype=torch.uint8, **pin), inpainted=torch.zeros(batch_size, Hs, Ws, 3, dtype=torch.uint8, **pin),
                          mask=torch.zeros(batch_size, Hs, Ws, dtype=torch.uint8, **pin)) for _ in range(2)]
        self.free = [None, None]                              # per host set: the event behind its last upload
        self.dev = {k: torch.empty_like(v, device=device) for k, v in self.host[0].items()}
        self.out_image = torch.empty(batch_size, 3, Hp, Wp, dtype=torch.float32, device=device)
        self.out_pred = torch.empty_like(self.out_image)
        self.sums = torch.empty(batch_size, dtype=torch.int64, device=device)

    def fill(self, k: int, items: List[dict]) -> List[Tuple[int, int]]:
        """Decoded items -> host set k (top-left corner of each slot).  Returns the (h, w) of each."""
        if self.free[k] is not None:
            self.free[k].synchronize()
            self.free[k] = None
        sizes = []
        for j, it in enumerate(items):
            h, w = it['mask'].shape
            for key in ('image', 'inpainted', 'mask'):
                self.host[k][key][j, :h, :w] = torch.from_numpy(it[key])
            sizes.append((h, w))
        return sizes

    def run(self, k: int, sizes: List[Tuple[int, int]]):
        """Upload host set k and issue the ingest launch: (image, prediction, mask sums) views of the first len(sizes) images."""
        n = len(sizes)
        for key in self.dev:
            self.dev[key][:n].copy_(self.host[k][key][:n], non_blocking=True)
        if self.on_gpu:
            self.free[k] = torch.cuda.Event()
            self.free[k].record(torch.cuda.current_stream(self.device))
        self.lib.eval_ingest_u8(self.dev['image'], self.dev['inpainted'], self.dev['mask'], sizes, self.pad_mod, self.out_image, self.out_pred,
                                self.sums, n, clamp=self.clamp, stream=L.LamaLib.stream_of(self.out_image))
        return self.out_image[:n], self.out_pred[:n], self.sums[:n]


def _keeps_activations(score) -> bool:
    return hasattr(score, 'activations') and hasattr(score, 'activations_pred')


def _score_module(name: str, score):
    if _keeps_activations(score):                           # FIDScore: two [n, dims] activation batches per call, no per-image value
        return score.activations
    if not hasattr(score, 'score') or not hasattr(score, 'individual_values'):
        raise TypeError(f'score {name!r} ({type(score).__name__}): the device loop serves the pairwise scores (SSIMScore, LPIPSScore) and the '
                        'scores that keep activations (FIDScore)')
    return score.score


def score_dataset(dataset, scores: dict, *, batch_size: int = 8, device='cuda', clamp_image_range=None, evaluator=None, io_threads: int = 8,
                  lib: Optional[L.LamaLib] = None, ingest=DeviceIngest, tap=None):
    """One pass over a dataset of u8 items (``evaluation.PrecomputedInpaintingResultsDataset``).  Leaves every score's ``individual_values`` in
    dataset order and returns (groups, interval names): the mask-area bin of every item under ``evaluator``'s rule (an ``InpaintingEvaluator``,
    default bins) from the integer mask sums.  ``tap(indices, image, prediction, values, mask_sums)`` is called after every batch with its
    device tensors (views of buffers the next batch overwrites); ``ingest`` is the class that turns decoded items into those tensors."""
    lib = lib or L.get_lib()
    device = torch.device(device)
    if not lib.host_emulated and device.type != 'cuda':
        raise L.LamaError(f'lama_amd.evaluate runs on the GPU, not on {device} (there is no CPU path)')
    evaluator = evaluator or EV.InpaintingEvaluator(dataset, scores)
    n_items, pad_mod = len(dataset), dataset.pad_mod
    modules = {name: _score_module(name, s) for name, s in scores.items()}
    for s in scores.values():
        s.to(device)
        s.reset()
    acts = {name: _keeps_activations(s) for name, s in scores.items()}
    values = {name: ([None, None] if acts[name] else np.zeros(n_items, dtype=np.float64)) for name in scores}
    groups = np.zeros(n_items, dtype=np.int64)
    pool = ThreadPoolExecutor(max(1, min(MAX_IO_THREADS, int(io_threads))))
    try:
        sizes = list(pool.map(dataset.size, range(n_items)))
        with torch.no_grad():
            for bucket in plan_buckets(sizes, pad_mod, batch_size):
                ing = ingest(lib, bucket, batch_size, device, pad_mod, clamp_image_range)
                batches = bucket['batches']
                decoded = [[pool.submit(dataset.__getitem__, i) for i in b] for b in batches[:2]]      # two batches ahead of the device
                kept = {name: [] for name in scores}
                kept_sums = []
                for r, idx in enumerate(batches):
                    items = [f.result() for f in decoded[r]]
                    decoded[r] = None
                    if r + 2 < len(batches):
                        decoded.append([pool.submit(dataset.__getitem__, i) for i in batches[r + 2]])
                    image, pred, sums = ing.run(r & 1, ing.fill(r & 1, items))
                    kept_sums.append(sums.clone())
                    for name, m in modules.items():
                        if acts[name]:
                            kept[name].append(tuple(a.clone() for a in m(pred, image)))
                        else:
                            kept[name].append(m(pred, image).flatten().clone())
                    if tap is not None:
                        tap(idx, image, pred, {name: kept[name][-1] for name in scores}, kept_sums[-1])
                flat = np.asarray(bucket['items'])
                for name in scores:                          # the bucket's one read-back
                    if acts[name]:
                        for side in (0, 1):                  # [N, dims] rows of the predictions / the ground truth, dataset order
                            rows = torch.cat([k[side] for k in kept[name]]).cpu().numpy()
                            if values[name][side] is None:
                                values[name][side] = np.zeros((n_items, rows.shape[1]), dtype=rows.dtype)
                            values[name][side][flat] = rows
                    else:
                        values[name][flat] = torch.cat(kept[name]).cpu().numpy()
                Hp, Wp = bucket['shape']
                groups[flat] = evaluator.bins_of_mask_sums(torch.cat(kept_sums), Hp * Wp)
    finally:
        pool.shutdown()
    for name, s in scores.items():
        if acts[name]:
            s.activations_pred, s.activations_target = ([torch.from_numpy(v)] for v in values[name])      # one [N, dims] array each: ``groups`` indexes them
        else:
            s.individual_values = values[name]               # what np.hstack([[], fp32 batches]) leaves: float64, dataset order
    return groups, evaluator.bin_edges()[1]


# ---- the report --------------------------------------------------------------------------------------------------------------------------

def format_report(results: dict) -> str:
    """The text of ``pd.DataFrame(results).stack(1).unstack(0).dropna(axis=1, how='all').to_csv(sep='\\t', float_format='%.4f')``
    (evaluate_predicts.py:41-43) for a result dict {(score, group): {'mean': .., 'std': ..}}: two header lines (score, statistic), one line per
    group in sorted order, scores in the dict's order; a missing or NaN cell is empty, a column of only such cells is dropped."""
    scores, rows = [], set()
    for score, group in results:
        if score not in scores:
            scores.append(score)
        rows.add(group)
    rows = sorted(rows)
    stats = []
    for v in results.values():
        for st in v:
            if st not in stats:
                stats.append(st)

    def cell(score, st, group):
        v = results.get((score, group), {}).get(st)
        return None if v is None or (isinstance(v, (float, np.floating)) and math.isnan(v)) else v

    cols = [(sc, st) for sc in scores for st in stats if any(cell(sc, st, g) is not None for g in rows)]
    lines = ['\t'.join([''] + [sc for sc, _ in cols]), '\t'.join([''] + [st for _, st in cols])]
    for g in rows:
        lines.append('\t'.join([g] + ['' if cell(sc, st, g) is None else '%.4f' % cell(sc, st, g) for sc, st in cols]))
    return '\n'.join(lines) + '\n'


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------------

OWN_KEYS = ('model_path', 'backbone', 'fid_weights', 'batch_size', 'io_threads', 'precision')
DATASET_KEYS = ('img_suffix', 'inpainted_suffix', 'pad_out_to_modulo', 'scale_factor')
EVALUATOR_KEYS = ('batch_size', 'device', 'area_grouping', 'bins', 'clamp_image_range')


def load_config(path: str) -> dict:
    import yaml
    with open(path, 'r') as f:
        cfg = yaml.safe_load(f) or {}
    if (cfg.get('segmentation') or {}).get('enable', False):
        raise NotImplementedError(f'{path}: segmentation.enable is true -- the segmentation-aware scores (an ADE20k segmenter) are not served '
                                  'on the HIP path; set it to false for the ssim / lpips columns')
    for section, known in (('dataset_kwargs', DATASET_KEYS), ('evaluator_kwargs', EVALUATOR_KEYS)):
        unknown = sorted(set(cfg.get(section) or {}) - set(known))
        if unknown:
            raise L.LamaError(f'{path}: {section} keys {unknown} are not served (known: {list(known)})')
    return cfg


def build_evaluator(config: dict, datadir: str, predictdir: str, *, model_path=None, backbone=None, fid_weights=None, batch_size=None,
                    precision: Optional[str] = None, log=print) -> EV.InpaintingEvaluator:
    """The dataset, the scores and the evaluator an eval config asks for (``.dataset``, ``.scores`` of the returned evaluator)."""
    dataset = EV.PrecomputedInpaintingResultsDataset(datadir, predictdir, **(config.get('dataset_kwargs') or {}))
    if len(dataset) == 0:
        raise L.LamaError(f'no *mask*.png under {datadir!r}')
    metrics = {'ssim': EV.SSIMScore()}
    if model_path is None and backbone is None:
        log('lama_amd.evaluate: neither model_path= (LPIPS heads) nor backbone= (VGG-16) given: scoring SSIM only')
    else:
        metrics['lpips'] = EV.LPIPSScore(model_path=model_path, backbone=backbone)
        if precision is not None:
            metrics['lpips'].score.set_precision(precision)
    kw = dict(config.get('evaluator_kwargs') or {})
    if fid_weights is None:
        log('lama_amd.evaluate: no fid_weights= (the FID Inception-v3 state dict) given: no fid column')
    else:
        metrics['fid'] = EV.FIDScore(weights=fid_weights)
        if precision is not None:
            if precision not in ('f16x3', 'bf16x3'):
                raise L.LamaError(f'precision={precision}: the FID Inception runs in f16x3 or bf16x3 (lama_conv2d_rect_fwd has no {precision} form)')
            metrics['fid'].model.set_precision(L.PREC_NAMES[precision])
        if 'lpips' in metrics:                               # bin/evaluate_predicts.py:29-30: the integral row of the reference's report
            kw.update(integral_func=EV.lpips_fid100_f1, integral_title='lpips_fid100_f1')
    if batch_size is not None:
        kw['batch_size'] = int(batch_size)
    return EV.InpaintingEvaluator(dataset, scores=metrics, **kw)


def evaluate_predicts(config: dict, datadir: str, predictdir: str, outpath: Optional[str], *, io_threads: int = 8, tap=None, **build_kw) -> dict:
    """``bin/evaluate_predicts.py`` main(): dataset, scores, evaluator (``build_evaluator``), one pass of the device loop, the report.  Returns
    the result dict; ``tap``: see ``score_dataset``."""
    evaluator = build_evaluator(config, datadir, predictdir, **build_kw)
    groups, names = score_dataset(evaluator.dataset, evaluator.scores, batch_size=evaluator.batch_size, device=evaluator.device,
                                  clamp_image_range=evaluator.clamp_image_range, evaluator=evaluator, io_threads=io_threads, tap=tap)
    results = evaluator.results_of(groups if evaluator.area_grouping else None, names)
    if outpath:
        if os.path.dirname(outpath):
            os.makedirs(os.path.dirname(outpath), exist_ok=True)
        with open(outpath, 'w') as f:
            f.write(format_report(results))
    return results


def main(argv: Optional[Sequence[str]] = None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    pos, rest = argv[:4], argv[4:]                           # four paths (whatever they contain), then key=value options
    opts = dict(a.split('=', 1) for a in rest if '=' in a)
    unknown = sorted((set(opts) - set(OWN_KEYS)) | {a for a in rest if '=' not in a})
    if len(pos) != 4 or unknown:
        print(__doc__, file=sys.stderr)
        if unknown:
            print(f'unknown options: {unknown}', file=sys.stderr)
        return 2
    config = load_config(pos[0])
    results = evaluate_predicts(config, pos[1], pos[2], pos[3], model_path=opts.get('model_path'), backbone=opts.get('backbone'), fid_weights=opts.get('fid_weights'),
                                batch_size=opts.get('batch_size'), io_threads=int(opts.get('io_threads', 8)), precision=opts.get('precision'))
    print(format_report(results), end='')
    return 0


if __name__ == '__main__':
    sys.exit(main())
