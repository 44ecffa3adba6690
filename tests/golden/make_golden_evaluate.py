"""Golden vectors of the evaluator (dataset loader, SSIMScore / LPIPSScore, InpaintingEvaluator, InpaintingEvaluatorOnline, the report), produced by
the REFERENCE's own classes on the CPU (run where a checkout of the reference exists; the tests read only what this writes).
usage: python tests/golden/make_golden_evaluate.py <reference root>  ->  tests/golden/evaluate.npz, tests/golden/evaluate_report.tsv

The reference modules are imported from their files through stub packages (no package __init__ runs) with stubs for what they import and do not
use here: cv2, models.ade20k, fid.inception, easydict's load_yaml, torchvision / skimage (lpips.py).  LPIPS runs on the seeded synthetic VGG-16 of
tests/lpips_util.py with the real linear heads, as tests/golden/make_golden_lpips.py does.

Recorded per item: the u8 image / mask / prediction as written to disk (PNG), the fp32 items the reference's PrecomputedInpaintingResultsDataset
returns for them, the reference's per-image SSIM and LPIPS values, its fp32 mask area and both evaluators' bin of it; then the result dicts of
InpaintingEvaluator.evaluate() and InpaintingEvaluatorOnline.evaluation_end(), and the report pandas writes (bin/evaluate_predicts.py:41-43).
Asserted here: every mask area lies >= 1e-4 from every k / 10 edge (or is exactly 0 or 1), and the integer definition of the area
(sum of the padded u8 mask / (255 Hp Wp) in fp64) selects the same bin as the reference's fp32 mean under both binning rules."""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch
import tqdm.auto  # noqa: F401  (evaluator.py uses tqdm.auto after a bare `import tqdm`)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import evaluate_ref as ER  # noqa: E402
import lpips_util as U  # noqa: E402

if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], 'saicinpainting')):
    sys.exit(__doc__)
REF = os.path.abspath(sys.argv[1])
SD = U.backbone_state_dict()


def _stub(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _FakeVGG(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.features = U.features_sequential(SD)


def _move_to_device(obj, device):
    """What the reference's loops need of their helper: the tensors of a batch (any nesting of dicts and lists) on ``device``."""
    return torch.utils._pytree.tree_map(lambda leaf: leaf.to(device) if torch.is_tensor(leaf) else leaf, obj)


_stub('cv2', INTER_AREA=3, INTER_NEAREST=0)
_stub('skimage')
_stub('skimage.metrics', structural_similarity=None)
_stub('pytorch_lightning')
tvm = _stub('torchvision.models', vgg16=lambda pretrained=False, **kw: _FakeVGG())
_stub('torchvision', models=tvm)
_stub('models')
_stub('models.ade20k', SegmentationModule=None, NUM_CLASS=150, segm_options=None)
_stub('saicinpainting', os.path.join(REF, 'saicinpainting'))
_stub('saicinpainting.utils', get_shape=None)
_stub('saicinpainting.evaluation', os.path.join(REF, 'saicinpainting/evaluation'))
_stub('saicinpainting.evaluation.utils', move_to_device=_move_to_device)
_stub('saicinpainting.evaluation.losses', os.path.join(REF, 'saicinpainting/evaluation/losses'))
_stub('saicinpainting.evaluation.losses.fid')
_stub('saicinpainting.evaluation.losses.fid.inception', InceptionV3=None)
ref_data = importlib.import_module('saicinpainting.evaluation.data')
ref_eval = importlib.import_module('saicinpainting.evaluation.evaluator')
ref_loss = importlib.import_module('saicinpainting.evaluation.losses.base_loss')

g = np.random.default_rng(20261019)


def smooth_u8(h, w):
    """A blocky random image under strong noise: structure for SSIM / LPIPS, and local variance far above SSIM's C2 = 9e-4 everywhere.  (On flat
    blocks the fp32 sigma^2 = E[x^2] - mu^2 of ssim.py cancels and the reference's own fp32 value drifts up to 3e-6 from its fp64 value -- more
    than the bar of the SSIM tests; see the assert on `ssim_values64` below.)"""
    base = g.integers(32, 224, ((h + 7) // 8, (w + 7) // 8, 3))
    img = np.kron(base, np.ones((8, 8, 1), dtype=np.int64))[:h, :w]
    return np.clip(img + g.integers(-48, 49, img.shape), 0, 255).astype(np.uint8)


def rect_mask(h, w, frac, grey=True):
    """A rectangle of about ``frac`` of the plane, grey-valued inside (1 .. 255), 0 outside."""
    m = np.zeros((h, w), np.uint8)
    if frac <= 0:
        return m
    if frac >= 1:
        m[:] = 255
        return m
    rh = max(1, int(round(h * frac ** 0.5)))
    rw = max(1, int(round(w * frac ** 0.5)))
    y0, x0 = int(g.integers(0, h - rh + 1)), int(g.integers(0, w - rw + 1))
    m[y0:y0 + rh, x0:x0 + rw] = g.integers(128, 256, (rh, rw)) if grey else 255
    return m


# dataset order = sorted file names.  The reference's batches of REF_BATCH hold one padded size each (its default collate stacks them), and the
# padded sizes alternate between batches so that a loop that buckets by padded size must restore the dataset order.
SPEC = [((37, 45), 0.05), ((37, 45), 0.30), ((40, 48), 1.0), ((37, 45), 0.55),
        ((32, 32), 0.0), ((32, 32), 0.18), ((32, 32), 0.62), ((32, 32), 0.30),
        ((40, 48), 0.45), ((37, 45), 0.80), ((40, 48), 0.12), ((37, 45), 0.66)]
out = {}
names = []
for i, ((h, w), frac) in enumerate(SPEC):
    n = f'img{i:02d}'
    names.append(n)
    img, mask = smooth_u8(h, w), rect_mask(h, w, frac, grey=(i % 4 != 1))
    pred = img.copy()
    hole = mask > 0
    pred[hole] = np.clip(smooth_u8(h, w)[hole].astype(np.int64) // 2 + img[hole].astype(np.int64) // 2 + g.integers(-20, 21, (int(hole.sum()), 3)),
                         0, 255).astype(np.uint8)
    if i == 4:                                    # the all-zero mask: still a prediction that differs (not NEAR-identical: tests/golden/make_golden_lpips.py, case h)
        pred = np.clip(img.astype(np.int64) + g.integers(-40, 41, img.shape), 0, 255).astype(np.uint8)
    out[f'{n}_image'], out[f'{n}_mask'], out[f'{n}_inpainted'] = img, mask, pred
out['names'] = np.array(names)

heads_path = os.path.join(REF, 'models/lpips_models/vgg.pth')
with tempfile.TemporaryDirectory() as td:
    datadir, preddir = ER.write_dataset(out, td)
    ds = ref_data.PrecomputedInpaintingResultsDataset(datadir, preddir, inpainted_suffix=ER.INPAINTED_SUFFIX, img_suffix=ER.IMG_SUFFIX,
                                                      pad_out_to_modulo=ER.PAD_MOD)
    assert len(ds) == len(names)
    out['rel_mask'] = np.array([os.path.relpath(f, datadir) for f in ds.mask_filenames])
    out['rel_img'] = np.array([os.path.relpath(f, datadir) for f in ds.img_filenames])
    out['rel_pred'] = np.array([os.path.relpath(f, preddir) for f in ds.pred_filenames])
    items = [ds[i] for i in range(len(ds))]
    for n, it in zip(names, items):
        out[f'{n}_item_image'], out[f'{n}_item_mask'], out[f'{n}_item_inpainted'] = it['image'], it['mask'], it['inpainted']
        assert it['image'].dtype == np.float32 and it['mask'].shape[0] == 1

    def scores():
        return {'ssim': ref_loss.SSIMScore(), 'lpips': ref_loss.LPIPSScore(model_path=heads_path, use_gpu=False)}

    # InpaintingEvaluator.evaluate()
    sc = scores()
    ev = ref_eval.InpaintingEvaluator(ds, scores=sc, batch_size=ER.REF_BATCH, device='cpu', area_grouping=True, bins=10)
    groups, interval_names = ev._get_bin_edges()
    res_eval = ev.evaluate()
    for k, s in sc.items():
        out[f'{k}_values'] = np.asarray(s.individual_values)          # float64 array of the fp32 per-image values, dataset order
        assert out[f'{k}_values'].shape == (len(names),)
    out['eval_groups'] = np.asarray(groups)

    # the reference's own fp64 values: the distance of its fp32 values from them is what the bars of the tests are measured in
    ssim64 = ref_loss.SSIMScore().double()
    lpips64 = ref_loss.LPIPSScore(model_path=heads_path, use_gpu=False).double()
    with torch.no_grad():
        for it in items:
            im, pr = torch.from_numpy(it['image'])[None].double(), torch.from_numpy(it['inpainted'])[None].double()
            ssim64(pr, im)
            lpips64(pr, im)
    out['ssim_values64'], out['lpips_values64'] = np.asarray(ssim64.individual_values), np.asarray(lpips64.individual_values)
    ssim_own = np.abs(out['ssim_values'] - out['ssim_values64'])
    lpips_own = np.abs(out['lpips_values'] - out['lpips_values64']) / out['lpips_values64']
    print('reference fp32 vs fp64: SSIM abs', ssim_own.max(), 'LPIPS rel', lpips_own.max(), 'in units of lpips.npz', lpips_own.max() / float(np.load(U.GOLDEN)['unit']))
    # the tests hold the device values to the bars of tests/test_eval_gpu.py (2e-6 absolute, against these fp32 vectors AND against fp64) and of
    # tests/test_lpips_gpu.py (16 units of lpips.npz against fp64, 17 against the fp32 vectors): the vectors' own distance from fp64 must leave
    # room under them for an implementation that is right
    assert ssim_own.max() <= 1.5e-6, ssim_own
    assert lpips_own.max() <= 2 * float(np.load(U.GOLDEN)['unit']), lpips_own

    # InpaintingEvaluatorOnline: forward per batch, evaluation_end()
    sc2 = scores()
    online = ref_eval.InpaintingEvaluatorOnline(scores=sc2, bins=10)
    loader = torch.utils.data.DataLoader(ds, shuffle=False, batch_size=ER.REF_BATCH)
    areas32 = []
    states = []
    for batch in loader:
        states.append(online(batch))
        areas32.append(batch['mask'].reshape(batch['mask'].shape[0], -1).mean(dim=-1).numpy())
    out['online_groups'] = np.asarray(online.groups)
    for k in sc2:
        assert np.array_equal(np.asarray(sc2[k].individual_values), out[f'{k}_values'])
    res_online = online.evaluation_end()
    for batch in loader:                                  # (evaluation_end reset the groups) the same end from gathered states: fp32 statistics
        online(batch)
    res_states = online.evaluation_end(states=states)
    areas32 = np.hstack(areas32)
    out['area_fp32'] = areas32

for prefix, res in (('eval', res_eval), ('online', res_online), ('states', res_states)):
    out[f'{prefix}_keys'] = np.array([f'{a}|{b}' for a, b in res])
    out[f'{prefix}_vals'] = np.array([[np.float64(v['mean']), np.float64(v['std'])] for v in res.values()], dtype=np.float64)

# the integer definition of the area against the reference's fp32 mean: the same bins under both rules, areas away from the edges
edges = np.linspace(0, 1, 11)
sums, planes = [], []
for n in names:
    m = out[f'{n}_mask']
    h, w = m.shape
    mp = np.pad(m, ((0, ER.ceil_modulo(h, ER.PAD_MOD) - h), (0, ER.ceil_modulo(w, ER.PAD_MOD) - w)), mode='symmetric')
    sums.append(int(mp.astype(np.int64).sum()))
    planes.append(mp.size)
area64 = np.array(sums, dtype=np.float64) / (255.0 * np.array(planes, dtype=np.float64))
out['mask_sums'], out['planes'] = np.array(sums, dtype=np.int64), np.array(planes, dtype=np.int64)
for a in area64:
    assert a in (0.0, 1.0) or np.abs(edges - a).min() >= 1e-4, a
assert (area64 == 1.0).sum() == 1 and (area64 == 0.0).sum() == 1
b_eval = np.searchsorted(edges, area64, side='right') - 1
b_eval[b_eval == 10] = 9
assert np.array_equal(b_eval, out['eval_groups']), (b_eval, out['eval_groups'])
assert np.array_equal(np.clip(np.searchsorted(edges, area64) - 1, 0, 9), out['online_groups'])
assert np.abs(area64 - areas32).max() < 1e-6
assert any(((out[f'{n}_mask'] > 0) & (out[f'{n}_mask'] < 255)).any() for n in names)
print('areas', np.round(area64, 4).tolist())
print('groups', out['eval_groups'].tolist(), out['online_groups'].tolist())

import pandas as pd  # noqa: E402
results = pd.DataFrame(res_eval).stack(1).unstack(0)
results.dropna(axis=1, how='all', inplace=True)
results.to_csv(ER.GOLDEN_TSV, sep='\t', float_format='%.4f')
print(open(ER.GOLDEN_TSV).read())
np.savez_compressed(ER.GOLDEN, **out)
print('bytes', os.path.getsize(ER.GOLDEN))
