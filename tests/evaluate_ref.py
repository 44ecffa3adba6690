"""Shared by the evaluator's golden script and its tests: the host statement of the ingest launch (numpy, the reference's own chain), the shapes the
ingest tests run, and access to tests/golden/evaluate.npz (see tests/golden/make_golden_evaluate.py)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'evaluate.npz')
GOLDEN_TSV = os.path.join(HERE, 'golden', 'evaluate_report.tsv')
PAD_MOD = 8                      # dataset_kwargs.pad_out_to_modulo of the recorded dataset
IMG_SUFFIX, INPAINTED_SUFFIX = '.png', '_inpainted.png'
REF_BATCH = 4                    # batch size of the reference run (its default collate needs one padded size per batch)

# name -> (slot (Hs, Ws), pad_mod, per-image (h, w) or None = every image fills its slot, batch)
INGEST_CASES = {
    'full_8x8': ((8, 8), 1, None, 2),
    'mixed_13x21': ((16, 24), 8, [(13, 21), (16, 24), (9, 17)], 3),          # three true sizes, one padded size, one launch
    'odd_w_16x19': ((16, 19), 8, None, 1),                                   # W % 4 != 0: no dword loads
    'odd_out_9x19': ((9, 19), 1, None, 2),                                   # Wp % 4 != 0: no float4 stores
}
CLAMPS = (None, (0.2, 0.7))


def ceil_modulo(x, mod):
    return x if x % mod == 0 else (x // mod + 1) * mod


def ingest_inputs(slot, sizes, batch, seed):
    """u8 slots [B,Hs,Ws,3] x 2 and [B,Hs,Ws], random everywhere (the bytes outside an image's h x w corner must not reach the output)."""
    g = np.random.default_rng(seed)
    Hs, Ws = slot
    gt = g.integers(0, 256, (batch, Hs, Ws, 3), dtype=np.uint8)
    pred = g.integers(0, 256, (batch, Hs, Ws, 3), dtype=np.uint8)
    mask = g.integers(0, 256, (batch, Hs, Ws), dtype=np.uint8)
    mask[0] = 255                                                            # the largest sum an image can have
    return gt, pred, mask


def host_item(u8_hwc, pad_mod):
    """data.py:12-20,29-33 on a decoded image [h,w,3] / mask [h,w]: CHW fp32 / 255, symmetric padding bottom / right."""
    img = u8_hwc[None] if u8_hwc.ndim == 2 else np.transpose(u8_hwc, (2, 0, 1))
    img = img.astype('float32') / 255
    _, h, w = img.shape
    return np.pad(img, ((0, 0), (0, ceil_modulo(h, pad_mod) - h), (0, ceil_modulo(w, pad_mod) - w)), mode='symmetric')


def ingest_ref(gt, pred, mask, sizes, pad_mod, clamp):
    """What the launch must leave: (image [B,3,Hp,Wp] fp32, prediction [B,3,Hp,Wp] fp32, [int sum of the padded u8 mask per image])."""
    B, Hs, Ws = mask.shape
    sizes = sizes or [(Hs, Ws)] * B
    imgs, preds, sums = [], [], []
    for b, (h, w) in enumerate(sizes):
        im = host_item(gt[b, :h, :w], pad_mod)
        if clamp is not None:
            im = np.clip(im, np.float32(clamp[0]), np.float32(clamp[1]))     # evaluator.py:87-90 on the ground truth only
        imgs.append(im)
        preds.append(host_item(pred[b, :h, :w], pad_mod))
        m = mask[b, :h, :w]
        mp = np.pad(m, ((0, ceil_modulo(h, pad_mod) - h), (0, ceil_modulo(w, pad_mod) - w)), mode='symmetric')
        sums.append(int(mp.astype(np.int64).sum()))
    return np.stack(imgs), np.stack(preds), sums


# ---- tests/golden/evaluate.npz ---------------------------------------------------------------------------------------------------------

def load_gold():
    return np.load(GOLDEN)


def item_names(gold):
    return [str(n) for n in gold['names']]


def write_dataset(gold, root):
    """The recorded triples as the files ``bin/gen_mask_dataset.py`` + a predict run leave: <root>/data/<name>.png, <name>_mask000.png and
    <root>/pred/<name>_mask000_inpainted.png.  Returns (datadir, predictdir)."""
    from PIL import Image
    datadir, preddir = os.path.join(root, 'data'), os.path.join(root, 'pred')
    os.makedirs(datadir, exist_ok=True)
    os.makedirs(preddir, exist_ok=True)
    for n in item_names(gold):
        Image.fromarray(gold[f'{n}_image']).save(os.path.join(datadir, n + IMG_SUFFIX))
        Image.fromarray(gold[f'{n}_mask']).save(os.path.join(datadir, n + '_mask000.png'))
        Image.fromarray(gold[f'{n}_inpainted']).save(os.path.join(preddir, n + '_mask000' + INPAINTED_SUFFIX))
    return datadir, preddir


def results_dict(gold, prefix):
    """The recorded result dict of ``InpaintingEvaluator.evaluate()`` (prefix 'eval') / ``InpaintingEvaluatorOnline.evaluation_end()`` ('online';
    'states': the same from the gathered per-batch states):
    {(score name, group name): {'mean': float64, 'std': float64}} in the reference's insertion order."""
    out = {}
    for key, (mean, std) in zip(gold[f'{prefix}_keys'], gold[f'{prefix}_vals']):
        score, group = str(key).split('|')
        out[(score, group)] = {'mean': mean, 'std': std}
    return out


def same_results(got, want):
    """Bit-equality of two result dicts, key order included."""
    assert list(got) == list(want), (list(got), list(want))
    for k in want:
        for stat in ('mean', 'std'):
            a, b = np.float64(got[k][stat]), np.float64(want[k][stat])
            assert a.tobytes() == b.tobytes(), (k, stat, a, b)
