"""CPU: the evaluator around the scores -- the ingest launch through the host emulator (bit-equal to the reference's numpy chain, exact mask sums,
error codes), and the host bookkeeping with the reference's recorded per-image values injected (tests/golden/evaluate.npz, written by
tests/golden/make_golden_evaluate.py from the reference's own classes): scores' get_value, both evaluators' grouping and result dicts, the
report text, the dataset's file pairing and decoded arrays."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emu  # noqa: E402
import evaluate_ref as ER  # noqa: E402
from lama_amd import _lib as L  # noqa: E402
from lama_amd import evaluate as EVL  # noqa: E402
from lama_amd import evaluation as EV  # noqa: E402

GOLD = ER.load_gold()
NAMES = ER.item_names(GOLD)


def _ingest(lib, gt, pred, mask, sizes, pad_mod, clamp, shape=None, **kw):
    B, Hs, Ws = mask.shape
    h, w = (sizes or [(Hs, Ws)])[0]
    Hp, Wp = shape or (ER.ceil_modulo(h, pad_mod), ER.ceil_modulo(w, pad_mod))
    oi = torch.full((B, 3, Hp, Wp), -7.0)
    op = torch.full((B, 3, Hp, Wp), -7.0)
    sums = torch.full((B,), -1, dtype=torch.int64)
    args = dict(out_image=oi, out_pred=op, mask_sum=sums)
    args.update(kw)
    lib.eval_ingest_u8(torch.from_numpy(gt), torch.from_numpy(pred), torch.from_numpy(mask), sizes, pad_mod, args['out_image'], args['out_pred'],
                       args['mask_sum'], B, clamp=clamp)
    return oi.numpy(), op.numpy(), sums.tolist()


@pytest.mark.parametrize('clamp', ER.CLAMPS, ids=['noclamp', 'clamp'])
@pytest.mark.parametrize('case', list(ER.INGEST_CASES))
def test_ingest_is_bit_equal_to_numpy(case, clamp):
    slot, pad_mod, sizes, batch = ER.INGEST_CASES[case]
    gt, pred, mask = ER.ingest_inputs(slot, sizes, batch, seed=len(case))
    want_i, want_p, want_s = ER.ingest_ref(gt, pred, mask, sizes, pad_mod, clamp)
    got_i, got_p, got_s = _ingest(emu.emu_lib(), gt, pred, mask, sizes, pad_mod, clamp)
    assert got_i.tobytes() == want_i.tobytes()
    assert got_p.tobytes() == want_p.tobytes()              # never clamped
    assert got_s == want_s                                  # exact integers
    if clamp is not None:
        assert want_i.min() >= np.float32(clamp[0]) and want_i.max() <= np.float32(clamp[1]) and want_p.max() > 0.9


def test_ingest_error_paths():
    lib = emu.emu_lib()
    gt, pred, mask = ER.ingest_inputs((16, 24), None, 2, seed=3)
    with pytest.raises(L.LamaError) as e:                    # padded sizes 16 x 24 and 8 x 24 in one launch
        _ingest(lib, gt, pred, mask, [(13, 21), (8, 21)], 8, None, shape=(16, 24))
    assert e.value.code == L.ERR_BAD_ARG
    with pytest.raises(L.LamaError) as e:                    # a null output
        _ingest(lib, gt, pred, mask, None, 8, None, out_pred=None)
    assert e.value.code == L.ERR_BAD_ARG
    with pytest.raises(L.LamaError) as e:                    # a null sum
        _ingest(lib, gt, pred, mask, None, 8, None, mask_sum=None)
    assert e.value.code == L.ERR_BAD_ARG
    with pytest.raises(L.LamaError) as e:                    # an image larger than its slot
        _ingest(lib, gt, pred, mask, [(17, 24), (16, 24)], 8, None, shape=(24, 24))
    assert e.value.code == L.ERR_BAD_ARG
    g3 = ER.ingest_inputs((3, 3), None, 1, seed=4)
    with pytest.raises(L.LamaError) as e:                    # 3 x 3 at pad_mod 8: five rows of padding from three
        _ingest(lib, *g3, None, 8, None)
    assert e.value.code == L.ERR_UNSUPPORTED


def test_ingest_more_images_than_one_argument_block():
    """70 images: the sizes ride in the argument block 64 at a time, so this is two launches behind one call."""
    sizes = [(5 + i % 4, 6 + i % 3) for i in range(70)]
    gt, pred, mask = ER.ingest_inputs((8, 8), sizes, 70, seed=5)
    want_i, want_p, want_s = ER.ingest_ref(gt, pred, mask, sizes, 8, None)
    got_i, got_p, got_s = _ingest(emu.emu_lib(), gt, pred, mask, sizes, 8, None)
    assert got_i.tobytes() == want_i.tobytes() and got_p.tobytes() == want_p.tobytes() and got_s == want_s


# ---- bookkeeping with the reference's per-image values injected ---------------------------------------------------------------------------

class _Recorded(EV.PairwiseScore):
    """A score whose forward hands out the reference's recorded values of the next items (the kernels are tested elsewhere)."""

    def __init__(self, values):
        super().__init__()
        self.values, self.at = values, 0
        self.reset()

    def reset(self):
        super().reset()
        self.at = 0

    def forward(self, pred_batch, target_batch, mask=None):
        n = pred_batch.shape[0]
        v = torch.from_numpy(self.values[self.at:self.at + n].astype(np.float32))
        self.at += n
        self.individual_values = np.hstack([self.individual_values, v.numpy()])
        return v


class _FloatItems(torch.utils.data.Dataset):
    """The reference dataset's fp32 items as recorded."""

    def __len__(self):
        return len(NAMES)

    def __getitem__(self, i):
        n = NAMES[i]
        return dict(image=GOLD[f'{n}_item_image'], mask=GOLD[f'{n}_item_mask'], inpainted=GOLD[f'{n}_item_inpainted'])


def _recorded_scores():
    return {'ssim': _Recorded(GOLD['ssim_values']), 'lpips': _Recorded(GOLD['lpips_values'])}


def test_scores_get_value_matches_the_reference():
    want = ER.results_dict(GOLD, 'eval')
    ssim, lpips = EV.SSIMScore(), EV.LPIPSScore.__new__(EV.LPIPSScore)       # (LPIPSScore's bookkeeping needs no weights)
    torch.nn.Module.__init__(lpips)
    names = EV.InpaintingEvaluator(None, {}).bin_edges()[1]
    for name, score in (('ssim', ssim), ('lpips', lpips)):
        score.individual_values = GOLD[f'{name}_values']
        total, groups = score.get_value(groups=GOLD['eval_groups'])
        got = {(name, 'total'): total}
        got.update({(name, names[k]): v for k, v in groups.items()})
        ER.same_results(got, {k: v for k, v in want.items() if k[0] == name})
        total_only, none = score.get_value()
        assert none is None and np.float64(total_only['mean']).tobytes() == np.float64(want[(name, 'total')]['mean']).tobytes()
    grouping = EV.get_groupings(GOLD['eval_groups'])
    assert sorted(np.concatenate(list(grouping.values())).tolist()) == list(range(len(NAMES)))
    assert all((GOLD['eval_groups'][idx] == label).all() for label, idx in grouping.items())


def test_inpainting_evaluator_matches_the_reference():
    ev = EV.InpaintingEvaluator(_FloatItems(), _recorded_scores(), batch_size=ER.REF_BATCH, device='cpu')
    groups, names = ev._get_bin_edges()
    assert np.array_equal(groups, GOLD['eval_groups'])
    assert np.array_equal(ev.bins_of_mask_sums(GOLD['mask_sums'], GOLD['planes']), GOLD['eval_groups'])       # the integer definition of the area
    ER.same_results(ev.evaluate(), ER.results_dict(GOLD, 'eval'))


def test_online_evaluator_matches_the_reference():
    want = ER.results_dict(GOLD, 'online')
    ev = EV.InpaintingEvaluatorOnline(_recorded_scores())
    loader = torch.utils.data.DataLoader(_FloatItems(), shuffle=False, batch_size=ER.REF_BATCH)
    states = [ev.process_batch(batch) for batch in loader]
    assert np.array_equal(np.array(ev.groups), GOLD['online_groups'])
    ER.same_results(ev.evaluation_end(), want)
    assert ev.groups == [] and ev.scores['ssim'].individual_values == []
    # the states form (what a distributed validation loop gathers), with the groups from the kernel's integer sums
    at = 0
    for batch in loader:
        n = batch['image'].shape[0]
        ev({'image': batch['image'], 'inpainted': batch['inpainted'], 'mask_sum': torch.from_numpy(GOLD['mask_sums'][at:at + n])})
        at += n
    assert np.array_equal(np.array(ev.groups), GOLD['online_groups'])
    for sc in ev.scores.values():
        sc.individual_values = None                          # the values must come from the states
    ER.same_results(ev.evaluation_end(states=states), ER.results_dict(GOLD, 'states'))     # (fp32 statistics: the states are fp32 tensors)


def test_binning_rules_differ_on_an_edge():
    """evaluator.py:59-61 against evaluator.py:165: an area ON an edge goes up in one and down in the other; area 1 is the last bin in both."""
    area = np.array([0.0, np.linspace(0, 1, 11)[3], 1.0])
    assert EV.InpaintingEvaluator(None, {}).bins_of_area(area.copy()).tolist() == [0, 3, 9]
    assert EV.InpaintingEvaluatorOnline({}).bins_of_area(area.copy()).tolist() == [0, 2, 9]
    assert EV.mask_area(np.array([255 * 40 * 48]), 40 * 48)[0] == 1.0


def test_report_text_is_byte_equal_to_pandas():
    text = EVL.format_report(ER.results_dict(GOLD, 'eval'))
    assert text.encode() == open(ER.GOLDEN_TSV, 'rb').read()


def test_dataset_pairs_and_decodes_as_the_reference(tmp_path):
    datadir, preddir = ER.write_dataset(GOLD, str(tmp_path))
    ds = EV.PrecomputedInpaintingResultsDataset(datadir, preddir, inpainted_suffix=ER.INPAINTED_SUFFIX, img_suffix=ER.IMG_SUFFIX,
                                                pad_out_to_modulo=ER.PAD_MOD)
    assert len(ds) == len(NAMES)
    assert [os.path.relpath(f, datadir) for f in ds.mask_filenames] == [str(s) for s in GOLD['rel_mask']]
    assert [os.path.relpath(f, datadir) for f in ds.img_filenames] == [str(s) for s in GOLD['rel_img']]
    assert [os.path.relpath(f, preddir) for f in ds.pred_filenames] == [str(s) for s in GOLD['rel_pred']]
    for i, n in enumerate(NAMES):
        it = ds[i]
        assert it['image'].dtype == np.uint8 and it['mask'].dtype == np.uint8 and it['inpainted'].dtype == np.uint8
        assert ds.size(i) == it['mask'].shape
        for key in ('image', 'mask', 'inpainted'):
            assert ER.host_item(it[key], ER.PAD_MOD).tobytes() == GOLD[f'{n}_item_{key}'].tobytes(), (n, key)
    with pytest.raises(NotImplementedError):
        EV.PrecomputedInpaintingResultsDataset(datadir, preddir, scale_factor=0.5)


def test_device_loop_through_the_emulator_restores_dataset_order(tmp_path):
    """The whole loop on the emulator with SSIM (LPIPS's thirteen convolutions are too slow there): buckets by padded size, values back in dataset
    order, groups from the integer sums; SSIM within the GPU suite's bar of the reference's recorded values."""
    datadir, preddir = ER.write_dataset(GOLD, str(tmp_path))
    ds = EV.PrecomputedInpaintingResultsDataset(datadir, preddir, inpainted_suffix=ER.INPAINTED_SUFFIX, img_suffix=ER.IMG_SUFFIX,
                                                pad_out_to_modulo=ER.PAD_MOD)
    score = EV.SSIMScore()
    score.score._lib = emu.emu_lib()
    seen = []
    groups, names = EVL.score_dataset(ds, {'ssim': score}, batch_size=8, device='cpu', lib=emu.emu_lib(), io_threads=2,
                                      tap=lambda idx, image, pred, values, sums: seen.append((list(idx), tuple(image.shape))))
    assert [s for _, s in seen] == [(8, 3, 40, 48), (4, 3, 32, 32)] and seen[1][0] == [4, 5, 6, 7]
    assert np.array_equal(groups, GOLD['eval_groups']) and names[0] == '0-10%'
    assert score.individual_values.dtype == np.float64 and np.abs(score.individual_values - GOLD['ssim_values']).max() < 2e-6


def test_make_evaluator_and_config_refusals(tmp_path):
    with pytest.raises(NotImplementedError, match='FID'):
        EV.make_evaluator(fid=True)
    with pytest.raises(NotImplementedError, match='FID'):
        EV.make_evaluator(lpips=False, integral_kind='ssim_fid100_f1')
    with pytest.raises(ValueError):
        EV.make_evaluator(lpips=False, integral_kind='nonsense')
    ev = EV.make_evaluator(lpips=False, bins=5)
    assert isinstance(ev, EV.InpaintingEvaluatorOnline) and list(ev.scores) == ['ssim'] and ev.interval_names[-1] == '80-100%'
    cfg = tmp_path / 'eval_segm.yaml'
    cfg.write_text('evaluator_kwargs:\n  batch_size: 8\ndataset_kwargs:\n  img_suffix: .png\nsegmentation:\n  enable: true\n')
    with pytest.raises(NotImplementedError, match='segmentation'):
        EVL.load_config(str(cfg))
