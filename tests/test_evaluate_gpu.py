"""GPU: the evaluator on the device -- the ingest launch against the reference's numpy chain (bit-equal, exact mask sums, graph capture, refusals
before any launch) and the evaluation loop / CLI end to end on the recorded dataset of tests/golden/evaluate.npz (the reference's own per-image
values, groups and report; LPIPS on the seeded synthetic backbone of tests/lpips_util.py with the real heads).

Bars (taken from the tests that already hold these quantities, not loosened): SSIM 2e-6 absolute against the reference's fp32 values and its fp64
values (tests/test_eval_gpu.py); LPIPS on the default f16x3 arithmetic 16 units relative against the reference's fp64 values, one unit = `unit` of
tests/golden/lpips.npz (tests/test_lpips_gpu.py).  This file's own, in addition: 17 units against the reference's fp32 values (16 plus the one
unit the fp32 reference itself may be off its fp64 twin; tests/test_lpips_gpu.py prints that distance without asserting it).  The report: every
number within one unit of the fourth decimal of the one pandas wrote from the reference's values."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import evaluate_ref as ER  # noqa: E402
import lpips_util as U  # noqa: E402
from lama_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = ER.load_gold()
NAMES = ER.item_names(GOLD)
LPIPS_GOLD = np.load(U.GOLDEN)
UNIT = float(LPIPS_GOLD['unit'])
SSIM_BAR, LPIPS_BAR = 2e-6, 16


def _ingest(gt, pred, mask, sizes, pad_mod, clamp, shape=None, **kw):
    B, Hs, Ws = mask.shape
    h, w = (sizes or [(Hs, Ws)])[0]
    Hp, Wp = shape or (ER.ceil_modulo(h, pad_mod), ER.ceil_modulo(w, pad_mod))
    oi = torch.full((B, 3, Hp, Wp), -7.0, device='cuda')
    op = torch.full((B, 3, Hp, Wp), -7.0, device='cuda')
    sums = torch.full((B,), -1, dtype=torch.int64, device='cuda')
    args = dict(out_image=oi, out_pred=op, mask_sum=sums)
    args.update(kw)
    L.get_lib().eval_ingest_u8(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), torch.from_numpy(mask).cuda(), sizes, pad_mod,
                               args['out_image'], args['out_pred'], args['mask_sum'], B, clamp=clamp, stream=L.LamaLib.stream_of(oi))
    return oi.cpu().numpy(), op.cpu().numpy(), sums.tolist()


@pytest.mark.parametrize('clamp', ER.CLAMPS, ids=['noclamp', 'clamp'])
@pytest.mark.parametrize('case', list(ER.INGEST_CASES))
def test_ingest_is_bit_equal_to_numpy(case, clamp):
    slot, pad_mod, sizes, batch = ER.INGEST_CASES[case]
    gt, pred, mask = ER.ingest_inputs(slot, sizes, batch, seed=len(case))
    want_i, want_p, want_s = ER.ingest_ref(gt, pred, mask, sizes, pad_mod, clamp)
    got_i, got_p, got_s = _ingest(gt, pred, mask, sizes, pad_mod, clamp)
    assert got_i.tobytes() == want_i.tobytes()
    assert got_p.tobytes() == want_p.tobytes()
    assert got_s == want_s


def test_ingest_production_shape():
    """8 x 512 x 512 at pad_mod 8 (dword loads, float4 stores, more conversion workgroups than the grid's cap), two of the images smaller than
    their slot (509 x 507 and 512 x 510: padded rows and columns, element loads at the right edge)."""
    sizes = [(512, 512)] * 6 + [(509, 507), (512, 510)]
    gt, pred, mask = ER.ingest_inputs((512, 512), sizes, 8, seed=8)
    want_i, want_p, want_s = ER.ingest_ref(gt, pred, mask, sizes, 8, (0.0, 1.0))
    got_i, got_p, got_s = _ingest(gt, pred, mask, sizes, 8, (0.0, 1.0))
    assert got_i.tobytes() == want_i.tobytes() and got_p.tobytes() == want_p.tobytes()
    assert got_s == want_s and got_s[0] == 255 * 512 * 512


def test_ingest_is_graph_safe(run):
    """One capture and one replay of the launch (in the child process: tests/evaluate_child.py) leave what the plain launch left."""
    plain, replayed = run['graph']['plain'], run['graph']['replayed']
    assert len(plain) == len(replayed) == 3 and float(plain[0].max()) > 0 and int(plain[2].min()) >= 0
    for x, y in zip(plain, replayed):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def test_ingest_refusals_come_before_any_launch():
    gt, pred, mask = ER.ingest_inputs((16, 24), None, 2, seed=3)
    for kw, sizes, shape, code in ((dict(), [(13, 21), (8, 21)], (16, 24), L.ERR_BAD_ARG), (dict(out_pred=None), None, None, L.ERR_BAD_ARG),
                                   (dict(mask_sum=None), None, None, L.ERR_BAD_ARG), (dict(), [(17, 24), (16, 24)], (24, 24), L.ERR_BAD_ARG)):
        with pytest.raises(L.LamaError) as e:
            _ingest(gt, pred, mask, sizes, 8, None, shape=shape, **kw)
        assert e.value.code == code
    with pytest.raises(L.LamaError) as e:
        _ingest(*ER.ingest_inputs((3, 3), None, 1, seed=4), None, 8, None)
    assert e.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(L.LamaError):                         # host tensors: no CPU path
        L.get_lib().eval_ingest_u8(torch.from_numpy(gt), torch.from_numpy(pred), torch.from_numpy(mask), None, 8, torch.zeros(2, 3, 16, 24),
                                   torch.zeros(2, 3, 16, 24), torch.zeros(2, dtype=torch.int64), 2)
    torch.cuda.synchronize()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def run(tmp_path_factory):
    """What tests/evaluate_child.py saw, in ONE process of its own: the CLI on the recorded dataset (its report), the same run through
    ``score_dataset`` with a tap on every batch, the direct score calls on the tapped tensors, the evaluator class and the captured ingest
    launch.  (This process keeps no graph, side stream or pinned buffer of that run.)"""
    root = tmp_path_factory.mktemp('evaluate')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'evaluate_child.py'), str(root)], cwd=os.path.dirname(HERE), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(root / 'child.pkl', 'rb') as f:
        seen = pickle.load(f)
    assert seen['rc'] == 0 and seen['rc_ssim'] == 0
    assert 'scoring SSIM only' in r.stdout                  # ... and says so
    return seen


def test_per_image_values_meet_the_bars_of_the_score_tests(run):
    ssim, lpips = run['individual']['ssim'], run['individual']['lpips']
    assert ssim.dtype == np.float64 and ssim.shape == (len(NAMES),) and lpips.shape == (len(NAMES),)
    e32, e64 = np.abs(ssim - GOLD['ssim_values']), np.abs(ssim - GOLD['ssim_values64'])
    v32, v64 = GOLD['lpips_values'], GOLD['lpips_values64']
    r64, r32 = np.abs(lpips - v64) / v64 / UNIT, np.abs(lpips - v32) / v64 / UNIT
    print(f'\n[evaluate] SSIM abs vs fp32 vectors {e32.max():.3e}, vs fp64 {e64.max():.3e} (bar {SSIM_BAR}); LPIPS f16x3 rel vs fp64 {r64.max():.3f} units, '
          f'vs fp32 vectors {r32.max():.3f} units (bars {LPIPS_BAR} / {LPIPS_BAR + 1}, unit {UNIT:.3e})')
    assert e32.max() < SSIM_BAR and e64.max() < SSIM_BAR
    assert r64.max() <= LPIPS_BAR and r32.max() <= LPIPS_BAR + 1


def test_groups_and_report_match_the_reference(run):
    assert np.array_equal(run['groups'], GOLD['eval_groups'])
    want = ER.results_dict(GOLD, 'eval')
    assert [k for k, _ in run['results']] == list(want)
    got_lines, want_lines = run['report'].splitlines(), open(ER.GOLDEN_TSV).read().splitlines()
    assert got_lines[:2] == want_lines[:2] and len(got_lines) == len(want_lines)
    for a, b in zip(got_lines[2:], want_lines[2:]):
        a, b = a.split('\t'), b.split('\t')
        assert a[0] == b[0] and len(a) == len(b) == 5
        for x, y in zip(a[1:], b[1:]):
            assert len(x.split('.')[1]) == 4 and abs(round(float(x) * 1e4) - round(float(y) * 1e4)) <= 1, (a[0], x, y)
    # without the LPIPS files the CLI scores SSIM only: the ssim columns of the same report
    assert run['ssim_only'].splitlines() == ['\t'.join(ln.split('\t')[:3]) for ln in got_lines]


def test_loop_values_equal_direct_calls_on_the_ingest_outputs(run):
    """Buckets of 8 (40 x 48, items of three true sizes) and 4 (32 x 32) images; every value the loop kept is what SSIM / PerceptualLoss give on
    the tensors the ingest launch left, bit for bit, and sits at its item's dataset index."""
    assert [(t['idx'], t['image'].shape) for t in run['taps']] == [([0, 1, 2, 3, 8, 9, 10, 11], (8, 3, 40, 48)), ([4, 5, 6, 7], (4, 3, 32, 32))]
    for t in run['taps']:
        idx, image, pred = t['idx'], t['image'], t['pred']
        for name in ('ssim', 'lpips'):
            got, direct = t['values'][name], t['direct'][name]
            assert got.dtype == direct.dtype == np.float32 and got.shape == direct.shape == (len(idx),)
            assert got.tobytes() == direct.tobytes()
            assert np.array_equal(run['individual'][name][idx], got.astype(np.float64))
        for j, i in enumerate(idx):                          # the ingest's tensors are the reference dataset's items
            n = NAMES[i]
            assert image[j].tobytes() == GOLD[f'{n}_item_image'].tobytes()
            assert pred[j].tobytes() == GOLD[f'{n}_item_inpainted'].tobytes()


def test_evaluator_class_runs_the_device_loop(run):
    """InpaintingEvaluator.evaluate() at another batch size (5): per-image values are batch-independent, the statistics equal."""
    got, want = dict(run['evaluator_class']), {k: v for k, v in run['results'] if k[0] == 'ssim'}
    assert list(got) == list(want) and len(want) > 1
    for k in want:
        assert got[k]['mean'] == want[k]['mean'] and got[k]['std'] == want[k]['std']
