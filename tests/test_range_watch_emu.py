"""CPU tests of the fp16 range watch through the host SIMT emulator: every site that splits an activation under
LAMA_PREC_F16X3 must OR 1 into ``range_flag`` when it meets |x| > 65504, an inf or a NaN -- at the first and the last element, in a ragged tile,
in the last image, in either operand of a fused launch -- must leave the flag alone on in-range data and under LAMA_PREC_BF16X3, must never clear
it, and an unflagged result must be a correct one.  Contract, positions, values and the bar: tests/range_watch_util.py;
tests/test_range_watch_gpu.py reruns the same check functions on the MI355X.

Sites and the test that covers each:
  * ``lama_conv2d_fwd``, every family and geometry of CONV_CASES (route asserted): test_conv2d_range_watch_emulated; the output-side watch of the three
    pointwise GEMMs with ONE unit per workgroup: test_conv2d_single_unit_range_watch_emulated
  * the second operand x2 of the fused global launch: test_fused_second_operand_range_watch_emulated
  * the re-split of y for the fused conv1: test_fuse1_range_watch_emulated
  * the producer-side watch of a LAMA_DT_SPLIT16 output (stem, 3x3 stride 2): test_split16_writer_range_watch_emulated
  * ``lama_winograd_conv3x3_fwd`` (reflect and zero padding; a transformed operand that overflows on in-range inputs):
    test_winograd_range_watch_emulated, test_winograd_transformed_overflow_emulated
  * ``lama_multidilated_conv3x3_fwd``, ``lama_conv2d_rect_fwd``: test_multidilated_range_watch_emulated, test_rect_range_watch_emulated
  * LAMA_PREC_F16 tensors that already hold inf / NaN: test_f16_io_range_watch_emulated
  * ``lama_fourier_unit_fwd``, one bin at a time on a power-of-two and a mixed-radix plane: test_fourier_unit_range_watch_emulated
  * the five sites above are the issue's "not covered" list; ``LPIPS.auto_fallback`` / ``InceptionV3.auto_fallback`` and the production routes:
    tests/test_range_watch_gpu.py (test_lpips_auto_fallback, test_inception_auto_fallback, test_conv2d_range_watch_production_routes)
GPU only (too large for the emulator): the production-route shapes, the NaN of a stand-alone FFC layer on the Winograd route (512 channels at
32 x 32 is the smallest such layer), LPIPS.auto_fallback and InceptionV3.auto_fallback (five forwards of a whole network each), the FIRST fuse1
spot (y beyond the range at channel 0, pixel 0; the last one runs here) and the rows of EMU_SKIPPED.  Not built: the operands come from this
helper's own generators, not from ``fused_terms`` of the split-exact module (its terms produce exact integer grids, not N(0, 1) data).

Sensitivity, on a scratch copy through the emulator, one watch site broken at a time or together -- the test that turns red:
  * ``cb_range_report`` dropped in conv_split3.inc:596 -> test_conv2d_range_watch_emulated[1-k3s1c12o40_9x7-f16x3] (every LDS row), fused cg24,
    test_fourier_unit_range_watch_emulated[10x12-f16x3]; in conv_wreg_dev.inc:484 / 676 -> rows 15, 16, 30 .. and test_fuse1_range_watch_emulated[f16x3];
    conv_wreg_dev.inc:685 (the split16 writer) -> test_split16_writer_range_watch_emulated[down-*-f16x3]; conv_stem_dev.inc:241 -> row 50 and
    [stem-*-f16x3]; conv_head_dev.inc:212 -> row 51; convt_dev.inc:354 -> row 22; mdconv_dev.inc:157 -> test_multidilated_range_watch_emulated[g1..-f16x3]
  * the output-side report dropped in conv_ws_dev.inc:250 -> row 35 and test_conv2d_single_unit_range_watch_emulated[k1s1c192o96_4x8-f16x3];
    gemm_wk_dev.inc:286 -> row 44 and the wk single-unit case; ``if (u == 0) bad = false`` made unconditional (conv_ws_dev.inc:518) -> rows 39 .. 43
    (42: eight rounds on one workgroup) -- the single-unit w4 case stays green there, as it must: its only unit IS unit 0
  * inception.hip:137 (rect) -> test_rect_range_watch_emulated[k3s2_3to32_11x9-f16x3]; the fp16-I/O watch (same report) -> test_f16_io_range_watch_emulated
  * wino_dev.inc:396 with 0.5 rmax for 2 rmax (a late watch) -> test_winograd_transformed_overflow_emulated; with 4 rmax (an eager one) -> the
    'pairs' launch of test_winograd_range_watch_emulated[*-f16x3]

Emulator time: a row runs the FULL plan of tests/range_watch_util.py (13 f16x3 + 5 bf16x3 launches) if it is the first of its (family, geometry)
and small; the other rows run the THIN plan (clean, 7e4 at the first and the last position, the float below 65520 and 65520 at the last one; clean,
7e4 and NaN under bf16x3); the rows of EMU_SKIPPED run on the GPU only -- each has a twin of the same family here
(test_gpu_only_rows_keep_an_emulator_twin)."""
import pytest

from lama_amd import _lib as L
from tests import range_watch_util as R
from tests import test_kernels_emu as KE
from tests import test_split_exact_emu as E
from tests import test_conv_zero_pad_emu as Z
from tests.emu import emu_lib

PRECS = [L.PREC_F16X3, L.PREC_BF16X3]
PREC_IDS = ['f16x3', 'bf16x3']


def _macs(c):
    """Multiply-adds of one launch (B = 2): what the emulator's time goes with.  A transposed row has H x W input pixels with k^2 taps each."""
    s = 1 if c.get('transposed') else c['stride']
    return c['cin'] * c['k'] ** 2 * c['cout'] * (c['H'] // s) * (c['W'] // s) * 2


def _route_key(c):
    return (c['fam'], c.get('egeo'), c['k'], c['stride'], bool(c.get('transposed')))


# row index -> 'full' | 'thin' | 'gpu': the first small row of a (family, geometry, kernel size, stride) runs the full plan, rows above 35 M
# multiply-adds that have such a twin run on the GPU only, everything else runs the thin plan
EMU_PLAN = {}
_seen = set()
for _i, _c in sorted(enumerate(KE.CONV_CASES), key=lambda ic: _macs(ic[1])):
    _k = _route_key(_c)
    if _k not in _seen and _macs(_c) <= 30e6:
        EMU_PLAN[_i] = 'full'
        _seen.add(_k)
    elif _macs(_c) > 35e6 and any(_route_key(KE.CONV_CASES[j])[0] == _k[0] for j in EMU_PLAN if EMU_PLAN[j] != 'gpu'):
        EMU_PLAN[_i] = 'gpu'
    else:
        EMU_PLAN[_i] = 'thin'
        _seen.add(_k)
EMU_SKIPPED = [KE.CONV_CASES[i] for i in sorted(EMU_PLAN) if EMU_PLAN[i] == 'gpu']
EMU_ROWS = [(i, KE.CONV_CASES[i]) for i in sorted(EMU_PLAN) if EMU_PLAN[i] != 'gpu']


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('row', EMU_ROWS, ids=lambda r: f'{r[0]}-{E.CONV_ID(r[1])}')
def test_conv2d_range_watch_emulated(row, prec, monkeypatch):
    i, case = row
    E.force_env(case, monkeypatch)
    R.check_conv(emu_lib(), case, prec, 'cpu', thin=EMU_PLAN[i] == 'thin')


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('case', R.SINGLE_UNIT_CASES, ids=E.CONV_ID)
def test_conv2d_single_unit_range_watch_emulated(case, prec, monkeypatch):
    E.force_env(case, monkeypatch)
    R.check_conv(emu_lib(), case, prec, 'cpu')


def test_gpu_only_rows_keep_an_emulator_twin():
    """Every CONV_CASES row the emulator leaves to the GPU has a row of the same kernel family that runs here, and every family of the table runs
    the full plan at least once."""
    here = {c['fam'] for _, c in EMU_ROWS}
    for c in EMU_SKIPPED:
        assert c['fam'] in here, E.CONV_ID(c)
    assert {KE.CONV_CASES[i]['fam'] for i, p in EMU_PLAN.items() if p == 'full'} | {c['fam'] for c in R.SINGLE_UNIT_CASES} == {c['fam'] for c in KE.CONV_CASES}
    from tests import test_split_exact_gpu as G
    for (B, cin, cout, k, H, W) in G.PROD_SHAPES:          # the production-route shapes of the GPU module
        assert any(c['k'] == k and c['cin'] == cin and c['stride'] == 1 and not c.get('transposed') and (c['cout'] <= 4) == (cout <= 4)
                   for _, c in EMU_ROWS), (cin, cout, k)


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('case', E.FUSED_CASES, ids=E.FUSED_ID)
def test_fused_second_operand_range_watch_emulated(case, prec):
    R.check_fused_second_operand(emu_lib(), case, prec, 'cpu')


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
def test_fuse1_range_watch_emulated(prec):
    R.check_fuse1(emu_lib(), 1, prec, 'cpu')               # y beyond the range at the last channel and pixel; the first: GPU module


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('spot', [0, 1], ids=R.SPLIT16_SPOTS)
@pytest.mark.parametrize('name', list(R.SPLIT16_CASES))
def test_split16_writer_range_watch_emulated(name, spot, prec):
    R.check_split16_writer(emu_lib(), name, spot, prec, 'cpu')


WINO_FULL = KE.WINO_CASES[4]                               # c32o128 9 x 30: the smallest plane, any-size geometry with reflected columns and an odd height


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('case', [c for c in KE.WINO_CASES if c['cin'] * c['cout'] * c['H'] * c['W'] * c['B'] <= 32 * 128 * 16 * 64], ids=KE.WINO_ID)
def test_winograd_range_watch_emulated(case, prec, monkeypatch):
    E.force_env(case, monkeypatch)
    R.check_winograd(emu_lib(), case, prec, 'cpu', thin=case is not WINO_FULL)


def test_winograd_zero_pad_range_watch_emulated():
    R.check_winograd(emu_lib(), WINO_FULL, L.PREC_F16X3, 'cpu', pad_mode=L.PAD_ZERO)


@pytest.mark.parametrize('case', [KE.WINO_CASES[0], WINO_FULL], ids=KE.WINO_ID)
def test_winograd_transformed_overflow_emulated(case):
    R.check_winograd_transformed_overflow(emu_lib(), case, 'cpu')


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('case', E.MD_CASES, ids=E.MD_ID)
def test_multidilated_range_watch_emulated(case, prec):
    R.check_multidilated(emu_lib(), case, prec, 'cpu', thin=case['G'] == 2)      # g2 (160 rows over 2 x 5 x 20): thin here, full on the GPU


RECT_FULL = ('k3s2_3to32_11x9', 'k1x7_128_5x6', 'k7x1_160to192_6x5', 'k1_64to80_5x7')      # K tail, 1x7, 7x1, M tail: the full plan; the rest thin


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('case', list(E.FE.RECT_CASES))
def test_rect_range_watch_emulated(case, prec):
    R.check_rect(emu_lib(), case, prec, 'cpu', thin=case not in RECT_FULL)


@pytest.mark.parametrize('case', Z.ZP_F16_CASES, ids=Z.ZP_ID)
def test_f16_io_range_watch_emulated(case):
    R.check_f16_io(emu_lib(), case, 'cpu')


def test_fourier_unit_planes_take_two_fft_families():
    R.check_fft_families_differ(emu_lib())


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('hw', R.FU_PLANES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_fourier_unit_range_watch_emulated(hw, prec):
    R.check_fourier_unit(emu_lib(), hw, prec, 'cpu')


def test_plan_and_judge_known_answers():
    """The helper itself: the positions, the launch budget, and that ``judge`` refuses what the contract forbids."""
    import torch
    pos = dict(R.positions((2, 8, 5, 7)))
    assert pos['first'] == (0, 0, 0, 0) and pos['last'] == (1, 7, 4, 6) and pos['c-1,w-1'] == (0, 7, 0, 6) and pos['b-1,h-1'] == (1, 0, 4, 0)
    full, bf = R.plan((2, 8, 5, 7), L.PREC_F16X3), R.plan((2, 8, 5, 7), L.PREC_BF16X3)
    assert len(full) == 12 and len(bf) == 5 and len(R.plan((2, 8, 5, 7), L.PREC_F16X3, thin=True)) == 5
    assert sorted(v for n, _, v in full if n == 'last' and v == v) == sorted([7.0e4, -1.0e5, R.INF, 65504.0, R.BELOW_TIE, R.TIE])
    assert R.BELOW_TIE < 65520.0 and torch.tensor(R.BELOW_TIE).half().item() == 65504.0 and torch.tensor(R.TIE).half().item() == R.INF
    y = torch.zeros(1, 1, 1, 1, dtype=torch.float64)
    ref = lambda: (y, y + 1.0)          # noqa: E731
    R.judge('t', 't', 't', L.PREC_F16X3, 'last', R.TIE, 1, y + 9.0, True, ref, 'cpu')            # flagged at the tie: the output is not looked at
    R.judge('t', 't', 't', L.PREC_F16X3, 'last', R.TIE, 0, y, True, ref, 'cpu')
    for kw in (dict(v=7.0e4, flag=0, y=y), dict(v=R.NAN, flag=0, y=y), dict(v=65504.0, flag=1, y=y), dict(v=None, flag=1, y=y),
               dict(v=R.TIE, flag=0, y=y + 1.0), dict(v=65504.0, flag=0, y=y + 1.0), dict(v=None, flag=0, y=y, ok=False),
               dict(v=None, flag=0, y=y, preset=1), dict(v=7.0e4, flag=1, y=y, prec=L.PREC_BF16X3)):
        with pytest.raises(AssertionError):
            R.judge('t', 't', 't', kw.get('prec', L.PREC_F16X3), 'last', kw['v'], kw['flag'], kw['y'], kw.get('ok', True), ref, 'cpu', preset=kw.get('preset', 0))
