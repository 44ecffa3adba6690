"""GPU: LPIPS (VGG-16, net-lin) of lama_amd.evaluation against the reference-generated vectors (tests/golden/lpips.npz) and the fp64 restatement
(tests/lpips_ref.py), on the seeded synthetic backbone of tests/lpips_util.py with the real linear heads.

Bars.  The unit is `unit` of lpips.npz: the largest fp32-vs-fp64 relative distance of the reference itself over the recorded cases (1.2e-7).
The relative error of the per-image value against fp64 is held to 4 units for f32 (another accumulation order) and 16 units for f16x3 (the split
keeps 22 of 24 mantissa bits: 4x, times the same 4x for order).  Against the fp32 vectors one more unit is allowed (the vectors are themselves
up to one unit from fp64).  The small-valued cases (c: inpainted rectangle, h: near-identical) are ALSO held to an absolute error of the same
number of units times the value of independent random images of their size (case f); case h, whose reference fp32 value is 2.4e-6 from fp64, is
measured in units of that own distance (`h_rel32`), not of the suite's.  Per-level terms: the absolute budget of the value.

Measured on MI355X, relative distance of the value to fp64 in units (bar 4 / 16), also in profiles/lpips.txt:
    f32:   a 0.28, b 0.44, c 0.90, f 0.13, g 1.00, h 1.18 (of h_rel32), 96x80 0.89, 250x187 0.79
    f16x3: a 0.28, b 0.44, c 0.90, f 0.13, g 1.55, h 4.00 (of h_rel32; level 5 carries 3.2 of it), 96x80 0.23, 250x187 0.23
    largest per-level absolute error / value: 0.67 units (f32, case c, level 5) and 0.92 units (f16x3, case g, level 4); identical pair 0.0 exactly.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lpips_ref as R  # noqa: E402
import lpips_util as U  # noqa: E402
from lama_amd import evaluation as EV  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(U.GOLDEN)
UNIT = float(GOLD['unit'])
BAR = {'f32': 4, 'f16x3': 16}
HEADS = [torch.from_numpy(GOLD[f'lin{k}']) for k in range(5)]


@pytest.fixture(scope='module')
def backbone():
    return U.backbone_state_dict()


@pytest.fixture(scope='module')
def losses(backbone):
    return {p: EV.PerceptualLoss(model_path=U.heads_state_dict(GOLD), backbone=backbone).cuda().set_precision(p) for p in BAR}


@pytest.fixture(scope='module')
def golden_ref(backbone):
    """tag -> (value [N], levels [5, N]) of the fp64 restatement, computed once."""
    out = {}
    for tag in U.CASES:
        pred, target, normalize = U.case_inputs(GOLD, tag)
        out[tag] = R.lpips_ref(pred, target, backbone, HEADS, normalize)
    return out


@pytest.fixture(scope='module')
def big_cases(backbone):
    """3 x 3 x 96 x 80 (512-channel levels of 12 x 10 and 6 x 5) and 1 x 3 x 250 x 187 (odd planes at every level, more than one workgroup per image
    in every reduction but the last): inputs and the fp64 restatement, computed once."""
    out = {}
    for name, shape in (('96x80', (3, 3, 96, 80)), ('250x187', (1, 3, 250, 187))):
        g = torch.Generator().manual_seed(shape[2])
        pred, target = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
        out[name] = (pred, target) + R.lpips_ref(pred, target, backbone, HEADS, True)
    return out


def _units(val, ref, unit=UNIT):
    return float(((val.flatten().double().cpu() - ref).abs() / ref).max()) / unit


@pytest.mark.parametrize('tag', U.CASES)
@pytest.mark.parametrize('prec', list(BAR))
def test_golden_cases(prec, tag, losses, golden_ref):
    m, bar = losses[prec], BAR[prec]
    pred, target, normalize = U.case_inputs(GOLD, tag)
    val, levels = m.forward_per_layer(pred.cuda(), target.cuda(), normalize=normalize)
    assert val.shape == (pred.shape[0], 1, 1, 1) and val.dtype == torch.float32 and val.is_cuda
    assert torch.equal(val, m(pred.cuda(), target.cuda(), normalize=normalize))
    ref, ref_levels = golden_ref[tag]
    v64, v32 = torch.from_numpy(GOLD[f'{tag}_value64']), torch.from_numpy(GOLD[f'{tag}_value']).double()
    if tag == 'd':
        assert val.flatten().tolist() == [0.0] * pred.shape[0]
        return
    unit = float(GOLD['h_rel32']) if tag == 'h' else UNIT
    got = val.flatten().double().cpu()
    lv = torch.stack([l.flatten() for l in levels]).double().cpu()
    lvl_err = (lv - ref_levels).abs().max(1).values / ref.max()
    print(f'\n[lpips {prec} {tag}] rel vs fp64 restatement {_units(val, ref, unit):.3f} units, vs reference fp64 {_units(val, v64, unit):.3f} units, '
          f'vs fp32 vectors {float(((got - v32).abs() / v64).max()) / unit:.3f} units; per-level abs / value in units: '
          f'{[round(float(e) / unit, 3) for e in lvl_err]} (unit {unit:.3e})')
    assert _units(val, ref, unit) <= bar
    assert _units(val, v64, unit) <= bar
    assert float(((got - v32).abs() / v64).max()) <= (bar + 1) * unit
    rnd = U.RANDOM_OF_SIZE.get(tag)
    if rnd:
        assert float((got - ref).abs().max()) <= bar * UNIT * float(GOLD[f'{rnd}_value64'].max())
    assert float(lvl_err.max()) <= bar * unit, f'level {int(lvl_err.argmax())}'
    assert float(((lv - torch.from_numpy(GOLD[f"{tag}_levels"]).double()).abs().max(1).values / ref.max()).max()) <= (bar + 1) * unit


@pytest.mark.parametrize('name', ['96x80', '250x187'])
@pytest.mark.parametrize('prec', list(BAR))
def test_larger_shapes_against_the_restatement(prec, name, losses, big_cases):
    m, bar = losses[prec], BAR[prec]
    pred, target, ref, ref_levels = big_cases[name]
    val, levels = m.forward_per_layer(pred.cuda(), target.cuda())
    lv = torch.stack([l.flatten() for l in levels]).double().cpu()
    lvl_err = (lv - ref_levels).abs().max(1).values / ref.max()
    print(f'\n[lpips {prec} {name}] rel vs fp64 restatement {_units(val, ref):.3f} units; per-level abs / value in units '
          f'{[round(float(e) / UNIT, 3) for e in lvl_err]}; convs {m.model.conv_paths(pred.shape, "cuda")}')
    assert _units(val, ref) <= bar
    assert float(lvl_err.max()) <= bar * UNIT, f'level {int(lvl_err.argmax())}'


@pytest.mark.parametrize('prec', list(BAR))
def test_determinism_caching_and_shape_change(prec, backbone, golden_ref):
    """A fresh module: the first call (buffers allocated, weights packed) and the second (cached) agree bitwise, as do two further runs; another
    shape after that still meets the bar, and so does the first shape when it comes back."""
    m = EV.PerceptualLoss(model_path=U.heads_state_dict(GOLD), backbone=backbone).cuda().set_precision(prec)
    pb, tb, _ = U.case_inputs(GOLD, 'b')
    first = m(pb.cuda(), tb.cuda()).clone()
    second = m(pb.cuda(), tb.cuda()).clone()
    assert torch.equal(first, second) and torch.equal(second, m(pb.cuda(), tb.cuda()))
    pa, ta, _ = U.case_inputs(GOLD, 'a')
    assert _units(m(pa.cuda(), ta.cuda()), golden_ref['a'][0]) <= BAR[prec]
    assert torch.equal(first, m(pb.cuda(), tb.cuda()))
    assert m(tb.cuda(), tb.clone().cuda()).flatten().tolist() == [0.0, 0.0]


def test_cpu_tensor_raises(losses):
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(EV.LamaError):
        losses['f32'](x, x)
    with pytest.raises(EV.LamaError):
        losses['f32'](x.cuda(), x)


def test_lpips_score_on_device(backbone, golden_ref):
    s = EV.LPIPSScore(model_path=U.heads_state_dict(GOLD), backbone=backbone).cuda()
    for tag in ('a', 'g'):
        pred, target, normalize = U.case_inputs(GOLD, tag)
        if normalize:
            out = s(pred.cuda(), target.cuda())
            assert out.shape == (pred.shape[0],) and _units(out, golden_ref[tag][0]) <= BAR['f16x3']
    total, groups = s.get_value()
    assert groups is None and abs(total['mean'] - float(golden_ref['a'][0].mean())) <= BAR['f16x3'] * UNIT
