"""CPU: FID (Inception-v3 pool3 features).  The new kernels of csrc/inception.hip on the host emulator against fp64 / exact references, the
plain-torch restatement (tests/inception_util.py) against the reference-generated vectors, and the host logic of lama_amd.evaluation /
lama_amd.evaluate (state-dict keys, refusals, the Frechet distance, FIDScore, the integrals, the device loop's ordering, the report).
The check functions take the library as an argument: tests/test_fid_gpu.py runs the same ones on the hardware."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import inception_util as U  # noqa: E402
from emu import emu_lib  # noqa: E402
from test_kernels_emu import CONV_TOL  # noqa: E402
from lama_amd import _lib as L  # noqa: E402
from lama_amd import evaluate as EVL  # noqa: E402
from lama_amd import evaluation as EV  # noqa: E402
from lama_amd.ffc import _Exec  # noqa: E402

GOLD = np.load(U.GOLDEN)
UNIT = float(GOLD['unit'])
F32_EPS = 2.0 ** -24
PRECS = [L.PREC_F16X3, L.PREC_BF16X3]


def _dev(lib):
    return 'cpu' if lib.host_emulated else 'cuda'


# ---- lama_conv2d_rect_fwd -----------------------------------------------------------------------------------------------------------------
# (B, cin, cout, H, W, (kh, kw), stride, (ph, pw))
RECT_CASES = {
    'k3s2_3to32_11x9': (2, 3, 32, 11, 9, (3, 3), 2, (0, 0)),            # K = 27: the K tail
    'k3s2_288to384_10x8': (1, 288, 384, 10, 8, (3, 3), 2, (0, 0)),      # even plane: the last row and column are not used
    'k1x7_128_5x6': (1, 128, 128, 5, 6, (1, 7), 1, (0, 3)),             # plane narrower than the kernel
    'k1x7_128_17x17': (1, 128, 128, 17, 17, (1, 7), 1, (0, 3)),
    'k7x1_160to192_6x5': (1, 160, 192, 6, 5, (7, 1), 1, (3, 0)),
    'k5_48to64_9x7': (1, 48, 64, 9, 7, (5, 5), 1, (2, 2)),
    'k1x3_384_8x8': (2, 384, 384, 8, 8, (1, 3), 1, (0, 1)),
    'k3x1_384_8x8': (2, 384, 384, 8, 8, (3, 1), 1, (1, 0)),
    'k3_448to384_8x8': (1, 448, 384, 8, 8, (3, 3), 1, (1, 1)),
    'k1_64to80_5x7': (1, 64, 80, 5, 7, (1, 1), 1, (0, 0)),              # cout not a multiple of 32
    'k1_2048to192_8x8': (1, 2048, 192, 8, 8, (1, 1), 1, (0, 0)),
}


def _rect_out(H, W, k, s, p):
    return (H + 2 * p[0] - k[0]) // s + 1, (W + 2 * p[1] - k[1]) // s + 1


def _ring(Ho, Wo, H, W, k, s, p, dev):
    """Mask of the outputs whose window leaves the plane."""
    oy, ox = torch.arange(Ho, device=dev)[:, None] * s - p[0], torch.arange(Wo, device=dev)[None, :] * s - p[1]
    return (oy < 0) | (oy + k[0] > H) | (ox < 0) | (ox + k[1] > W)


def check_rect_conv(lib, case, prec):
    """Against F.conv2d in fp64 at CONV_TOL[prec] of tests/test_kernels_emu.py (|y - ref| <= atol + rtol |ref|), ring and interior looked at
    separately."""
    B, cin, cout, H, W, k, s, p = RECT_CASES[case]
    dev = _dev(lib)
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    x = torch.randn(B, cin, H, W, generator=g).to(dev)
    w = (torch.randn(cout, cin, *k, generator=g) / (cin * k[0] * k[1]) ** 0.5).to(dev)
    scale, bias = (torch.rand(cout, generator=g) + 0.5).to(dev), torch.randn(cout, generator=g).to(dev)
    Ho, Wo = _rect_out(H, W, k, s, p)
    y = torch.full((B, cout, Ho, Wo), float('nan'), device=dev)
    wp = lib.pack_conv_rect_weight(w, scale, prec)
    lib.conv2d_rect(L.view(x), wp, L.view(y), B, k[0], k[1], s, p[0], p[1], bias=bias, act=L.ACT_RELU, precision=prec, stream=L.LamaLib.stream_of(x))
    ref = F.relu(F.conv2d(x.double().cpu(), (w.double() * scale.double().view(-1, 1, 1, 1)).cpu(), bias.double().cpu(), stride=s, padding=p))
    tol = CONV_TOL[prec]
    share = (y.double().cpu() - ref).abs() / (tol['atol'] + tol['rtol'] * ref.abs())       # 1 = on the bar
    ring = _ring(Ho, Wo, H, W, k, s, p, 'cpu')
    for name, sel in (('ring', ring), ('interior', ~ring)):
        if sel.any():
            e = float(share[:, :, sel].max())
            print(f'{case} prec {prec} {name}: worst share of the bar {e:.3f}')
            assert e <= 1.0, (case, prec, name, e)


def check_rect_tap_count(lib, case, prec):
    """x = 1, w = 1: every output is exactly cin x (the taps inside the plane) -- small integers, exact in every term of the split."""
    B, cin, cout, H, W, k, s, p = RECT_CASES[case]
    dev = _dev(lib)
    x, w = torch.ones(B, cin, H, W, device=dev), torch.ones(cout, cin, *k, device=dev)
    Ho, Wo = _rect_out(H, W, k, s, p)
    y = torch.full((B, cout, Ho, Wo), float('nan'), device=dev)
    lib.conv2d_rect(L.view(x), lib.pack_conv_rect_weight(w, None, prec), L.view(y), B, k[0], k[1], s, p[0], p[1], precision=prec,
                    stream=L.LamaLib.stream_of(x))
    taps = F.conv2d(torch.ones(1, 1, H, W), torch.ones(1, 1, *k), stride=s, padding=p)[0, 0]
    want = (cin * taps).expand(B, cout, Ho, Wo)
    ring = _ring(Ho, Wo, H, W, k, s, p, 'cpu')
    got = y.cpu()
    for sel in (ring, ~ring):
        assert torch.equal(got[:, :, sel], want[:, :, sel]), case


def check_rect_slice(lib, prec):
    """Stored into channels [64, 160) of a 288-channel NaN-filled buffer (InceptionA's 3x3dbl branch): everything outside stays bit-identical."""
    dev = _dev(lib)
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 7, 6
    xw = torch.randn(B, 160, H, W, generator=g).to(dev)                 # the input is a slice too: channels [32, 128) of a 160-channel buffer
    w = (torch.randn(96, 96, 3, 3, generator=g) / 30).to(dev)
    bias = torch.randn(96, generator=g).to(dev)
    buf = torch.full((B, 288, H, W), float('nan'), device=dev)
    before = buf.clone()
    lib.conv2d_rect(L.view(xw, 32, 96), lib.pack_conv_rect_weight(w, None, prec), L.view(buf, 64, 96), B, 3, 3, 1, 1, 1, bias=bias, act=L.ACT_RELU,
                    precision=prec, stream=L.LamaLib.stream_of(xw))
    ref = F.relu(F.conv2d(xw[:, 32:128].double().cpu(), w.double().cpu(), bias.double().cpu(), padding=1))
    got = buf.cpu()
    tol = CONV_TOL[prec]
    assert bool(((got[:, 64:160].double() - ref).abs() <= tol['atol'] + tol['rtol'] * ref.abs()).all())
    outside = torch.ones(288, dtype=torch.bool)
    outside[64:160] = False
    assert torch.equal(got[:, outside].view(torch.int32), before.cpu()[:, outside].view(torch.int32))


def check_rect_refusals(lib):
    dev = _dev(lib)
    x, w = torch.zeros(1, 8, 9, 9, device=dev), torch.zeros(16, 8, 3, 3, device=dev)
    wp = lib.pack_conv_rect_weight(w, None, L.PREC_F16X3)
    for kw, shape, code in ((dict(kh=3, kw=3, stride=1), (1, 16, 8, 7), L.ERR_BAD_ARG),          # y of the wrong size
                            (dict(kh=8, kw=3, stride=1), (1, 16, 2, 7), L.ERR_UNSUPPORTED),
                            (dict(kh=3, kw=3, stride=3), (1, 16, 3, 3), L.ERR_UNSUPPORTED)):
        with pytest.raises(L.LamaError) as e:
            lib.conv2d_rect(L.view(x), wp, L.view(torch.zeros(shape, device=dev)), 1, kw['kh'], kw['kw'], kw['stride'])
        assert e.value.code == code, (kw, e.value.code)
    with pytest.raises(L.LamaError) as e:                               # PREC_F32 is not served by this entry
        lib.pack_conv_rect_weight(w, None, L.PREC_F32)
    assert e.value.code == L.ERR_UNSUPPORTED


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', list(RECT_CASES))
def test_rect_conv(case, prec):
    check_rect_conv(emu_lib(), case, prec)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', ['k3s2_3to32_11x9', 'k1x7_128_5x6', 'k7x1_160to192_6x5', 'k5_48to64_9x7', 'k1_64to80_5x7', 'k3s2_288to384_10x8'])
def test_rect_conv_tap_count(case, prec):
    check_rect_tap_count(emu_lib(), case, prec)


@pytest.mark.parametrize('prec', PRECS)
def test_rect_conv_channel_slice(prec):
    check_rect_slice(emu_lib(), prec)


def test_rect_conv_refusals():
    check_rect_refusals(emu_lib())


# ---- lama_pool3x3_fwd, lama_global_avgpool_fwd, lama_fid_input_fwd -------------------------------------------------------------------------
POOL_CASES = [(1, 1, 1, 1), (3, 3, 1, 1), (5, 4, 1, 1), (7, 7, 2, 0), (8, 6, 2, 0)]       # (H, W, stride, pad)


def check_pool(lib, H, W, s, p, sliced=False):
    """MAX bit-equal to F.max_pool2d; the average within 10 x 2^-24 x (the window mean of |x|, fp64) of the fp64 value: at most 8 fp32 additions and
    one division, each rounding relative to a partial sum that is bounded by the window's sum of |x|."""
    dev = _dev(lib)
    g = torch.Generator().manual_seed(H * 10 + W)
    B, C = 2, 5
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    Ho, Wo = (H + 2 * p - 3) // s + 1, (W + 2 * p - 3) // s + 1
    for mode in (L.POOL_MAX, L.POOL_AVG_EXCLUDE_PAD):
        buf = torch.full((B, C + 4 if sliced else C, Ho, Wo), float('nan'), device=dev)
        yv = L.view(buf, 3, C) if sliced else L.view(buf)
        lib.pool3x3(L.view(x), yv, B, mode, s, p, stream=L.LamaLib.stream_of(x))
        got = (buf[:, 3:3 + C] if sliced else buf).cpu()
        if sliced:
            assert bool(torch.isnan(buf[:, :3]).all()) and bool(torch.isnan(buf[:, 3 + C:]).all())
        if mode == L.POOL_MAX:
            assert torch.equal(got, F.max_pool2d(x.cpu(), 3, s, p))
        else:
            xd = x.double().cpu()
            ref = F.avg_pool2d(xd, 3, s, p, count_include_pad=False)
            bar = 10 * F32_EPS * F.avg_pool2d(xd.abs(), 3, s, p, count_include_pad=False)
            assert bool(((got.double() - ref).abs() <= bar).all())


def check_global_avgpool(lib, h, w):
    dev = _dev(lib)
    g = torch.Generator().manual_seed(h * 10 + w)
    x = torch.randn(3, 37, h, w, generator=g).to(dev)
    y = torch.full((3, 37), float('nan'), device=dev)
    lib.global_avgpool(L.view(x), y, 3, stream=L.LamaLib.stream_of(x))
    ref = x.double().cpu().mean(dim=(2, 3)).float()                    # the fp64 mean, rounded once
    assert torch.equal(y.cpu().view(torch.int32), ref.view(torch.int32))


def check_fid_input(lib, H, W):
    """Against F.interpolate(fp32).double() (the same fp32 coordinates and weights), 2x - 1 taken in fp64: six fp32 roundings of the four-tap
    window's |x| <= 1 (the products and sums of the two rows and their blend; the two sides may round differently), doubled by the 2x, then one
    rounding of the result, |2x - 1| <= 1."""
    dev = _dev(lib)
    g = torch.Generator().manual_seed(H + W)
    B = 2
    a, b = torch.rand(B, 3, H, W, generator=g).to(dev), torch.rand(B, 3, H, W, generator=g).to(dev)
    y = torch.full((2 * B, 3, 299, 299), float('nan'), device=dev)
    lib.fid_input(L.view(a), L.view(b), L.view(y), B, resize=True, stream=L.LamaLib.stream_of(a))
    x = torch.cat([a, b]).cpu()
    ref = 2 * F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False).double() - 1
    if (H, W) == (299, 299):
        assert torch.equal(y.cpu(), (2 * torch.cat([a, b]).cpu() - 1))  # the identity: exact
        return
    bar = (2 * 6 + 1) * F32_EPS                                        # |x| <= 1 over every window
    err = float((y.double().cpu() - ref).abs().max())
    print(f'fid_input {H}x{W}: err {err:.3e} bar {bar:.3e}')
    assert err <= bar
    y2 = torch.full((2 * B, 3, H, W), float('nan'), device=dev)
    lib.fid_input(L.view(a), L.view(b), L.view(y2), B, resize=False, stream=L.LamaLib.stream_of(a))
    assert torch.equal(y2.cpu(), 2 * torch.cat([a, b]).cpu() - 1)


@pytest.mark.parametrize('H,W,s,p', POOL_CASES)
def test_pool3x3(H, W, s, p):
    check_pool(emu_lib(), H, W, s, p)


def test_pool3x3_slice_view():
    check_pool(emu_lib(), 7, 7, 2, 0, sliced=True)
    check_pool(emu_lib(), 5, 4, 1, 1, sliced=True)


def test_pool3x3_refusals():
    lib = emu_lib()
    x = torch.zeros(1, 2, 5, 5)
    for y, kw, code in ((torch.zeros(1, 2, 4, 4), dict(mode=L.POOL_MAX, stride=1, pad=1), L.ERR_BAD_ARG),
                        (torch.zeros(1, 2, 5, 5), dict(mode=2, stride=1, pad=1), L.ERR_UNSUPPORTED),
                        (torch.zeros(1, 2, 1, 1), dict(mode=L.POOL_MAX, stride=3, pad=0), L.ERR_UNSUPPORTED)):
        with pytest.raises(L.LamaError) as e:
            lib.pool3x3(L.view(x), L.view(y), 1, kw['mode'], kw['stride'], kw['pad'])
        assert e.value.code == code


@pytest.mark.parametrize('h,w', [(8, 8), (3, 5), (1, 1)])
def test_global_avgpool(h, w):
    check_global_avgpool(emu_lib(), h, w)


@pytest.mark.parametrize('H,W', [(64, 48), (320, 299), (299, 299)])
def test_fid_input(H, W):
    check_fid_input(emu_lib(), H, W)


# ---- the whole network ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def weights():
    return U.synthetic_state_dict(GOLD)


def network_distance(model, tag):
    """max |a - a64| / max |a64| of the [2N, 2048] activations of a recorded case, in units of the fixture's `unit`."""
    pred, target = U.case_inputs(GOLD, tag)
    dev = next(model.parameters()).device
    ap, at = model.pair(pred.to(dev), target.to(dev))
    got = torch.cat([ap, at]).flatten(1).double().cpu().numpy()
    a64 = GOLD[f'{tag}_act64']
    return np.abs(got - a64).max() / np.abs(a64).max() / UNIT, got


def test_whole_network_on_the_emulator(weights):
    """Case d (75 x 75, resize_input=False) through all 94 convolutions on the emulator in f16x3 against the reference's fp64 activations.
    Bar: 8 x unit on max-abs over max |a64| (unit = the reference's own fp32-vs-fp64 distance; the margin is for the three-term split keeping
    about 22 of fp32's 24 mantissa bits and for another summation order).  Measured: 0.0081 units (3.7e-6 relative); about 100 s on the emulator."""
    model = EV.InceptionV3([3], resize_input=False, weights=weights).set_exec(_Exec(emu_lib()))
    units, _ = network_distance(model, 'd')
    print('whole network, case d, f16x3:', units, 'units of', UNIT)
    assert units <= 8.0
    assert model.conv_paths((2, 3, 75, 75), 'cpu') == ['rect'] * 94


# ---- host ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', U.CASES)
def test_restatement_reproduces_the_reference(tag, weights):
    pred, target = U.case_inputs(GOLD, tag)
    got = U.restated_features(weights, torch.cat([pred, target]), bool(GOLD[f'{tag}_resize'])).numpy()
    a64 = GOLD[f'{tag}_act64']
    assert np.abs(got - a64).max() <= 1e-12 * np.abs(a64).max()
    assert np.abs(GOLD[f'{tag}_act32'] - a64).max() <= UNIT * np.abs(a64).max()


def test_state_dict_loading_in_both_key_styles(weights, tmp_path):
    m = EV.InceptionV3(weights=weights)
    own = m.state_dict()
    assert len([k for k in own if k.endswith('conv.weight')]) == 94
    assert torch.equal(own['blocks.0.0.conv.weight'], weights['Conv2d_1a_3x3.conv.weight'])
    assert torch.equal(own['blocks.2.5.branch7x7dbl_3.bn.running_var'], weights['Mixed_6c.branch7x7dbl_3.bn.running_var'])
    assert torch.equal(own['blocks.3.2.branch_pool.conv.weight'], weights['Mixed_7c.branch_pool.conv.weight'])
    assert not any(k.startswith('fc') for k in own) and 'fc.weight' in weights                # fc.* is ignored
    m2 = EV.InceptionV3(weights={k: v.clone() for k, v in own.items()})                        # the module's own keys
    assert all(torch.equal(v, own[k]) for k, v in m2.state_dict().items())
    torch.save(weights, tmp_path / 'inception.pth')
    m3 = EV.InceptionV3(weights=str(tmp_path / 'inception.pth'))
    assert torch.equal(m3.state_dict()['blocks.1.1.bn.bias'], weights['Conv2d_4a_3x3.bn.bias'])
    assert EV.InceptionV3.BLOCK_INDEX_BY_DIM == {64: 0, 192: 1, 768: 2, 2048: 3}


def test_refusals(weights, tmp_path):
    with pytest.raises(EV.LamaError, match='nothing is downloaded'):
        EV.InceptionV3(weights=None)
    with pytest.raises(EV.LamaError, match='not found'):
        EV.InceptionV3(weights=str(tmp_path / 'nope.pth'))
    with pytest.raises(NotImplementedError):
        EV.InceptionV3(use_fid_inception=False, weights=weights)
    with pytest.raises(EV.LamaError, match='Mixed_6a|blocks.2.3'):
        EV.InceptionV3(weights={k: v for k, v in weights.items() if not k.startswith('Mixed_6a.branch3x3.')})
    bad = dict(weights)
    bad['Mixed_5b.branch1x1.conv.weight'] = torch.zeros(64, 191, 1, 1)
    with pytest.raises(EV.LamaError, match='blocks.2.0.branch1x1.conv.weight'):
        EV.InceptionV3(weights=bad)
    m = EV.InceptionV3(weights=weights)                                 # the default exec: the real library, device tensors only
    with pytest.raises(EV.LamaError, match='GPU'):
        m(torch.rand(2, 3, 80, 80))
    with pytest.raises(NotImplementedError):
        m.train()


@pytest.mark.parametrize('k', range(4))
def test_frechet_distance_against_the_reference(k):
    """The reference's scipy.linalg.sqrtm form, recorded.  Full-rank pairs (k = 0, 1): 1e-10 relative; rank-deficient ones (k = 2, 3: N < D): 1e-5 =
    100 x the 1.1e-7 measured up to D = 2048, where the reference's own result carries imaginary parts of 1e-7.  Measured on the fixture's pairs:
    1.2e-14, 1.9e-14, 2.0e-8, 5.6e-8.  (The full-rank pairs are well conditioned -- independent features, N > D.  On full-rank covariances of
    condition 6e7 the two-eigh form was 1.1e-9 from sqrtm: the small eigenvalues of S1 carry eps x lambda_max absolute.)"""
    got = EV.calculate_frechet_distance(GOLD[f'fd{k}_pred'], GOLD[f'fd{k}_target'])
    want = float(GOLD[f'fd{k}_value'])
    rel = abs(got - want) / abs(want)
    print('frechet pair', k, got, want, rel)
    assert rel <= (1e-10 if k < 2 else 1e-5)


def test_fid_score_get_value_and_reset(weights):
    s = EV.FIDScore(weights=weights)
    assert isinstance(s.model, EV.InceptionV3) and not s.model.training
    ap, at, groups = GOLD['score_pred'], GOLD['score_target'], GOLD['score_groups']
    for lo in (0, 4, 8):
        s.activations_pred.append(torch.from_numpy(ap[lo:lo + 4]))
        s.activations_target.append(torch.from_numpy(at[lo:lo + 4]))
    total, per_group = s.get_value(groups=groups)
    assert abs(total['mean'] - float(GOLD['score_total'])) <= 1e-5 * float(GOLD['score_total'])          # 12 items of 48 dims: rank-deficient
    assert sorted(per_group) == GOLD['score_labels'].tolist()
    for label, want in zip(GOLD['score_labels'], GOLD['score_group_values']):
        got = per_group[label]['mean']
        assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-5 * abs(want)
    assert np.isnan(per_group[9]['mean'])                               # the group of one item
    assert s.activations_pred == [] and s.activations_target == []      # get_value resets, as the reference's does
    total2, none = s.get_value(states=[(torch.from_numpy(ap[:6]), torch.from_numpy(at[:6])), (torch.from_numpy(ap[6:]), torch.from_numpy(at[6:]))])
    assert none is None and total2['mean'] == total['mean']


def test_integral_functions():
    ssim, lpips, fid = GOLD['integral_inputs']
    metrics = {('ssim', 'total'): dict(mean=ssim), ('lpips', 'total'): dict(mean=lpips), ('fid', 'total'): dict(mean=fid)}
    assert EV.ssim_fid100_f1(metrics) == GOLD['integral_values'][0]
    assert EV.lpips_fid100_f1(metrics) == GOLD['integral_values'][1]
    metrics[('fid', 'total')] = dict(mean=250.0)                        # beyond the scale: max(0, .) = 0
    assert EV.ssim_fid100_f1(metrics) == 0.0 and EV.lpips_fid100_f1(metrics) == 0.0


def test_make_evaluator_builds_fid(weights):
    ev = EV.make_evaluator(lpips=False, fid=True, fid_kwargs=dict(weights=weights), integral_kind='ssim_fid100_f1')
    assert list(ev.scores) == ['ssim', 'fid'] and isinstance(ev.scores['fid'], EV.FIDScore)
    assert ev.integral_func is EV.ssim_fid100_f1 and ev.integral_title == 'ssim_fid100_f1'
    with pytest.raises(NotImplementedError, match='FID'):
        EV.make_evaluator(lpips=False, fid=True, fid_kwargs=dict(weights=None))


class _StubNet(torch.nn.Module):
    """In place of Inception: a row of simple image statistics per image (so that a row identifies its image)."""

    def pair(self, pred, target):
        def rows(x):
            return torch.stack([x.mean(dim=(1, 2, 3)), x[:, 0].amax(dim=(1, 2)), x[:, 2].amin(dim=(1, 2)), x.flatten(1)[:, 0], x.flatten(1)[:, -1]], dim=1)
        return rows(pred).view(-1, 5, 1, 1), rows(target).view(-1, 5, 1, 1)


def test_device_loop_puts_activation_rows_back_in_dataset_order(tmp_path, weights):
    """The recorded dataset of tests/golden/evaluate.npz (three padded sizes, interleaved): the loop buckets by size, the rows must come back in
    dataset order, pred and target apart, beside a pairwise score."""
    import evaluate_ref as ER
    gold = ER.load_gold()
    datadir, preddir = ER.write_dataset(gold, str(tmp_path))
    ds = EV.PrecomputedInpaintingResultsDataset(datadir, preddir, inpainted_suffix=ER.INPAINTED_SUFFIX, img_suffix=ER.IMG_SUFFIX, pad_out_to_modulo=ER.PAD_MOD)
    fid = EV.FIDScore(weights=weights)
    fid.model = _StubNet()
    ssim = EV.SSIMScore()
    ssim.score._lib = emu_lib()
    scores = {'ssim': ssim, 'fid': fid}
    groups, names = EVL.score_dataset(ds, scores, batch_size=3, device='cpu', lib=emu_lib(), io_threads=2)
    (ap,), (at,) = fid.activations_pred, fid.activations_target
    assert ap.shape == at.shape == (len(ds), 5)
    stub = _StubNet()
    for i, n in enumerate(ER.item_names(gold)):
        im = torch.from_numpy(ER.host_item(gold[f'{n}_image'], ER.PAD_MOD))[None]
        pr = torch.from_numpy(ER.host_item(gold[f'{n}_inpainted'], ER.PAD_MOD))[None]
        wp, wt = stub.pair(pr, im)
        assert torch.equal(ap[i], wp.flatten()) and torch.equal(at[i], wt.flatten()), n
    total, per_group = fid.get_value(groups=groups)
    assert np.isfinite(total['mean']) and set(per_group) == set(np.unique(groups).tolist())
    assert len(ssim.individual_values) == len(ds)


def test_report_has_a_fid_column_without_std():
    results = {('ssim', 'total'): dict(mean=0.9, std=0.01), ('ssim', '0-10%'): dict(mean=0.95, std=0.02),
               ('fid', 'total'): dict(mean=12.5), ('fid', '0-10%'): dict(mean=float('nan')), ('lpips_fid100_f1', 'total'): dict(mean=0.8)}
    lines = EVL.format_report(results).splitlines()
    assert lines[0].split('\t') == ['', 'ssim', 'ssim', 'fid', 'lpips_fid100_f1']
    assert lines[1].split('\t') == ['', 'mean', 'std', 'mean', 'mean']
    assert lines[2].split('\t') == ['0-10%', '0.9500', '0.0200', '', '']
    assert lines[3].split('\t') == ['total', '0.9000', '0.0100', '12.5000', '0.8000']
