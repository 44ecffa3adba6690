"""CPU tests of ``lama_conv2d_fwd`` with ``pad_mode = LAMA_PAD_ZERO`` on NON-transposed convolutions through the host SIMT emulator, one case
per kernel family and per zero-fill code path (``cb_src_coord`` of conv_split3.inc / conv_wreg_dev.inc, ``conv_src_coord`` of conv_mfma.hip,
the ``col + kx - s.vpad`` column walk of the folded 7x7), against ``torch.nn.functional.conv2d(padding=pad)`` in float64.

The shapes are the smallest that still reach each branch of the dispatcher with the geometry of the three features that run zero-padded
direct convolutions in production:
  * LPIPS (lama_amd/evaluation.py): 3x3, stride 1, pad 1, bias + ReLU, 3 -> 64 up to 512 -> 512, planes down to 1 x 1;
  * the reverse pass (lama_amd/backward.py): the dgrad convs -- 3x3 stride 1 pad 2 (output two pixels larger than the input), 7x7 stride 1
    pad 6 (3 -> 64, the folded stem mode with vpad = 6), 3x3 stride 2 pad 1;
  * the regular and dilated generators (lama_amd/pix2pixhd.py): 3x3 stride 2 pad 1 with folded BatchNorm + ReLU, 3x3 stride 1 pad 1 with
    a residual.
``pad > (k - 1) / 2`` and planes smaller than the halo exist under zero padding only (reflect refuses ``pad >= H``).

The case tables are module-level constants and every test body is a ``check_*(lib, case, prec, dev)`` function: tests/test_conv_zero_pad_gpu.py
imports both and reruns them through the production library on the MI355X (``dev='cuda'``).

What a check asserts:
  * the input is channels [2, 2 + cin) of a buffer whose other channels hold NaN, the output channels [2, 2 + cout) of a buffer filled with
    7.0: a zero fill that loads outside the plane and multiplies by zero shows up as NaN (and, on the f16 split, in ``range_flag``), the
    guard channels of the output must keep 7.0 and no output element may be 7.0 or NaN;
  * ``check_zero_pad_conv``: ``CONV_TOL`` of tests/test_kernels_emu.py (|y - ref| <= atol + rtol |ref|) against float64, the worst error
    taken separately over the ring (output pixels whose window touches padding) and the interior, each against the same bar.  The bar was
    set for reflect padding at these channel counts; the padding mode changes no arithmetic, so it is not widened here;
  * ``check_tap_count``: x = 1, w = 1, no epilogue: every output must EQUAL cin * (taps of its window inside the plane), computed with
    integers.  All operands and partial sums are integers below 2^24 (512 * 49 = 25088), exact in fp32 and in both 3-term splits, so this
    separates "zero" from "clamped", "reflected" and "off by one" at every border pixel without any tolerance;
  * fp16 I/O (``PREC_F16``): the same check with fp16 tensors, the operands of ``_conv_f16_ref`` and the tolerance of ``_run_f16_case``
    (tests/test_kernels_emu.py: one fp16 rounding of the output)."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lama_amd import _lib as L
from tests import test_kernels_emu as KE
from tests.emu import emu_lib

SENT = 7.0
PRE, POST = 2, 1            # guard channels in front of / behind the view (both buffers)


def _c(form, cin, cout, k, stride, pad, H, W, act=L.ACT_NONE, bias=False, resid=False, scale=False):
    return dict(form=form, cin=cin, cout=cout, k=k, stride=stride, pad=pad, H=H, W=W, act=act, bias=bias, resid=resid, scale=scale)


def _lpips(cin, cout, H, W, emu=True):
    return dict(_c('lpips', cin, cout, 3, 1, 1, H, W, act=L.ACT_RELU, bias=True), emu=emu)


def _gen(cin, cout, stride, H, W, resid=False):
    return _c('gen', cin, cout, 3, stride, 1, H, W, act=L.ACT_RELU, bias=True, scale=True, resid=resid)


# ``emu=False``: GPU only.  The two 512 -> 512 cases cost about two minutes each on the emulator (both checks, three precisions); the same kernel and the
# same 2 x 3 / 1 x 1 planes run there at 64 -> 128, and 256 -> 512 / 512 -> 128 (about a minute each) stay
ZP_CASES = [
    # ---- LPIPS form: k3 s1 pad 1, bias, ReLU ---------------------------------------------------------------------------------------------
    _lpips(3, 64, 5, 7), _lpips(3, 64, 1, 1),                                  # LDS-staged kernel, channel tail (3 of 16); the whole window but one tap is padding
    _lpips(64, 64, 9, 37),                                                     # 64 rows: below the weights-in-registers kernel's 96
    _lpips(64, 128, 7, 37), _lpips(64, 128, 2, 3), _lpips(64, 128, 1, 1),      # weights in registers, K split; ragged 32 x 4 tiles, 8 x 16 tiles
    _lpips(128, 256, 6, 10),                                                   # two M tiles, 16 x 8 tiles
    _lpips(256, 512, 3, 5),
    _lpips(512, 512, 2, 3, emu=False), _lpips(512, 512, 1, 1, emu=False),
    # ---- reverse pass: dgrad convs, no bias, no activation ----------------------------------------------------------------------------
    _c('dgrad', 64, 128, 3, 1, 2, 7, 37),                                      # pad 2: output 9 x 39, two tile columns
    _c('dgrad', 96, 40, 3, 1, 2, 5, 6),                                        # LDS-staged kernel, pad 2
    _c('dgrad', 128, 384, 3, 1, 2, 4, 33),                                     # three M tiles; 35 output columns
    _c('dgrad', 64, 128, 3, 1, 2, 1, 1),                                       # pad >= H: every output sees exactly one tap
    _c('dgrad', 512, 128, 3, 1, 2, 8, 8),
    _c('dgrad_head', 3, 64, 7, 1, 6, 10, 12),                                  # folded 7x7 (virtual input channels), vpad = 6
    _c('dgrad_head', 3, 64, 7, 1, 6, 4, 4),                                    # plane smaller than the halo
    _c('dgrad_up', 64, 128, 3, 2, 1, 16, 70),                                  # weights in registers, parity-split columns; even sizes
    _c('dgrad_up', 64, 128, 3, 2, 1, 11, 37),                                  # odd sizes: the last window ends ON the last pixel
    _c('dgrad_up', 32, 64, 3, 2, 1, 12, 32),                                   # LDS-staged stride 2
    _c('dgrad_up', 6, 16, 3, 2, 1, 10, 14),                                    # ... with a channel tail
    # ---- generators: folded BatchNorm (scale + bias) + ReLU ----------------------------------------------------------------------------
    _gen(64, 128, 2, 11, 37), _gen(64, 128, 2, 16, 24), _gen(128, 256, 2, 8, 8),
    _gen(64, 130, 1, 7, 37, resid=True),                                       # ragged M tile
    _gen(12, 40, 1, 9, 7, resid=True),
]
ZP_F16_CASES = [_gen(64, 128, 2, 11, 37), _lpips(64, 128, 7, 37)]              # fp16 I/O: the stride-2 and the stride-1 weights-in-registers kernels


def ZP_ID(c):
    return f"{c['form']}_k{c['k']}s{c['stride']}p{c['pad']}_c{c['cin']}o{c['cout']}_{c['H']}x{c['W']}"


ZP_EMU_CASES = [c for c in ZP_CASES if c.get('emu', True)]
ZP_PRECS, ZP_PREC_IDS = KE.PRECISIONS, KE.PREC_IDS
ZP_PREC_NAME = dict(zip(KE.PRECISIONS, KE.PREC_IDS))
ZP_PREC_NAME[L.PREC_F16] = 'f16'


def _st(dev):
    return 0 if dev == 'cpu' else torch.cuda.current_stream().cuda_stream


def _sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


def out_size(c):
    return ((c['H'] + 2 * c['pad'] - c['k']) // c['stride'] + 1, (c['W'] + 2 * c['pad'] - c['k']) // c['stride'] + 1)


def taps_inside(n, n_out, k, stride, pad):
    """For each of the ``n_out`` output positions along one axis: how many of the k taps of its window lie inside [0, n) (integers)."""
    pos = np.arange(n_out)[:, None] * stride - pad + np.arange(k)[None, :]
    return ((pos >= 0) & (pos < n)).sum(1)


def ring_mask(c):
    """[Ho, Wo] bool: the window of this output pixel touches padding."""
    Ho, Wo = out_size(c)
    ty, tx = taps_inside(c['H'], Ho, c['k'], c['stride'], c['pad']), taps_inside(c['W'], Wo, c['k'], c['stride'], c['pad'])
    return (ty[:, None] < c['k']) | (tx[None, :] < c['k'])


@functools.lru_cache(None)
def _operands(idx, half):
    """Host operands and the float64 result of case ``idx`` of ZP_CASES + ZP_F16_CASES: computed once, shared by the precisions and by
    the emulator / GPU runs of one process, never written to."""
    c = (ZP_CASES + ZP_F16_CASES)[idx]
    g = torch.Generator().manual_seed(1000 + idx)
    B, cin, cout, k = c.get('B', 2), c['cin'], c['cout'], c['k']
    Ho, Wo = out_size(c)
    x = torch.randn(B, cin, c['H'], c['W'], generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * (cin * k * k) ** -0.5        # outputs O(1) at every channel count
    scale = torch.rand(cout, generator=g) + 0.5 if c['scale'] else None
    bias = torch.randn(cout, generator=g) if c['bias'] else None
    resid = torch.randn(B, cout, Ho, Wo, generator=g) if c['resid'] else None
    if half:                                                                        # fp16 tensors: the kernel sees the rounded values
        x = x.half()
        resid = None if resid is None else resid.half()
    # float64, the order of KE._conv_ref: scale folded into the weights, conv, bias, activation, residual
    wd = w.double() if scale is None else w.double() * scale.double()[:, None, None, None]
    ref = F.conv2d(x.double(), wd, None, stride=c['stride'], padding=c['pad'])
    if bias is not None:
        ref = ref + bias.double()[None, :, None, None]
    ref = {L.ACT_NONE: lambda t: t, L.ACT_RELU: torch.relu, L.ACT_SIGMOID: torch.sigmoid, L.ACT_TANH: torch.tanh}[c['act']](ref)
    if resid is not None:
        ref = ref + resid.double()
    assert tuple(ref.shape) == (B, cout, Ho, Wo)
    return types.SimpleNamespace(case=c, B=B, x=x, w=w, scale=scale, bias=bias, resid=resid, ref=ref, ring=torch.from_numpy(ring_mask(c)))


def operands(case, half=False):
    return _operands(next(i for i, c in enumerate(ZP_CASES + ZP_F16_CASES) if c is case), half)


def _guarded_input(x, dev):
    """``x`` as channels [PRE, PRE + cin) of a buffer whose other channels hold NaN."""
    B, C, H, W = x.shape
    buf = torch.full((B, PRE + C + POST, H, W), float('nan'), dtype=x.dtype)
    buf[:, PRE:PRE + C] = x
    return buf.to(dev)


def run_zero_pad(lib, c, prec, dev, x, w, scale=None, bias=None, resid=None, pad_mode=L.PAD_ZERO, y_dtype=torch.float32):
    """One lama_conv2d_fwd call on guarded buffers; returns the written channels on the host as float32 after the guard assertions."""
    B, cin, cout = x.shape[0], c['cin'], c['cout']
    Ho, Wo = out_size(c)
    xbuf = _guarded_input(x, dev)
    ybuf = torch.full((B, PRE + cout + POST, Ho, Wo), SENT, dtype=y_dtype, device=dev)
    wp = lib.pack_conv_weight(w.to(dev), None if scale is None else scale.to(dev), stride=c['stride'], precision=prec)
    bias_d = None if bias is None else bias.to(dev)
    resid_d = None if resid is None else resid.to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.conv2d(L.view(xbuf, PRE, cin), wp, L.view(ybuf, PRE, cout), B, c['k'], c['stride'], c['pad'], pad_mode, False, bias_d, c['act'],
               None if resid_d is None else L.view(resid_d), precision=prec, stream=_st(dev), range_flag=flag)
    _sync(dev)
    h = ybuf.cpu().float()
    guards = torch.cat([h[:, :PRE], h[:, PRE + cout:]], 1)
    assert float(guards.min()) == SENT == float(guards.max()), 'a channel outside the output view was written'
    y = h[:, PRE:PRE + cout].contiguous()
    assert not bool(torch.isnan(y).any()), f'NaN in the output: {int(torch.isnan(y).sum())} elements (a load outside the input view)'
    assert not bool((y == SENT).any()), f'{int((y == SENT).sum())} output elements were never written'
    assert int(flag) == 0, 'range_flag raised: the f16 split met a NaN / an out-of-range activation that is not part of the input view'
    return y


def ring_interior_errors(y, ref, ring, atol, rtol):
    """(worst |y - ref|, worst |y - ref| / (atol + rtol |ref|)) over the ring and over the interior; an empty set counts as 0."""
    err = (y.double() - ref).abs()
    rel = err / (atol + rtol * ref.abs())
    out = []
    for m in (ring, ~ring):
        out.append((float(err[:, :, m].max()), float(rel[:, :, m].max())) if bool(m.any()) else (0.0, 0.0))
    return out


def check_zero_pad_conv(lib, case, prec, dev):
    """Random operands against float64: CONV_TOL over the ring and over the interior (fp16 I/O: the tolerance of KE._run_f16_case)."""
    half = prec == L.PREC_F16
    o = operands(case, half)
    y = run_zero_pad(lib, case, prec, dev, o.x, o.w, o.scale, o.bias, o.resid, y_dtype=torch.float16 if half else torch.float32)
    if half:
        tol = dict(atol=2e-3 * max(1.0, float(o.ref.abs().max())), rtol=0.0)      # one fp16 rounding of the output
        ref32 = KE._conv_f16_ref(o.x, o.w, case['stride'], case['pad'], False, False, o.bias, case['act'], o.resid, scale=o.scale)
        assert float((y - ref32).abs().max()) < tol['atol'], float((y - ref32).abs().max())
    else:
        tol = KE.CONV_TOL[prec]
    (ring_err, ring_rel), (int_err, int_rel) = ring_interior_errors(y, o.ref, o.ring, **tol)
    if dev != 'cpu':
        print(f'[zero-pad] {ZP_ID(case)} {ZP_PREC_NAME[prec]}: ring max err = {ring_err:.3e} ({ring_rel:.3f} of the bar), '
              f'interior max err = {int_err:.3e} ({int_rel:.3f} of the bar)')
    assert ring_rel <= 1.0, f'ring: {ring_err:.3e} = {ring_rel:.2f} x the bar (interior {int_err:.3e} = {int_rel:.2f} x)'
    assert int_rel <= 1.0, f'interior: {int_err:.3e} = {int_rel:.2f} x the bar (ring {ring_err:.3e} = {ring_rel:.2f} x)'
    assert torch.allclose(y.double(), o.ref, **tol), float((y.double() - o.ref).abs().max())


def check_tap_count(lib, case, prec, dev):
    """x = 1, w = 1, no epilogue: every output equals cin * (taps of its window inside the plane), exactly."""
    c = dict(case, act=L.ACT_NONE)
    half = prec == L.PREC_F16
    B, cin, cout, k = case.get('B', 2), case['cin'], case['cout'], case['k']
    Ho, Wo = out_size(case)
    ty, tx = taps_inside(case['H'], Ho, k, case['stride'], case['pad']), taps_inside(case['W'], Wo, k, case['stride'], case['pad'])
    want = cin * (ty[:, None] * tx[None, :])                                      # int64 [Ho, Wo]
    assert int(want.max()) < 2 ** (11 if half else 24) and int(want.min()) >= cin, 'every window holds a pixel; the sums are exact'
    x = torch.ones(B, cin, case['H'], case['W'], dtype=torch.float16 if half else torch.float32)
    y = run_zero_pad(lib, c, prec, dev, x, torch.ones(cout, cin, k, k), y_dtype=x.dtype)
    want_t = torch.from_numpy(want.astype(np.float32)).expand(B, cout, Ho, Wo)
    if not torch.equal(y, want_t):
        bad = (y != want_t).nonzero()
        b, m, oy, ox = (int(v) for v in bad[0])
        raise AssertionError(f'{len(bad)} of {y.numel()} outputs differ; first at image {b} channel {m} pixel ({oy}, {ox}): '
                             f'got {float(y[b, m, oy, ox])}, want {int(want[oy, ox])} = {cin} x {int(ty[oy])} x {int(tx[ox])} taps')


def check_zero_pad_geometry(lib, dev):
    """``pad >= H`` runs under PAD_ZERO (the 1 x 1 and 4 x 4 cases above) and is LAMA_ERR_BAD_ARG under PAD_REFLECT with the same operands;
    an output view with H + 1 instead of H + 2 rows for pad = 2 is LAMA_ERR_BAD_ARG."""
    small = [c for c in ZP_EMU_CASES if c['pad'] >= min(c['H'], c['W'])]
    assert {(c['H'], c['W']) for c in small} >= {(1, 1), (4, 4)}
    for c in small:
        o = operands(c)
        for prec in ZP_PRECS:
            with pytest.raises(L.LamaError) as ei:
                run_zero_pad(lib, c, prec, dev, o.x, o.w, o.scale, o.bias, o.resid, pad_mode=L.PAD_REFLECT)
            assert ei.value.code == L.ERR_BAD_ARG, (ZP_ID(c), prec, ei.value.code)
    c = next(c for c in ZP_CASES if c['pad'] == 2 and c['k'] == 3 and c['H'] > 1)
    o = operands(c)
    B, cin, cout, H, W = o.B, c['cin'], c['cout'], c['H'], c['W']
    xbuf = _guarded_input(o.x, dev)
    for prec in ZP_PRECS:
        wp = lib.pack_conv_weight(o.w.to(dev), None, precision=prec)
        for rows, cols in ((H + 1, W + 2), (H + 2, W + 1), (H, W)):
            ybuf = torch.full((B, PRE + cout + POST, rows, cols), SENT, device=dev)
            with pytest.raises(L.LamaError) as ei:
                lib.conv2d(L.view(xbuf, PRE, cin), wp, L.view(ybuf, PRE, cout), B, 3, 1, 2, L.PAD_ZERO, False, None, L.ACT_NONE, precision=prec,
                           stream=_st(dev))
            _sync(dev)
            assert ei.value.code == L.ERR_BAD_ARG, (prec, rows, cols, ei.value.code)
            assert float(ybuf.min()) == SENT == float(ybuf.max())


def test_ring_mask_and_tap_count_reference():
    """The numpy geometry the checks rely on, against torch on an all-ones plane."""
    for c in ZP_CASES:
        Ho, Wo = out_size(c)
        ones = F.conv2d(torch.ones(1, 1, c['H'], c['W'], dtype=torch.float64), torch.ones(1, 1, c['k'], c['k'], dtype=torch.float64),
                        stride=c['stride'], padding=c['pad'])[0, 0]
        ty, tx = taps_inside(c['H'], Ho, c['k'], c['stride'], c['pad']), taps_inside(c['W'], Wo, c['k'], c['stride'], c['pad'])
        assert tuple(ones.shape) == (Ho, Wo) and np.array_equal(ones.numpy().astype(np.int64), ty[:, None] * tx[None, :])
        assert np.array_equal(ring_mask(c), ones.numpy() < c['k'] ** 2) and ring_mask(c).any()


def test_gpu_only_cases_keep_an_emulator_twin():
    """A case left to the GPU has 256 or more input channels and a case of the same form, geometry and plane with fewer channels here."""
    geo = lambda c: tuple(c[f] for f in ('form', 'k', 'stride', 'pad', 'H', 'W', 'act', 'bias', 'resid', 'scale'))      # noqa: E731
    for c in ZP_CASES:
        if not c.get('emu', True):
            assert c['cin'] >= 256 and any(geo(e) == geo(c) and e['cin'] % 32 == 0 and e['cout'] >= 96 for e in ZP_EMU_CASES), ZP_ID(c)


@pytest.mark.parametrize('prec', ZP_PRECS, ids=ZP_PREC_IDS)
@pytest.mark.parametrize('case', ZP_EMU_CASES, ids=ZP_ID)
def test_zero_pad_conv_emulated(case, prec):
    check_zero_pad_conv(emu_lib(), case, prec, 'cpu')


@pytest.mark.parametrize('prec', ZP_PRECS, ids=ZP_PREC_IDS)
@pytest.mark.parametrize('case', ZP_EMU_CASES, ids=ZP_ID)
def test_tap_count_emulated(case, prec):
    check_tap_count(emu_lib(), case, prec, 'cpu')


@pytest.mark.parametrize('case', ZP_F16_CASES, ids=ZP_ID)
def test_zero_pad_conv_fp16_io_emulated(case):
    check_zero_pad_conv(emu_lib(), case, L.PREC_F16, 'cpu')
    check_tap_count(emu_lib(), case, L.PREC_F16, 'cpu')


def test_zero_pad_geometry_emulated():
    check_zero_pad_geometry(emu_lib(), 'cpu')
