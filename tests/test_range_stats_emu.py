"""CPU tests of the activation-range diagnostics, driven through the host SIMT emulator (tests/hipemu):

  * lama_range_stats_fwd, bit for bit against the numpy statement in tests/range_ref.py, on every kind of view the library hands around
    (channel slices, element-aligned plane starts, planes that are no multiple of the vector width, several 32 KiB pieces per plane), with
    the special values planted where the kernel changes path; its overwrite / reproducibility / return-code contract;
  * lama_fourier_unit_workspace_views against what lama_rfft2_fwd writes;
  * lama_amd.probe.probe_ranges on the small generators of the three kinds.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from lama_amd import _lib as L
from lama_amd import ffc as F
from lama_amd.modules import make_generator
from lama_amd.probe import probe_ranges
from oracle import lama_oracle as O
from tests import range_ref as R
from tests.emu import emu_lib

from tests.range_ref import IDS, VIEWS, _bits, check_rows_against_reference, check_view


@pytest.mark.parametrize('dtype', [np.float32, np.float16], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('shape,c0,c', VIEWS, ids=IDS)
def test_range_stats_bit_equal_to_reference(shape, c0, c, dtype):
    lib = emu_lib()
    full, limit = R.planted(shape, dtype, c0, c, limit=65504.0, seed=len(shape) + shape[1])
    out, ref = check_view(lib, full, c0, c, limit)
    if shape == (3, 70, 4, 4):                       # the planted kinds are really there, each in a channel of its own
        amax, nn, ni, no = ref
        assert nn[-1] == 3 * 16 and amax[-1] == 0 and np.signbit(amax[-1]) == False      # noqa: E712  the all-NaN channel: +0.0
        assert amax[-2] == 0 and nn[-2] == ni[-2] == no[-2] == 0                           # the all-zero channel
        if dtype == np.float32:
            assert no[0] == 0 and amax[0] == np.float32(65504.0)                           # exactly limit: not over
            assert no[1] > 0 and no[2] > 0 and ni[3] > 0 and ni[4] > 0 and nn[5] > 0 and nn[6] > 0
        else:
            assert no[0] == 0 and amax[0] == np.float32(65504.0) and ni[2] > 0 and ni[3] > 0 and nn[4] > 0 and nn[5] > 0


def test_range_stats_limit_between_halves_and_denormals():
    """fp16 with a limit that is no half value, and the smallest denormals of both types against a denormal limit."""
    lib = emu_lib()
    h = np.zeros((1, 2, 3, 5), dtype=np.float16)
    h[0, 0, 0, :3] = [1000.0, 1000.5, 1001.0]        # neighbours at this magnitude: 1000.25 lies between two of them
    h[0, 1, 2, 4] = np.array([0x0001], dtype=np.uint16).view(np.float16)[0]
    _, ref = check_view(lib, h, 0, None, 1000.25)
    assert list(ref[3]) == [2, 0]
    _, ref = check_view(lib, h, 0, None, 5.0e-8)     # below the smallest half denormal (5.96e-8): every non-zero element is over
    assert list(ref[3]) == [3, 1]
    f = np.zeros((1, 1, 2, 3), dtype=np.float32)
    f[0, 0, 0, 0] = np.array([1], dtype=np.uint32).view(np.float32)[0]
    f[0, 0, 1, 2] = -np.array([2], dtype=np.uint32).view(np.float32)[0]
    lim = float(np.array([1], dtype=np.uint32).view(np.float32)[0])
    _, ref = check_view(lib, f, 0, None, lim)
    assert list(ref[3]) == [1] and _bits(ref[0])[0] == 2


def test_range_stats_is_reproducible_and_overwrites():
    lib = emu_lib()
    full, limit = R.planted((2, 6, 8, 5), np.float32, seed=4)
    t = torch.from_numpy(full)
    a = lib.range_stats(L.view(t), 2, limit, out=torch.full((6, 4), -1, dtype=torch.int32))
    b = lib.range_stats(L.view(t), 2, limit, out=torch.full((6, 4), 12345, dtype=torch.int32))
    assert a.numpy().tobytes() == b.numpy().tobytes()
    c = lib.range_stats(L.view(t), 2, limit)                     # allocates out and the workspace itself
    assert tuple(c.shape) == (6, 4) and c.dtype == torch.int32 and c.numpy().tobytes() == a.numpy().tobytes()


def test_range_stats_return_codes_leave_out_untouched():
    lib = emu_lib()
    x = torch.randn(2, 3, 4, 5)
    xv = L.view(x)
    nbytes = lib.range_stats_workspace_bytes(2, 3, 4, 5)
    assert nbytes == 2 * 3 * 16 and lib.range_stats_workspace_bytes(0, 3, 4, 5) == 0
    ws = torch.zeros(nbytes // 4, dtype=torch.int32)
    out = torch.full((3, 4), 77, dtype=torch.int32)
    fn = lib._l.lama_range_stats_fwd

    def call(x=xv, batch=2, limit=65504.0, out_p=out.data_ptr(), ws_p=ws.data_ptr(), ws_n=nbytes):
        rc = fn(0, None if x is None else C.byref(x), batch, limit, out_p, ws_p, ws_n)
        assert bool((out == 77).all()), 'out was written on an error'
        return rc

    assert call(x=None) == L.ERR_BAD_ARG
    assert call(x=L.Tensor4(None, 60, 3, 4, 5, 0)) == L.ERR_BAD_ARG
    assert call(out_p=None) == L.ERR_BAD_ARG
    assert call(ws_p=None) == L.ERR_BAD_ARG
    assert call(batch=0) == L.ERR_BAD_ARG and call(batch=-1) == L.ERR_BAD_ARG
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        assert call(limit=bad) == L.ERR_BAD_ARG, bad
    assert call(x=L.Tensor4(x.data_ptr(), 59, 3, 4, 5, 0)) == L.ERR_BAD_ARG              # batch_stride < C H W
    assert call(ws_n=nbytes - 1) == L.ERR_WORKSPACE
    assert call(x=L.Tensor4(x.data_ptr(), 60, 3, 4, 5, 7)) == L.ERR_UNSUPPORTED           # unknown dtype
    # batch H W >= 2^32: the 32-bit counters could wrap (nothing is dereferenced: the check comes first)
    assert call(x=L.Tensor4(x.data_ptr(), 1 << 40, 1, 1 << 15, 1 << 15, 0), batch=4, ws_n=1 << 62) == L.ERR_UNSUPPORTED
    assert fn(0, C.byref(xv), 2, 65504.0, out.data_ptr(), ws.data_ptr(), nbytes) == 0 and not bool((out == 77).any())


def test_fourier_unit_views_are_the_spectra_of_the_call():
    """spec_in seen through lama_fourier_unit_workspace_views after lib.fourier_unit == what lib.rfft2 writes for the same input, bit for bit."""
    lib = emu_lib()
    torch.manual_seed(0)
    B, Cn, H, W = 2, 4, 8, 6
    x = torch.randn(B, Cn, H, W)
    w = torch.randn(2 * Cn, 2 * Cn, 1, 1) * 0.3
    wp = lib.pack_conv_weight(w, None, precision=L.PREC_F16X3)
    bias = torch.randn(2 * Cn) * 0.1
    ws = torch.full((lib.fourier_unit_workspace_bytes(B, Cn, H, W) // 4 + 1,), float('nan'))
    y = torch.empty_like(x)
    lib.fourier_unit(L.view(x), wp, bias, L.view(y), B, True, ws, precision=L.PREC_F16X3)
    si, so = lib.fourier_unit_views(ws, B, Cn, H, W, L.DT_F32)
    assert (si.C, si.H, si.W, si.batch_stride) == (2 * Cn, H, W // 2 + 1, 2 * Cn * H * (W // 2 + 1)) and si.ptr == ws.data_ptr()
    assert (so.C, so.H, so.W) == (si.C, si.H, si.W) and (so.ptr - si.ptr) % 256 == 0 and so.ptr - si.ptr >= B * si.batch_stride * 4
    n = B * si.batch_stride
    spec_in = ws[:n].view(B, 2 * Cn, H, W // 2 + 1)
    spec = torch.empty(B, 2 * Cn, H, W // 2 + 1)
    fws = torch.empty(lib.fft_workspace_bytes(B, Cn, H, W) // 4 + 1)
    lib.rfft2(L.view(x), L.view(spec), B, fws)
    assert spec_in.numpy().tobytes() == spec.numpy().tobytes()
    off = (so.ptr - ws.data_ptr()) // 4
    spec_out = ws[off:off + n].view(B, 2 * Cn, H, W // 2 + 1)
    want = torch.relu(torch.nn.functional.conv2d(spec.double(), w.double(), bias.double()))
    assert float((spec_out.double() - want).abs().max()) < 1e-4 and float(spec_out.min()) >= 0
    with pytest.raises(L.LamaError) as e:
        lib.fourier_unit_views(ws[:8], B, Cn, H, W, L.DT_F32)
    assert e.value.code == L.ERR_WORKSPACE


# ---- the probe ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def ffc_small():
    """The set-up of test_f16_split_overflow_falls_back_to_bf16x3 (tests/test_host_emu.py)."""
    cfg = O.small_config(ngf=8, n_blocks=1)
    sd = O.make_synthetic_state_dict(cfg, seed=5, calib_hw=32)
    gen = make_generator(None, kind='ffc_resnet', **cfg)
    gen.load_state_dict(sd, strict=True)
    gen.set_exec(F._Exec(emu_lib()))
    batch = O.make_synthetic_batch(1, 64, 64, seed=2)
    x = torch.cat([batch['image'] * (1 - batch['mask']), batch['mask']], 1)
    return cfg, sd, gen, x


def test_probe_rows_of_the_ffc_generator(ffc_small):
    cfg, sd, gen, x = ffc_small
    rep = probe_ranges(gen, x, keep=True)
    names = rep.names()
    # model: 0 pad, 1 stem, 2-4 downsampling (4 produces the x_l | x_g pair), 5 the block, 6 concat, 7-15 three (convT, BN, ReLU), 16 pad, 17 head, 18 sigmoid
    want = ['in', 'model.1', 'model.2', 'model.3', 'model.4:x_l', 'model.4:x_g', 'model.5:x_l', 'model.5:x_g', 'model.9', 'model.12', 'model.15', 'model.18']
    for blk in ('model.5.conv1', 'model.5.conv2'):
        p = blk + '.ffc.convg2g'
        want += [p + '.conv1', p + '.fu:spectrum', p + '.fu:spectrum_out', p + ':t']
    want += ['model.5.conv1:x_l', 'model.5.conv1:x_g']
    assert set(want) <= set(names) and len(set(names)) == len(names), sorted(set(want) - set(names))
    assert names[0] == 'in' and names[-1] == 'model.18'
    assert names.index('model.5.conv1.ffc.convg2g.fu:spectrum') < names.index('model.5.conv1:x_l') < names.index('model.5.conv2.ffc.convg2g.conv1')
    sp = rep['model.5.conv1.ffc.convg2g.fu:spectrum']
    x1 = rep['model.5.conv1.ffc.convg2g.conv1']
    assert sp.shape == (1, 2 * x1.shape[1], 8, 5) and x1.shape[2:] == (8, 8)
    check_rows_against_reference(rep)
    # the spectrum row really is the operand of the spectral 1x1: rfft2 of the kept x1
    kx1 = rep.tensors['model.5.conv1.ffc.convg2g.conv1']
    ff = torch.fft.rfft2(kx1.double(), norm='ortho')
    ref = torch.stack((ff.real, ff.imag), 2).reshape(1, -1, 8, 5)
    assert float((rep.tensors[sp.name].double() - ref).abs().max()) < 1e-5 * max(1.0, float(ref.abs().max()))
    # clean input: nothing out of range, and the generator agrees
    assert rep.first_over() is None and all(r.bound is None for r in rep.rows)       # (64 channels: no Winograd launch at this size)
    y = gen(x)
    assert gen.precision == L.PREC_F16X3
    assert float((rep.output - y).abs().max()) < 1e-3
    assert [r.name for r in rep.worst(3)] == [r.name for r in sorted(rep.rows, key=lambda r: -r.abs_max)[:3]]
    text = rep.format()
    assert len(text.splitlines()) == len(rep.rows) + 1 and 'model.5.conv2.ffc.convg2g:t' in text
    assert probe_ranges(gen, x).tensors is None


def test_probe_names_the_tensor_that_left_the_range(ffc_small):
    cfg, sd, gen, x = ffc_small
    xb = x.clone()
    xb[0, 1, 20:24, 30:34] = 3.0e5
    plans = dict(gen._plans)
    rep = probe_ranges(gen, xb)                                   # never raises LamaRangeError
    first = rep.first_over()
    assert first is not None and first.name == 'in' and first.channel == 1 and first.n_over == 16 and first.bad_channel == 1
    assert first.abs_max == 3.0e5 and first.n_nan == 0 and first.n_inf == 0
    assert rep.worst(1)[0].abs_max >= 3.0e5
    assert gen.precision == L.PREC_F16X3 and dict(gen._plans) == plans and gen.use_graph is False
    assert all(m.precision == L.PREC_F16X3 for m in gen.modules() if isinstance(m, F._HipModule))
    assert gen._exec.range_flag_raised() is False                 # what the probe's forward raised is discarded
    gen.auto_fallback = False
    try:
        with pytest.raises(L.LamaRangeError):
            gen(xb)
    finally:
        gen.auto_fallback = True
    assert gen.precision == L.PREC_F16X3


def test_probe_keeps_a_pending_deferred_report(ffc_small):
    cfg, sd, gen, x = ffc_small
    xb = x.clone()
    xb[0, 1, 20:24, 30:34] = 3.0e5
    gen.defer_range_check, gen.auto_fallback = True, False
    try:
        gen(xb)                                                   # raises the flag on the device; nobody has looked yet
        rep = probe_ranges(gen, x)                                # a clean probe in between
        assert rep.first_over() is None
        with pytest.raises(L.LamaRangeError):
            gen.check_range()                                     # ... the pending report is still there
        assert gen.check_range() is True
        probe_ranges(gen, xb)                                     # and a probe that saw an overflow leaves nothing behind
        assert gen.check_range() is True
    finally:
        gen.defer_range_check, gen.auto_fallback = False, True
    assert gen.precision == L.PREC_F16X3


def test_probe_reports_a_refused_weight_and_goes_on(ffc_small):
    """A folded weight beyond the fp16 split's range is refused at pack time (what makes generator(x) fall back before its first launch): the
    probe reports it as a row under the layer and measures the rest on the bf16 split for that layer only."""
    cfg, sd, gen, x = ffc_small
    key = 'model.5.conv1.bn_l.weight'
    bad = {k: (v * 1e7 if k == key else v) for k, v in sd.items()}
    gen.load_state_dict(bad, strict=True)
    try:
        rep = probe_ranges(gen, x)
        first = rep.first_over()
        assert first is not None and first.name.startswith('model.5.conv1') and rep.names().index(first.name) > rep.names().index('model.4:x_g')
        assert 'model.5.conv1:weights' in rep.names() and rep['model.5.conv1:x_l'].n_over > 0
        wrow = rep['model.5.conv1:weights']
        assert wrow.refused and wrow.bad == 1 and (wrow.n_over, wrow.n_nan, wrow.n_inf) == (0, 0, 0) and wrow.as_dict()['abs_max'] is None
        assert not any(r.refused for r in rep.rows if r is not wrow)
        assert gen.precision == L.PREC_F16X3 and all(m.precision == L.PREC_F16X3 for m in gen.modules() if isinstance(m, F._HipModule))
        assert rep.names()[-1] == 'model.18'
    finally:
        gen.load_state_dict(sd, strict=True)


def test_probe_refuses_cpu_tensors_on_the_default_exec():
    cfg = O.small_config(ngf=8, n_blocks=1)
    gen = make_generator(None, kind='ffc_resnet', **cfg)
    with pytest.raises(L.LamaError):
        probe_ranges(gen, torch.zeros(1, 4, 64, 64))
    with pytest.raises(L.LamaError):
        probe_ranges(torch.nn.Identity(), torch.zeros(1, 4, 64, 64))


def _pix_small(kind):
    if kind == 'pix2pixhd_global':
        from tests import regular_util as U
        cfg = U.small_config(ngf=4, n_blocks=1)
        sd = U.make_state_dict(cfg, seed=2, calib_hw=32)
        x = torch.rand(1, 4, 40, 48)
    else:
        from tests import multidilated_util as U
        cfg = U.small_config(ngf=8, n_blocks=1)           # 64 bottleneck channels: four dilation groups of 16
        sd = U.make_state_dict(cfg, seed=2)
        x = torch.rand(1, 4, 72, 80)
    gen = make_generator(None, kind=kind, **cfg)
    gen.load_state_dict(sd, strict=True)
    gen.set_exec(F._Exec(emu_lib()))
    return U, cfg, sd, gen, x


@pytest.mark.parametrize('kind', ['pix2pixhd_global', 'pix2pixhd_multidilated'])
def test_probe_rows_of_the_pix2pixhd_generators(kind):
    U, cfg, sd, gen, x = _pix_small(kind)
    rep = probe_ranges(gen, x, keep=True)
    names = rep.names()
    # model: 0 pad, 1-3 stem (conv, BN, ReLU), 4-12 three (conv, BN, ReLU), 13 the block, 14-22 three (convT, BN, ReLU), 23 pad, 24 head, 25 act
    mid = 'model.13.conv_block.3' if kind == 'pix2pixhd_global' else 'model.13.conv_block.2'
    assert names == ['in', 'model.3', 'model.6', 'model.9', 'model.12', mid, 'model.13', 'model.16', 'model.19', 'model.22', 'model.25']
    assert rep['model.13'].module.startswith('model.13.conv_block.') and rep['model.16'].module == 'model.14' and rep['model.25'].module == 'model.24'
    check_rows_against_reference(rep)
    assert rep.first_over() is None
    y = gen(x)
    assert float((rep.output - y).abs().max()) < 1e-3
    with torch.no_grad():
        ref = U.forward(sd, cfg, x)
    assert float((rep.output - ref).abs().max()) < 1e-3
    xb = x.clone()
    xb[0, 2, 5, 7] = float('nan')
    first = probe_ranges(gen, xb).first_over()
    assert first.name == 'in' and first.n_nan == 1 and first.bad_channel == 2
    assert gen.precision == L.PREC_F16X3
