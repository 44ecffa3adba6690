"""GPU tests of the activation-range diagnostics: lama_range_stats_fwd on the device, bit for bit against tests/range_ref.py (the views of the
emulator test plus the real operands: a bottleneck spectrum and the x_g slice of the 512-channel state), and lama_amd.probe.probe_ranges against
the CPU oracle's per-layer taps."""
import re

import numpy as np
import pytest
import torch

from lama_amd import _lib as L
from lama_amd.modules import make_generator
from lama_amd.probe import probe_ranges
from oracle import lama_oracle as O
from tests import range_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

REAL = [((2, 384, 64, 33), 0, None),            # the spectrum of the 192-channel x1 at a 64 x 64 bottleneck
        ((2, 512, 64, 64), 128, 384)]           # x_g inside the (x_l | x_g) state buffer


@pytest.fixture(scope='module')
def lib():
    return L.get_lib()


@pytest.mark.parametrize('dtype', [np.float32, np.float16], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('shape,c0,c', R.VIEWS + REAL, ids=R.IDS + ['2x384x64x33', '2x512x64x64[128:512]'])
def test_range_stats_bit_equal_to_reference_on_the_device(lib, shape, c0, c, dtype):
    full, limit = R.planted(shape, dtype, c0, c, limit=65504.0, seed=shape[1] + shape[3])
    out, ref = R.check_view(lib, full, c0, c, limit, device=DEV)
    # two calls, identical bytes (a second output buffer pre-filled with other garbage)
    t = torch.from_numpy(full).to(DEV)
    again = lib.range_stats(L.view(t, c0, c), shape[0], limit, out=torch.full_like(out, -3), stream=lib.stream_of(t))
    assert torch.equal(again, out)


@pytest.mark.parametrize('dtype', [np.float32, np.float16], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('shape,c0,c', [R.VIEWS[1], R.VIEWS[5], REAL[0]], ids=['2x5x7x9[1:4]', '1x2x300x301', '2x384x64x33'])
def test_range_stats_counts_over_a_limit_inside_the_data(lib, shape, c0, c, dtype):
    """limit = 37.3 (no half value, well inside randn x 100): n_over is non-zero in every channel for both element types -- on fp16 views this is
    the host's conversion of the limit to a half magnitude and the 15-bit compare."""
    full, limit = R.planted(shape, dtype, c0, c, limit=65504.0, seed=shape[3])
    out, ref = R.check_view(lib, full, c0, c, 37.3, device=DEV)
    live = ref[1] < shape[0] * shape[2] * shape[3]                 # (not the all-NaN channel)
    assert (ref[3][live & (ref[0] > 0)] > 0).all()


def _bound_rows(rep):
    for r in rep.rows:
        if r.bound is not None:
            assert r.winograd and r.bound == 4.0 * r.abs_max, r.name
    return [r.name for r in rep.rows if r.bound is not None]


def test_probe_winograd_bound_rows_pix2pixhd(lib):
    """A ResnetBlock of 128 channels on a 32 x 32 plane: the exact Winograd geometry, which the library always prefers.  The rows the two
    Winograd launches READ carry bound = 4 x abs_max; no other row has a bound."""
    from tests import regular_util as U
    cfg = U.small_config(ngf=16, n_blocks=1)
    torch.manual_seed(1)
    gen = make_generator(None, kind='pix2pixhd_global', **cfg).cuda()
    x = torch.rand(1, 4, 256, 256, device=DEV)
    assert lib.winograd_preferred(1, 128, 128, 32, 32, L.PREC_F16X3)
    rep = probe_ranges(gen, x)
    assert _bound_rows(rep) == ['model.12', 'model.13.conv_block.3'], rep.format()
    y = gen(x)
    assert gen.conv_paths(x.shape, x.device) == ['winograd', 'winograd']
    assert float((rep.output - y).abs().max()) < 1e-3
    gen._exec.winograd = False                                    # the same generator on the direct kernel: no bound anywhere
    try:
        assert _bound_rows(probe_ranges(gen, x)) == []
    finally:
        gen._exec.winograd = True


def test_probe_winograd_bound_rows_ffc(lib):
    """One big-lama block (512 channels: 128 local outputs over the 512-channel state) on a 32 x 32 plane: the local conv of both layers takes
    the Winograd kernel and reads the whole (x_l | x_g) state, so the block's input pair and its middle pair carry the bound."""
    cfg = dict(O.BIG_LAMA, n_blocks=1)
    torch.manual_seed(2)
    gen = make_generator(None, kind='ffc_resnet', **cfg).cuda()
    x = torch.rand(1, 4, 256, 256, device=DEV)
    assert lib.winograd_preferred(1, 128, 512, 32, 32, L.PREC_F16X3)
    rep = probe_ranges(gen, x)
    assert _bound_rows(rep) == ['model.4:x_l', 'model.4:x_g', 'model.5.conv1:x_l', 'model.5.conv1:x_g'], rep.format()
    assert rep.names()[-1] == 'model.18' and gen.precision == L.PREC_F16X3      # one block: the sigmoid is model.18


@pytest.fixture(scope='module')
def small():
    """The generator, input and oracle taps of test_small_generator_layerwise_and_sliced (tests/test_generator_gpu.py), computed once."""
    cfg = O.small_config(ngf=8, n_blocks=2)
    sd = O.make_synthetic_state_dict(cfg, seed=7, calib_hw=32)
    gen = make_generator(None, kind='ffc_resnet', **cfg)
    gen.load_state_dict(sd, strict=True)
    gen = gen.cuda()
    batch = O.make_synthetic_batch(2, 128, 128, seed=3)
    x = torch.cat([batch['image'] * (1 - batch['mask']), batch['mask']], 1)
    taps = {}
    with torch.no_grad():
        ref = O.generator_forward(x, sd, cfg, taps=taps)
    rep = probe_ranges(gen, x.to(DEV), keep=True)
    return gen, x, taps, ref, rep


def test_probe_rows_against_the_oracle_taps(small):
    gen, x, taps, ref, rep = small
    seen = set()
    for r in rep.rows:
        mt = re.fullmatch(r'model\.(\d+)(:x_l|:x_g)?', r.name)
        if not mt:
            continue
        i = int(mt.group(1))
        tap = taps[i]
        if mt.group(2):
            tap = tap[0] if mt.group(2) == ':x_l' else tap[1]
        elif isinstance(tap, tuple):                          # a layer without a global output: the oracle hands on (x_l, 0)
            assert not torch.is_tensor(tap[1])
            tap = tap[0]
        assert tuple(tap.shape) == tuple(r.shape), r.name
        want = float(tap.abs().max())
        print(f'{r.name}: abs_max {r.abs_max:.6g} oracle {want:.6g} diff {abs(r.abs_max - want):.3g}')
        assert abs(r.abs_max - want) <= 1e-3, (r.name, r.abs_max, want)      # the bar the layer-by-layer test holds these tensors to
        seen.add(i)
    # every launching layer of generator.model: stem, three downsamplings, two blocks, three (convT + BN + ReLU), head + sigmoid
    assert seen == {1, 2, 3, 4, 5, 6, 10, 13, 16, 19}, sorted(seen)
    assert rep.first_over() is None
    assert float((rep.output.cpu() - ref).abs().max()) < 1e-3
    R.check_rows_against_reference(rep)
    assert gen.precision == L.PREC_F16X3 and len(gen._plans) == 0


def test_probe_spectrum_row_is_the_rfft2_of_x1(small):
    """The fu:spectrum row (through lama_fourier_unit_workspace_views) against torch.fft.rfft2 in fp64 of the kept x1.  Bar: what
    tests/test_kernels_gpu.py::test_rfft2_irfft2 holds lama_rfft2_fwd to at planes up to 128 -- atol 3e-5, rtol 1e-4 on unit-variance input.
    The transform is linear, so its absolute error scales with the input: atol = 3e-5 x rms(x1)."""
    gen, x, taps, ref, rep = small
    for blk in ('model.5.conv1', 'model.5.conv2', 'model.6.conv1', 'model.6.conv2'):
        p = blk + '.ffc.convg2g'
        x1 = rep.tensors[p + '.conv1'].double().cpu()
        B, C1, h, w = x1.shape
        ff = torch.fft.rfft2(x1, norm='ortho')
        want = torch.stack((ff.real, ff.imag), 2).reshape(B, 2 * C1, h, w // 2 + 1)
        atol = 3e-5 * float(x1.pow(2).mean().sqrt())
        got = rep.tensors[p + '.fu:spectrum'].double().cpu()
        row = rep[p + '.fu:spectrum']
        err = float((got - want).abs().max())
        print(f'{row.name}: abs_max {row.abs_max:.6g} fp64 {float(want.abs().max()):.6g} max err {err:.3g} atol {atol:.3g}')
        assert tuple(row.shape) == tuple(want.shape)
        assert torch.allclose(got, want, atol=atol, rtol=1e-4), err
        assert abs(row.abs_max - float(want.abs().max())) <= atol + 1e-4 * float(want.abs().max())
        # the DC term is what grows with sqrt(h w): the row's maximum sits in a Re channel
        assert row.channel % 2 == 0


def test_probe_names_the_poisoned_layer():
    """model.7.conv1.bn_l.weight x 1e6.  (model.7 is a resnet block from three blocks on -- model.5, 6, 7 behind three downsamplings; in a
    two-block generator model.7 is the ConcatTupleLayer -- so this generator has three.)"""
    cfg = O.small_config(ngf=8, n_blocks=3)
    sd = O.make_synthetic_state_dict(cfg, seed=7, calib_hw=32)
    sd = {k: (v * 1e6 if k == 'model.7.conv1.bn_l.weight' else v) for k, v in sd.items()}
    gen = make_generator(None, kind='ffc_resnet', **cfg)
    gen.load_state_dict(sd, strict=True)
    gen = gen.cuda()
    batch = O.make_synthetic_batch(1, 128, 128, seed=4)
    x = torch.cat([batch['image'] * (1 - batch['mask']), batch['mask']], 1).to(DEV)
    rep = probe_ranges(gen, x)
    first = rep.first_over()
    print(rep.format(rep.worst(5)))
    assert first is not None and re.match(r'model\.7(\.|:|$)', first.name), first
    names = rep.names()
    assert all(not r.bad for r in rep.rows[:names.index(first.name)])
    assert rep['model.7.conv1:x_l'].n_over > 0 and rep['model.6:x_l'].bad == 0 and rep['model.6:x_g'].bad == 0
    assert gen.precision == L.PREC_F16X3
