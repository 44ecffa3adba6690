"""GPU tests of ``lama_conv2d_fwd`` with ``pad_mode = LAMA_PAD_ZERO`` on non-transposed convolutions on the MI355X (run with -m gpu, -s prints
the worst ring / interior error of every case): the cases and assertions of tests/test_conv_zero_pad_emu.py -- the two 512 -> 512 cases the emulator
leaves out included -- through the production library (``L.get_lib()``), device tensors, one process, every launch on
``torch.cuda.current_stream()``.

Reference, guards, bars and the exact tap count: see tests/test_conv_zero_pad_emu.py.

Measured on the MI355X, worst case of the table per precision (bar = CONV_TOL, atol + rtol |ref|; fp16 I/O: 2e-3 max(1, max |ref|)):
  f32     ring 5.4e-6, interior 9.0e-6   (at most 0.027 of the bar)
  bf16x3  ring 2.3e-5, interior 2.6e-5   (at most 0.035 of the bar)
  f16x3   ring 4.2e-6, interior 4.6e-6   (at most 0.022 of the bar)
  f16     ring 1.9e-3, interior 1.9e-3   (at most 0.16 of the bar: half a unit in the last place of fp16 outputs in [4, 8))
In no precision is the ring worse than the interior; every tap count is exact."""
import pytest
import torch

from lama_amd import _lib as L
from tests import test_conv_zero_pad_emu as E

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return L.get_lib()          # raises if liblama_hip.so was not built: no fallback


@pytest.mark.parametrize('prec', E.ZP_PRECS, ids=E.ZP_PREC_IDS)
@pytest.mark.parametrize('case', E.ZP_CASES, ids=E.ZP_ID)
def test_zero_pad_conv(lib, case, prec):
    """lib.conv2d( ..., L.PAD_ZERO, False, ...) against float64, ring and interior: E.check_zero_pad_conv.
    Measured on the MI355X (worst ring / interior |y - ref| over the cases): f32 5.4e-6 / 9.0e-6, bf16x3 2.3e-5 / 2.6e-5, f16x3 4.2e-6 / 4.6e-6;
    none above 0.035 of its CONV_TOL bar."""
    E.check_zero_pad_conv(lib, case, prec, DEV)


@pytest.mark.parametrize('prec', E.ZP_PRECS, ids=E.ZP_PREC_IDS)
@pytest.mark.parametrize('case', E.ZP_CASES, ids=E.ZP_ID)
def test_tap_count(lib, case, prec):
    """x = 1, w = 1: cin * (taps inside the plane) at every output pixel, exactly: E.check_tap_count."""
    E.check_tap_count(lib, case, prec, DEV)


@pytest.mark.parametrize('case', E.ZP_F16_CASES, ids=E.ZP_ID)
def test_zero_pad_conv_fp16_io(lib, case):
    """fp16 tensors (PREC_F16) through the same two checks; a refusal is a failure.
    Measured on the MI355X: ring 1.9e-3, interior 1.9e-3 (0.16 of the bar) in both cases."""
    E.check_zero_pad_conv(lib, case, L.PREC_F16, DEV)
    E.check_tap_count(lib, case, L.PREC_F16, DEV)


def test_zero_pad_geometry(lib):
    """pad >= H runs under PAD_ZERO and is ERR_BAD_ARG under PAD_REFLECT; a one-row-short output view is ERR_BAD_ARG: E.check_zero_pad_geometry."""
    E.check_zero_pad_geometry(lib, DEV)
