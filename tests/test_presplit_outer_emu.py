"""LAMA_DT_SPLIT16 -- stem and stride-2 outputs stored pre-split in staging order (include/lama_hip.h) -- on the host emulator: the
kernel sources compiled for x86 (tests/hipemu), the shapes small.  The checks are those of tests/test_presplit_outer_gpu.py (shared:
tests/presplit_outer_util.py); no tolerance anywhere, and every successful launch with a split tensor is one of the two dedicated kernels (there
is no fallback behind them).

  1. layout: the stem's split output holds rne16(y) / rne16(y - hi) of its fp32 run bit for bit, every byte written, none behind the tensor;
  2. chain: stem -> down1 -> down2 -> down3 with split intermediates equals the fp32 chain; each stride-2 conv alone on host-packed tensors
     (odd plane, reflect and zero padding, fp32 and split output);
  3. range flag: raised by the PRODUCER for what it stores and nothing else;
  4. generator: presplit_outer on against off, eager and split plans, fallback to bf16x3;
  5. refusals."""
import pytest
import torch

from lama_amd import _lib as L
from lama_amd import ffc as F
from tests import presplit_outer_util as U
from tests.emu import emu_lib

DEV = 'cpu'
PREC = pytest.mark.parametrize('prec', U.PRECS, ids=lambda p: U.PREC_ID[p])


def _ex():
    return F._Exec(emu_lib())


# ---- 1. layout -----------------------------------------------------------------------------------------------------------------------------------
@PREC
@pytest.mark.parametrize('shape', [(2, 32, 64), (1, 48, 96)], ids=lambda s: 'x'.join(map(str, s)))
def test_stem_split_layout(shape, prec):
    U.check_stem_layout(emu_lib(), DEV, shape, prec)


# ---- 2. chain identity -----------------------------------------------------------------------------------------------------------------------------
@PREC
def test_chain_identity(prec):
    """1 x 4 x 32 x 48 through 64 / 128 / 256 / 512 channels: the third conv works on an 8 x 12 plane (ragged 8 x 16 tiles, reflection on all four
    borders inside one tile); the GPU twin runs 2 x 64 x 96."""
    U.check_chain(emu_lib(), DEV, prec, B=1, H=32, W=48)


@PREC
@pytest.mark.parametrize('pad_mode', [L.PAD_REFLECT, L.PAD_ZERO], ids=['reflect', 'zero'])
def test_down1_odd_plane(pad_mode, prec):
    """1 x 64 x 35 x 50, packed on the host: reflection at an odd edge, the last parity column."""
    U.check_down_alone(emu_lib(), DEV, prec, 64, 128, 35, 50, pad_mode)


@PREC
@pytest.mark.parametrize('pad_mode', [L.PAD_REFLECT, L.PAD_ZERO], ids=['reflect', 'zero'])
@pytest.mark.parametrize('cin,cout,hw,y_split', [(64, 128, (13, 22), True), (128, 256, (10, 36), True), (256, 512, (9, 14), False)])
def test_each_down_alone(cin, cout, hw, y_split, pad_mode, prec):
    U.check_down_alone(emu_lib(), DEV, prec, cin, cout, hw[0], hw[1], pad_mode, y_split=y_split)


# ---- 3. range flag ---------------------------------------------------------------------------------------------------------------------------------
def test_range_just_under_the_limit():
    v = 65504.0 * (1 - 2.0 ** -12)
    got, flag = U.stem_one_element(emu_lib(), DEV, L.PREC_F16X3, 10, 40, 1.0, v)
    assert got == v and flag == 0


def test_range_over_the_limit_in_the_last_pixel_of_a_ragged_tile():
    """2 x 35 000 = 7 x 10^4 from operands inside the range, in pixel (9, 39) of a 10 x 40 plane: the last lane the ragged second segment stores."""
    _, flag = U.stem_one_element(emu_lib(), DEV, L.PREC_F16X3, 10, 40, 2.0, 35000.0)
    assert flag == 1


def test_range_nan_in_the_image():
    _, flag = U.stem_one_element(emu_lib(), DEV, L.PREC_F16X3, 10, 40, 1.0, 1.0, nan_input=True)
    assert flag == 1


def test_range_ragged_tile_lanes_outside_the_plane_are_not_watched():
    ys, flag = U.ragged_tile_case(emu_lib(), DEV, L.PREC_F16X3, big_row=11)
    assert flag == 0
    hi, lo = L.split16_unpack(ys, L.PREC_F16X3)
    assert float(hi.float().abs().max()) == 0.0 and float(lo.float().abs().max()) == 0.0
    _, flag = U.ragged_tile_case(emu_lib(), DEV, L.PREC_F16X3, big_row=9)       # the control: the same value inside the plane
    assert flag == 1


def test_range_bf16x3_never_raises():
    got, flag = U.stem_one_element(emu_lib(), DEV, L.PREC_BF16X3, 10, 40, 2.0, 35000.0)
    assert flag == 0 and got == 70000.0
    _, flag = U.ragged_tile_case(emu_lib(), DEV, L.PREC_BF16X3, big_row=9)
    assert flag == 0


def test_generator_falls_back_like_the_fp32_plan():
    U.check_generator_fallback(_ex, DEV, head_only=True)


# ---- 4. generator identity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,split_batch', [((1, 32, 64), None), ((2, 16, 64), 2)], ids=['1x32x64', '2x16x64-two-parts'])
def test_generator_identity(shape, split_batch):
    """The plan builder's host logic on the plan of the generator's head (pad, stem, down1, down2 -> the fp32 state; a 64-channel residual block
    takes the emulator minutes): split edges, the cached plan, a forced two-part plan.  The whole generator at 2 x 64 x 96 and 1 x 96 x 64, the u8
    outputs and graph replay run on the GPU: tests/test_presplit_outer_gpu.py."""
    U.check_generator_identity(_ex, DEV, shape, split_batch=split_batch, reps=1, head_only=True)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    U.check_refusals(emu_lib(), DEV)
