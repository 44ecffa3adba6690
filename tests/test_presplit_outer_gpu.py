"""LAMA_DT_SPLIT16 -- stem and stride-2 outputs stored pre-split in staging order (include/lama_hip.h) -- on the MI355X (run with
-m gpu): the checks of tests/test_presplit_outer_emu.py (shared: tests/presplit_outer_util.py) through the production library where production
itself takes the dedicated kernels, and through the profiling build with the stem kernel forced (LAMA_STEM_WS=2, tests/emu.py) at the small
shapes.  No tolerance anywhere; every successful launch with a split tensor is one of the two dedicated kernels (there is no fallback)."""
import pytest
import torch

from lama_amd import _lib as L
from lama_amd import ffc as F
from tests import presplit_outer_util as U
from tests.test_kernels_gpu import lib, lib_forced  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
PREC = pytest.mark.parametrize('prec', U.PRECS, ids=lambda p: U.PREC_ID[p])


@pytest.fixture(scope='module')
def ex_forced(lib_forced):      # noqa: F811
    return lambda: F._Exec(lib_forced)


# ---- 1. layout -----------------------------------------------------------------------------------------------------------------------------------
@PREC
@pytest.mark.parametrize('shape', [(2, 32, 64), (1, 48, 96)], ids=lambda s: 'x'.join(map(str, s)))
def test_stem_split_layout(lib_forced, shape, prec):      # noqa: F811
    U.check_stem_layout(lib_forced, DEV, shape, prec)


@PREC
def test_stem_split_layout_production(lib, prec):      # noqa: F811
    """2 x 64 x 1024: the smallest launch production routes to the stem kernel (4096 row segments)."""
    U.check_stem_layout(lib, DEV, (2, 64, 1024), prec)


# ---- 2. chain identity -----------------------------------------------------------------------------------------------------------------------------
@PREC
def test_chain_identity(lib_forced, prec):      # noqa: F811
    """2 x 4 x 64 x 96 through 64 / 128 / 256 / 512 channels: the third conv works on a 16 x 24 plane."""
    U.check_chain(lib_forced, DEV, prec, B=2, H=64, W=96)


@PREC
@pytest.mark.parametrize('pad_mode', [L.PAD_REFLECT, L.PAD_ZERO], ids=['reflect', 'zero'])
def test_down1_odd_plane(lib, pad_mode, prec):      # noqa: F811
    U.check_down_alone(lib, DEV, prec, 64, 128, 35, 50, pad_mode)


@PREC
@pytest.mark.parametrize('pad_mode', [L.PAD_REFLECT, L.PAD_ZERO], ids=['reflect', 'zero'])
@pytest.mark.parametrize('cin,cout,hw,y_split', [(64, 128, (13, 22), True), (128, 256, (10, 36), True), (256, 512, (9, 14), False),
                                                 (64, 128, (70, 130), True)])
def test_each_down_alone(lib, cin, cout, hw, y_split, pad_mode, prec):      # noqa: F811
    """(the last case: several tiles in both directions, more workgroups than one round of two per CU would hide an ordering fault in)"""
    U.check_down_alone(lib, DEV, prec, cin, cout, hw[0], hw[1], pad_mode, y_split=y_split, B=2 if hw[0] == 70 else 1)


# ---- 3. range flag ---------------------------------------------------------------------------------------------------------------------------------
def test_range_just_under_the_limit(lib_forced):      # noqa: F811
    v = 65504.0 * (1 - 2.0 ** -12)
    got, flag = U.stem_one_element(lib_forced, DEV, L.PREC_F16X3, 10, 40, 1.0, v)
    assert got == v and flag == 0


def test_range_over_the_limit_in_the_last_pixel_of_a_ragged_tile(lib_forced):      # noqa: F811
    _, flag = U.stem_one_element(lib_forced, DEV, L.PREC_F16X3, 10, 40, 2.0, 35000.0)
    assert flag == 1


def test_range_nan_in_the_image(lib_forced):      # noqa: F811
    _, flag = U.stem_one_element(lib_forced, DEV, L.PREC_F16X3, 10, 40, 1.0, 1.0, nan_input=True)
    assert flag == 1


def test_range_ragged_tile_lanes_outside_the_plane_are_not_watched(lib):      # noqa: F811
    ys, flag = U.ragged_tile_case(lib, DEV, L.PREC_F16X3, big_row=11)
    assert flag == 0
    hi, lo = L.split16_unpack(ys, L.PREC_F16X3)
    assert float(hi.float().abs().max()) == 0.0 and float(lo.float().abs().max()) == 0.0
    _, flag = U.ragged_tile_case(lib, DEV, L.PREC_F16X3, big_row=9)       # the control: the same value inside the plane
    assert flag == 1


def test_range_bf16x3_never_raises(lib, lib_forced):      # noqa: F811
    got, flag = U.stem_one_element(lib_forced, DEV, L.PREC_BF16X3, 10, 40, 2.0, 35000.0)
    assert flag == 0 and got == 70000.0
    _, flag = U.ragged_tile_case(lib, DEV, L.PREC_BF16X3, big_row=9)
    assert flag == 0


def test_generator_falls_back_like_the_fp32_plan(ex_forced):
    U.check_generator_fallback(ex_forced, DEV)


# ---- 4. generator identity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('shape,split_batch', [((2, 64, 96), None), ((2, 64, 96), 2), ((1, 96, 64), None)],
                         ids=['2x64x96', '2x64x96-two-parts', '1x96x64'])
def test_generator_identity(ex_forced, shape, split_batch, graph):
    U.check_generator_identity(ex_forced, DEV, shape, graph=graph, split_batch=split_batch)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(lib):      # noqa: F811
    U.check_refusals(lib, DEV)
