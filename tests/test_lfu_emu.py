"""CPU tests of the local Fourier unit (enable_lfu=True): lama_amd/csrc/lfu.hip and the host wiring through the host SIMT emulator,
against the torch restatement of the kernels and tests/golden/lfu.npz (the reference's own classes, make_golden_lfu.py).  The checks are
tests/lfu_util.py's, shared with the GPU twin tests/test_lfu_gpu.py, which adds the 512-channel block at the production routes, graph replay, the
predict CLI and the two larger generator inputs under every precision (an emulated forward of those takes half a minute)."""
import pytest
import torch

from lama_amd import ffc as F
from tests import lfu_util as U
from tests.emu import emu_lib

DEV = torch.device('cpu')


def _prepare(m):
    return m.set_exec(F._Exec(emu_lib()))


@pytest.fixture(scope='module')
def small():
    return U.small_generator(_prepare)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['f32', 'f16'])
@pytest.mark.parametrize('B,C,h,layout', U.KERNEL_SHAPES, ids=['2x8x6-scalar', '1x16x8-slice', '3x8x64-wide', '1x4x130'])
def test_kernels_bit_for_bit(B, C, h, layout, dtype):
    U.check_kernels(emu_lib(), DEV, B, C, h, layout, dtype)


def test_kernel_refusals_leave_the_outputs_alone():
    U.check_refusals(emu_lib(), DEV)


@pytest.mark.parametrize('prec', list(U.PRECS), ids=list(U.PRECS))
def test_units_match_reference_goldens(prec):
    U.check_units(_prepare, DEV, U.PRECS[prec])


# (every precision on the smallest input; the emulated 80 x 80 and 96 x 96 forwards -- 5 x 5 and 6 x 6 LFU planes -- under the default one)
@pytest.mark.parametrize('case,prec', [('a', 'f32'), ('a', 'bf16x3'), ('a', 'f16x3'), ('b', 'f16x3'), ('c', 'f16x3')])
def test_small_generator_matches_reference_golden(small, case, prec):
    gen, sd, g = small
    U.check_generator_golden(gen, g, DEV, U.PRECS[prec], case)


def test_small_generator_plans_keys_and_refused_plane(small):
    gen, sd, g = small
    U.check_generator_plans(gen, sd, DEV, graph=False)       # (no graph capture on the emulator: eager and the split plan)


def test_probe_rows_and_refusals(small):
    gen, sd, g = small
    U.check_probe_and_refusals(gen, DEV)
