"""GPU tests of the fp16 range watch on the MI355X (run with -m gpu; -s prints one line per launch: family, shape, precision, position, value,
flag, err / bar): the check functions of tests/range_watch_util.py, as tests/test_range_watch_emu.py runs them on the emulator -- here on every
row of CONV_CASES in the full plan, through the production library and the forced profiling build, plus what is too large for the emulator:
  * the specialised families at the smallest shapes production itself routes to them (PROD_SHAPES of tests/test_split_exact_gpu.py): the clean
    baseline and 7e4 at the first and the last position, the family asserted through the route query (PROD_FAM).  Every input position of a stride-1 'same' convolution is read by an output, so the
    float64 reference is computed once per shape, for the clean input only; the operands are not kept;
  * a NaN in x_l of a stand-alone FFC layer whose local conv takes the Winograd route (the kernel is blind to it by contract; the global-branch
    launch of the same layer raises the exec's flag);
  * LPIPS.auto_fallback and InceptionV3.auto_fallback.
The collected lines of a run: profiles/range_watch.txt."""
import pytest
import torch

from lama_amd import _lib as L
from tests import range_watch_util as R
from tests import test_conv_zero_pad_emu as Z
from tests import test_split_exact_emu as E
from tests.test_kernels_emu import CONV_CASES, WINO_CASES, WINO_ID, WINO_ZERO_CASES
from tests.test_kernels_gpu import anylib, lib, lib_forced  # noqa: F401  (fixtures)
from tests.test_split_exact_gpu import PROD_SHAPES, _prod_case

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# the family production takes at each PROD_SHAPES entry (the comments of THRESHOLD_SHAPES and test_conv2d_big_tiles in tests/test_kernels_gpu.py),
# asserted through the route query before the first launch
PROD_FAM = [L.CONV_FAM_GEMM1X1_WS, L.CONV_FAM_GEMM1X1_WS, L.CONV_FAM_CONV_WR, L.CONV_FAM_CONV_WR, L.CONV_FAM_STEM7, L.CONV_FAM_HEAD7,
            L.CONV_FAM_GEMM1X1_WS, L.CONV_FAM_GEMM1X1_W4, L.CONV_FAM_GEMM1X1_W4, L.CONV_FAM_GEMM1X1_WK, L.CONV_FAM_GEMM1X1_WK, L.CONV_FAM_GEMM1X1_W4]
PRECS = [L.PREC_F16X3, L.PREC_BF16X3]
PREC_IDS = ['f16x3', 'bf16x3']


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('case', CONV_CASES, ids=E.CONV_ID)
def test_conv2d_range_watch(anylib, lib_forced, case, prec, monkeypatch):
    E.force_env(case, monkeypatch)
    R.check_conv(anylib, case, prec, DEV, production=anylib is not lib_forced)


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('case', R.SINGLE_UNIT_CASES, ids=E.CONV_ID)
def test_conv2d_single_unit_range_watch(lib_forced, case, prec, monkeypatch):
    """One unit per workgroup of the three output-side watchers: forced build (production takes none of them at 32 pixels)."""
    E.force_env(case, monkeypatch)
    R.check_conv(lib_forced, case, prec, DEV)


@pytest.mark.parametrize('shape', PROD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_conv2d_range_watch_production_routes(lib, shape):
    case = dict(_prod_case(shape), fam=PROD_FAM[PROD_SHAPES.index(shape)])
    o = R._make_conv_operands(case, 9900 + sum(shape))
    R.check_conv(lib, case, L.PREC_F16X3, DEV, production=True, names=('first', 'last'), family='conv2d-production', operands=o, assert_read=False)


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('case', E.FUSED_CASES, ids=E.FUSED_ID)
def test_fused_second_operand_range_watch(anylib, case, prec):
    R.check_fused_second_operand(anylib, case, prec, DEV)


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('spot', [0, 1], ids=['first', 'last'])
def test_fuse1_range_watch(lib_forced, spot, prec):
    """Forced build, as tests/test_split_exact_gpu.py::test_fuse1_split_exact: the 9 x 37 plane is below production's size for the 12-wave workgroup."""
    R.check_fuse1(lib_forced, spot, prec, DEV)


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('spot', [0, 1], ids=R.SPLIT16_SPOTS)
@pytest.mark.parametrize('name', list(R.SPLIT16_CASES))
def test_split16_writer_range_watch(lib_forced, name, spot, prec):
    R.check_split16_writer(lib_forced, name, spot, prec, DEV)


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('case', WINO_CASES, ids=WINO_ID)
def test_winograd_range_watch(lib, lib_forced, case, prec, monkeypatch):
    E.force_env(case, monkeypatch)
    R.check_winograd(lib_forced if case.get('qr') else lib, case, prec, DEV)


@pytest.mark.parametrize('case', WINO_ZERO_CASES, ids=WINO_ID)
def test_winograd_zero_pad_range_watch(lib, case):
    R.check_winograd(lib, case, L.PREC_F16X3, DEV, pad_mode=L.PAD_ZERO)


@pytest.mark.parametrize('case', WINO_CASES, ids=WINO_ID)
def test_winograd_transformed_overflow(lib, lib_forced, case, monkeypatch):
    E.force_env(case, monkeypatch)
    R.check_winograd_transformed_overflow(lib_forced if case.get('qr') else lib, case, DEV)


def test_ffc_layer_on_the_winograd_route_reports_nan(lib):
    R.check_ffc_layer_nan(lib, DEV)


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('case', E.MD_CASES, ids=E.MD_ID)
def test_multidilated_range_watch(lib, case, prec):
    R.check_multidilated(lib, case, prec, DEV)


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('case', list(E.FE.RECT_CASES))
def test_rect_range_watch(lib, case, prec):
    R.check_rect(lib, case, prec, DEV)


@pytest.mark.parametrize('case', Z.ZP_F16_CASES, ids=Z.ZP_ID)
def test_f16_io_range_watch(lib, case):
    R.check_f16_io(lib, case, DEV)


@pytest.mark.parametrize('prec', PRECS, ids=PREC_IDS)
@pytest.mark.parametrize('hw', R.FU_PLANES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_fourier_unit_range_watch(lib, hw, prec):
    R.check_fft_families_differ(lib)
    R.check_fourier_unit(lib, hw, prec, DEV)


def test_lpips_auto_fallback(lib):
    R.check_lpips_fallback(DEV)


def test_inception_auto_fallback(lib):
    R.check_inception_fallback(DEV)


def test_worst_ratios_printed():
    """Not a check: the worst err / bar per family and precision of the launches above (every one of them was asserted <= 1 where it ran)."""
    for (family, prec), r in sorted(R.Worst.seen.items()):
        print(f'[range-watch] worst {family} {prec} err/bar={r:.4f}')
