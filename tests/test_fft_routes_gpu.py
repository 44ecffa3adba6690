"""GPU tests of the FFT routes no other test reaches, on the MI355X (run with -m gpu; -s prints one line per check: route from the query, shape,
dtype, view variant, max error forward / inverse with residual / inverse without): the checks of tests/test_fft_routes_emu.py on the device --
the alignment fallbacks of the plane-in-LDS family, the separable DFT in production routing and forced, fp16 I/O of the two-launch
mixed-radix form, the DFT and the two-pass kernels on a non-square plane, irfft2 without a residual everywhere, and the refusals.

Every case asserts its route by ``lama_fft_route_query`` on the loaded library for the views it built, then compares with float64 numpy.fft at
the bars of tests/fft_route_util.py inside sentinel-guarded buffers.  Cases without an environment switch run through the product library,
the LAMA_FFT_MR cases through the profiling build.  The collected lines of a run: profiles/fft_routes.txt."""
import pytest

from tests import fft_route_util as U
from tests import test_fft_routes_emu as E
from tests.test_kernels_gpu import lib, lib_forced  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.mark.parametrize('case', E.ALIGN_F32 + E.ALIGN_F16, ids=E.case_id)
def test_alignment_variants(lib, case):
    E.run_case(lib, DEV, case)


@pytest.mark.parametrize('case', E.DFT_PRODUCTION, ids=E.case_id)
def test_dft_in_production_routing(lib, case):
    E.run_case(lib, DEV, case)


@pytest.mark.parametrize('case', E.DFT_FORCED, ids=E.case_id)
def test_dft_forced(lib_forced, case, monkeypatch):
    monkeypatch.setenv('LAMA_FFT_MR', '0')
    E.run_case(lib_forced, DEV, case, ' LAMA_FFT_MR=0')


@pytest.mark.parametrize('case', E.MR2_FORCED, ids=E.case_id)
def test_two_launch_mixed_radix_fp16(lib_forced, case, monkeypatch):
    monkeypatch.setenv('LAMA_FFT_MR', '2')
    E.run_case(lib_forced, DEV, case, ' LAMA_FFT_MR=2')


@pytest.mark.parametrize('hw', E.REFUSED, ids=lambda s: f'{s[0]}x{s[1]}')
def test_refused_in_both_directions(lib, hw):
    U.check_refused(lib, DEV, *hw)


def test_fourier_unit_refused_before_its_first_launch(lib):
    U.check_fourier_unit_refused(lib, DEV)
