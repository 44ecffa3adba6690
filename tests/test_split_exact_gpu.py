"""GPU tests of the 3-term split of every conv kernel family on the MI355X, bit for bit (run with -m gpu; -s prints one line per check: family,
shape, precision, form, outputs compared): the checks of tests/test_split_exact_emu.py -- operands on which the split convolution is exact, compared
with the float64 reference by ``torch.equal`` -- through the production library and the forced profiling build, as ``test_conv2d`` of
tests/test_kernels_gpu.py runs them, and once per specialised family on the production library at the smallest shape that production itself
routes there (the "on" rows of THRESHOLD_SHAPES and the K = 384 rows of ``test_conv2d_big_tiles``; nnz and grid re-derived by the builder for the
larger K).

Operands, exactness conditions and where each is asserted: tests/split_exact_util.py; guards, range_flag and the report of a mismatch:
tests/test_split_exact_emu.py.  No tolerance anywhere.  The collected lines of a run: profiles/split_exact.txt.

``test_f16_subnormal_lo_recorded`` is a measurement, not a bar: form A scaled by 2^-8 puts every lo word of the f16 split below 2^-14 (fp16
subnormals); it prints how many outputs stay exact and asserts finiteness only.

Measured on the MI355X (profiles/split_exact.txt): all 1446 checks equal in every family, precision and form, 65 s for the module; the subnormal
measurement: every output exact on both kernels (fp16-subnormal lo words are kept)."""
import pytest
import torch

from lama_amd import _lib as L
from tests import test_split_exact_emu as E
from tests.test_kernels_emu import CONV_CASES
from tests.test_kernels_gpu import THRESHOLD_SHAPES, anylib, lib, lib_forced  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SPLIT_FORMS = [pf for pf in E.PREC_FORMS if pf[0] != L.PREC_F32]

# (B, cin, cout, k, H, W): the production selection's own thresholds -- the "on" rows of THRESHOLD_SHAPES (persistent GEMM with 1 / 2 row groups,
# full-M 1x1 workgroups whole and ragged, stem, head) and the K = 384 rows of test_conv2d_big_tiles (persistent GEMM, its w4 and wk forms)
PROD_SHAPES = [THRESHOLD_SHAPES[i] for i in (0, 2, 4, 5, 8, 10)] + [(1, 384, 192, 1, 64, 64), (4, 384, 192, 1, 64, 64), (6, 384, 384, 1, 64, 33),
                                                                   (8, 384, 384, 1, 64, 33), (2, 384, 384, 1, 128, 65), (4, 384, 384, 1, 128, 65)]
assert PROD_SHAPES[:6] == [(2, 192, 96, 1, 32, 32), (1, 384, 192, 1, 32, 32), (3, 128, 384, 1, 64, 64), (2, 128, 384, 1, 64, 95),
                           (2, 4, 64, 7, 64, 1024), (2, 64, 3, 7, 256, 416)]


def _prod_case(shape):
    B, cin, cout, k, H, W = shape
    return dict(B=B, cin=cin, cout=cout, k=k, stride=1, pad=k // 2, H=H, W=W, act=L.ACT_RELU, bias=True, resid=False, scale=False)


@pytest.mark.parametrize('pf', E.PREC_FORMS, ids=E.PF_ID)
@pytest.mark.parametrize('case', CONV_CASES, ids=E.CONV_ID)
def test_conv2d_split_exact(anylib, case, pf, monkeypatch):
    """Every geometry of CONV_CASES, production and forced build: E.check_conv."""
    E.force_env(case, monkeypatch)
    E.check_conv(anylib, case, pf[0], pf[1], DEV)


@pytest.mark.parametrize('pf', SPLIT_FORMS, ids=E.PF_ID)
@pytest.mark.parametrize('shape', PROD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_conv2d_split_exact_production_routes(lib, shape, pf):
    """The specialised families at the smallest shapes production routes to them.  The operands are not kept (up to 150 MB a case)."""
    case = _prod_case(shape)
    o = E._conv_operands.__wrapped__(tuple(sorted(case.items())), pf[0], pf[1], 1.0)
    ybuf, flag = E.run_conv(lib, case, pf[0], o, DEV)
    n = E.assert_exact(ybuf, flag, o.ref, f'{E.CONV_ID(case)} {E.PREC_NAME[pf[0]]} form {pf[1]} (nnz {o.nnz}, grid {o.q})')
    E.report(DEV, 'conv2d-production', 'x'.join(map(str, shape)), pf[0], pf[1], n)


@pytest.mark.parametrize('pf', E.FUSED_FORMS, ids=E.PF_ID)
@pytest.mark.parametrize('case', E.FUSED_CASES, ids=E.FUSED_ID)
def test_fused_second_operand_split_exact(anylib, case, pf):
    E.check_fused_second_operand(anylib, case, pf[0], pf[1], DEV)


@pytest.mark.parametrize('prec', [L.PREC_BF16X3, L.PREC_F16X3], ids=['bf16x3', 'f16x3'])
def test_fuse1_split_exact(lib_forced, prec):
    """The ragged 9 x 37 plane is below the launch size from which production takes the 12-wave workgroup that carries conv1: the profiling build
    with LAMA_CW_G12=2 (tests/emu.py), as the ragged case of test_conv2d_fused_next_conv1."""
    E.check_fuse1(lib_forced, prec, DEV)


@pytest.mark.parametrize('pf', E.PREC_FORMS, ids=E.PF_ID)
@pytest.mark.parametrize('case', E.MD_CASES, ids=E.MD_ID)
def test_multidilated_split_exact(lib, case, pf):
    E.check_multidilated(lib, case, pf[0], pf[1], DEV)


@pytest.mark.parametrize('pf', E.RECT_FORMS, ids=E.PF_ID)
@pytest.mark.parametrize('case', list(E.FE.RECT_CASES))
def test_rect_split_exact(lib, case, pf):
    E.check_rect(lib, case, pf[0], pf[1], DEV)


@pytest.mark.parametrize('pf', E.WINO_FORMS, ids=E.PF_ID)
@pytest.mark.parametrize('case', E.WINO_CASES, ids=E.KE.WINO_ID)
def test_winograd_split_exact(lib, lib_forced, case, pf, monkeypatch):
    E.force_env(case, monkeypatch)
    E.check_winograd(lib_forced if case.get('qr') else lib, case, pf[0], pf[1], DEV)      # LAMA_WG_QR is a switch of the profiling build


SUBNORMAL_CASES = [next(c for c in CONV_CASES if (c['k'], c['cin'], c['cout']) == (1, 128, 100)),       # flat 1x1, weights in registers
                   next(c for c in CONV_CASES if (c['k'], c['cin'], c['cout'], c['stride']) == (3, 64, 130, 1))]


@pytest.mark.parametrize('case', SUBNORMAL_CASES, ids=E.CONV_ID)
def test_f16_subnormal_lo_recorded(lib, case):
    """RECORDED, NOT ASSERTED: form A times 2^-8, x = +-2^-8 (1 + m 2^-14): hi = +-2^-8, lo = +-m 2^-22, an fp16 subnormal.  Everything else of the
    exact construction holds (the scaling is by a power of two), so an output differs from the float64 reference only if a subnormal lo word is
    lost on its way through the conversion or the MFMA.  Prints the exact outputs and the worst error in units of 2^-22 |ref|."""
    o = E.conv_operands(case, L.PREC_F16X3, 'A', x_scale=2.0 ** -8)
    ybuf, flag = E.run_conv(lib, case, L.PREC_F16X3, o, DEV)
    y = ybuf[:, E.PRE:E.PRE + case['cout']].cpu().double()
    assert bool(torch.isfinite(y).all())
    nz = o.ref != 0
    rel = ((y - o.ref).abs()[nz] / o.ref.abs()[nz]).max() * 2.0 ** 22 if bool(nz.any()) else torch.zeros(())
    print(f'[split-exact] subnormal-lo {E.CONV_ID(case)} f16x3 form A x 2^-8: {int((y == o.ref).sum())} of {y.numel()} outputs exact, '
          f'worst error {float(rel):.3f} x 2^-22 |ref|, worst absolute {float((y - o.ref).abs().max()):.3e}, range_flag {int(flag)}')
