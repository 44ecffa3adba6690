"""GPU tests of the glue kernels on the MI355X (run with -m gpu, -s prints the matched contraction variants, the sigmoid / tanh unit and ratio
and the SSIM errors): the cases and assertions of tests/test_glue_kernels_emu.py through the production library (``L.get_lib()``), device
tensors, one process, every launch on ``torch.cuda.current_stream()``.

Entries reached here by name: lib.mask_compose_u8 / lib.blend_quantize_u8 (the first and last launch of every production predict step),
lib.mask_compose / lib.blend / lib.quantize_u8_hwc on channel-slice views and past the 2048-workgroup cap, lib.affine_act / lib.reflect_pad
(the stand-alone layers of lama_amd/ffc.py), lib.ssim on ragged planes, strided views, every window size and more than 256 tiles per image,
and the deferred Winograd output transform: winograd_conv3x3(defer_out=True) + lib.winograd_out / lib.rfft2_wino_out, lib.fourier_unit with
wino_out (lama_fourier_unit_winograd_out_fwd / lama_fourier_unit_ex_fwd with wino_args), winograd_conv3x3(pad_mode=L.PAD_ZERO).

Tolerances: see tests/test_glue_kernels_emu.py -- bit-equality, one legal contraction, 4 units for sigmoid / tanh, 2e-6 for SSIM."""
import pytest
import torch

from lama_amd import _lib as L
from tests import test_glue_kernels_emu as E
from tests import test_kernels_emu as KE

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return L.get_lib()          # raises if liblama_hip.so was not built: no fallback


@pytest.mark.parametrize('binarize', [True, False], ids=['binarize', 'fractional'])
@pytest.mark.parametrize('case', E.U8_CASES, ids=E.U8_IDS)
def test_u8_predict_ends(lib, case, binarize):
    """lib.mask_compose_u8( ... ) / lib.blend_quantize_u8( ... ): E.check_u8_predict_ends."""
    E.check_u8_predict_ends(lib, case, binarize, DEV)


@pytest.mark.parametrize('fractional', [False, True], ids=['binary', 'fractional'])
@pytest.mark.parametrize('case', E.EW_CASES, ids=lambda c: '%dx%dx%d' % c)
def test_elementwise_views(lib, case, fractional):
    E.check_elementwise_views(lib, case, fractional, DEV)


@pytest.mark.parametrize('case', E.AFFINE_CASES, ids=lambda c: 'b%d_c%d_%dx%d_act%d_affine%d' % c)
def test_affine_act(lib, case):
    """lib.affine_act( ... ): E.check_affine_act.
    Measured on the MI355X (bar: 4 units): sigmoid unit 5.4e-8 .. 8.9e-8, worst error 1.000 units in every case; tanh unit 2.76e-8 .. 2.97e-8,
    worst error 1.45 .. 1.83 units.  x * scale + shift compiles to one FMA there ("product fused")."""
    E.check_affine_act(lib, case, DEV)


@pytest.mark.parametrize('case', E.PAD_CASES, ids=lambda c: 'b%d_c%d_%dx%d_pad%d' % c)
def test_reflect_pad(lib, case):
    """lib.reflect_pad( ... ): E.check_reflect_pad."""
    E.check_reflect_pad(lib, case, DEV)


def test_glue_refusals(lib):
    E.check_glue_refusals(lib, DEV)


@pytest.mark.parametrize('case', E.SSIM_CASES, ids=lambda c: 'b%d_c%d_%dx%d_w%d_%s' % c)
def test_ssim(lib, case):
    """lib.ssim( ... ): E.check_ssim."""
    E.check_ssim(lib, case, DEV)


def test_ssim_refusals(lib):
    E.check_ssim_refusals(lib, DEV)


@pytest.mark.parametrize('prec', E.WINO_PRECS, ids=E.WINO_PREC_IDS)
@pytest.mark.parametrize('case', KE.WINO_DEFER_CASES, ids=KE.WINO_ID)
def test_winograd_deferred_out(lib, case, prec):
    """winograd_conv3x3(defer_out=True) + lib.winograd_out( ... ) / lib.rfft2_wino_out( ... ) against the one-call form: the block the
    emulator suite runs inside test_winograd_conv3x3_emulated (KE.check_winograd_deferred_out)."""
    o = KE.wino_operands(lib, case, prec, DEV)
    ybuf = torch.full((o.B, o.cout + 3, o.H, o.W), 7.0, device=DEV)
    KE.wino_run(lib, o, ybuf)
    torch.cuda.synchronize()
    y = ybuf[:, 2:2 + o.cout].cpu()
    assert torch.allclose(y, o.ref, **o.tol), float((y - o.ref).abs().max())
    KE.check_winograd_deferred_out(lib, o, ybuf)


@pytest.mark.parametrize('prec', E.WINO_PRECS, ids=E.WINO_PREC_IDS)
@pytest.mark.parametrize('case', KE.WINO_ZERO_CASES, ids=KE.WINO_ID)
def test_winograd_pad_zero(lib, case, prec):
    """winograd_conv3x3(pad_mode=L.PAD_ZERO), the form the reverse pass uses (KE.check_winograd_pad_zero)."""
    o = KE.wino_operands(lib, case, prec, DEV)
    ybuf = torch.full((o.B, o.cout + 3, o.H, o.W), 7.0, device=DEV)
    KE.check_winograd_pad_zero(lib, o, ybuf)


@pytest.mark.parametrize('n', E.WINO_FU_PLANES)
@pytest.mark.parametrize('prec', E.WINO_PRECS, ids=E.WINO_PREC_IDS)
def test_winograd_deferred_into_fourier_unit(lib, prec, n):
    """lib.fourier_unit( ..., wino_out=(wino_args, workspace)): E.check_winograd_deferred_into_fourier_unit."""
    E.check_winograd_deferred_into_fourier_unit(lib, prec, n, DEV)


# =====================================================================================================================================
# the same entries once more at a production shape, called here directly
# =====================================================================================================================================
def test_u8_predict_ends_production_slot(lib):
    """One production step's worth of slots: 8 x 512 x 512 (2 M pixels: four trips of the grid-stride loop), ragged sizes, one empty slot."""
    B, Hp, Wp = 8, 512, 512
    sizes = [(512, 512), (500, 375), (375, 500), (509, 511), (256, 512), (512, 3), (2, 2), (0, 0)]
    st = torch.cuda.current_stream().cuda_stream
    img, mask, pred, img_f, m = E.u8_case_operands((B, Hp, Wp, sizes), True)
    imgd, maskd, szd = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV)
    obuf = torch.full((B, 7, Hp, Wp), E.SENT, device=DEV)
    lib.mask_compose_u8(imgd, maskd, szd, L.view(obuf, 1, 4), B, True, st)
    got = E._take(obuf, 1, 4, DEV)
    assert E._bits_equal(got, E.GR.compose(img_f, m)), E._first_diff(got, E.GR.compose(img_f, m))
    pbuf, pview = E._wide(torch.from_numpy(pred), 2, 1, DEV, fill=3.0)
    dst = E._u8_out(B * Hp * Wp * 3, DEV)
    lib.blend_quantize_u8(imgd, maskd, szd, pview, dst, B, True, st)
    got8 = E._take_u8(dst, (B, Hp, Wp, 3), DEV)
    want8 = E.GR.quantize_hwc(E.GR.blend_variants(img_f, m, pred)['unfused'])              # a {0, 1} mask: every evaluation is the same
    assert (got8 == want8).all(), E._first_diff(got8, want8)


def test_stand_alone_layers_at_generator_shapes(lib):
    """generator.model[0] (ReflectionPad2d(3) of the 4-channel input) and a BatchNorm2dEval + ReLU over 64 channels, 2 x 256 x 256."""
    st = torch.cuda.current_stream().cuda_stream
    x = torch.randn(2, 4, 256, 256, generator=torch.Generator().manual_seed(1))
    xbuf, xview = E._wide(x, 1, 1, DEV, fill=3.0)
    ybuf = torch.full((2, 7, 262, 262), E.SENT, device=DEV)
    lib.reflect_pad(xview, 3, L.view(ybuf, 2, 4), 2, st)
    got = E._take(ybuf, 2, 4, DEV)
    assert E._bits_equal(got, torch.nn.functional.pad(x, (3,) * 4, mode='reflect').numpy())
    x, scale, shift = E.affine_case_operands((2, 64, 256, 256, L.ACT_RELU, True))
    xbuf, xview = E._wide(torch.from_numpy(x), 1, 1, DEV, fill=3.0)
    ybuf = torch.full((2, 67, 256, 256), E.SENT, device=DEV)
    lib.affine_act(xview, torch.from_numpy(scale).to(DEV), torch.from_numpy(shift).to(DEV), L.ACT_RELU, L.view(ybuf, 2, 64), 2, st)
    got = E._take(ybuf, 2, 64, DEV)
    name = E.GR.match_variant(got, {k: E.np.maximum(v, E.np.float32(0)) for k, v in E.GR.affine_variants(x, scale, shift).items()})
    print(f'[glue] affine_act 2x64x256x256: matched "{name}"')
    assert name is not None


def test_ssim_photo_size_strided(lib):
    """2 x 3 x 500 x 375 (32 x 12 x 3 = 1152 tiles per image) on channel-slice views against the fp64 oracle."""
    B, C, H, W = 2, 3, 500, 375
    a, b = E.ssim_case_operands((B, C, H, W, 11, 'near'))
    abuf, aview = E._wide(a, 1, 1, DEV, fill=0.5)
    bbuf, bview = E._wide(b, 2, 1, DEV, fill=0.25)
    wsp, out = torch.zeros(lib.ssim_workspace_bytes(B, C, H, W) // 4, device=DEV), torch.zeros(B, device=DEV)
    lib.ssim(aview, bview, B, E.EO.gaussian_1d(11).tolist(), out, wsp, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    err = float((out.cpu().double() - E.EO.ssim_per_image(a.double(), b.double(), 11)).abs().max())
    print(f'[glue] ssim {B}x{C}x{H}x{W}: worst error = {err:.3e}')
    assert err <= E.SSIM_BAR


@pytest.mark.parametrize('prec', E.WINO_PRECS, ids=E.WINO_PREC_IDS)
def test_winograd_deferred_out_bottleneck_shape(lib, prec):
    """The bottleneck's local conv (512 -> 128 at 64 x 64, batch 2): the deferred output transform on its own and inside the rfft2 launch of a
    [2,192,64,64] FourierUnit input: bit-equal to the one-call form and to the plain rfft2."""
    case = dict(cin=512, cout=128, H=64, W=64, B=2, act=1, bias=True, resid=True, scale=True)
    o = KE.wino_operands(lib, case, prec, DEV)
    st = o.st
    xv, yv = L.view(o.xbuf, 1, o.cin), lambda t: L.view(t, 2, o.cout)      # noqa: E731
    ybuf = torch.full((o.B, o.cout + 3, o.H, o.W), 7.0, device=DEV)
    lib.winograd_conv3x3(xv, o.wp, yv(ybuf), o.B, o.ws, o.bias_d, o.act, L.view(o.resid_d), precision=prec, stream=st)
    xf = torch.randn(2, 192, 64, 64, generator=o.g).to(DEV)
    sp0 = torch.zeros(2, 384, 64, 33, device=DEV)
    lib.rfft2(L.view(xf), L.view(sp0), 2, None, stream=st)
    for fused in (False, True):
        y2 = torch.full((o.B, o.cout + 3, o.H, o.W), 7.0, device=DEV)
        pend = lib.winograd_conv3x3(xv, o.wp, yv(y2), o.B, o.ws, o.bias_d, o.act, L.view(o.resid_d), precision=prec, stream=st, defer_out=True)
        torch.cuda.synchronize()
        assert float(y2.min()) == 7.0 == float(y2.max())
        if fused:
            sp = torch.zeros(2, 384, 64, 33, device=DEV)
            lib.rfft2_wino_out(L.view(xf), L.view(sp), 2, None, pend, o.ws, stream=st)
            torch.cuda.synchronize()
            assert torch.equal(sp, sp0)
        else:
            lib.winograd_out(pend, o.ws, stream=st)
        torch.cuda.synchronize()
        assert torch.equal(y2, ybuf)
    assert float(ybuf[:, :2].min()) == 7.0 and float(ybuf[:, -1].max()) == 7.0 and float(ybuf[:, 2:2 + o.cout].abs().max()) > 1.0
