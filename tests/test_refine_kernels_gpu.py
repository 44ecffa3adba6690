"""GPU parity tests of the refinement kernels (lama_amd/csrc/refine.hip), per kernel, on the MI355X (run with -m gpu, -s prints the headroom).

Through ``lama_amd._lib`` and the C ABI only, the production library (``L.get_lib()``), device tensors, one process -- the pattern of
tests/test_kernels_gpu.py.  References are fp64 torch / numpy on the host (tests/refine_ref.py, oracle/refine_oracle.py).

Part A reruns the emulator suite's cases (tests/test_refine_emu.py, tests/test_refine_batch_emu.py) with its assertions on hardware.

Part B runs every kernel at production sizes.  No tolerance below is tuned to what a kernel returned; each is one of
  * bit-equality (a result that involves no rounding, or the same fp32 expression on the host),
  * an exact count,
  * ``gamma(k) * ref_abs``: gamma(k) = k u / (1 - k u), u = 2^-24, k = the number of fp32 roundings on the longest path of the kernel's
    expression (n + 2 for a sum of n products: the product, the sum, and one rounding of each of the two weights), ref_abs = the same
    reference applied to |input|.  With non-negative
    weights a sum of n products computed in ANY order, fused (FMA) or not, stays inside gamma(n) * sum |products| (Higham, Accuracy and
    Stability of Numerical Algorithms, section 3.1), which is where each k below comes from.
Each case names the launch cap or code path it crosses:
  [1M]    more than 1,048,576 elements: rf_grid caps the launch at 4096 workgroups x 256 threads, the grid-stride loop takes further trips;
  [L1-512]  the L1 forward kernels cap at 512 workgroups;
  [PI-4096/B] the per-image L1 backward caps grid.x at 4096 / batch;
  [V4] / [V1]  the 16-byte and the scalar path of act_bwd / add / the fused fold (chosen by the host from per % 4 and pointer alignment);
  [LDS]   dgrad_ring_kernel's dynamic LDS (52 KB up to 512 gradient channels, 92 KB at 1536, refused above 96 KB)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lama_amd import _lib as L
from oracle import refine_oracle as R
from tests import refine_ref as RR
from tests import test_refine_batch_emu as EB
from tests import test_refine_emu as E

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = RR.U
gamma = RR.gamma


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return L.get_lib()          # raises if liblama_hip.so was not built: no fallback


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sync():
    torch.cuda.synchronize()


def _host(t):
    _sync()
    return t.cpu()


def _check_bar(name, got, ref, ref_abs, k):
    """|got - ref| <= gamma(k) * ref_abs elementwise (exactly 0 where ref_abs is 0); prints and returns the worst error / bar."""
    err = (got.double() - ref).abs()
    bar = gamma(k) * ref_abs
    pos = bar > 0
    worst0 = float(err[~pos].max()) if bool((~pos).any()) else 0.0
    ratio = float((err[pos] / bar[pos]).max()) if bool(pos.any()) else 0.0
    print(f'[refine-kernels] {name}: worst error / bar = {ratio:.4f} (k = {k})')
    assert worst0 == 0.0, f'{name}: {worst0} where the reference is exactly 0'
    if ratio > 1.0:
        idx = np.unravel_index(int(torch.argmax(torch.where(pos, err / bar.clamp_min(1e-300), torch.zeros_like(err)))), tuple(err.shape))
        raise AssertionError(f'{name}: error / bar = {ratio} at index {idx}')
    return ratio


# =====================================================================================================================================
# Part A -- the emulator cases, on hardware, with the emulator suite's assertions (guard values and LamaError cases included)
# =====================================================================================================================================

@pytest.mark.parametrize('act', E.ACT_CASES)
def test_emu_act_bwd_and_add(lib, act):
    E.check_act_bwd_and_add(lib, act, DEV)


@pytest.mark.parametrize('case', E.PAD_CASES)
def test_emu_reflect_pad_adjoint(lib, case):
    E.check_reflect_pad_adjoint(lib, case, DEV)


@pytest.mark.parametrize('case', E.PAD_FUSED_CASES)
def test_emu_reflect_pad_adjoint_fused(lib, case):
    E.check_reflect_pad_adjoint_fused(lib, case, DEV)


@pytest.mark.parametrize('case', E.RING_CASES)
def test_emu_dgrad_ring_and_fold_from_interior(lib, case):
    E.check_dgrad_ring_and_fold_from_interior(lib, case, DEV)


@pytest.mark.parametrize('shape', E.GAUSS_CASES)
def test_emu_gauss5_crop_fwd_and_adjoint(lib, shape):
    E.check_gauss5_crop_fwd_and_adjoint(lib, shape, DEV)


@pytest.mark.parametrize('shape', E.BILINEAR_CASES)
def test_emu_bilinear_fwd_and_adjoint(lib, shape):
    E.check_bilinear_fwd_and_adjoint(lib, shape, DEV)


def test_emu_pyrdown_and_mask_pipeline(lib):
    E.check_pyrdown_and_mask_pipeline(lib, DEV)


def test_emu_masked_l1_and_adam(lib):
    E.check_masked_l1_and_adam(lib, DEV)


@pytest.mark.parametrize('mask_c', EB.PER_IMAGE_MASK_C)
@pytest.mark.parametrize('select_ge', EB.PER_IMAGE_SELECT_GE)
def test_emu_l1_masked_per_image_kernels_against_numpy(lib, mask_c, select_ge):
    EB.check_l1_masked_per_image_kernels_against_numpy(lib, mask_c, select_ge, DEV)


# =====================================================================================================================================
# Part B -- production sizes against fp64
# =====================================================================================================================================

# (B, XH, XW, H, W, Ho, Wo): gauss5 blurs the top-left H x W crop of x [B, 3, XH, XW]; bilinear resizes that blur to Ho x Wo
PYRAMID_CASES = [
    (1, 2048, 2048, 2000, 2040, 1000, 1020),   # [1M] 12.2 M blur outputs = 12 trips, 12.6 M gx elements; a crop (XW != W) in every index
    (2, 1080, 1920, 1080, 1920, 540, 960),     # [1M] 12.4 M: the batch boundary (b = i / per) falls inside the 6th trip
    (1, 1000, 1504, 1000, 1504, 500, 752),     # [1M] 4.5 M; the resize output (1.13 M) ends 7 % into its second trip
    (1, 500, 752, 500, 752, 1000, 1504),       # [1M] upsampling x2 (refinement.py:233): the adjoint gathers up to 4 x 4 outputs per input
]


def _band(H, W, n=8):
    m = torch.zeros(H, W, dtype=torch.float64)
    m[:n], m[-n:], m[:, :n], m[:, -n:] = 1.0, 1.0, 1.0, 1.0
    return m


@pytest.mark.parametrize('case', PYRAMID_CASES, ids=lambda c: 'b%d_%dx%d_crop%dx%d_to%dx%d' % c)
def test_pyramid_fwd_bwd_against_fp64(lib, case):
    """gauss5 / bilinear, forward and adjoint, against R.gaussian_blur2d / F.interpolate on .double() and their fp64 autograd.

    Bars (derived, not measured): every output is a sum of n products with non-negative weights -- n = 25 (blur: the kernel forms it as 5 rows
    of 5 products and 5 more products, every term then carries at most 5 + 1 + 5 + ... <= 25 roundings), 4 (bilinear), and up to 75 / 16 for
    the adjoints near a border (three mirrored positions per axis -> 3 x 25; 4 x 4 outputs per input at x2 upsampling).  The weights
    themselves are exact here (every resize ratio below is 2 or 1/2, so the source coordinates and the bilinear weights 1/4, 1/2, 3/4 are
    exact in fp32) or carry one rounding (the product k[dy] * k[dx]).  Bar per element: gamma(n + 2) * ref_abs.
    The adjoint identity <A x, y> = <x, A^T y> is checked in fp64 from the kernels' OWN outputs on non-negative x, y (no reference, no
    cancellation): both sides are sums of non-negative terms, each inside its elementwise bar, so they differ by at most
    (gamma(n_f + 2) + gamma(n_b + 2)) * max(lhs, rhs).  A second pair with y supported on an 8-pixel band along the border makes a
    dropped mirror term a large share of the sum."""
    B, XH, XW, H, W, Ho, Wo = case
    g = _gen(100 + H)
    tag = 'x'.join(map(str, case))

    def run_gauss(xh):
        xd, yb = xh.to(DEV), torch.full((B, 5, H, W), 7.0, device=DEV)          # output = channels 1..3 of a wider buffer
        lib.gauss5(L.view(xd), L.view(yb, 1, 3), B)
        yb = _host(yb)
        assert float(yb[:, 0].min()) == 7.0 == float(yb[:, 0].max()) and float(yb[:, 4].min()) == 7.0 == float(yb[:, 4].max())
        return yb[:, 1:4].contiguous()

    def run_gauss_bwd(gyh):
        gyd, gxb = gyh.to(DEV), torch.full((B, 5, XH, XW), 9.0, device=DEV)
        lib.gauss5_bwd(L.view(gyd), L.view(gxb, 1, 3), B)
        gxb = _host(gxb)
        assert float(gxb[:, 0].min()) == 9.0 == float(gxb[:, 0].max()) and float(gxb[:, 4].min()) == 9.0 == float(gxb[:, 4].max())
        return gxb[:, 1:4].contiguous()

    def run_bilinear(xh):
        xd, yb = xh.to(DEV), torch.full((B, 5, Ho, Wo), 7.0, device=DEV)
        lib.bilinear(L.view(xd), L.view(yb, 1, 3), B)
        yb = _host(yb)
        assert float(yb[:, 0].min()) == 7.0 == float(yb[:, 0].max()) and float(yb[:, 4].min()) == 7.0 == float(yb[:, 4].max())
        return yb[:, 1:4].contiguous()

    def run_bilinear_bwd(gyh):
        gyd, gxb = gyh.to(DEV), torch.full((B, 5, H, W), 9.0, device=DEV)
        lib.bilinear_bwd(L.view(gyd), L.view(gxb, 1, 3), B)
        gxb = _host(gxb)
        assert float(gxb[:, 0].min()) == 9.0 == float(gxb[:, 0].max()) and float(gxb[:, 4].min()) == 9.0 == float(gxb[:, 4].max())
        return gxb[:, 1:4].contiguous()

    # forward
    x = torch.randn(B, 3, XH, XW, generator=g)
    blur = run_gauss(x)
    _check_bar(f'gauss5_fwd {tag}', blur, RR.blur64(x, H, W), RR.blur64(x.abs(), H, W), 25 + 2)
    down = run_bilinear(blur)                                                     # on the kernel's own fp32 blur: the same fp32 input as the reference
    _check_bar(f'bilinear_fwd {tag}', down, RR.resize64(blur, (Ho, Wo)), RR.resize64(blur.abs(), (Ho, Wo)), 4 + 2)
    # adjoints against fp64 autograd
    gy = torch.randn(B, 3, H, W, generator=g)
    gx = run_gauss_bwd(gy)
    assert float(gx[:, :, H:].abs().max() if XH > H else 0.0) == 0.0 and float(gx[:, :, :, W:].abs().max() if XW > W else 0.0) == 0.0   # zeros outside the crop
    blur_of_crop = lambda t: R.gaussian_blur2d(t[:, :, :H, :W])                   # noqa: E731
    _check_bar(f'gauss5_bwd {tag}', gx, RR.vjp64(blur_of_crop, (B, 3, XH, XW), gy), RR.vjp64(blur_of_crop, (B, 3, XH, XW), gy.abs()), 75 + 2)
    gyo = torch.randn(B, 3, Ho, Wo, generator=g)
    gxi = run_bilinear_bwd(gyo)
    resize = lambda t: F.interpolate(t, size=(Ho, Wo), mode='bilinear', align_corners=False)   # noqa: E731
    _check_bar(f'bilinear_bwd {tag}', gxi, RR.vjp64(resize, (B, 3, H, W), gyo), RR.vjp64(resize, (B, 3, H, W), gyo.abs()), 16 + 2)
    # adjoint identities from the kernels' own outputs, non-negative data
    x2 = torch.rand(B, 3, XH, XW, generator=g)
    ax = run_gauss(x2).double()
    xi2 = torch.rand(B, 3, H, W, generator=g)
    axi = run_bilinear(xi2).double()
    for what, band_g, band_b in (('full', None, None), ('border band', _band(H, W), _band(Ho, Wo))):
        y2 = torch.rand(B, 3, H, W, generator=g)
        yo2 = torch.rand(B, 3, Ho, Wo, generator=g)
        if band_g is not None:
            y2, yo2 = (y2 * band_g).float(), (yo2 * band_b).float()
        lhs, rhs = float((ax * y2.double()).sum()), float((x2.double() * run_gauss_bwd(y2).double()).sum())
        bar = (gamma(27) + gamma(77)) * max(lhs, rhs)
        print(f'[refine-kernels] gauss5 adjoint identity ({what}) {tag}: |lhs - rhs| / bar = {abs(lhs - rhs) / bar:.4f}')
        assert abs(lhs - rhs) <= bar, (what, lhs, rhs)
        lhs, rhs = float((axi * yo2.double()).sum()), float((xi2.double() * run_bilinear_bwd(yo2).double()).sum())
        bar = (gamma(6) + gamma(18)) * max(lhs, rhs)
        print(f'[refine-kernels] bilinear adjoint identity ({what}) {tag}: |lhs - rhs| / bar = {abs(lhs - rhs) / bar:.4f}')
        assert abs(lhs - rhs) <= bar, (what, lhs, rhs)


# -------------------------------------------------------------------------------------------------------------------------------------
# mask chain
# -------------------------------------------------------------------------------------------------------------------------------------
MASK_SIZES = [(2048, 2048), (1080, 1920), (1001, 1505)]      # [1M] all; 1001 x 1505 -> 500 x 752: the bilinear weights are not 1/2


def _se_pair():
    se2 = torch.zeros(3, 5)
    se2[0, 1] = 1; se2[2, 4] = 1; se2[1, 2] = 1                # asymmetric: kornia's flip matters
    return (('ellipse15', R.ellipse_kernel(15)), ('asym3x5', se2))


def _erode(lib, xh, se):
    xd, sed = xh.to(DEV), se.to(DEV)
    out = torch.full((xh.shape[0], 3, xh.shape[2], xh.shape[3]), 7.0, device=DEV)
    lib.erode(L.view(xd), sed, L.view(out, 1, 1), xh.shape[0])
    out = _host(out)
    assert float(out[:, 0].min()) == 7.0 == float(out[:, 0].max()) and float(out[:, 2].min()) == 7.0 == float(out[:, 2].max())
    return out[:, 1:2].contiguous()


def _threshold(lib, xh, thr):
    xd = xh.to(DEV)
    out = torch.full((xh.shape[0], 3, xh.shape[2], xh.shape[3]), 7.0, device=DEV)
    lib.threshold(L.view(xd), thr, L.view(out, 1, 1), xh.shape[0])
    out = _host(out)
    assert float(out[:, 0].min()) == 7.0 == float(out[:, 0].max()) and float(out[:, 2].min()) == 7.0 == float(out[:, 2].max())
    return out[:, 1:2].contiguous()


@pytest.mark.parametrize('size', MASK_SIZES, ids=lambda s: '%dx%d' % s)
def test_threshold_and_erode_bit_equal(lib, size):
    """lama_threshold_fwd and lama_erode_fwd alone, bit-equal to a host restatement: a comparison and a minimum of inputs round nothing.
    Binary masks and random float input; the 15 x 15 ellipse and an asymmetric 3 x 5 element.  The host restatement (a running minimum over
    the shifted members, RR.erode_ref) is itself checked against R.erosion at 64 x 80 here (R.erosion's unfold needs gigabytes at 2048^2)."""
    H, W = size
    g = _gen(7)
    small = torch.randn(2, 1, 64, 80, generator=g)
    for name, se in _se_pair():
        assert torch.equal(RR.erode_ref(small, se), R.erosion(small, se)), name
        assert torch.equal(RR.erode_ref((small > 0).float(), se), R.erosion((small > 0).float(), se)), name
    xf = torch.randn(1, 1, H, W, generator=g)
    # values on and next to both thresholds of the pipeline: (float)(1 - 1e-8) == 1.0f and (float)1e-8
    edge = torch.tensor([1.0, float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2))), 1e-8,
                         float(np.nextafter(np.float32(1e-8), np.float32(0))), float(np.nextafter(np.float32(1e-8), np.float32(1))), 0.0, -0.0])
    xf.view(-1)[::H * W // 8 - 1][:8] = edge
    xf.view(-1)[-8:] = edge                                    # ... and in the last trip of the grid-stride loop
    for thr in (1e-8, 1.0 - 1e-8):
        assert torch.equal(_threshold(lib, xf, thr), RR.threshold_ref(xf, thr)), thr
    inputs = [('random float', xf)] + [(k, m) for k, m in RR.make_masks(H, W).items()]
    for iname, xin in inputs:
        for sname, se in _se_pair():
            assert torch.equal(_erode(lib, xin, se), RR.erode_ref(xin, se)), (iname, sname)


@pytest.mark.parametrize('family', ['rectangle', 'discs', 'strokes'])
@pytest.mark.parametrize('size', MASK_SIZES, ids=lambda s: '%dx%d' % s)
def test_mask_pyramid_chain(lib, size, family):
    """The two pyramid uses of the mask chain (lama_amd/refinement.py _pyrdown_mask / _erode_mask), restated with the kernels.

    (a) resize + ``>= (float)(1 - 1e-8) = 1.0f`` + erosion by the 15 x 15 ellipse + threshold (mask_down of every scale) must be BIT-EQUAL to
        R.pyrdown_mask(blur_mask=False, round_up=False) and the erode-mask step in fp32 on the host: which pixels survive is a rounding
        decision, and the kernel has to take it as ATen does.
    (b) blur + resize + ``>= 1e-8``: with v = the fp64 value before the threshold, v == 0 -> 0 and v > 1e-6 -> 1 (every term is
        non-negative, so an exact zero stays zero; above 1e-6 no fp32 rounding of a value that is a sum of <= 100 non-negative products
        reaches 1e-8); pixels in between are undecidable and left out, and their share must be at most 1e-4 of the pixels (asserted, so
        that a bad mask cannot hide a failure).  On the decided pixels the result also equals the fp32 oracle."""
    H, W = size
    mask = RR.make_masks(H, W)[family]
    Ho, Wo = H // 2, W // 2
    md = mask.to(DEV)
    se = R.ellipse_kernel(15)
    # (a)
    small = torch.empty(1, 1, Ho, Wo, device=DEV)
    lib.bilinear(L.view(md), L.view(small), 1)
    thr = torch.empty_like(small)
    lib.threshold(L.view(small), 1.0 - 1e-8, L.view(thr), 1)
    er = torch.empty_like(small)
    lib.erode(L.view(thr), se.to(DEV), L.view(er), 1)
    out = torch.empty_like(small)
    lib.threshold(L.view(er), 1.0 - 1e-8, L.view(out), 1)
    thr_h, out_h = _host(thr), _host(out)
    want_down = R.pyrdown_mask(mask, blur_mask=False, round_up=False)
    diff = (thr_h != want_down).nonzero()
    assert diff.numel() == 0, f'{diff.shape[0]} pixels of the resized mask differ from ATen, first at {diff[0].tolist()}'
    want = RR.threshold_ref(RR.erode_ref(want_down, se), 1.0 - 1e-8)
    assert torch.equal(out_h, want)
    assert 0 < float(want_down.sum()) < Ho * Wo
    # (b)
    blur = torch.empty_like(md)
    lib.gauss5(L.view(md), L.view(blur), 1)
    lib.bilinear(L.view(blur), L.view(small), 1)
    lib.threshold(L.view(small), 1e-8, L.view(out), 1)
    got = _host(out)
    v = RR.resize64(RR.blur64(mask, H, W), (Ho, Wo))
    zero, one = v == 0, v > 1e-6
    share = 1.0 - float((zero | one).double().mean())
    print(f'[refine-kernels] pyrdown_mask {family} {H}x{W}: undecidable share = {share:.2e}')
    assert share <= 1e-4
    assert float(got[zero].max()) == 0.0 and float(got[one].min()) == 1.0
    oracle = R.pyrdown_mask(mask)
    decided = zero | one
    assert torch.equal(got[decided], oracle[decided])


# -------------------------------------------------------------------------------------------------------------------------------------
# masked L1
# -------------------------------------------------------------------------------------------------------------------------------------
L1_BATCHES = [1, 3, 8]
L1_PLANES = [(2048, 2048),    # [1M] [L1-512] 12.6 M elements per image: 96 trips of 512 workgroups; B = 3 / 8: [PI-4096/B] grid.x = 1365 / 512
             (1000, 1504),    # [1M] [L1-512] 4.5 M per image, not a multiple of the launch size
             (9, 14)]         # 378 elements per image: fewer than one workgroup per image, most workgroups of the capped launches idle


def _l1_data(B, H, W):
    """pred / target on the 2^-24 grid of torch.rand: |pred - target| is then exact in fp32 and every fp64 partial sum of up to 2^27 of them
    is exact too, so the sums do not depend on the order in which 512 workgroups reach their atomicAdd."""
    g = _gen(1000 * B + H)
    pred, target = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    target[:, :, 2:5, 3:11] = pred[:, :, 2:5, 3:11]                     # exact ties: |d| = 0, sign(0) = 0
    target.view(-1)[-5:] = pred.view(-1)[-5:]
    masks = {}
    for mc in (1, 3):
        m = (torch.rand(B, mc, H, W, generator=g) > 0.6).float()
        m[:, :, 2:4, 3:8] = 1.0
        m[:, :, 4:5, 3:11] = 0.0                                       # ties on both sides of the selection
        if B >= 3:
            m[1] = 0.0                                                 # image 1: empty for select_ge, everything otherwise
            m[2] = 1.0                                                 # image 2: everything for select_ge, empty otherwise
        masks[mc] = m
    return pred, target, masks


@pytest.mark.parametrize('plane', L1_PLANES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('B', L1_BATCHES)
def test_l1_masked_fwd_bwd(lib, B, plane):
    """lama_l1_masked_fwd / _bwd and the per-image pair, 1- and 3-channel masks, both select_ge values.

    Forward: the count equals the host count exactly; the sum is within N * 2^-52 * sum of |pred - target| formed in fp32 and summed in
    fp64 on the host (only the order of an fp64 summation of N non-negative terms differs: gamma_N in fp64 <= N * 2^-52).  Two runs into
    zeroed accumulators: identical counts, both sums inside the bar.  Per image: image b's pair depends on image b alone -- perturbing
    image 0 leaves the pairs of images 1.. bit-identical (see _l1_data: the sums are exact, so the order of the atomics cannot show).
    Backward: bit-equal to scale * sign(pred - target) * selected in fp32 on the host, scale = float32(1 / n) (the per-image form takes n
    from the count the forward left on the device; an empty image gets zeros); accumulate on and off; g is a channel view of a wider buffer
    whose other channels keep their fill."""
    H, W = plane
    pred, target, masks = _l1_data(B, H, W)
    predd, targetd = pred.to(DEV), target.to(DEV)
    pert = pred.clone()
    pert[0] = 1.0 - pert[0]
    pertd = pert.to(DEV)
    base = torch.randn(B, 3, H, W, generator=_gen(5))
    for mc in (1, 3):
        maskd = masks[mc].to(DEV)
        for select_ge in (False, True):
            tag = f'B{B} {H}x{W} mask_c={mc} select_ge={select_ge}'
            sel = RR.l1_select(masks[mc], 3, select_ge)
            s_img, n_img = RR.l1_terms(pred, target, sel)
            if B >= 3:
                assert 0.0 in n_img.tolist() and float(3 * H * W) in n_img.tolist()       # an empty image and a full one
            s_all, n_all = float(s_img.sum()), float(n_img.sum())
            # whole-batch forward, twice
            for run in range(2):
                acc = torch.zeros(2, dtype=torch.float64, device=DEV)
                lib.l1_masked(L.view(predd), L.view(targetd), L.view(maskd), 1e-8, select_ge, acc, B)
                acc = _host(acc)
                assert float(acc[1]) == n_all, (tag, run)
                assert abs(float(acc[0]) - s_all) <= n_all * 2.0 ** -52 * s_all, (tag, run, float(acc[0]), s_all)
            # per-image forward, twice, then with image 0 perturbed
            accs = []
            for run, pd in enumerate((predd, predd, pertd)):
                a = torch.zeros(B, 2, dtype=torch.float64, device=DEV)
                lib.l1_masked_per_image(L.view(pd), L.view(targetd), L.view(maskd), 1e-8, select_ge, a, B)
                _sync()
                accs.append(a)
            a0, a1, a2 = (a.cpu() for a in accs)
            for a in (a0, a1):
                assert torch.equal(a[:, 1], n_img), tag
                for b in range(B):
                    assert abs(float(a[b, 0]) - float(s_img[b])) <= float(n_img[b]) * 2.0 ** -52 * float(s_img[b]), (tag, b)
            assert torch.equal(a2[1:], a0[1:]), tag                                   # images 1.. do not see image 0
            if float(n_img[0]) > 0:
                assert float(a2[0, 0]) != float(a0[0, 0]) and float(a2[0, 1]) == float(a0[0, 1])
            # backward, whole batch: scale from the host, as lama_amd/refinement.py forms it
            scale = float(np.float32(1.0 / n_all)) if n_all else 0.0
            want = RR.l1_grad(pred, target, sel, torch.full((B,), scale))
            want_pi = RR.l1_grad(pred, target, sel, torch.tensor([float(np.float32(1.0 / n)) if n else 0.0 for n in a0[:, 1].tolist()]))
            if B >= 3:
                assert float(want_pi[n_img.tolist().index(0.0)].abs().max()) == 0.0
            for accumulate in (False, True):
                for form in ('batch', 'per_image'):
                    gb = torch.full((B, 5, H, W), 5.0, device=DEV)
                    if accumulate:
                        gb[:, 1:4] = base.to(DEV)
                    if form == 'batch':
                        lib.l1_masked_bwd(L.view(predd), L.view(targetd), L.view(maskd), 1e-8, select_ge, scale, accumulate, L.view(gb, 1, 3), B)
                    else:
                        lib.l1_masked_per_image_bwd(L.view(predd), L.view(targetd), L.view(maskd), 1e-8, select_ge, accs[0], accumulate,
                                                    L.view(gb, 1, 3), B)
                    gb = _host(gb)
                    w = want if form == 'batch' else want_pi
                    assert torch.equal(gb[:, 1:4], base + w if accumulate else w), (tag, form, accumulate)
                    assert float(gb[:, 0].min()) == 5.0 == float(gb[:, 0].max()) and float(gb[:, 4].min()) == 5.0 == float(gb[:, 4].max())
            print(f'[refine-kernels] l1_masked {tag}: counts exact ({int(n_all)}), sums exact to the bar, gradients bit-equal')


# -------------------------------------------------------------------------------------------------------------------------------------
# Adam
# -------------------------------------------------------------------------------------------------------------------------------------
ADAM_SIZES = [1000,                   # one workgroup row; also against torch.optim.Adam
              2 ** 20 + 3,            # [1M] three elements into the second trip
              512 * 125 * 188,        # [1M] z of a 1000 x 1504 image: 11.5 trips
              512 * 256 * 256]        # [1M] z of a 2048^2 image: 32 trips


@pytest.mark.parametrize('n', ADAM_SIZES)
def test_adam_step_against_fp64(lib, n):
    """lama_adam_step, 15 steps (production's n_iters), gradients spanning 1e-8 .. 1e2 per element with exact zeros (elements whose gradient
    is always 0 keep m = v = 0: the denominator is eps and the update 0).  Reference: the kernel's update restated in fp64, every step from
    the kernel's OWN fp32 state of the step before, with the fp32 constants the host code forms -- one step of rounding, no drift.

    Bars, from the kernel's expression (u = 2^-24; FMA contraction only removes roundings):
      m' = fl(fl(b1 m) + fl(c1 g)), c1 = 1 - b1 exact:           |dm| <= gamma(3) (b1 |m| + c1 |g|) = gamma(3) m_abs.  (m_abs = |m'| unless
           the two terms have opposite signs; "3u |m|" would not be a bound under that cancellation.)
      v' = fl(fl(b2 v) + fl(fl(c2 g) g)), all terms >= 0:         |dv| <= gamma(3) v'
      p' = fl(p - fl(a q)), a = fl(lr / bc1), q = fl(m' / d), d = fl(fl(sqrt(v') / bc2s) + eps):
           relative roundings on a q: m' 3 (against m_abs), sqrt(v') 3/2 + 1, / bc2s 1, + eps 1 (eps is exact, the sum is of
           non-negative terms), a 1, the quotient 1, the product 1 -- 10.5, taken as 11;  the last subtraction adds u |p'|:
           |dp| <= u |p'| + gamma(11) a m_abs / d.
    On n = 1000 the 15 steps are also compared with torch.optim.Adam on the host at the emulator test's tolerance."""
    g = _gen(n)
    lr = 0.002
    p0 = torch.randn(n, generator=g)
    always_zero = torch.rand(n, generator=g) < 0.01
    pd, md, vd = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    p_prev, m_prev, v_prev = p0.clone(), torch.zeros(n), torch.zeros(n)
    if n == 1000:
        pt = p0.clone().requires_grad_(True)
        opt = torch.optim.Adam([pt], lr=lr)
    worst = [0.0, 0.0, 0.0]
    for step in range(1, 16):
        gr = torch.sign(torch.randn(n, generator=g)) * 10.0 ** (torch.rand(n, generator=g) * 10.0 - 8.0)
        gr[always_zero] = 0.0
        gr[torch.rand(n, generator=g) < 0.01] = 0.0                     # ... and zeros that come and go
        grd = gr.to(DEV)
        lib.adam_step(pd, grd, md, vd, lr, step)
        p_new, m_new, v_new = _host(pd), md.cpu(), vd.cpu()
        p64, m64, v64, m_abs, upd_abs = RR.adam_step64(p_prev, gr, m_prev, v_prev, RR.adam_constants(lr, step))
        for i, (got, ref, bar) in enumerate(((m_new, m64, gamma(3) * m_abs), (v_new, v64, gamma(3) * v64),
                                             (p_new, p64, U * p64.abs() + gamma(11) * upd_abs))):
            err = (got.double() - ref).abs()
            pos = bar > 0
            assert float(err[~pos].max() if bool((~pos).any()) else 0.0) == 0.0, (step, 'mvp'[i])
            ratio = float((err[pos] / bar[pos]).max())
            worst[i] = max(worst[i], ratio)
            assert ratio <= 1.0, (step, 'mvp'[i], ratio, int(torch.argmax(torch.where(pos, err / bar.clamp_min(1e-300), torch.zeros_like(err)))))
        assert float(m_new[always_zero].abs().max()) == 0.0 and float(v_new[always_zero].abs().max()) == 0.0
        assert torch.equal(p_new[always_zero], p0[always_zero])
        if n == 1000:
            opt.zero_grad(); pt.grad = gr.clone(); opt.step()
        p_prev, m_prev, v_prev = p_new, m_new, v_new
    print(f'[refine-kernels] adam_step n={n}: worst error / bar over 15 steps: m {worst[0]:.4f}, v {worst[1]:.4f}, p {worst[2]:.4f}')
    if n == 1000:
        assert torch.allclose(p_prev, pt.detach(), atol=1e-6, rtol=1e-5)


# -------------------------------------------------------------------------------------------------------------------------------------
# act_bwd / add
# -------------------------------------------------------------------------------------------------------------------------------------
# (B, H, W): views at channel offset 128, width 384, of 512-channel buffers -- how lama_amd/backward.py calls them
ACT_SHAPES = [(1, 256, 256),      # [1M] [V4] 25.2 M elements = 6.3 M float4: 6 trips
              (2, 125, 188),      # [1M] [V4] 18 M; odd plane, batch stride (512 planes) != per (384 planes)
              (1, 135, 240)]      # [1M] [V4] 12.4 M


def _act_fn(act, x):
    return {L.ACT_RELU: torch.relu, L.ACT_SIGMOID: torch.sigmoid, L.ACT_TANH: torch.tanh, L.ACT_NONE: lambda t: t.clone()}[act](x)


def _act_ref64(act, g, y):
    g, y = g.double(), y.double()
    d = {L.ACT_RELU: (y > 0).double(), L.ACT_SIGMOID: y * (1.0 - y), L.ACT_TANH: 1.0 - y * y, L.ACT_NONE: torch.ones_like(y)}[act]
    return g * d


@pytest.mark.parametrize('shape', ACT_SHAPES, ids=lambda s: 'b%d_%dx%d' % s)
def test_act_bwd_and_add_production_views(lib, shape):
    """lama_act_bwd (all four activations, in place: gout is g, lama_amd/backward.py:177) and lama_add_fwd on channel views [128, 512) of
    512-channel buffers.  add, ReLU and "none" are bit-equal to torch fp32 (one exact product / one correctly rounded sum); sigmoid
    (g * fl(y * fl(1 - y))) and tanh (g * fl(1 - y^2)) are within 3 roundings of fp64: gamma(3) relative."""
    B, H, W = shape
    g = _gen(H)
    c0, c = 128, 384
    for act in E.ACT_CASES:
        y = torch.zeros(B, 512, H, W)
        y[:, c0:] = _act_fn(act, torch.randn(B, c, H, W, generator=g))
        gbuf = torch.full((B, 512, H, W), 3.0)
        gbuf[:, c0:] = torch.randn(B, c, H, W, generator=g)
        yd, gd = y.to(DEV), gbuf.to(DEV)
        lib.act_bwd(L.view(gd, c0, c), L.view(yd, c0, c), act, L.view(gd, c0, c), B)         # in place
        out = _host(gd)
        assert float(out[:, :c0].min()) == 3.0 == float(out[:, :c0].max())
        ref = _act_ref64(act, gbuf[:, c0:], y[:, c0:])
        if act in (L.ACT_RELU, L.ACT_NONE):
            assert torch.equal(out[:, c0:], ref.float()), act
        else:
            _check_bar(f'act_bwd act={act} {B}x{c}x{H}x{W}', out[:, c0:], ref, ref.abs(), 3)
    a, b = torch.randn(B, 512, H, W, generator=g), torch.randn(B, 512, H, W, generator=g)
    ad, bd, od = a.to(DEV), b.to(DEV), torch.full((B, 512, H, W), 3.0, device=DEV)
    lib.add(L.view(ad, c0, c), L.view(bd, c0, c), L.view(od, c0, c), B)
    out = _host(od)
    assert torch.equal(out[:, c0:], a[:, c0:] + b[:, c0:]) and float(out[:, :c0].min()) == 3.0 == float(out[:, :c0].max())


def test_act_bwd_and_add_scalar_path_equals_vector_path(lib):
    """[V1] against [V4] on the same data: a 125 x 187 plane (odd) at channel offset 1 of a 512-channel buffer puts the view 93,500 bytes in --
    not a multiple of 16 -- while per = 384 * 23,375 stays a multiple of 4: the host must fall back to the scalar kernel.  The same data in
    a standalone (aligned) tensor takes the 16-byte kernel.  Both must be bit-equal to each other and to the host."""
    B, H, W, c0, c = 2, 125, 187, 1, 384
    assert (c0 * H * W * 4) % 16 != 0 and (c * H * W) % 4 == 0 and (512 * H * W) % 4 == 0
    g = _gen(3)
    gv, bv = torch.randn(B, c, H, W, generator=g), torch.randn(B, c, H, W, generator=g)
    for act in E.ACT_CASES:
        yv = _act_fn(act, torch.randn(B, c, H, W, generator=g))
        res = []
        for aligned in (True, False):
            if aligned:
                gd, yd, od = gv.to(DEV), yv.to(DEV), torch.full((B, c, H, W), 3.0, device=DEV)
                views = (L.view(gd), L.view(yd), L.view(od))
            else:
                gw, yw = torch.zeros(B, 512, H, W), torch.zeros(B, 512, H, W)
                gw[:, c0:c0 + c], yw[:, c0:c0 + c] = gv, yv
                gd, yd, od = gw.to(DEV), yw.to(DEV), torch.full((B, 512, H, W), 3.0, device=DEV)
                views = (L.view(gd, c0, c), L.view(yd, c0, c), L.view(od, c0, c))
                assert views[0].ptr % 16 != 0
            lib.act_bwd(views[0], views[1], act, views[2], B)
            o = _host(od)
            if not aligned:
                assert float(o[:, :c0].min()) == 3.0 == float(o[:, :c0].max()) and float(o[:, c0 + c:].min()) == 3.0 == float(o[:, c0 + c:].max())
                o = o[:, c0:c0 + c]
            res.append(o.contiguous())
        assert torch.equal(res[0], res[1]), act
        ref = _act_ref64(act, gv, yv)
        if act in (L.ACT_RELU, L.ACT_NONE):
            assert torch.equal(res[1], ref.float())
        else:
            _check_bar(f'act_bwd scalar path act={act}', res[1], ref, ref.abs(), 3)
    aw, bw = torch.zeros(B, 512, H, W), torch.zeros(B, 512, H, W)
    aw[:, c0:c0 + c], bw[:, c0:c0 + c] = gv, bv
    ad, bd, od = aw.to(DEV), bw.to(DEV), torch.full((B, 512, H, W), 3.0, device=DEV)
    lib.add(L.view(ad, c0, c), L.view(bd, c0, c), L.view(od, c0, c), B)
    o = _host(od)
    a2, b2, o2 = gv.to(DEV), bv.to(DEV), torch.empty(B, c, H, W, device=DEV)
    lib.add(L.view(a2), L.view(b2), L.view(o2), B)
    assert torch.equal(o[:, c0:c0 + c], gv + bv) and torch.equal(_host(o2), gv + bv)
    assert float(o[:, :c0].min()) == 3.0 == float(o[:, :c0].max()) and float(o[:, c0 + c:].min()) == 3.0 == float(o[:, c0 + c:].max())


# -------------------------------------------------------------------------------------------------------------------------------------
# reflect-pad adjoint, its fused form, the ring
# -------------------------------------------------------------------------------------------------------------------------------------
FOLD_CASES = [(1, 384, 256, 256, 1),     # (B, C, H, W, pad)  [1M] [V4] 25 M
              (2, 128, 125, 188, 3),     # [1M] [V4] odd plane, pad 3: 2 x 2 mirrored positions in the corners
              (1, 128, 168, 168, 3),     # [1M] [V4]
              (2, 384, 168, 168, 1),     # [1M] [V4] batch boundary inside a trip
              (1, 128, 256, 256, 3),
              (1, 384, 125, 188, 1)]


@pytest.mark.parametrize('case', FOLD_CASES, ids=lambda c: 'b%d_c%d_%dx%d_pad%d' % c)
def test_reflect_pad_bwd_and_fused_against_fp64(lib, case):
    """lama_reflect_pad_bwd (with and without addend) and lama_reflect_pad_bwd_fused (1x1 path + identity in place + ReLU mask, the call of
    lama_amd/backward.py:181) against fp64 autograd through F.pad(mode='reflect').  A fold is a sum of at most 9 terms (pad 3 corner: 2 x 2
    mirrored positions, the addends, the zero it starts from), all weights 1: gamma(9) * ref_abs.  The ReLU mask multiplies by exactly 0 or 1."""
    B, C, H, W, pad = case
    g = _gen(C + H + pad)
    tag = 'x'.join(map(str, case))
    gp = torch.randn(B, C, H + 2 * pad, W + 2 * pad, generator=g)
    add1 = torch.randn(B, C, H, W, generator=g)
    ident = torch.randn(B, C + 128, H, W, generator=g)                  # the identity operand / in-place output: channels [128, 128 + C) of a wider state
    y = torch.randn(B, C + 128, H, W, generator=g)
    f64, f64a = RR.fold64(gp, pad), RR.fold64(gp.abs(), pad)
    gpd, add1d = gp.to(DEV), add1.to(DEV)
    out = torch.full((B, C + 2, H, W), 9.0, device=DEV)
    lib.reflect_pad_bwd(L.view(gpd), None, pad, L.view(out, 1, C), B)
    o = _host(out)
    assert float(o[:, 0].min()) == 9.0 == float(o[:, 0].max()) and float(o[:, -1].min()) == 9.0 == float(o[:, -1].max())
    _check_bar(f'reflect_pad_bwd {tag}', o[:, 1:-1], f64, f64a, 9)
    lib.reflect_pad_bwd(L.view(gpd), L.view(add1d), pad, L.view(out, 1, C), B)
    o = _host(out)
    _check_bar(f'reflect_pad_bwd + addend {tag}', o[:, 1:-1], f64 + add1.double(), f64a + add1.abs().double(), 9)
    # fused: s = fold + add1 + identity (in place over the identity), gm = s * relu'(y)
    identd, yd, gmd = ident.to(DEV), y.to(DEV), torch.full((B, C + 128, H, W), 9.0, device=DEV)
    lib.reflect_pad_bwd_fused(L.view(gpd), L.view(add1d), L.view(identd, 128, C), pad, L.view(yd, 128, C), L.ACT_RELU, L.view(identd, 128, C),
                              L.view(gmd, 128, C), B)
    s, gm = _host(identd), _host(gmd)
    ref = f64 + add1.double() + ident[:, 128:].double()
    ref_abs = f64a + add1.abs().double() + ident[:, 128:].abs().double()
    _check_bar(f'reflect_pad_bwd_fused g {tag}', s[:, 128:], ref, ref_abs, 9)
    assert torch.equal(s[:, :128], ident[:, :128]) and float(gm[:, :128].min()) == 9.0 == float(gm[:, :128].max())
    assert torch.equal(gm[:, 128:], s[:, 128:] * (y[:, 128:] > 0).float())          # the mask is exact on the kernel's own s
    corners = [(yy, xx) for yy in (0, 1, pad, H - 1 - pad, H - 2, H - 1) for xx in (0, 1, pad, W - 1 - pad, W - 2, W - 1)]
    for yy, xx in corners:                                                          # so that a failure names the corner
        e = (s[:, 128:, yy, xx].double() - ref[:, :, yy, xx]).abs()
        assert bool((e <= gamma(9) * ref_abs[:, :, yy, xx]).all()), (yy, xx)


# (B, gradient channels, data channels, H, W)
RING_CASES = [(2, 64, 128, 256, 256),      # [LDS] 52 KB
              (2, 128, 384, 125, 188),     # three 128-channel output groups (grid.y = 3), odd plane: the last workgroup of every edge is partial
              (1, 64, 384, 168, 168),
              (1, 128, 128, 168, 168),
              (1, 512, 128, 256, 256),     # production (lama_amd/backward.py:143: the 512 gradient channels of a block -> in_cl = 128), 2048^2 image
              (2, 512, 128, 125, 188),     # production, 1000 x 1504 image, batch 2
              (1, 1536, 128, 168, 168)]    # [LDS] 92 KB: the largest channel count the entry accepts (1600 needs 112 KB and is refused)


@pytest.mark.parametrize('case', RING_CASES, ids=lambda c: 'b%d_c%d_o%d_%dx%d' % c)
def test_dgrad_ring_and_fold_against_fp64(lib, case):
    """lama_dgrad_ring_fwd against the frame of the fp64 zero-padded correlation, and the fold from the interior + ring against fp64 autograd
    through F.pad(mode='reflect') of the padded plane assembled from the same interior and the kernel's own ring.

    Ring: exact-fp32 FMAs over at most 9 * C_in terms (3 * C_in per element, in 8 partial sums joined in a fixed order): bar
    gamma(9 * C_in) * ref_abs, ref_abs = the same correlation of |g| with |w'|.  The four edges and the four corners are asserted one by
    one.  Fold: at most interior + 3 ring terms + identity, weights 1: gamma(9) * ref_abs."""
    B, C, M, H, W = case
    g = _gen(C + M + H)
    tag = 'x'.join(map(str, case))
    wd = torch.randn(M, C, 3, 3, generator=g) / (3.0 * C ** 0.5)                       # w' [cout, cin, 3, 3]
    gwide = torch.full((B, C + 64, H, W), 2.0)                                          # the gradient: channels [64, 64 + C) of a wider buffer
    gwide[:, 64:] = torch.randn(B, C, H, W, generator=g)
    gy = gwide[:, 64:].contiguous()
    nring = lib.dgrad_ring_bytes(B, M, H, W) // 4
    assert nring == B * M * (2 * (W + 2) + 2 * H)
    ringd = torch.full((nring + 64,), 5.0, device=DEV)
    gd, wrd = gwide.to(DEV), lib.dgrad_ring_weight(wd).to(DEV)
    lib.dgrad_ring(L.view(gd, 64, C), wrd, M, ringd, B)
    ring = _host(ringd)
    assert float(ring[nring:].min()) == 5.0 == float(ring[nring:].max())                # trailing elements keep their fill
    r = ring[:nring].view(B, M, -1)
    parts = (r[:, :, :W + 2], r[:, :, W + 2:2 * W + 4], r[:, :, 2 * W + 4:2 * W + 4 + H], r[:, :, 2 * W + 4 + H:])
    refs, refs_abs = RR.ring64(gy, wd), RR.ring64(gy.abs(), wd.abs())
    k = 9 * C
    for name, got, ref, ra in zip(('top', 'bottom', 'left', 'right'), parts, refs, refs_abs):
        if name in ('top', 'bottom'):
            for cname, j in (('left corner', 0), ('right corner', -1)):
                _check_bar(f'dgrad_ring {tag} {name} {cname}', got[:, :, j], ref[:, :, j], ra[:, :, j], k)
            _check_bar(f'dgrad_ring {tag} {name} edge', got[:, :, 1:-1], ref[:, :, 1:-1], ra[:, :, 1:-1], k)
        else:
            _check_bar(f'dgrad_ring {tag} {name} edge', got, ref, ra, k)
    # the fold from an interior and this ring
    interior = torch.randn(B, M, H, W, generator=g)
    ident, y = torch.randn(B, M + 128, H, W, generator=g), torch.randn(B, M + 128, H, W, generator=g)
    intd, identd, yd, gmd = interior.to(DEV), ident.to(DEV), y.to(DEV), torch.full((B, M + 128, H, W), 9.0, device=DEV)
    lib.reflect_pad_bwd_fused(L.view(intd), None, L.view(identd, 0, M), 1, L.view(yd, 0, M), L.ACT_RELU, L.view(identd, 0, M), L.view(gmd, 0, M), B,
                              ring=ringd)
    s, gm = _host(identd), _host(gmd)
    gp64 = RR.assemble_padded(interior, *parts)
    ref = RR.fold64(gp64, 1) + ident[:, :M].double()
    ref_abs = RR.fold64(gp64.abs(), 1) + ident[:, :M].abs().double()
    _check_bar(f'fold from interior + ring {tag}', s[:, :M], ref, ref_abs, 9)
    assert torch.equal(s[:, M:], ident[:, M:]) and float(gm[:, M:].min()) == 9.0 == float(gm[:, M:].max())
    assert torch.equal(gm[:, :M], s[:, :M] * (y[:, :M] > 0).float())
    for yy in (0, 1, H - 2, H - 1):
        for xx in (0, 1, W - 2, W - 1):
            e = (s[:, :M, yy, xx].double() - ref[:, :, yy, xx]).abs()
            assert bool((e <= gamma(9) * ref_abs[:, :, yy, xx]).all()), (yy, xx)


def test_dgrad_ring_refuses_unsupported_shapes(lib):
    """ERR_UNSUPPORTED (not a launch, not a fallback) for gradient channels % 64, data channels % 128, H < 2 and for a channel count whose
    staging buffer needs more than 96 KB of LDS: (ceil(C * 10 / 5120) * 5120 + 8 * 8 * 128) * 4 bytes = 112 KB at C = 1600."""
    ring = torch.zeros(1 << 16, device=DEV)
    for C, M, H, W in ((96, 128, 8, 8), (64, 64, 8, 8), (64, 192, 8, 8), (64, 128, 1, 8), (1600, 128, 8, 8)):
        gy = torch.zeros(1, C, H, W, device=DEV)
        wr = torch.zeros(4, C, 3, M, device=DEV)
        with pytest.raises(L.LamaError) as ei:
            lib.dgrad_ring(L.view(gy), wr, M, ring, 1)
        assert ei.value.code == L.ERR_UNSUPPORTED, (C, M, H, W, ei.value.code)
    _sync()
    gy, wr = torch.zeros(1, 1536, 8, 8, device=DEV), torch.zeros(4, 1536, 3, 128, device=DEV)
    lib.dgrad_ring(L.view(gy), wr, 128, ring, 1)                                  # the largest accepted channel count launches
    _sync()
    assert float(ring.abs().max()) == 0.0
