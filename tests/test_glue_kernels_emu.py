"""CPU tests of the glue kernels through the host SIMT emulator: the two ends of the u8 predict step (mask_compose_u8 / blend_quantize_u8), the
fp32 compose / blend / quantise entries on channel-slice views, the stand-alone layers (affine_act, reflect_pad), SSIM through ``lib.ssim`` and
the deferred Winograd output transform feeding a FourierUnit -- each against a plain host reference (tests/glue_ref.py, oracle/eval_oracle.py).

The case lists are module-level constants and every test body is a ``check_*(lib, case, dev)`` function: tests/test_glue_kernels_gpu.py
imports both and reruns the same cases with the same assertions through the production library on the MI355X (``dev='cuda'``).

Every output is a view of a wider buffer (extra channels before and after, or guard bytes after a u8 buffer) filled with a sentinel (7.0 /
0xA5) that must survive.  No tolerance is tuned to what a kernel returned:
  * bit-equality with the fp32 restatement where nothing can be contracted (compose, reflect_pad, quantise, affine_act without scale) or the
    sum has an exact zero term (blend with a {0, 1} mask);
  * ``m * pred + k * img`` with a fractional mask and ``x * scale + shift``: the output must equal ONE legal evaluation (unfused, first product
    fused, second product fused) everywhere in the case; which one is printed (-s);
  * sigmoid / tanh: 4 units, the unit being the largest distance of torch's own CPU fp32 function from its fp64 evaluation on the same inputs
    (the margin tests/test_lpips_gpu.py gives one fp32 evaluation in another order);
  * SSIM: 2e-6 absolute per image against the oracle in fp64 (the bar of tests/test_eval_gpu.py, inputs in [0, 1])."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lama_amd import _lib as L
from oracle import eval_oracle as EO
from tests import glue_ref as GR
from tests import test_kernels_emu as KE
from tests.emu import emu_lib

SENT, GUARD, NGUARD = 7.0, 0xA5, 64

# ---- the u8 ends of the predict step: (B, Hp, Wp, per-image (h, w) or None) --------------------------------------------------------------
U8_CASES = [
    (3, 16, 24, [(16, 24), (13, 19), (0, 0)]),          # a full slot, a ragged one (3 padded rows, 5 padded columns), an empty one -> zeros
    (4, 8, 8, [(3, 8), (8, 2), (2, 3), (1, 1)]),        # padding wider than the image: np.pad(mode='symmetric') is periodic
    (2, 11, 13, None),                                  # sizes = None: every image fills its slot
    (3, 424, 416, [(424, 416), (401, 397), (7, 5)]),    # 529,152 pixels > 2048 workgroups x 256: the grid-stride loop takes a second trip
]
U8_IDS = ['3x16x24_ragged_empty', '4x8x8_pad_wider_than_image', '2x11x13_no_sizes', '3x424x416_grid_stride']

# ---- fp32 compose / blend / quantise on views: (B, H, W) -----------------------------------------------------------------------------------
EW_CASES = [(2, 5, 7),            # hw odd
            (2, 40, 56),
            (3, 424, 416)]        # past the 2048-workgroup cap
# ---- affine_act: (B, C, H, W, act, with scale / shift) ----------------------------------------------------------------------------------
AFFINE_CASES = [(2, C, 5, 7, act, aff) for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_SIGMOID, L.ACT_TANH) for aff in (False, True) for C in (1, 5)]
AFFINE_CASES += [(1, 5, 330, 320, L.ACT_SIGMOID, True), (1, 5, 330, 320, L.ACT_RELU, True)]      # 528,000 elements: past the cap
# ---- reflect_pad: (B, C, H, W, pad); pad = min(H, W) - 1 is the largest the entry accepts ------------------------------------------------
PAD_CASES = [(2, 3, 5, 7, 0), (2, 3, 5, 7, 1), (2, 3, 5, 7, 3), (2, 3, 5, 7, 4), (2, 1, 9, 4, 3), (1, 3, 416, 420, 3)]
# ---- SSIM: (B, C, H, W, window, pair) -------------------------------------------------------------------------------------------------------
SSIM_PAIRS = ('identical', 'near', 'independent')
SSIM_PLANES = [(5, 7),           # smaller than the window radius
               (17, 33), (37, 70),   # one pixel past a tile in both directions; ragged, several tiles
               (16, 32)]         # exactly one tile
SSIM_WINDOWS = (1, 3, 7, 11, 15)
SSIM_CASES = []
for _i, (_h, _w) in enumerate(SSIM_PLANES):
    for _j, _ws in enumerate(SSIM_WINDOWS):
        _n = _i * len(SSIM_WINDOWS) + _j
        SSIM_CASES.append(((1, 3)[(_i + _j) % 2], (3, 1)[(_n // 2) % 2], _h, _w, _ws, SSIM_PAIRS[_n % 3]))
SSIM_CASES += [(1, 3, 160, 288, 11, 'independent'),       # 270 tiles per image: ssim_reduce_kernel's second trip (per_image > 256)
               (3, 3, 160, 288, 15, 'near'), (1, 3, 160, 288, 7, 'identical')]
SSIM_BAR = 2e-6
# ---- the deferred Winograd output transform in front of a FourierUnit: the plane size of the FourierUnit ---------------------------------
WINO_FU_PLANES = [64,     # the transform rides inside the rfft2 launch (the one-buffer 64 x 64 kernel)
                  32]     # no kernel does both: winograd_out, then rfft2
WINO_FU_CASE = dict(cin=32, cout=128, H=16, W=32, B=1, act=1, bias=True, resid=True, scale=True)
WINO_PRECS = [L.PREC_BF16X3, L.PREC_F16X3]
WINO_PREC_IDS = ['bf16x3', 'f16x3']


def _st(dev):
    return 0 if dev == 'cpu' else torch.cuda.current_stream().cuda_stream


def _sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _wide(t, pre, post, dev, fill=SENT):
    """``t`` [B,C,H,W] as channels [pre, pre + C) of a wider buffer on ``dev`` whose other channels hold ``fill``: (buffer, view)."""
    B, C, H, W = t.shape
    buf = torch.full((B, pre + C + post, H, W), fill, dtype=t.dtype)
    buf[:, pre:pre + C] = t
    buf = buf.to(dev)
    return buf, L.view(buf, pre, C)


def _out(B, C, H, W, pre, post, dev):
    buf = torch.full((B, pre + C + post, H, W), SENT, device=dev)
    return buf, L.view(buf, pre, C)


def _take(buf, pre, C, dev):
    """The written channels of an output buffer on the host, after asserting that every other channel kept the sentinel."""
    _sync(dev)
    h = buf.cpu()
    rest = torch.cat([h[:, :pre], h[:, pre + C:]], 1)
    assert rest.numel() > 0 and float(rest.min()) == SENT == float(rest.max()), 'a channel outside the view was written'
    return h[:, pre:pre + C].contiguous().numpy()


def _u8_out(n, dev):
    return torch.full((n + NGUARD,), GUARD, dtype=torch.uint8, device=dev)


def _take_u8(buf, shape, dev):
    _sync(dev)
    h = buf.cpu().numpy()
    n = int(np.prod(shape))
    assert h.size == n + NGUARD and bool((h[n:] == GUARD).all()), 'bytes past the u8 output were written'
    return h[:n].reshape(shape)


def _bits_equal(got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref, dtype=got.dtype)
    if got.shape != ref.shape:
        return False
    return np.array_equal(got.view(np.uint32), ref.view(np.uint32)) if got.dtype == np.float32 else np.array_equal(got, ref)


def _first_diff(got, ref):
    d = np.argwhere(np.ascontiguousarray(got) != np.ascontiguousarray(ref))
    return None if d.size == 0 else (tuple(d[0]), got[tuple(d[0])], ref[tuple(d[0])], len(d))


# =====================================================================================================================================
# operands (host): shared by the checks and by the fp64 / longdouble cross-check of the contraction variants
# =====================================================================================================================================
def u8_case_operands(case, binarize):
    B, Hp, Wp, sizes = case
    img, mask = GR.u8_operands(B, Hp, Wp, seed=100 + Hp)
    pred = (torch.rand(B, 3, Hp, Wp, generator=_g(200 + Wp)) * 1.2 - 0.1).numpy()      # [-0.1, 1.1]: both clips of the quantisation are hit
    img_f, m = GR.host_image_mask(img, mask, sizes, binarize)
    return img, mask, pred, img_f, m


def ew_case_operands(case, fractional):
    B, H, W = case
    g = _g(300 + H)
    img = torch.rand(B, 3, H, W, generator=g).numpy()
    pred = (torch.rand(B, 3, H, W, generator=g) * 1.2 - 0.1).numpy()
    m = torch.rand(B, 1, H, W, generator=g)
    m = (m if fractional else (m > 0.5).float()).numpy()
    if fractional:
        m.reshape(-1)[:2] = (0.0, 1.0)
    return img, m, pred


def affine_case_operands(case):
    B, C, H, W, act, aff = case
    g = _g(400 + C + 7 * act + H)
    x = torch.where(torch.rand(B, C, H, W, generator=g) < 0.5, torch.rand(B, C, H, W, generator=g) * 40 - 20, torch.randn(B, C, H, W, generator=g))
    x.view(-1)[:2] = torch.tensor([-20.0, 20.0])                                          # sigmoid and tanh saturate
    scale = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)
    shift = torch.randn(C, generator=g)
    return x.numpy(), scale.numpy(), shift.numpy()


# =====================================================================================================================================
# checks
# =====================================================================================================================================
def check_u8_predict_ends(lib, case, binarize, dev='cpu'):
    """lama_mask_compose_u8_fwd and lama_blend_quantize_u8_fwd against the loader's chain in numpy (tests/glue_ref.py).  Compose: bit-equal.
    Blend + quantise: byte-equal to one legal evaluation of the sum (all three coincide for a {0, 1} mask), and byte-equal to
    quantize_u8_hwc(blend(...)) of the host-built fp32 operands on the same device (the contract of forward_u8).  Returns the variant."""
    B, Hp, Wp, sizes = case
    st = _st(dev)
    img, mask, pred, img_f, m = u8_case_operands(case, binarize)
    imgd, maskd = torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev)
    szd = None if sizes is None else torch.tensor(sizes, dtype=torch.int32).to(dev)
    obuf, oview = _out(B, 4, Hp, Wp, 1, 2, dev)
    lib.mask_compose_u8(imgd, maskd, szd, oview, B, binarize, st)
    got = _take(obuf, 1, 4, dev)
    want = GR.compose(img_f, m)
    assert _bits_equal(got, want), ('mask_compose_u8', _first_diff(got, want))
    if sizes is not None:
        for b, (h, w) in enumerate(sizes):
            if h == 0:
                assert float(np.abs(got[b]).max()) == 0.0                                   # an empty slot comes out as zeros
    pbuf, pview = _wide(torch.from_numpy(pred), 2, 1, dev, fill=3.0)
    dst = _u8_out(B * Hp * Wp * 3, dev)
    lib.blend_quantize_u8(imgd, maskd, szd, pview, dst, B, binarize, st)
    got8 = _take_u8(dst, (B, Hp, Wp, 3), dev)
    variants = {k: GR.quantize_hwc(v) for k, v in GR.blend_variants(img_f, m, pred).items()}
    name = GR.match_variant(got8, variants)
    print(f'[glue] blend_quantize_u8 {B}x{Hp}x{Wp} binarize={binarize}: matched "{name}"')
    assert name is not None, ('blend_quantize_u8 equals no legal evaluation', {k: _first_diff(got8, v) for k, v in variants.items()})
    assert 0 in got8 and 255 in got8                                                        # both clips were hit
    if binarize:
        assert all(np.array_equal(v, variants['unfused']) for v in variants.values())       # an exact zero term: nothing to choose
    # the same result from the fp32 entries on the same device
    ibuf, iview = _wide(torch.from_numpy(img_f), 1, 1, dev, fill=3.0)
    mbuf, mview = _wide(torch.from_numpy(m), 2, 0, dev, fill=3.0)
    bbuf, bview = _out(B, 3, Hp, Wp, 3, 1, dev)
    lib.blend(iview, mview, pview, bview, B, st)
    dst2 = _u8_out(B * Hp * Wp * 3, dev)
    lib.quantize_u8_hwc(bview, dst2, B, Hp, Wp, st)
    _take(bbuf, 3, 3, dev)
    chain = _take_u8(dst2, (B, Hp, Wp, 3), dev)
    assert np.array_equal(got8, chain), ('blend_quantize_u8 != quantize_u8_hwc(blend(...))', _first_diff(got8, chain))
    return name


def check_elementwise_views(lib, case, fractional, dev='cpu'):
    """lama_mask_compose_fwd, lama_blend_fwd and lama_quantize_u8_hwc_fwd with every operand a channel-slice view of a wider buffer
    (batch_stride > C * H * W, as the plan's static buffers are).  Returns the contraction variant blend matched."""
    B, H, W = case
    st = _st(dev)
    img, m, pred = ew_case_operands(case, fractional)
    ibuf, iview = _wide(torch.from_numpy(img), 1, 1, dev, fill=3.0)
    mbuf, mview = _wide(torch.from_numpy(m), 2, 0, dev, fill=3.0)
    pbuf, pview = _wide(torch.from_numpy(pred), 2, 1, dev, fill=3.0)
    obuf, oview = _out(B, 4, H, W, 1, 2, dev)
    lib.mask_compose(iview, mview, oview, B, st)
    got = _take(obuf, 1, 4, dev)
    want = GR.compose(img, m)
    assert _bits_equal(got, want), ('mask_compose', _first_diff(got, want))
    bbuf, bview = _out(B, 3, H, W, 3, 1, dev)
    lib.blend(iview, mview, pview, bview, B, st)
    got = _take(bbuf, 3, 3, dev)
    variants = GR.blend_variants(img, m, pred)
    name = GR.match_variant(got, variants)
    print(f'[glue] blend {B}x{H}x{W} {"fractional" if fractional else "binary"} mask: matched "{name}"')
    assert name is not None, ('blend equals no legal evaluation', {k: _first_diff(got, v) for k, v in variants.items()})
    if not fractional:
        assert all(_bits_equal(v, variants['unfused']) for v in variants.values())
    for ch, cw in ((H, W), (H - 2, W - 3)):                                                 # the whole plane and a crop
        dst = _u8_out(B * ch * cw * 3, dev)
        lib.quantize_u8_hwc(pview, dst, B, ch, cw, st)
        got8 = _take_u8(dst, (B, ch, cw, 3), dev)
        want8 = GR.quantize_hwc(pred, ch, cw)
        assert np.array_equal(got8, want8), ('quantize_u8_hwc', ch, cw, _first_diff(got8, want8))
        assert 0 in got8 and 255 in got8
    for buf, t, pre in ((ibuf, img, 1), (mbuf, m, 2), (pbuf, pred, 2)):                     # the inputs are untouched
        _sync(dev)
        assert _bits_equal(buf.cpu()[:, pre:pre + t.shape[1]].contiguous().numpy(), t)
    return name


_ACT_FN = {L.ACT_SIGMOID: torch.sigmoid, L.ACT_TANH: torch.tanh}
ACT_BAR_UNITS = 4.0


def check_affine_act(lib, case, dev='cpu'):
    """lama_affine_act_fwd (stand-alone BatchNorm2dEval / ReLU / Sigmoid / Tanh).  act none / ReLU: bit-equal to one legal evaluation of
    x * scale + shift (to x itself without scale).  Sigmoid / tanh: within 4 units of the fp64 function of one legal evaluation of the affine
    step, unit = the largest |torch CPU fp32 fn - fp64 fn| on those inputs.
    Measured: unit 5.4e-8 .. 8.9e-8 (sigmoid) / 2.8e-8 .. 3.0e-8 (tanh); the MI355X is at 1.00 / 1.83 units at the worst
    (tests/test_glue_kernels_gpu.py::test_affine_act).  Returns (variant, unit, ratio)."""
    B, C, H, W, act, aff = case
    st = _st(dev)
    x, scale, shift = affine_case_operands(case)
    xbuf, xview = _wide(torch.from_numpy(x), 1, 1, dev, fill=3.0)
    ybuf, yview = _out(B, C, H, W, 2, 1, dev)
    sd, hd = (torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)) if aff else (None, None)
    lib.affine_act(xview, sd, hd, act, yview, B, st)
    got = _take(ybuf, 2, C, dev)
    variants = GR.affine_variants(x, scale, shift) if aff else {'no affine step': x}
    tag = f'affine_act act={act} affine={aff} {B}x{C}x{H}x{W}'
    if act in (L.ACT_NONE, L.ACT_RELU):
        if act == L.ACT_RELU:
            variants = {k: np.maximum(v, np.float32(0)) for k, v in variants.items()}
        name = GR.match_variant(got, variants)
        print(f'[glue] {tag}: matched "{name}"')
        assert name is not None, (tag, {k: _first_diff(got, v) for k, v in variants.items()})
        return name, 0.0, 0.0
    best = None
    for name, v in variants.items():
        ref, unit = GR.act_unit(v, _ACT_FN[act])
        err = float((torch.from_numpy(got).double() - ref).abs().max())
        assert unit > 0
        if best is None or err / unit < best[2]:
            best = (name, unit, err / unit)
    print(f'[glue] {tag}: unit = {best[1]:.3e}, worst error = {best[2]:.3f} units against "{best[0]}" (bar {ACT_BAR_UNITS})')
    assert best[2] <= ACT_BAR_UNITS, (tag, best)
    assert float(got.min()) < 0.01 + (-1.0 if act == L.ACT_TANH else 0.0) and float(got.max()) > 0.99      # both saturated ends are present
    return best


def check_reflect_pad(lib, case, dev='cpu'):
    """lama_reflect_pad_fwd (stand-alone nn.ReflectionPad2d) bit-equal to F.pad(mode='reflect')."""
    B, C, H, W, pad = case
    x = torch.randn(B, C, H, W, generator=_g(500 + H + pad))
    xbuf, xview = _wide(x, 1, 1, dev, fill=3.0)
    ybuf, yview = _out(B, C, H + 2 * pad, W + 2 * pad, 2, 1, dev)
    lib.reflect_pad(xview, pad, yview, B, _st(dev))
    got = _take(ybuf, 2, C, dev)
    want = F.pad(x, (pad,) * 4, mode='reflect').numpy() if pad else x.numpy()
    assert _bits_equal(got, want), ('reflect_pad', case, _first_diff(got, want))


def _refused(code, fn, *a, **kw):
    with pytest.raises(L.LamaError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, (fn.__name__, ei.value.code, code)


def check_glue_refusals(lib, dev='cpu'):
    """Every refusal of the glue entries, by code: wrong channel counts, mismatched H / W, pad >= H, scale without shift, a crop larger than
    the plane (ERR_BAD_ARG); fp16 views (ERR_UNSUPPORTED).  Nothing is launched: the outputs keep their fill."""
    st = _st(dev)
    B, H, W = 2, 6, 8
    f = lambda c, h=H, w=W, dt=torch.float32: torch.full((B, c, h, w), SENT, dtype=dt, device=dev)      # noqa: E731
    img, mask, pred, o4, o3 = f(3), f(1), f(3), f(4), f(3)
    u8i, u8m = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=dev), torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
    dst = _u8_out(B * H * W * 3, dev)
    V, BAD, UNS = L.view, L.ERR_BAD_ARG, L.ERR_UNSUPPORTED
    h16 = lambda c, h=H, w=W: V(f(c, h, w, torch.float16))      # noqa: E731
    # mask_compose
    _refused(BAD, lib.mask_compose, V(f(4), 0, 2), V(mask), V(o4), B, st)                  # image channels
    _refused(BAD, lib.mask_compose, V(img), V(f(2)), V(o4), B, st)                         # mask channels
    _refused(BAD, lib.mask_compose, V(img), V(mask), V(o3), B, st)                         # output channels
    _refused(BAD, lib.mask_compose, V(img), V(f(1, H + 1)), V(o4), B, st)                  # mask H
    _refused(BAD, lib.mask_compose, V(img), V(mask), V(f(4, H, W + 1)), B, st)             # output W
    _refused(UNS, lib.mask_compose, h16(3), V(mask), V(o4), B, st)
    _refused(UNS, lib.mask_compose, V(img), V(mask), h16(4), B, st)
    # blend
    _refused(BAD, lib.blend, V(img), V(mask), V(f(4)), V(o3), B, st)                       # pred channels
    _refused(BAD, lib.blend, V(img), V(mask), V(pred), V(o4), B, st)                       # output channels
    _refused(BAD, lib.blend, V(img), V(mask), V(f(3, H, W - 1)), V(o3), B, st)             # pred W
    _refused(BAD, lib.blend, V(img), V(mask), V(pred), V(f(3, H - 1)), B, st)              # output H
    _refused(UNS, lib.blend, V(img), h16(1), V(pred), V(o3), B, st)
    _refused(UNS, lib.blend, V(img), V(mask), h16(3), V(o3), B, st)
    # quantize_u8_hwc
    _refused(BAD, lib.quantize_u8_hwc, V(o4), dst, B, H, W, st)                            # source channels
    _refused(BAD, lib.quantize_u8_hwc, V(pred), dst, B, H + 1, W, st)                      # a crop larger than the plane
    _refused(BAD, lib.quantize_u8_hwc, V(pred), dst, B, H, W + 1, st)
    _refused(BAD, lib.quantize_u8_hwc, V(pred), dst, B, 0, W, st)
    _refused(UNS, lib.quantize_u8_hwc, h16(3), dst, B, H, W, st)
    # the u8 ends
    _refused(BAD, lib.mask_compose_u8, u8i, u8m, None, V(o3), B, True, st)                 # output channels
    _refused(UNS, lib.mask_compose_u8, u8i, u8m, None, h16(4), B, True, st)
    _refused(BAD, lib.blend_quantize_u8, u8i, u8m, None, V(o4), dst, B, True, st)          # pred channels
    _refused(UNS, lib.blend_quantize_u8, u8i, u8m, None, h16(3), dst, B, True, st)
    # affine_act
    sc = torch.ones(3, device=dev)
    _refused(BAD, lib.affine_act, V(img), None, None, L.ACT_RELU, V(o4), B, st)            # channels
    _refused(BAD, lib.affine_act, V(img), None, None, L.ACT_RELU, V(f(3, H, W + 1)), B, st)
    _refused(BAD, lib.affine_act, V(img), None, None, L.ACT_RELU, V(f(3, H + 1)), B, st)
    _refused(BAD, lib.affine_act, V(img), sc, None, L.ACT_NONE, V(o3), B, st)              # scale without shift
    _refused(BAD, lib.affine_act, V(img), None, sc, L.ACT_NONE, V(o3), B, st)              # shift without scale
    _refused(UNS, lib.affine_act, h16(3), None, None, L.ACT_TANH, V(o3), B, st)
    _refused(UNS, lib.affine_act, V(img), None, None, L.ACT_TANH, h16(3), B, st)
    # reflect_pad
    _refused(BAD, lib.reflect_pad, V(img), 1, V(f(4, H + 2, W + 2)), B, st)                # channels
    _refused(BAD, lib.reflect_pad, V(img), 1, V(f(3, H + 2, W + 1)), B, st)                # output W
    _refused(BAD, lib.reflect_pad, V(img), 1, V(f(3, H + 1, W + 2)), B, st)                # output H
    _refused(BAD, lib.reflect_pad, V(img), H, V(f(3, 3 * H, W + 2 * H)), B, st)            # pad >= H
    _refused(BAD, lib.reflect_pad, V(f(3, W, H)), H, V(f(3, W + 2 * H, 3 * H)), B, st)     # pad >= W
    _refused(BAD, lib.reflect_pad, V(img), -1, V(f(3, H - 2, W - 2)), B, st)
    _refused(UNS, lib.reflect_pad, h16(3), 1, V(f(3, H + 2, W + 2)), B, st)
    _refused(UNS, lib.reflect_pad, V(img), 1, h16(3, H + 2, W + 2), B, st)
    _sync(dev)
    for t in (o4, o3):
        assert float(t.min()) == SENT == float(t.max())
    assert bool((dst.cpu() == GUARD).all())


def ssim_case_operands(case):
    B, C, H, W, ws, pair = case
    g = _g(600 + H + ws)
    a = torch.rand(B, C, H, W, generator=g)
    if pair == 'identical':
        b = a.clone()
    elif pair == 'near':
        b = (a + 1e-3 * torch.randn(B, C, H, W, generator=g)).clamp(0, 1)
    else:
        b = torch.rand(B, C, H, W, generator=g)
    return a, b


def check_ssim(lib, case, dev='cpu'):
    """lama_ssim_fwd through lib.ssim on channel-slice views (batch_stride > C * H * W for both operands) against
    oracle/eval_oracle.ssim_per_image in fp64: 2e-6 absolute per image.  Returns the worst error."""
    B, C, H, W, ws, pair = case
    a, b = ssim_case_operands(case)
    ref = EO.ssim_per_image(a.double(), b.double(), ws)
    if pair == 'identical':
        assert float((ref - 1.0).abs().max()) < 1e-12
    abuf, aview = _wide(a, 1, 1, dev, fill=0.5)
    bbuf, bview = _wide(b, 2, 1, dev, fill=0.25)
    assert aview.batch_stride > C * H * W and bview.batch_stride > C * H * W and aview.batch_stride != bview.batch_stride
    nws = lib.ssim_workspace_bytes(B, C, H, W) // 4
    wsp = torch.full((nws + 8,), SENT, device=dev)
    out = torch.full((B + 4,), SENT, device=dev)
    lib.ssim(aview, bview, B, EO.gaussian_1d(ws).tolist(), out, wsp, _st(dev))
    _sync(dev)
    oh, wh = out.cpu(), wsp.cpu()
    assert float(oh[B:].min()) == SENT == float(oh[B:].max()) and float(wh[nws:].min()) == SENT == float(wh[nws:].max())
    err = float((oh[:B].double() - ref).abs().max())
    print(f'[glue] ssim {B}x{C}x{H}x{W} window {ws} {pair}: worst error = {err:.3e} ({err / SSIM_BAR:.3f} of the bar), ssim = {[round(v, 6) for v in ref.tolist()]}')
    assert err <= SSIM_BAR, (case, oh[:B].tolist(), ref.tolist())
    return err


def check_ssim_refusals(lib, dev='cpu'):
    """An even window and window 17: ERR_UNSUPPORTED.  A channel mismatch and a short workspace: ERR_BAD_ARG.  out keeps its fill."""
    B, C, H, W = 2, 3, 37, 70
    a, b = torch.rand(B, C + 2, H, W, generator=_g(7)).to(dev), torch.rand(B, C + 2, H, W, generator=_g(8)).to(dev)
    nws = lib.ssim_workspace_bytes(B, C, H, W) // 4
    assert nws == B * C * 3 * 3
    wsp, out, st = torch.zeros(nws, device=dev), torch.full((B,), SENT, device=dev), _st(dev)
    g11 = EO.gaussian_1d(11).tolist()
    _refused(L.ERR_UNSUPPORTED, lib.ssim, L.view(a, 1, C), L.view(b, 1, C), B, EO.gaussian_1d(10).tolist(), out, wsp, st)
    _refused(L.ERR_UNSUPPORTED, lib.ssim, L.view(a, 1, C), L.view(b, 1, C), B, EO.gaussian_1d(17).tolist(), out, wsp, st)
    _refused(L.ERR_BAD_ARG, lib.ssim, L.view(a, 1, C), L.view(b, 0, C - 1), B, g11, out, wsp, st)
    _refused(L.ERR_BAD_ARG, lib.ssim, L.view(a, 1, C), L.view(b, 1, C), B, g11, out, wsp[:nws - 1], st)
    _sync(dev)
    assert float(out.min()) == SENT == float(out.max())
    lib.ssim(L.view(a, 1, C), L.view(b, 1, C), B, g11, out, wsp, st)                       # the same call with a full workspace runs
    _sync(dev)
    ref = EO.ssim_per_image(a[:, 1:1 + C].cpu().double(), b[:, 1:1 + C].cpu().double(), 11)
    assert float((out.cpu().double() - ref).abs().max()) <= SSIM_BAR


def check_winograd_deferred_into_fourier_unit(lib, prec, n, dev='cpu'):
    """A Winograd local conv with LAMA_CONV_DEFER_OUT whose output transform is finished by the FourierUnit of the next layer
    (lama_fourier_unit_winograd_out_fwd, and lama_fourier_unit_ex_fwd with wino_args) on an n x n fp32 plane with C = 2 (spectral 4 -> 4):
    at 64 x 64 the transform rides inside the rfft2 launch, at 32 x 32 the entry falls back to winograd_out + rfft2.  Bit-equality only:
    the conv output with the one-call form, the FourierUnit output with lama_fourier_unit_fwd on the same input; the sentinel channels are
    intact and the deferred call itself wrote nothing."""
    st = _st(dev)
    o = KE.wino_operands(lib, WINO_FU_CASE, prec, dev)
    ybuf = torch.full((o.B, o.cout + 3, o.H, o.W), SENT, device=dev)
    KE.wino_run(lib, o, ybuf)
    _sync(dev)
    yh = ybuf.cpu()
    assert torch.allclose(yh[:, 2:2 + o.cout], o.ref, **o.tol) and float(yh[:, :2].min()) == SENT == float(yh[:, :2].max()) and float(yh[:, -1].min()) == SENT
    # the FourierUnit: fp32, C = 2
    g = _g(700 + n)
    Cn = 2
    x = torch.randn(1, Cn, n, n, generator=g)
    w1 = torch.randn(2 * Cn, 2 * Cn, 1, 1, generator=g) * 0.3
    scale, shift = torch.rand(2 * Cn, generator=g) + 0.5, torch.randn(2 * Cn, generator=g) * 0.2
    wp1 = lib.pack_conv_weight(w1.to(dev), scale.to(dev))
    shd = shift.to(dev)
    xbuf, xview = _wide(x, 1, 1, dev, fill=3.0)
    fws = torch.zeros(lib.fourier_unit_workspace_bytes(1, Cn, n, n) // 4 + 1, device=dev)
    for sib in (0, 1):                                                                       # 1: lama_fourier_unit_ex_fwd
        f0buf, f0view = _out(1, Cn, n, n, 2, 1, dev)
        lib.fourier_unit(xview, wp1, shd, f0view, 1, True, fws, stream=st, siblings_log2=sib)
        f0 = _take(f0buf, 2, Cn, dev)
        assert float(np.abs(f0 - x.numpy()).max()) > 1e-3                                   # the unit did something
        y2 = torch.full((o.B, o.cout + 3, o.H, o.W), SENT, device=dev)
        o.ws.zero_()
        pend = KE.wino_run(lib, o, y2, defer_out=True)
        _sync(dev)
        assert pend is not None and float(y2.min()) == SENT == float(y2.max())              # the deferred call wrote nothing
        fws.zero_()
        f1buf, f1view = _out(1, Cn, n, n, 2, 1, dev)
        lib.fourier_unit(xview, wp1, shd, f1view, 1, True, fws, stream=st, wino_out=(pend, o.ws), siblings_log2=sib)
        f1 = _take(f1buf, 2, Cn, dev)
        assert _bits_equal(f1, f0), ('FourierUnit output', n, sib, _first_diff(f1, f0))
        assert torch.equal(y2.cpu(), yh), ('conv output', n, sib)                            # sentinel channels included


# =====================================================================================================================================
# the emulator suite
# =====================================================================================================================================
@pytest.mark.parametrize('binarize', [True, False], ids=['binarize', 'fractional'])
@pytest.mark.parametrize('case', U8_CASES, ids=U8_IDS)
def test_u8_predict_ends(case, binarize):
    check_u8_predict_ends(emu_lib(), case, binarize)


@pytest.mark.parametrize('fractional', [False, True], ids=['binary', 'fractional'])
@pytest.mark.parametrize('case', EW_CASES, ids=lambda c: '%dx%dx%d' % c)
def test_elementwise_views(case, fractional):
    check_elementwise_views(emu_lib(), case, fractional)


@pytest.mark.parametrize('case', AFFINE_CASES, ids=lambda c: 'b%d_c%d_%dx%d_act%d_affine%d' % c)
def test_affine_act(case):
    check_affine_act(emu_lib(), case)


@pytest.mark.parametrize('case', PAD_CASES, ids=lambda c: 'b%d_c%d_%dx%d_pad%d' % c)
def test_reflect_pad(case):
    check_reflect_pad(emu_lib(), case)


def test_glue_refusals():
    check_glue_refusals(emu_lib())


@pytest.mark.parametrize('case', SSIM_CASES, ids=lambda c: 'b%d_c%d_%dx%d_w%d_%s' % c)
def test_ssim(case):
    check_ssim(emu_lib(), case)


def test_ssim_refusals():
    check_ssim_refusals(emu_lib())


@pytest.mark.parametrize('n', WINO_FU_PLANES)
@pytest.mark.parametrize('prec', WINO_PRECS, ids=WINO_PREC_IDS)
def test_winograd_deferred_into_fourier_unit(prec, n):
    check_winograd_deferred_into_fourier_unit(emu_lib(), prec, n)


def test_contraction_variants_do_not_depend_on_the_wide_type():
    """The fused evaluations of glue_ref are formed in fp64; a double-rounding tie would make such a reference wrong.  For the fixed seeds of
    every case above the same variants formed in longdouble agree bit for bit."""
    assert np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant
    for case in U8_CASES:
        _, _, pred, img_f, m = u8_case_operands(case, False)
        v64, vld = GR.blend_variants(img_f, m, pred), GR.blend_variants(img_f, m, pred, np.longdouble)
        assert all(_bits_equal(v64[k], vld[k]) for k in v64), case
    for case in EW_CASES:
        img, m, pred = ew_case_operands(case, True)
        v64, vld = GR.blend_variants(img, m, pred), GR.blend_variants(img, m, pred, np.longdouble)
        assert all(_bits_equal(v64[k], vld[k]) for k in v64), case
        assert not _bits_equal(v64['unfused'], v64['first product fused']) or case[1] * case[2] < 100      # the variants can be told apart
    for case in AFFINE_CASES:
        if case[5]:
            x, scale, shift = affine_case_operands(case)
            v64, vld = GR.affine_variants(x, scale, shift), GR.affine_variants(x, scale, shift, np.longdouble)
            assert all(_bits_equal(v64[k], vld[k]) for k in v64), case
