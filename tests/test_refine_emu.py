"""CPU tests of the refinement kernels (lama_amd/csrc/refine.hip) through the host SIMT emulator against the CPU oracle
(oracle/refine_oracle.py): forward values against the restated kornia / torch ops, adjoints against torch autograd.

The case lists are module-level constants and every test body is a ``check_*(lib, case, dev)`` function: tests/test_refine_kernels_gpu.py
imports both and reruns the same cases with the same assertions through the production library on the MI355X (``dev='cuda'``)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lama_amd import _lib as L
from oracle import refine_oracle as R
from tests.emu import emu_lib

ACT_CASES = [L.ACT_RELU, L.ACT_SIGMOID, L.ACT_TANH, L.ACT_NONE]
PAD_CASES = [(1, 7, 9), (3, 12, 5), (2, 4, 4), (3, 8, 11)]                       # (pad, H, W)
PAD_FUSED_CASES = [(1, 8, 8), (1, 6, 12), (3, 12, 5), (2, 4, 4), (3, 8, 16)]     # (pad, H, W): W % 4 == 0 -> 16-byte path
RING_CASES = [(8, 8), (5, 12), (20, 7), (3, 3), (2, 4)]                          # (H, W)
GAUSS_CASES = [(16, 24, 16, 24), (16, 24, 13, 21), (9, 8, 5, 6)]                 # (XH, XW, H, W): the blur of the top-left crop
BILINEAR_CASES = [(16, 24, 8, 12), (13, 21, 6, 10), (9, 7, 4, 3), (10, 12, 17, 20), (8, 8, 8, 8)]   # (H, W, Ho, Wo)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


def check_act_bwd_and_add(lib, act, dev='cpu'):
    x = torch.randn(2, 5, 7, 9, generator=_g(1), requires_grad=True)
    y = {L.ACT_RELU: torch.relu, L.ACT_SIGMOID: torch.sigmoid, L.ACT_TANH: torch.tanh, L.ACT_NONE: lambda t: t * 1.0}[act](x)
    g = torch.randn(2, 5, 7, 9, generator=_g(2))
    y.backward(g)
    wide = torch.zeros(2, 8, 7, 9, device=dev)
    gd, yd = g.to(dev), y.detach().contiguous().to(dev)
    lib.act_bwd(L.view(gd), L.view(yd), act, L.view(wide, 2, 5), 2)
    _sync(dev)
    wh = wide.cpu()
    assert torch.allclose(wh[:, 2:7], x.grad, atol=1e-6) and float(wh[:, :2].abs().max()) == 0 and float(wh[:, 7:].abs().max()) == 0
    out = torch.zeros(2, 5, 7, 9, device=dev)
    lib.add(L.view(gd), L.view(wide, 2, 5), L.view(out), 2)
    _sync(dev)
    assert torch.equal(out.cpu(), g + wh[:, 2:7])


def check_reflect_pad_adjoint(lib, case, dev='cpu'):
    pad, H, W = case
    x = torch.randn(2, 3, H, W, generator=_g(3), requires_grad=True)
    xp = F.pad(x, (pad,) * 4, mode='reflect')
    gp = torch.randn(xp.shape, generator=_g(4))
    xp.backward(gp)
    add = torch.randn(2, 3, H, W, generator=_g(5))
    g = torch.zeros(2, 3, H, W, device=dev)
    gpd, addd = gp.to(dev), add.to(dev)
    lib.reflect_pad_bwd(L.view(gpd), None, pad, L.view(g), 2)
    _sync(dev)
    assert torch.allclose(g.cpu(), x.grad, atol=1e-6)
    lib.reflect_pad_bwd(L.view(gpd), L.view(addd), pad, L.view(g), 2)
    _sync(dev)
    assert torch.allclose(g.cpu(), x.grad + add, atol=1e-6)


def check_reflect_pad_adjoint_fused(lib, case, dev='cpu'):
    pad, H, W = case
    gp = torch.randn(2, 5, H + 2 * pad, W + 2 * pad, generator=_g(4))
    add1, add2 = torch.randn(2, 5, H, W, generator=_g(5)), torch.randn(2, 7, H, W, generator=_g(6))
    y = torch.randn(2, 7, H, W, generator=_g(7))
    gpd, add1d, add2d, yd = gp.to(dev), add1.to(dev), add2.to(dev), y.to(dev)
    foldd = torch.zeros(2, 5, H, W, device=dev)
    lib.reflect_pad_bwd(L.view(gpd), None, pad, L.view(foldd), 2)
    _sync(dev)
    fold = foldd.cpu()
    for act, d in ((L.ACT_RELU, (y > 0).float()), (L.ACT_TANH, 1 - y * y)):
        s = fold + add1 + add2[:, 2:7]
        gd, gmd = torch.full((2, 7, H, W), 9.0, device=dev), torch.full((2, 7, H, W), 9.0, device=dev)
        lib.reflect_pad_bwd_fused(L.view(gpd), L.view(add1d), L.view(add2d, 2, 5), pad, L.view(yd, 2, 5), act, L.view(gd, 2, 5), L.view(gmd, 2, 5), 2)
        _sync(dev)
        g, gm = gd.cpu(), gmd.cpu()
        assert torch.equal(g[:, 2:7], s) or torch.allclose(g[:, 2:7], s, atol=1e-6)
        assert torch.allclose(gm[:, 2:7], s * d[:, 2:7], atol=1e-6) and float(g[:, :2].min()) == 9.0 and float(gm[:, :2].min()) == 9.0
    # in place over the identity operand, no mask, one output at a time
    accd = add2.clone().to(dev)
    lib.reflect_pad_bwd_fused(L.view(gpd), None, L.view(accd, 2, 5), pad, None, L.ACT_NONE, L.view(accd, 2, 5), None, 2)
    _sync(dev)
    acc = accd.cpu()
    assert torch.allclose(acc[:, 2:7], fold + add2[:, 2:7], atol=1e-6) and torch.equal(acc[:, :2], add2[:, :2])
    gmd = torch.zeros(2, 5, H, W, device=dev)
    lib.reflect_pad_bwd_fused(L.view(gpd), None, None, pad, L.view(yd, 0, 5), L.ACT_RELU, None, L.view(gmd), 2)
    _sync(dev)
    assert torch.allclose(gmd.cpu(), fold * (y[:, :5] > 0).float(), atol=1e-6)
    with pytest.raises(L.LamaError):
        lib.reflect_pad_bwd_fused(L.view(gpd), None, None, pad, None, L.ACT_NONE, None, None, 2)


def check_dgrad_ring_and_fold_from_interior(lib, case, dev='cpu'):
    H, W = case
    cin, cout = 64, 128                                      # dgrad: 64 gradient channels in (8 channel groups x 8 channels ahead), 128 data channels out
    wf = torch.randn(cin, cout, 3, 3, generator=_g(8)) * 0.1   # forward conv weight [out = 64, in = 128]
    x = torch.randn(2, cout, H, W, generator=_g(9), requires_grad=True)
    gy = torch.randn(2, cin, H, W, generator=_g(10))
    F.conv2d(F.pad(x, (1,) * 4, mode='reflect'), wf).backward(gy)
    wd = wf.permute(1, 0, 2, 3).flip(2, 3).contiguous()      # w' [128, 64, 3, 3]
    gp = F.conv2d(F.pad(gy, (2,) * 4), wd)                   # the padded plane [2, 128, H + 2, W + 2]
    ringd = torch.full((lib.dgrad_ring_bytes(2, cout, H, W) // 4 + 3,), 5.0, device=dev)
    gyd, wrd = gy.to(dev), lib.dgrad_ring_weight(wd).to(dev)
    lib.dgrad_ring(L.view(gyd), wrd, cout, ringd, 2)
    _sync(dev)
    ring = ringd.cpu()
    r = ring[:-3].view(2, cout, -1)
    assert float(ring[-3:].min()) == 5.0
    assert torch.allclose(r[:, :, :W + 2], gp[:, :, 0], atol=1e-5) and torch.allclose(r[:, :, W + 2:2 * W + 4], gp[:, :, -1], atol=1e-5)
    assert torch.allclose(r[:, :, 2 * W + 4:2 * W + 4 + H], gp[:, :, 1:-1, 0], atol=1e-5)
    assert torch.allclose(r[:, :, 2 * W + 4 + H:], gp[:, :, 1:-1, -1], atol=1e-5)
    interior = gp[:, :, 1:-1, 1:-1].contiguous().to(dev)
    ident, y = torch.randn(2, cout, H, W, generator=_g(11)), torch.randn(2, cout, H, W, generator=_g(12))
    identd, yd = ident.to(dev), y.to(dev)
    gd, gmd = torch.zeros(2, cout, H, W, device=dev), torch.zeros(2, cout, H, W, device=dev)
    lib.reflect_pad_bwd_fused(L.view(interior), None, L.view(identd), 1, L.view(yd), L.ACT_RELU, L.view(gd), L.view(gmd), 2, ring=ringd)
    _sync(dev)
    g, gm = gd.cpu(), gmd.cpu()
    assert torch.allclose(g, x.grad + ident, atol=2e-5), float((g - x.grad - ident).abs().max())
    assert torch.allclose(gm, (x.grad + ident) * (y > 0).float(), atol=2e-5)
    gpd = gp.to(dev)
    with pytest.raises(L.LamaError):
        lib.reflect_pad_bwd_fused(L.view(gpd), None, None, 1, None, L.ACT_NONE, L.view(gd), None, 2, ring=ringd)     # gp must be the interior
    _sync(dev)


def check_gauss5_crop_fwd_and_adjoint(lib, shape, dev='cpu'):
    XH, XW, H, W = shape
    x = torch.randn(2, 3, XH, XW, generator=_g(6), requires_grad=True)
    ref = R.gaussian_blur2d(x[:, :, :H, :W])
    y = torch.zeros(2, 3, H, W, device=dev)
    xd = x.detach().to(dev)
    lib.gauss5(L.view(xd), L.view(y), 2)
    _sync(dev)
    assert torch.allclose(y.cpu(), ref.detach(), atol=1e-6)
    gy = torch.randn(2, 3, H, W, generator=_g(7))
    ref.backward(gy)
    gx = torch.full((2, 3, XH, XW), 9.0, device=dev)
    gyd = gy.to(dev)
    lib.gauss5_bwd(L.view(gyd), L.view(gx), 2)
    _sync(dev)
    assert torch.allclose(gx.cpu(), x.grad, atol=1e-6)


def check_bilinear_fwd_and_adjoint(lib, shape, dev='cpu'):
    H, W, Ho, Wo = shape
    x = torch.randn(2, 3, H, W, generator=_g(8), requires_grad=True)
    ref = F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=False)
    y = torch.zeros(2, 3, Ho, Wo, device=dev)
    xd = x.detach().to(dev)
    lib.bilinear(L.view(xd), L.view(y), 2)
    _sync(dev)
    assert torch.allclose(y.cpu(), ref.detach(), atol=1e-6)
    gy = torch.randn(2, 3, Ho, Wo, generator=_g(9))
    ref.backward(gy)
    gx = torch.full((2, 3, H, W), 9.0, device=dev)
    gyd = gy.to(dev)
    lib.bilinear_bwd(L.view(gyd), L.view(gx), 2)
    _sync(dev)
    assert torch.allclose(gx.cpu(), x.grad, atol=1e-5)


def check_pyrdown_and_mask_pipeline(lib, dev='cpu'):
    im = torch.rand(1, 3, 21, 30, generator=_g(10))
    imd = im.to(dev)
    blur = torch.zeros_like(imd)
    lib.gauss5(L.view(imd), L.view(blur), 1)
    down = torch.zeros(1, 3, 10, 15, device=dev)
    lib.bilinear(L.view(blur), L.view(down), 1)
    _sync(dev)
    assert torch.allclose(down.cpu(), R.pyrdown(im), atol=1e-6)
    mask = (torch.rand(1, 1, 40, 44, generator=_g(11)) > 0.35).float()
    mask[:, :, 8:30, 10:36] = 1.0
    maskd = mask.to(dev)
    for blur_mask, round_up in ((True, True), (False, False)):
        src = maskd
        if blur_mask:
            src = torch.zeros_like(maskd)
            lib.gauss5(L.view(maskd), L.view(src), 1)
        small = torch.zeros(1, 1, 20, 22, device=dev)
        lib.bilinear(L.view(src), L.view(small), 1)
        out = torch.zeros_like(small)
        lib.threshold(L.view(small), 1e-8 if round_up else 1.0 - 1e-8, L.view(out), 1)
        _sync(dev)
        assert torch.equal(out.cpu(), R.pyrdown_mask(mask, blur_mask=blur_mask, round_up=round_up))
    se = R.ellipse_kernel(15)
    assert se.shape == (15, 15) and float(se.sum()) == 169 and float(se[0].sum()) == 1 and float(se[7].sum()) == 15 and torch.equal(se, se.flip(0, 1))
    er = torch.zeros_like(maskd)
    lib.erode(L.view(maskd), se.to(dev), L.view(er), 1)
    _sync(dev)
    assert torch.equal(er.cpu(), R.erosion(mask, se))
    out = torch.zeros_like(maskd)
    lib.threshold(L.view(er), 1.0 - 1e-8, L.view(out), 1)
    _sync(dev)
    assert torch.equal(out.cpu(), R.erode_mask(mask, se))
    se2 = torch.zeros(3, 5); se2[0, 1] = 1; se2[2, 4] = 1; se2[1, 2] = 1          # asymmetric element: kornia's flip matters
    er2 = torch.zeros_like(maskd)
    lib.erode(L.view(maskd), se2.to(dev), L.view(er2), 1)
    _sync(dev)
    assert torch.equal(er2.cpu(), R.erosion(mask, se2))


def check_masked_l1_and_adam(lib, dev='cpu'):
    g = _g(12)
    pred = torch.rand(1, 3, 9, 14, generator=g, requires_grad=True)
    image = torch.rand(1, 3, 9, 14, generator=g)
    image[0, 1, 2, 3] = float(pred[0, 1, 2, 3])                 # an exact tie: abs'(0) = 0
    mask = (torch.rand(1, 1, 9, 14, generator=g) > 0.5).float()
    m3 = mask.repeat(1, 3, 1, 1)
    loss = torch.mean(torch.abs(pred[m3 < 1e-8] - image[m3 < 1e-8]))
    loss.backward()
    predd, imaged, maskd, m3d = pred.detach().to(dev), image.to(dev), mask.to(dev), m3.to(dev)
    accd = torch.zeros(2, dtype=torch.float64, device=dev)
    lib.l1_masked(L.view(predd), L.view(imaged), L.view(maskd), 1e-8, False, accd, 1)
    _sync(dev)
    acc = accd.cpu()
    assert int(acc[1]) == int((m3 < 1e-8).sum()) and abs(float(acc[0] / acc[1]) - float(loss)) < 1e-6
    gbuf = torch.full((1, 3, 9, 14), 5.0, device=dev)
    lib.l1_masked_bwd(L.view(predd), L.view(imaged), L.view(maskd), 1e-8, False, float(1.0 / acc[1]), False, L.view(gbuf), 1)
    _sync(dev)
    assert torch.allclose(gbuf.cpu(), pred.grad, atol=1e-7)
    lib.l1_masked_bwd(L.view(predd), L.view(imaged), L.view(m3d), 1e-8, True, 0.25, True, L.view(gbuf), 1)   # accumulate, 3-channel mask, >=
    _sync(dev)
    assert torch.allclose(gbuf.cpu(), pred.grad + 0.25 * torch.sign(pred.detach() - image) * (m3 >= 1e-8), atol=1e-7)
    # Adam against torch.optim.Adam, three steps
    p0 = torch.randn(1000, generator=g)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=0.002)
    ph, m, v = p0.clone().to(dev), torch.zeros(1000, device=dev), torch.zeros(1000, device=dev)
    for step in range(1, 4):
        gr = torch.randn(1000, generator=g) * (10.0 ** (step - 2))
        opt.zero_grad(); pt.grad = gr.clone(); opt.step()
        lib.adam_step(ph, gr.to(dev), m, v, 0.002, step)
        _sync(dev)
        assert torch.allclose(ph.cpu(), pt.detach(), atol=1e-6, rtol=1e-5), step


@pytest.mark.parametrize('act', ACT_CASES)
def test_act_bwd_and_add(act):
    check_act_bwd_and_add(emu_lib(), act)


@pytest.mark.parametrize('case', PAD_CASES)
def test_reflect_pad_adjoint(case):
    check_reflect_pad_adjoint(emu_lib(), case)


@pytest.mark.parametrize('case', PAD_FUSED_CASES)
def test_reflect_pad_adjoint_fused(case):
    """lama_reflect_pad_bwd_fused (v108): fold + the 1x1 path + the identity path (in place) + the activation derivative of the layer upstream,
    against the separate launches it replaces; W % 4 == 0 takes the 16-byte path, the rest the scalar one; views with a channel offset."""
    check_reflect_pad_adjoint_fused(emu_lib(), case)


@pytest.mark.parametrize('case', RING_CASES)
def test_dgrad_ring_and_fold_from_interior(case):
    """Round 4 (v108): the data gradient of a reflect-padded 3x3 conv without its padded plane -- lama_dgrad_ring_fwd computes the one-pixel
    frame of the zero-padded correlation (exact fp32), lama_reflect_pad_bwd_fused(ring=...) folds it onto the interior (a zero-pad-1 conv).
    Reference: autograd through F.pad(mode='reflect') + conv2d."""
    check_dgrad_ring_and_fold_from_interior(emu_lib(), case)


@pytest.mark.parametrize('shape', GAUSS_CASES)
def test_gauss5_crop_fwd_and_adjoint(shape):
    check_gauss5_crop_fwd_and_adjoint(emu_lib(), shape)


@pytest.mark.parametrize('shape', BILINEAR_CASES)
def test_bilinear_fwd_and_adjoint(shape):
    check_bilinear_fwd_and_adjoint(emu_lib(), shape)


def test_pyrdown_and_mask_pipeline():
    """refinement.py:19-73: _pyrdown / _pyrdown_mask / _erode_mask restated with the HIP kernels."""
    check_pyrdown_and_mask_pipeline(emu_lib())


def test_masked_l1_and_adam():
    check_masked_l1_and_adam(emu_lib())
