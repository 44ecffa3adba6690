"""Shared by tests/test_crop_shrink_emu.py, tests/test_crop_shrink_gpu.py and tests/test_crop_shrink_gloo.py: the numpy restatement of
lama_crop_shrink_compose_u8_fwd / lama_crop_shrink_paste_u8_fwd (csrc/elementwise.hip) and the checks the suites run -- through the host SIMT
emulator and on the GPU, through the same C ABI.

``crop_max_side`` has no counterpart in the reference.  ITS DEFINITION IS THE RESTATEMENT BELOW: the window of ``crop_to_mask`` shrunk by an
integer k for the generator -- k x k box means of the image in the integer-shrink arithmetic of lama_resize_u8_fwd, the MAX of each box's mask
bytes (a one-pixel stroke stays a hole) -- and, under the mask, the k-fold bilinear upsampling of the prediction (``paste_back_ref`` on the
cropped arrays, pasted by slicing).  The kernels are also held to the existing entries on host-cropped slots wherever those compute the same
thing: lama_resize_u8_fwd / ``predict._resize_area`` with factor 1 / k where k divides the window, lama_paste_back_u8_fwd always, and the crop
entries at k = 1.  There is no tolerance anywhere in this file: fp32 bit for bit, u8 byte for byte."""
import ctypes as C
import functools
import io
import os

import numpy as np
import torch

from lama_amd import _lib as L
from lama_amd import predict as P
from tests import crop_util as CU
from tests import paste_back_util as PB

F32 = np.float32
FAR = PB.FAR
CANARY = CU.CANARY
_stream, _sync, _same_bits = CU._stream, CU._sync, CU._same_bits


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def low_size(ch: int, cw: int, k: int):
    return (ch + k - 1) // k, (cw + k - 1) // k


def shrink_ref(c_u8: np.ndarray, m_u8: np.ndarray, k: int):
    """C [ch,cw,3] u8, M [ch,cw] u8 -> (S [dh,dw,3] float32, mu [dh,dw] u8).  A whole k x k box: each byte / 255.f, the box in row-major order summed
    four at a time as acc + (((a + b) + c) + d), the remainder one by one, times float32(1.0 / k^2); a box cut by the bottom / right edge: the
    row-major sum of the pixels inside, one by one, / float32(count).  mu = the max of the box's mask bytes, cut boxes included."""
    ch, cw = m_u8.shape
    dh, dw = low_size(ch, cw, k)
    fh, fw = ch // k, cw // k
    x = c_u8.astype(F32) / F32(255)
    S, mu = np.zeros((dh, dw, 3), F32), np.zeros((dh, dw), np.uint8)
    if fh and fw:
        box = x[:fh * k, :fw * k].reshape(fh, k, fw, k, 3).transpose(0, 2, 1, 3, 4).reshape(fh, fw, k * k, 3)
        acc, n = np.zeros((fh, fw, 3), F32), 0
        while n + 4 <= k * k:
            acc = acc + (((box[:, :, n] + box[:, :, n + 1]) + box[:, :, n + 2]) + box[:, :, n + 3])
            n += 4
        while n < k * k:
            acc = acc + box[:, :, n]
            n += 1
        S[:fh, :fw] = acc * F32(1.0 / (k * k))
    for y in range(dh):
        for xx in range(dw):
            ys, xs = slice(y * k, min(y * k + k, ch)), slice(xx * k, min(xx * k + k, cw))
            mu[y, xx] = m_u8[ys, xs].max()
            if y >= fh or xx >= fw:
                px = x[ys, xs].reshape(-1, 3)
                acc = np.zeros(3, F32)
                for t in px:
                    acc = acc + t
                S[y, xx] = acc / F32(len(px))
    assert S.dtype == F32
    return S, mu


def compose_ref(image_u8, mask_u8, rect, k, Hp, Wp, binarize) -> np.ndarray:
    """-> the generator's input [4,Hp,Wp] float32: cat(S * (1 - m), m) after the symmetric padding of the dh x dw planes."""
    y0, x0, ch, cw = rect
    S, mu = shrink_ref(image_u8[y0:y0 + ch, x0:x0 + cw], mask_u8[y0:y0 + ch, x0:x0 + cw], k)
    ys, xs = CU._symmetric(Hp, S.shape[0]), CU._symmetric(Wp, S.shape[1])
    S, m = S[ys][:, xs], CU._mask_f32(mu[ys][:, xs], binarize)
    out = np.concatenate([np.transpose(S * (F32(1) - m)[:, :, None], (2, 0, 1)), m[None]], 0)
    assert out.dtype == F32 and out.shape == (4, Hp, Wp)
    return out


def paste_ref(image_u8, mask_u8, rect, k, lowres_f32, binarize) -> np.ndarray:
    """-> [h,w,3] u8: the source, with ``paste_back_ref(C, M, lowres, (dh, dw))`` pasted into the window by slicing."""
    y0, x0, ch, cw = rect
    out = image_u8.copy()
    out[y0:y0 + ch, x0:x0 + cw] = PB.paste_back_ref(image_u8[y0:y0 + ch, x0:x0 + cw], mask_u8[y0:y0 + ch, x0:x0 + cw], lowres_f32,
                                                    low_size(ch, cw, k), binarize)
    return out


# ---- kernel cases ---------------------------------------------------------------------------------------------------------------------------
# name: (Hs, Ws, Hp, Wp, [(h, w, (y0, x0, ch, cw), k) or None per image])
CASES = {
    'k2-divisible': (12, 16, 8, 8, [(12, 16, (2, 4, 8, 8), 2)]),
    'k3': (20, 24, 8, 8, [(20, 24, (1, 3, 18, 21), 3)]),
    'k2-cut-boxes': (13, 11, 8, 8, [(13, 11, (0, 0, 13, 11), 2)]),                       # 7 x 6: a cut row, a cut column and the cut corner
    'k4-sums-of-four': (16, 32, 8, 8, [(16, 32, (0, 0, 16, 32), 4)]),
    'k5-remainder-loop': (20, 20, 8, 8, [(20, 20, (0, 0, 20, 20), 5)]),
    'k16-largest': (64, 64, 8, 8, [(64, 64, (0, 0, 64, 64), 16)]),
    'k16-cut': (50, 70, 8, 8, [(50, 70, (0, 0, 50, 70), 16)]),                           # 4 x 5
    'k1-is-the-crop': (9, 7, 8, 8, [(9, 7, (2, 1, 5, 4), 1)]),
    'x0-mod-4': (8, 24, 8, 8, [(8, 24, (1, x0, 6, 16), 2) for x0 in range(4)]),
    'ws-7-bytes': (8, 7, 8, 8, [(8, 7, (1, x0, 6, 4), 2) for x0 in range(4)]),
    'periodic-padding': (12, 16, 16, 12, [(12, 16, (2, 4, 6, 4), 2)]),                   # 3 x 2 padded to 16 x 12
    'unpadded-view': (16, 16, 7, 6, [(16, 16, (1, 2, 14, 12), 2)]),
    'mixed-k-one-empty': (24, 32, 8, 8, [(24, 32, (2, 4, 16, 16), 2), None, (20, 30, (1, 3, 18, 21), 3), (10, 13, (1, 3, 7, 5), 1)]),
    'two-workgroups': (128, 136, 72, 64, [(128, 136, (0, 4, 128, 128), 2)]),
    'rows-6x772': (6, 772, 8, 8, [(6, 772, (0, 700, 6, 16), 2)]),                        # the paste's row-wise form
}
LAYOUTS = CU.LAYOUTS


@functools.lru_cache(maxsize=None)
def case_data(name: str):
    """(image slots [B,Hs,Ws,3], mask slots [B,Hs,Ws], sizes [B,2], rects [B,4], shrinks [B], lowres [B,3,Hp,Wp]).  The slots outside an image
    hold 77 in image AND mask; lowres holds FAR outside each image's [:dh, :dw] (one read of it saturates a byte) and finite samples inside:
    the gather reads the neighbours of a pixel whatever the low-resolution mask says there."""
    Hs, Ws, Hp, Wp, images = CASES[name]
    B = len(images)
    img, msk = np.full((B, Hs, Ws, 3), 77, np.uint8), np.full((B, Hs, Ws), 77, np.uint8)
    ssz, rects, ks = np.zeros((B, 2), np.int32), np.zeros((B, 4), np.int32), np.zeros(B, np.int32)
    low = np.full((B, 3, Hp, Wp), FAR, F32)
    for j, it in enumerate(images):
        if it is None:
            continue
        h, w, (y0, x0, ch, cw), k = it
        img[j, :h, :w], msk[j, :h, :w] = CU._image(h, w, 10 * j + h), CU._mask(h, w, 10 * j + w)
        ssz[j], rects[j], ks[j] = (h, w), (y0, x0, ch, cw), k
        dh, dw = low_size(ch, cw, k)
        low[j, :, :dh, :dw] = CU._pred(dh, dw, 10 * j + ch)
    for a in (img, msk, ssz, rects, ks, low):
        a.setflags(write=False)
    return img, msk, ssz, rects, ks, low


def ref_want(img, msk, ssz, rects, ks, low, Hp, Wp, binarize):
    """The restatement over a slot batch -> (compose [B,4,Hp,Wp] float32, paste [B,Hs,Ws,3] u8): zeros for an empty slot, zeros outside h x w."""
    B = len(ssz)
    comp, paste = np.zeros((B, 4, Hp, Wp), F32), np.zeros_like(img)
    for j in range(B):
        h, w = ssz[j]
        if h > 0:
            comp[j] = compose_ref(img[j, :h, :w], msk[j, :h, :w], rects[j], int(ks[j]), Hp, Wp, binarize)
            paste[j, :h, :w] = paste_ref(img[j, :h, :w], msk[j, :h, :w], rects[j], int(ks[j]), low[j], binarize)
    return comp, paste


@functools.lru_cache(maxsize=None)
def case_want(name: str, binarize: bool):
    Hs, Ws, Hp, Wp, _ = CASES[name]
    comp, paste = ref_want(*case_data(name), Hp, Wp, binarize)
    comp.setflags(write=False)
    paste.setflags(write=False)
    return comp, paste


def run_kernels(lib, dev, img, msk, ssz, rects, ks, low, Hp, Wp, layout, binarize, shift=0):
    """One launch of each entry on copies of the operands -> (compose [B,4,Hp,Wp], paste [B,Hs,Ws,3]); asserts the canaries around both outputs
    and that no operand changed."""
    B, Hs, Ws = msk.shape
    f_img, t_img = CU.u8_at(img, dev, shift)
    f_msk, t_msk = CU.u8_at(msk, dev, shift)
    t_ssz, t_rc, t_k = (torch.from_numpy(a.copy()).to(dev) for a in (ssz, rects, ks))
    out = CU.F32View(B, 4, Hp, Wp, layout, dev)
    lo = CU.F32View(B, 3, Hp, Wp, layout, dev, data=low)
    f_out, t_out = CU.u8_at(img, dev, shift, fill=CANARY)
    lib.crop_shrink_compose_u8(t_img, t_msk, t_ssz, t_rc, t_k, out.view, B, binarize=binarize, stream=_stream(dev))
    lib.crop_shrink_paste_u8(t_img, t_msk, t_ssz, t_rc, t_k, lo.view, t_out, B, binarize=binarize, stream=_stream(dev))
    _sync(dev)
    comp, comp_guards = out.read()
    assert comp_guards, 'the compose wrote outside its view'
    assert CU.guards_intact(f_out, t_out), 'the paste wrote outside its slots'
    assert lo.unchanged() and CU.guards_intact(f_img, t_img) and CU.guards_intact(f_msk, t_msk)
    assert np.array_equal(t_img.cpu().numpy(), img) and np.array_equal(t_msk.cpu().numpy(), msk)
    assert np.array_equal(t_ssz.cpu().numpy(), ssz) and np.array_equal(t_rc.cpu().numpy(), rects) and np.array_equal(t_k.cpu().numpy(), ks)
    return comp, t_out.cpu().numpy()


check_outputs = CU.check_outputs


def _cropped_slots(img, msk, ssz, rects, Hc, Wc):
    """Host-cropped slots [B,Hc,Wc] holding each window in their top-left corner, 77 elsewhere, with sizes (ch, cw)."""
    B = len(ssz)
    c_img, c_msk, c_sz = np.full((B, Hc, Wc, 3), 77, np.uint8), np.full((B, Hc, Wc), 77, np.uint8), np.zeros((B, 2), np.int32)
    for j in range(B):
        if ssz[j, 0] > 0:
            y0, x0, ch, cw = rects[j]
            c_img[j, :ch, :cw], c_msk[j, :ch, :cw], c_sz[j] = img[j, y0:y0 + ch, x0:x0 + cw], msk[j, y0:y0 + ch, x0:x0 + cw], (ch, cw)
    return c_img, c_msk, c_sz


def check_against_entries(lib, dev, got, img, msk, ssz, rects, ks, low, Hp, Wp, binarize, what):
    """The second oracle, on HOST-CROPPED slots.  Paste: lama_paste_back_u8_fwd with sizes (ch, cw) / (dh, dw), pasted with numpy.  Compose, for
    every image whose window k divides (and all of whose batch shares k: the factor is one per launch): the image planes of lama_resize_u8_fwd
    with factor 1.0 / k and ``predict._resize_area(C / 255, 1.0 / k)``, times this engine's own (1 - m)."""
    comp, paste = got
    B = len(ssz)
    Hc, Wc = max(1, int(rects[:, 2].max())), max(1, int(rects[:, 3].max()))
    c_img, c_msk, c_sz = _cropped_slots(img, msk, ssz, rects, Hc, Wc)
    d_sz = np.array([low_size(ch, cw, int(k)) if k > 0 else (0, 0) for (ch, cw), k in zip(c_sz, ks)], np.int32)
    t_img, t_msk, t_sz, t_dsz = (torch.from_numpy(a).to(dev) for a in (c_img, c_msk, c_sz, d_sz))
    t_low = torch.from_numpy(np.array(low)).to(dev)
    blend = torch.zeros(B, Hc, Wc, 3, dtype=torch.uint8, device=dev)
    lib.paste_back_u8(t_img, t_msk, t_sz, t_dsz, L.view(t_low), blend, B, binarize=binarize, stream=_stream(dev))
    _sync(dev)
    blend = blend.cpu().numpy()
    for j in range(B):
        h, w = ssz[j]
        want = np.zeros_like(img[j])
        if h > 0:
            y0, x0, ch, cw = rects[j]
            want[:h, :w] = img[j, :h, :w]
            want[y0:y0 + ch, x0:x0 + cw] = blend[j, :ch, :cw]
        assert np.array_equal(paste[j], want), (what, 'paste_back_u8 on the cropped slots', j)
    for k in sorted(set(int(v) for v in ks if v > 0)):
        sel = [j for j in range(B) if ks[j] == k and rects[j, 2] % k == 0 and rects[j, 3] % k == 0]
        if not sel:
            continue
        f_img = torch.zeros(B, 3, Hp, Wp, dtype=torch.float32, device=dev)
        f_msk = torch.zeros(B, 1, Hp, Wp, dtype=torch.float32, device=dev)
        s_sz, s_dsz = c_sz.copy(), d_sz.copy()
        for j in range(B):
            if j not in sel:
                s_sz[j] = s_dsz[j] = (0, 0)
        lib.resize_u8(t_img, t_msk, torch.from_numpy(s_sz).to(dev), torch.from_numpy(s_dsz).to(dev), 1.0 / k, L.view(f_img), L.view(f_msk), B,
                      binarize=binarize, stream=_stream(dev))
        _sync(dev)
        f_img = f_img.cpu().numpy()
        for j in sel:
            y0, x0, ch, cw = rects[j]
            one_minus_m = F32(1) - comp[j, 3]
            assert _same_bits(comp[j, :3], f_img[j] * one_minus_m[None]), (what, 'resize_u8 on the cropped slots', j, k)
            dh, dw = low_size(ch, cw, k)
            area = P._resize_area(img[j, y0:y0 + ch, x0:x0 + cw].astype(F32) / F32(255), 1.0 / k)
            assert area.shape == (dh, dw, 3)
            assert _same_bits(comp[j, :3, :dh, :dw], np.transpose(area, (2, 0, 1)) * one_minus_m[None, :dh, :dw]), (what, '_resize_area', j, k)


def check_case(lib, dev, name, binarize, layout):
    """Both kernels against the restatement and against the existing entries on host-cropped slots; the source bytes wherever the mask byte is
    0 and outside the window; the low-resolution mask is the max rule."""
    Hs, Ws, Hp, Wp, _ = CASES[name]
    data = case_data(name)
    got = run_kernels(lib, dev, *data, Hp, Wp, layout, binarize)
    check_outputs(got, case_want(name, binarize), (name, binarize, layout, 'restatement'))
    check_against_entries(lib, dev, got, *data, Hp, Wp, binarize, (name, binarize, layout))
    img, msk, ssz, rects, ks, _ = data
    for j in range(len(ssz)):
        h, w = ssz[j]
        keep = msk[j, :h, :w] == 0
        assert np.array_equal(got[1][j, :h, :w][keep], img[j, :h, :w][keep])
        if h > 0:
            y0, x0, ch, cw = rects[j]
            outside = np.ones((h, w), bool)
            outside[y0:y0 + ch, x0:x0 + cw] = False
            assert np.array_equal(got[1][j, :h, :w][outside], img[j, :h, :w][outside])
            assert (got[1][j, :h, :w] != img[j, :h, :w]).any()
        else:
            assert not got[0][j].view(np.uint32).any() and not got[1][j].any()


def check_k1_is_the_crop(lib, dev):
    """k = 1 with binarize and finite samples: both entries give what lama_crop_compose_u8_fwd / lama_crop_paste_u8_fwd give."""
    for name in ('k1-is-the-crop', 'mixed-k-one-empty'):
        Hs, Ws, Hp, Wp, _ = CASES[name]
        img, msk, ssz, rects, ks, low = case_data(name)
        sel = np.flatnonzero(ks == 1)
        assert sel.size
        data = [np.ascontiguousarray(a[sel]) for a in (img, msk, ssz, rects)]
        k1, lo = np.ones(len(sel), np.int32), np.ascontiguousarray(low[sel])
        for layout in LAYOUTS:
            got = run_kernels(lib, dev, *data, k1, lo, Hp, Wp, layout, True)
            want = CU.run_kernels(lib, dev, *data, lo, Hp, Wp, layout, True)
            check_outputs(got, want, (name, layout, 'the crop entries'))


def check_misaligned_slots(lib, dev):
    """Slot pointers that are not 4-byte aligned take the byte path although Ws % 4 == 0: the same bits."""
    name = 'x0-mod-4'
    Hs, Ws, Hp, Wp, _ = CASES[name]
    for shift in (1, 2, 3):
        for binarize in (True, False):
            got = run_kernels(lib, dev, *case_data(name), Hp, Wp, 'plain', binarize, shift=shift)
            check_outputs(got, case_want(name, binarize), (name, binarize, shift))


def check_one_pixel_strokes(lib, dev):
    """For k in (2, 3, 16) and each of the k^2 positions inside a box: a mask with that single non-zero byte makes its low-resolution mask pixel
    a hole -- that pixel alone -- and the paste replaces exactly that source pixel.  One batch of k^2 images per k."""
    for k in (2, 3, 16):
        side = 3 * k
        B = k * k
        src = np.minimum(CU._image(side, side, k), 254)           # (no source byte is 255: a replaced pixel shows)
        img = np.broadcast_to(src, (B, side, side, 3)).copy()
        msk = np.zeros((B, side, side), np.uint8)
        for j in range(B):
            msk[j, k + j // k, k + j % k] = 1 + j % 255           # (inside the middle box; any non-zero byte)
        ssz, rects, ks = np.full((B, 2), side, np.int32), np.tile(np.array([0, 0, side, side], np.int32), (B, 1)), np.full(B, k, np.int32)
        low = np.full((B, 3, 8, 8), FAR, F32)
        low[:, :, :3, :3] = F32(2.0)                              # (every sample saturates: a replaced pixel is 255, 255, 255 with binarize)
        comp, paste = run_kernels(lib, dev, img, msk, ssz, rects, ks, low, 8, 8, 'plain', True)
        for j in range(B):
            hole = comp[j, 3, :3, :3]
            assert hole[1, 1] == 1 and hole.sum() == 1, (k, j)
            assert np.argwhere((paste[j] != src).any(-1)).tolist() == [[k + j // k, k + j % k]], (k, j)
            assert (paste[j, k + j // k, k + j % k] == 255).all(), (k, j)


# every way of not fitting for a 10 x 12 image in a 12 x 16 slot with a 4 x 4 view: (h, w, (y0, x0, ch, cw), k) -- the crop suite's table at
# k = 1 (its windows are 4 x 4, its 'ch > Hp' / 'cw > Wp' rows have 9), and the shrink's own
DOES_NOT_FIT = {why: (h, w, rect, 1) for why, (h, w, rect) in CU.DOES_NOT_FIT.items()}
DOES_NOT_FIT.update({'k = 0': (10, 12, (2, 2, 4, 4), 0), 'k = 17': (10, 12, (2, 2, 4, 4), 17), 'k < 0': (10, 12, (2, 2, 4, 4), -2),
                     'k = -2^31': (10, 12, (2, 2, 4, 4), -2 ** 31), 'dh > Hp': (10, 12, (0, 2, 5, 4), 1), 'dw > Wp': (10, 12, (2, 0, 4, 5), 1),
                     'dh > Hp at k = 2': (10, 12, (0, 2, 9, 4), 2), 'dw > Wp at k = 2': (10, 12, (2, 0, 4, 9), 2)})


def check_rects_that_do_not_fit(lib, dev, layout='plain'):
    """A batch of three -- a served image, an empty slot, a rect that does not fit -- for each way of not fitting: the compose writes zeros for
    that image and the paste its whole slot as 0, nothing out of bounds, the image beside them is served."""
    Hs, Ws, Hp, Wp = 12, 16, 4, 4
    good = (10, 12, (1, 3, 8, 7), 2)
    for why, bad in DOES_NOT_FIT.items():
        img, msk = np.full((3, Hs, Ws, 3), 200, np.uint8), np.full((3, Hs, Ws), 255, np.uint8)
        img[0, :10, :12], msk[0, :10, :12] = CU._image(10, 12, 4), CU._mask(10, 12, 4)
        ssz = np.array([good[:2], (0, 0), bad[:2]], np.int32)
        rects = np.array([good[2], (0, 0, 0, 0), bad[2]], np.int32)
        ks = np.array([good[3], 0, bad[3]], np.int32)
        low = CU._pred(Hp, Wp, 7)[None].repeat(3, 0)
        for binarize in (True, False):
            comp, paste = run_kernels(lib, dev, img, msk, ssz, rects, ks, low, Hp, Wp, layout, binarize)
            assert not comp[1:].view(np.uint32).any() and not paste[1:].any(), (why, binarize)
            assert _same_bits(comp[0], compose_ref(img[0, :10, :12], msk[0, :10, :12], good[2], good[3], Hp, Wp, binarize)), why
            want = np.zeros((Hs, Ws, 3), np.uint8)
            want[:10, :12] = paste_ref(img[0, :10, :12], msk[0, :10, :12], good[2], good[3], low[0], binarize)
            assert np.array_equal(paste[0], want), why


def check_non_finite(lib, dev):
    """A NaN sample quantises to 0 under the mask, +-1e38 saturate to 255 / 0, +-inf saturate wherever every tap has a weight (an infinite tap
    times a zero weight is a NaN: the clamped first row and column) -- the restatement's bytes in every case; no sample is read where the mask
    byte is 0 or outside the window."""
    img, msk = np.full((1, 8, 8, 3), 9, np.uint8), np.zeros((1, 8, 8), np.uint8)
    msk[0, :, 1:] = 255
    msk[0, 3, 3] = 128
    ssz, rects, ks = np.array([[8, 8]], np.int32), np.array([[2, 0, 4, 8]], np.int32), np.array([2], np.int32)
    for val, want in ((np.nan, 0), (np.inf, 255), (-np.inf, 0), (1e38, 255), (-1e38, 0)):
        low = np.full((1, 3, 8, 8), val, F32)
        for binarize in (True, False):
            comp, paste = run_kernels(lib, dev, img, msk, ssz, rects, ks, low, 8, 8, 'plain', binarize)
            assert np.array_equal(paste[0], paste_ref(img[0], msk[0], rects[0], 2, low[0], binarize)), (val, binarize)
            inner = paste[0, 3:5, 1:7] if np.isinf(val) else paste[0, 2:6, 1:]
            assert (inner == want).all(), (val, binarize)
            assert (paste[0, :, 0] == 9).all() and (paste[0, :2] == 9).all() and (paste[0, 6:] == 9).all(), (val, binarize)


def check_refusals(lib, dev):
    """Every LAMA_ERR_* case of both entries returns its code and launches nothing: the canary-filled outputs stay as they are."""
    name = 'x0-mod-4'
    Hs, Ws, Hp, Wp, _ = CASES[name]
    img, msk, ssz, rects, ks, low = case_data(name)
    B = len(ssz)
    t = [torch.from_numpy(a.copy()).to(dev) for a in (img, msk, ssz, rects, ks)]
    out = CU.F32View(B, 4, Hp, Wp, 'plain', dev)
    lo = CU.F32View(B, 3, Hp, Wp, 'plain', dev, data=low)
    f_out, t_out = CU.u8_at(img, dev, fill=CANARY)
    stream = _stream(dev)
    good = [x.data_ptr() for x in t]
    bad, uns = L.ERR_BAD_ARG, L.ERR_UNSUPPORTED

    def mod(view, **kw):
        w = L.Tensor4(view.ptr, view.batch_stride, view.C, view.H, view.W, view.dtype)
        for key, val in kw.items():
            setattr(w, key, val)
        return w

    def compose(ptrs=good, Hs=Hs, Ws=Ws, v=out.view, batch=B):
        rc = lib._l.lama_crop_shrink_compose_u8_fwd(stream, *ptrs, Hs, Ws, None if v is None else C.byref(v), batch, 1)
        _sync(dev)
        assert out.unchanged(), 'a refused compose wrote'
        return rc

    def paste(ptrs=good, Hs=Hs, Ws=Ws, v=lo.view, o=t_out.data_ptr(), batch=B):
        rc = lib._l.lama_crop_shrink_paste_u8_fwd(stream, *ptrs, Hs, Ws, None if v is None else C.byref(v), o, batch, 1)
        _sync(dev)
        assert bool((f_out == CANARY).all()), 'a refused paste wrote'
        return rc

    for call, view, ch in ((compose, out.view, 4), (paste, lo.view, 3)):
        for k in range(5):                                    # each null operand pointer, ``shrinks`` among them
            a = list(good)
            a[k] = None
            assert call(ptrs=a) == bad, (call.__name__, k)
        assert call(v=None) == bad and call(v=mod(view, ptr=None)) == bad
        assert call(batch=0) == bad and call(batch=-1) == bad
        assert call(Hs=0) == bad and call(Ws=0) == bad and call(Hs=-8) == bad and call(Ws=-8) == bad
        assert call(v=mod(view, C=ch + 1)) == bad and call(v=mod(view, C=1)) == bad
        assert call(v=mod(view, H=0)) == bad and call(v=mod(view, W=0)) == bad and call(v=mod(view, H=-8)) == bad
        assert call(v=mod(view, batch_stride=ch * Hp * Wp - 1)) == bad
        assert call(v=mod(view, ptr=view.ptr + 2)) == bad
        assert call(v=mod(view, dtype=L.DT_F16)) == uns and call(v=mod(view, dtype=L.DT_SPLIT16)) == uns
        assert call(v=mod(view, H=2 ** 16, W=2 ** 16, batch_stride=2 ** 40)) == uns
    assert paste(o=None) == bad
    assert paste(o=good[0]) == bad                                                             # in place
    assert paste(Hs=2 ** 30, Ws=8) == uns
    assert paste(Hs=2 ** 31 - 1, Ws=4096) == uns
    for fn, args in ((lib.crop_shrink_compose_u8, (mod(out.view, dtype=L.DT_F16),)), (lib.crop_shrink_paste_u8, (mod(lo.view, dtype=L.DT_F16), t_out))):
        try:
            fn(*t, *args, B, stream=stream)
        except L.LamaError as e:
            assert e.code == uns
        else:
            raise AssertionError('not refused')
    assert lib._l.lama_crop_shrink_compose_u8_fwd(stream, *good, Hs, Ws, C.byref(out.view), B, 1) == 0
    assert lib._l.lama_crop_shrink_paste_u8_fwd(stream, *good, Hs, Ws, C.byref(lo.view), t_out.data_ptr(), B, 1) == 0
    _sync(dev)
    check_outputs((out.read()[0], t_out.cpu().numpy()), case_want(name, True), 'after the refusals')
    assert out.read()[1] and CU.guards_intact(f_out, t_out)


# ---- crop_rect_limited ----------------------------------------------------------------------------------------------------------------------
def check_limited_properties(mask: np.ndarray, margin: int, step: int, pad_mod: int, max_side: int):
    """The properties of a served window, or None where ``crop_rect_limited`` refuses -- then no k up to 16 fits."""
    h, w = mask.shape
    mod = pad_mod if pad_mod > 1 else 1

    def at(k):
        y0, x0, ch, cw, _, _ = P.crop_rect(mask, margin * k, step * k, pad_mod)
        dh, dw = -(-ch // k), -(-cw // k)
        return y0, x0, ch, cw, k, dh, dw, -(-dh // mod) * mod, -(-dw // mod) * mod

    fits = [k for k in range(1, 17) if max(at(k)[7:]) <= max_side]
    try:
        got = P.crop_rect_limited(mask, margin, step, pad_mod, max_side)
    except L.LamaError as e:
        assert not fits and 'crop_max_side' in str(e)
        return None
    assert all(isinstance(v, int) for v in got) and len(got) == 9
    y0, x0, ch, cw, k, dh, dw, Hp, Wp = got
    assert fits and k == fits[0] and got == at(k)                                            # k is minimal
    ys, xs = np.flatnonzero((mask > 0).any(1)), np.flatnonzero((mask > 0).any(0))
    if ys.size:
        assert y0 <= ys[0] and ys[-1] < y0 + ch and x0 <= xs[0] and xs[-1] < x0 + cw
    assert 0 <= y0 and y0 + ch <= h and 0 <= x0 and x0 + cw <= w and ch >= 1 and cw >= 1
    assert Hp <= max_side and Wp <= max_side and Hp % mod == 0 and Wp % mod == 0
    assert dh == -(-ch // k) and dw == -(-cw // k) and dh <= Hp < dh + mod and dw <= Wp < dw + mod
    if k == 1:
        assert (y0, x0, ch, cw, Hp, Wp) == P.crop_rect(mask, margin, step, pad_mod)
    return got


# ---- HostFedStep, the loop and the CLI --------------------------------------------------------------------------------------------------------
MARGIN, STEP, PAD_MOD, MAX_SIDE = 4, 16, 8, 32
# (h, w), the mask's box (y, x, height, width) -> crop_rect_limited's (y0, x0, ch, cw, k, dh, dw, Hp, Wp) with the options above
PAIRS = [((40, 56), (10, 20, 8, 12)),     # box + 8 = 16 x 20 -> 16 x 32 at k = 1: fits
         ((72, 80), (20, 10, 30, 40)),    # k = 1: 48 x 48; k = 2 (margin 8, step 32): 46 x 56 -> 64 x 64 -> 32 x 32
         ((100, 110), (4, 6, 60, 70))]    # k = 2: 76 x 86 -> 96 x 96 -> 48 x 48; k = 3 (margin 12, step 48): 84 x 94 -> 96 x 96 -> 32 x 32
WINDOWS = [(6, 10, 16, 32, 1, 16, 32, 16, 32), (3, 0, 64, 64, 2, 32, 32, 32, 32), (0, 0, 96, 96, 3, 32, 32, 32, 32)]


def write_pairs(root, seed=3, pairs=None):
    """The three PNG pairs (or those of ``pairs``); each mask is a box of 255 with one pixel of 1 in its corner and zeros."""
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    for i, ((h, w), (by, bx, bh, bw)) in enumerate(PAIRS if pairs is None else pairs):
        mask = np.zeros((h, w), np.uint8)
        mask[by:by + bh, bx:bx + bw] = 255
        mask[by, bx] = 1
        Image.fromarray(CU._image(h, w, seed + i)).save(os.path.join(root, f'im{i}.png'))
        Image.fromarray(mask).save(os.path.join(root, f'im{i}_mask.png'))
    return P.list_dataset(root if root.endswith(os.sep) else root + os.sep, '.png')


def item_windows(items, windows=None, max_side=MAX_SIDE):
    wins = [P.crop_rect_limited(P.load_item_u8(*it)[1], MARGIN, STEP, PAD_MOD, max_side) for it in items]
    assert wins == (WINDOWS if windows is None else windows), wins
    return wins


def batches_of(wins, batch_size, shrink_k1=False, pairs=None):
    """[(Hp, Wp), shrunk?, source slot (Hs, Ws), item indices] per batch in the order of the loop: buckets keyed by the padded size and by
    whether k > 1 (``shrink_k1``: the k = 1 windows take the shrink step too, as the step tests run them)."""
    shapes = [(w[7], w[8]) if w[4] == 1 and not shrink_k1 else (w[7], w[8], 1) for w in wins]
    pairs = PAIRS if pairs is None else pairs
    out = []
    for rd in P.plan_rounds(shapes, batch_size, 1):
        members = [i for i, s in enumerate(shapes) if s == rd['shape']]
        src_hw = (max(pairs[i][0][0] for i in members), max(pairs[i][0][1] for i in members))
        out.append((rd['shape'][:2], len(rd['shape']) > 2, src_hw, rd['batches'][0]))
    return out


def definition_want(model, items, wins, device, batch_size, shrink_k1=False, pairs=None):
    """The definition, per batch of the loop: the numpy-cropped and -shrunk arrays (zeros in the empty slots) -> lama_mask_compose_fwd -> the
    generator call of the step (its dense tail) -> ``paste_back_ref``, pasted by slicing.  k = 1: S = C / 255 and the gather at scale 1 returns
    the sample, which is the crop step's result."""
    lib = model.generator._exec.lib
    want = [None] * len(items)
    for (Hp, Wp), _, _, batch in batches_of(wins, batch_size, shrink_k1=shrink_k1, pairs=pairs):
        f_img = torch.zeros(batch_size, 3, Hp, Wp, dtype=torch.float32)
        f_msk = torch.zeros(batch_size, 1, Hp, Wp, dtype=torch.float32)
        u8 = [P.load_item_u8(*items[i]) for i in batch]
        for j, i in enumerate(batch):
            y0, x0, ch, cw, k, dh, dw = wins[i][:7]
            S, mu = shrink_ref(u8[j][0][y0:y0 + ch, x0:x0 + cw], u8[j][1][y0:y0 + ch, x0:x0 + cw], k)
            ys, xs = CU._symmetric(Hp, dh), CU._symmetric(Wp, dw)
            f_img[j] = torch.from_numpy(np.ascontiguousarray(np.transpose(S[ys][:, xs], (2, 0, 1))))
            f_msk[j, 0] = torch.from_numpy((mu[ys][:, xs] > 0).astype(F32))
        f_img, f_msk = f_img.to(device), f_msk.to(device)
        with torch.no_grad():
            pred = model._generate_u8((batch_size, 4, Hp, Wp), torch.device(device), False,
                                      lambda masked: lib.mask_compose(L.view(f_img), L.view(f_msk), L.view(masked), batch_size, _stream(device)))
            pred = pred.cpu().numpy()
        for j, i in enumerate(batch):
            want[i] = paste_ref(u8[j][0], u8[j][1], wins[i][:4], wins[i][4], pred[j], True)
    return want


run_step = CU.run_step


def check_step(model, items, wins, device, mode, want, batch_size, encode_png=False, encode_jpeg=False, jpeg_quality=95, jpeg_subsampling='420',
               pairs=None):
    """HostFedStep(crop=True, crop_shrink=True) in ``mode`` per batch of the loop (the k = 1 window through the shrink step as well; the batches
    of one bucket through ONE step object, as the loop runs them): source-slot results equal to ``want``, zeros around each image and in the empty
    slots; ``encode_png``: the streams decode to the same pixels; ``encode_jpeg``: the scans are tests/jpeg_ref.py's scans of ``want``, byte for
    byte.  ``pairs``: the table the items were written from (the default: PAIRS)."""
    from PIL import Image
    from tests import jpeg_ref
    pairs = PAIRS if pairs is None else pairs
    u8 = [P.load_item_u8(*it) for it in items]
    got = [None] * len(items)
    enc = dict(encode_jpeg=True, jpeg_quality=jpeg_quality, jpeg_subsampling=jpeg_subsampling) if encode_jpeg else {}
    hs = bucket = None
    for (Hp, Wp), _, src_hw, batch in batches_of(wins, batch_size, shrink_k1=True, pairs=pairs):
        if bucket != (Hp, Wp, src_hw):
            hs = P.HostFedStep(model, batch_size, Hp, Wp, device, drain=True, mode=mode, crop=True, crop_shrink=True, src_hw=src_hw,
                               encode_png=encode_png, **enc)
            bucket = (Hp, Wp, src_hw)
        assert hs.mode == mode and hs.crop and hs.crop_shrink and hs.out_hw == src_hw and tuple(hs.u8[0].shape) == (batch_size, *src_hw, 3)
        run_step(hs, [(u8[i][0], u8[i][1], wins[i][:5]) for i in batch])
        assert np.array_equal(hs.crop_sizes(0)[:len(batch)], [pairs[i][0] for i in batch]) and not hs.crop_sizes(0)[len(batch):].any()
        if encode_png:
            for j, i in enumerate(batch):
                got[i] = np.array(Image.open(io.BytesIO(P.png_from_zlib(*pairs[i][0], 3, bytes(hs.result_png(0, j))))))
            assert all(len(hs.result_png(0, j)) == 0 for j in range(len(batch), batch_size)) and CU.result_raises(hs)
            continue
        if encode_jpeg:
            for j, i in enumerate(batch):
                got[i] = bytes(hs.result_jpeg(0, j))
            assert all(len(hs.result_jpeg(0, j)) == 0 for j in range(len(batch), batch_size)) and CU.result_raises(hs)
            continue
        res = hs.result(0).copy()
        for j, i in enumerate(batch):
            h, w = pairs[i][0]
            got[i] = res[j, :h, :w]
            assert not res[j, h:].any() and not res[j, :, w:].any()
        assert not res[len(batch):].any()
    if encode_jpeg:                                           # byte for byte the restatement's scan of the definition
        ss = jpeg_ref.J444 if str(jpeg_subsampling) == '444' else jpeg_ref.J420
        for i, (g, w) in enumerate(zip(got, want)):
            assert w.shape == pairs[i][0] + (3,)
            assert g == jpeg_ref.scan_ref(w, *pairs[i][0], jpeg_quality, ss), (mode, i, 'jpeg', len(g))
        return got
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape == pairs[i][0] + (3,)
        assert np.array_equal(g, w), (mode, i, encode_png, np.argwhere(g != w)[:4].tolist())
        mask = u8[i][1]
        assert np.array_equal(g[mask == 0], u8[i][0][mask == 0]) and (g[mask != 0] != u8[i][0][mask != 0]).any()
    return got


check_written_pngs = CU.check_written_pngs
