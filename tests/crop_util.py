"""Shared by tests/test_crop_emu.py, tests/test_crop_gpu.py and tests/test_crop_gloo.py: the numpy restatement of lama_crop_compose_u8_fwd /
lama_crop_paste_u8_fwd (csrc/elementwise.hip) and the checks the suites run -- through the host SIMT emulator and on the GPU, through the same
C ABI.

``crop_to_mask`` has no counterpart in the reference (a crop sees less context than the whole image).  Its definition is THE EXISTING U8 STEP RUN
ON THE CROPPED ARRAYS, PASTED BY SLICING, so every kernel result is held to two oracles, fp32 outputs bit for bit and u8 outputs byte for byte:
``crop_compose_ref`` / ``crop_paste_ref`` below, and the existing entries lama_mask_compose_u8_fwd / lama_blend_quantize_u8_fwd called on
host-cropped slots (``entry_want``), pasted with numpy slicing.  There is no tolerance anywhere in this file."""
import ctypes as C
import functools
import io
import os

import numpy as np
import torch

from lama_amd import _lib as L
from lama_amd import predict as P

F32 = np.float32
CANARY = 0xA5
CANARY_F32 = np.frombuffer(bytes([CANARY] * 4), F32)[0]      # the fp32 outputs are filled with the same byte
GUARD = 64                  # bytes in front of and behind every u8 buffer (keeps the buffer 4-byte aligned)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _symmetric(n_out: int, n: int) -> np.ndarray:
    """np.pad(mode='symmetric') as an index map for any amount of padding: the mirror is periodic with period 2 n."""
    i = np.arange(n_out)
    t = i % (2 * n)
    return np.where(i < n, i, np.where(t < n, t, 2 * n - 1 - t))


def fma32(a, b, c) -> np.ndarray:
    """fmaf(a, b, c) on float32 arrays: ONE rounding.  The product of two float32 is exact in float64; the float64 sum is rounded to odd (from
    its TwoSum residual), which makes the final rounding to float32 the rounding of the exact value (53 >= 2 * 24 + 2 bits)."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid='ignore', over='ignore'):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(inexact, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def _quantize(r: np.ndarray) -> np.ndarray:
    """clip(r * 255, 0, 255) truncated, a NaN -> 0 (fmaxf returns its other operand), as lama_blend_quantize_u8_fwd does it."""
    with np.errstate(invalid='ignore', over='ignore'):
        t = r * F32(255)
        return np.fmin(np.fmax(t, F32(0)), F32(255)).astype(np.uint8)


def _mask_f32(m_u8: np.ndarray, binarize: bool) -> np.ndarray:
    return (m_u8 > 0).astype(F32) if binarize else m_u8.astype(F32) / F32(255)


def crop_compose_ref(image_u8: np.ndarray, mask_u8: np.ndarray, rect, Hp: int, Wp: int, binarize: bool) -> np.ndarray:
    """image [h,w,3] u8, mask [h,w] u8, rect (y0, x0, ch, cw) -> the generator's input [4,Hp,Wp] float32 of the window: / 255, symmetric padding
    at the bottom / right, cat(C * (1 - m), m)."""
    y0, x0, ch, cw = rect
    ys, xs = y0 + _symmetric(Hp, ch), x0 + _symmetric(Wp, cw)
    c = image_u8[ys][:, xs].astype(F32) / F32(255)
    m = _mask_f32(mask_u8[ys][:, xs], binarize)
    out = np.concatenate([np.transpose(c * (F32(1) - m)[:, :, None], (2, 0, 1)), m[None]], 0)
    assert out.dtype == F32 and out.shape == (4, Hp, Wp)
    return out


def crop_paste_ref(image_u8: np.ndarray, mask_u8: np.ndarray, rect, pred_f32: np.ndarray, binarize: bool) -> np.ndarray:
    """image [h,w,3] u8, mask [h,w] u8, pred [3, >= ch, >= cw] float32 -> [h,w,3] u8: the source, with clip((m * pred + (1 - m) * C / 255) * 255,
    0, 255) truncated inside the window (one fused multiply-add, as ew_blend in csrc/elementwise.hip).  pred is not read where the mask byte is 0:
    it counts as 0 there, and the blend then gives the source byte back."""
    y0, x0, ch, cw = rect
    c, mu = image_u8[y0:y0 + ch, x0:x0 + cw], mask_u8[y0:y0 + ch, x0:x0 + cw]
    pr = np.where((mu != 0)[:, :, None], np.transpose(pred_f32[:, :ch, :cw], (1, 2, 0)), F32(0)).astype(F32)
    m = _mask_f32(mu, binarize)[:, :, None]
    r = fma32(m, pr, (F32(1) - m) * (c.astype(F32) / F32(255)))
    out = image_u8.copy()
    out[y0:y0 + ch, x0:x0 + cw] = _quantize(r)
    return out


# ---- kernel cases ---------------------------------------------------------------------------------------------------------------------------
# name: (Hs, Ws, Hp, Wp, [(h, w, (y0, x0, ch, cw)) or None per image])
CASES = {
    'interior-9x7': (9, 7, 8, 8, [(9, 7, (2, 1, 5, 4))]),
    'periodic-padding-9x7': (9, 7, 16, 12, [(9, 7, (2, 1, 5, 4))]),                      # more than 2 ch rows / 2 cw columns of padding
    'edges-top-bottom-left-right': (12, 16, 8, 8, [(12, 16, (0, 4, 5, 8)), (12, 16, (7, 4, 5, 8)), (12, 16, (3, 0, 6, 5)), (12, 16, (3, 11, 6, 5))]),
    'whole-image-13x11-padded': (13, 11, 16, 16, [(13, 11, (0, 0, 13, 11))]),
    'x0-mod-4-dword-slots': (8, 16, 8, 8, [(8, 16, (1, x0, 6, 8)) for x0 in (0, 1, 2, 3)] + [(8, 16, (1, 8, 6, 8))]),
    'x0-mod-4-ws-7': (8, 7, 8, 8, [(8, 7, (1, x0, 6, 4)) for x0 in (0, 1, 2, 3)]),
    'cw-not-a-multiple-of-4': (8, 16, 8, 8, [(8, 16, (0, 4, 7, 6)), (8, 16, (1, 8, 7, 3))]),
    'unpadded-view-7x6': (8, 16, 7, 6, [(8, 16, (0, 4, 7, 6))]),                         # Wp % 4 != 0: scalar stores
    'batch-of-three-one-empty': (12, 16, 8, 8, [(12, 16, (2, 4, 8, 8)), None, (10, 13, (1, 3, 7, 5))]),
    'two-workgroups-64x64': (64, 64, 48, 40, [(64, 64, (8, 12, 40, 36)), (61, 63, (13, 0, 48, 40))]),
    # (beyond the issue's table) more than one workgroup PER IMAGE in both kernels, and the row-wise form of the paste (192 items a row or more)
    'chunks-66x68': (66, 68, 72, 64, [(66, 68, (1, 3, 65, 64))]),
    'rows-6x772': (6, 772, 8, 8, [(6, 772, (0, 700, 6, 8)), (5, 770, (1, 3, 4, 7))]),
    'rows-bytes-6x771': (6, 771, 8, 8, [(6, 771, (0, 761, 6, 8))]),
}
LAYOUTS = ('plain', 'view', 'stride')


def _image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _mask(h, w, seed):
    # about 40 % hole, with the values 1 and 128 beside 255 so that mask > 0 and mask / 255 differ
    return np.random.RandomState(seed + 1000).choice(np.array([0, 1, 128, 255], np.uint8), size=(h, w), p=[0.6, 0.1, 0.1, 0.2])


def _pred(Hp, Wp, seed):
    """[3, Hp, Wp] in [-0.1, 1.1]: the clip is hit at both ends."""
    return (np.random.RandomState(seed + 2000).rand(3, Hp, Wp) * 1.2 - 0.1).astype(F32)


@functools.lru_cache(maxsize=None)
def case_data(name: str):
    """(image slots [B,Hs,Ws,3], mask slots [B,Hs,Ws], sizes [B,2], rects [B,4], pred [B,3,Hp,Wp]).  The slots outside an image hold 77 in image
    AND mask (a kernel that used them would paste there); pred is NaN wherever it must not be read -- outside the window's ch x cw corner and
    where the mask byte is 0: one read of it there turns a source byte into 0."""
    Hs, Ws, Hp, Wp, images = CASES[name]
    B = len(images)
    img, msk = np.full((B, Hs, Ws, 3), 77, np.uint8), np.full((B, Hs, Ws), 77, np.uint8)
    ssz, rects = np.zeros((B, 2), np.int32), np.zeros((B, 4), np.int32)
    pred = np.full((B, 3, Hp, Wp), np.nan, F32)
    for j, it in enumerate(images):
        if it is None:
            continue
        h, w, (y0, x0, ch, cw) = it
        img[j, :h, :w], msk[j, :h, :w] = _image(h, w, 10 * j + h), _mask(h, w, 10 * j + w)
        img[j, 0, 0] = 0                                  # (a byte that a stray NaN could not change, beside 255 bytes that it could)
        ssz[j], rects[j] = (h, w), (y0, x0, ch, cw)
        hole = msk[j, y0:y0 + ch, x0:x0 + cw] != 0
        pred[j, :, :ch, :cw] = np.where(hole[None], _pred(ch, cw, 10 * j + ch), np.nan)
    for a in (img, msk, ssz, rects, pred):
        a.setflags(write=False)
    return img, msk, ssz, rects, pred


def ref_want(img, msk, ssz, rects, pred, Hp, Wp, binarize):
    """The restatement over a slot batch -> (compose [B,4,Hp,Wp] float32, paste [B,Hs,Ws,3] u8): zeros for an empty slot, zeros outside h x w."""
    B = len(ssz)
    comp, paste = np.zeros((B, 4, Hp, Wp), F32), np.zeros_like(img)
    for j in range(B):
        h, w = ssz[j]
        if h > 0:
            comp[j] = crop_compose_ref(img[j, :h, :w], msk[j, :h, :w], rects[j], Hp, Wp, binarize)
            paste[j, :h, :w] = crop_paste_ref(img[j, :h, :w], msk[j, :h, :w], rects[j], pred[j], binarize)
    return comp, paste


def entry_want(lib, dev, img, msk, ssz, rects, pred, Hp, Wp, binarize):
    """The second oracle: lama_mask_compose_u8_fwd / lama_blend_quantize_u8_fwd on HOST-CROPPED slots [B,Hp,Wp] with sizes (ch, cw), the blend's
    bytes pasted into the source with numpy slicing."""
    B = len(ssz)
    c_img, c_msk, c_sz = np.full((B, Hp, Wp, 3), 77, np.uint8), np.full((B, Hp, Wp), 77, np.uint8), np.zeros((B, 2), np.int32)
    for j in range(B):
        if ssz[j, 0] > 0:
            y0, x0, ch, cw = rects[j]
            c_img[j, :ch, :cw], c_msk[j, :ch, :cw], c_sz[j] = img[j, y0:y0 + ch, x0:x0 + cw], msk[j, y0:y0 + ch, x0:x0 + cw], (ch, cw)
    t_img, t_msk, t_sz = (torch.from_numpy(a).to(dev) for a in (c_img, c_msk, c_sz))
    comp = torch.zeros(B, 4, Hp, Wp, dtype=torch.float32, device=dev)
    t_pred = torch.from_numpy(np.array(pred)).to(dev)
    blend = torch.zeros(B, Hp, Wp, 3, dtype=torch.uint8, device=dev)
    lib.mask_compose_u8(t_img, t_msk, t_sz, L.view(comp), B, binarize, _stream(dev))
    lib.blend_quantize_u8(t_img, t_msk, t_sz, L.view(t_pred), blend, B, binarize, _stream(dev))
    _sync(dev)
    blend = blend.cpu().numpy()
    paste = np.zeros_like(img)
    for j in range(B):
        h, w = ssz[j]
        if h > 0:
            y0, x0, ch, cw = rects[j]
            paste[j, :h, :w] = img[j, :h, :w]
            paste[j, y0:y0 + ch, x0:x0 + cw] = blend[j, :ch, :cw]
    return comp.cpu().numpy(), paste


@functools.lru_cache(maxsize=None)
def case_want(name: str, binarize: bool):
    """The restatement's outputs for a case, computed once; every layout and both suites share them."""
    Hs, Ws, Hp, Wp, _ = CASES[name]
    comp, paste = ref_want(*case_data(name), Hp, Wp, binarize)
    comp.setflags(write=False)
    paste.setflags(write=False)
    return comp, paste


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream if torch.device(dev).type == 'cuda' else 0


def _sync(dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize(dev)


class F32View:
    """A [B,C,Hp,Wp] float32 operand inside a canary-filled buffer.  'plain': contiguous, 16-byte aligned (the float4 stores of the compose);
    'view': channels 1 .. C of a [B,C+2,Hp,Wp] tensor (a channel slice: batch_stride = (C + 2) Hp Wp); 'stride': a padded batch stride of
    C Hp Wp + 7 behind a 4-byte aligned, not 16-byte aligned pointer (scalar stores)."""

    def __init__(self, B, Cn, Hp, Wp, layout, dev, data=None):
        hw = Hp * Wp
        self.lead, self.bs = {'plain': (16, Cn * hw), 'view': (16 + hw, (Cn + 2) * hw), 'stride': (17, Cn * hw + 7)}[layout]
        self.B, self.C, self.Hp, self.Wp = B, Cn, Hp, Wp
        flat = np.full(self.lead + B * self.bs + 16, CANARY_F32, F32)
        self.inside = np.zeros(flat.shape, bool)
        for b in range(B):
            o = self.lead + b * self.bs
            self.inside[o:o + Cn * hw] = True
            if data is not None:
                flat[o:o + Cn * hw] = data[b].reshape(-1)
        self.before = flat.copy()
        self.t = torch.empty(flat.size, dtype=torch.float32, device=dev)
        self.t.copy_(torch.from_numpy(flat))
        assert self.t.data_ptr() % 16 == 0
        self.view = L.Tensor4(self.t.data_ptr() + 4 * self.lead, self.bs, Cn, Hp, Wp, L.DT_F32)

    def read(self):
        """(the operand [B,C,Hp,Wp], True if every float around it still holds the canary)."""
        flat = self.t.cpu().numpy()
        got = np.stack([flat[self.lead + b * self.bs:self.lead + b * self.bs + self.C * self.Hp * self.Wp].reshape(self.C, self.Hp, self.Wp)
                        for b in range(self.B)])
        return got, np.array_equal(flat.view(np.uint32)[~self.inside], self.before.view(np.uint32)[~self.inside])

    def unchanged(self) -> bool:
        return np.array_equal(self.t.cpu().numpy().view(np.uint32), self.before.view(np.uint32))


def u8_at(arr: np.ndarray, dev, shift=0, fill=None):
    """``arr`` (or, with ``fill``, that byte) in a canary-filled u8 buffer, ``shift`` bytes behind its 4-byte aligned middle: (flat, view)."""
    n = arr.size
    flat = torch.full((GUARD + shift + n + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    assert (flat.data_ptr() + GUARD) % 4 == 0
    view = flat[GUARD + shift:GUARD + shift + n].view(*arr.shape)
    if fill is None:
        view.copy_(torch.from_numpy(np.array(arr)))
    else:
        view.fill_(fill)
    return flat, view


def guards_intact(flat, view) -> bool:
    n, off = view.numel(), view.storage_offset()
    return bool((flat[:off] == CANARY).all()) and bool((flat[off + n:] == CANARY).all())


def run_kernels(lib, dev, img, msk, ssz, rects, pred, Hp, Wp, layout, binarize, shift=0):
    """One launch of each entry on copies of the operands -> (compose [B,4,Hp,Wp], paste [B,Hs,Ws,3]); asserts the canaries around both outputs
    and that no operand changed."""
    B, Hs, Ws = msk.shape
    f_img, t_img = u8_at(img, dev, shift)
    f_msk, t_msk = u8_at(msk, dev, shift)
    t_ssz, t_rc = torch.from_numpy(ssz.copy()).to(dev), torch.from_numpy(rects.copy()).to(dev)
    out = F32View(B, 4, Hp, Wp, layout, dev)
    prd = F32View(B, 3, Hp, Wp, layout, dev, data=pred)
    f_out, t_out = u8_at(img, dev, shift, fill=CANARY)
    lib.crop_compose_u8(t_img, t_msk, t_ssz, t_rc, out.view, B, binarize=binarize, stream=_stream(dev))
    lib.crop_paste_u8(t_img, t_msk, t_ssz, t_rc, prd.view, t_out, B, binarize=binarize, stream=_stream(dev))
    _sync(dev)
    comp, comp_guards = out.read()
    assert comp_guards, 'the compose wrote outside its view'
    assert guards_intact(f_out, t_out), 'the paste wrote outside its slots'
    assert prd.unchanged() and guards_intact(f_img, t_img) and guards_intact(f_msk, t_msk)
    assert np.array_equal(t_img.cpu().numpy(), img) and np.array_equal(t_msk.cpu().numpy(), msk)
    assert np.array_equal(t_ssz.cpu().numpy(), ssz) and np.array_equal(t_rc.cpu().numpy(), rects)
    return comp, t_out.cpu().numpy()


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype == F32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_outputs(got, want, what):
    comp, paste = got
    wcomp, wpaste = want
    assert _same_bits(comp, wcomp), (what, 'compose', np.argwhere(comp.view(np.uint32) != wcomp.view(np.uint32))[:4].tolist())
    bad = np.argwhere(paste != wpaste)
    assert bad.size == 0, (what, 'paste', len(bad), bad[:4].tolist())


def check_case(lib, dev, name, binarize, layout):
    """Both kernels against the restatement AND against the existing entries on host-cropped slots, bit for bit / byte for byte."""
    Hs, Ws, Hp, Wp, _ = CASES[name]
    data = case_data(name)
    got = run_kernels(lib, dev, *data, Hp, Wp, layout, binarize)
    check_outputs(got, case_want(name, binarize), (name, binarize, layout, 'restatement'))
    check_outputs(got, entry_want(lib, dev, *data, Hp, Wp, binarize), (name, binarize, layout, 'entries'))
    img, msk, ssz, rects, _ = data
    for j in range(len(ssz)):                                 # source pixels come back byte for byte wherever the mask byte is 0 ...
        h, w = ssz[j]
        keep = msk[j, :h, :w] == 0
        assert np.array_equal(got[1][j, :h, :w][keep], img[j, :h, :w][keep])
        if h > 0:                                             # ... and outside the window whatever the mask says
            y0, x0, ch, cw = rects[j]
            outside = np.ones((h, w), bool)
            outside[y0:y0 + ch, x0:x0 + cw] = False
            assert np.array_equal(got[1][j, :h, :w][outside], img[j, :h, :w][outside])
            assert (got[1][j, :h, :w] != img[j, :h, :w]).any()


def check_misaligned_slots(lib, dev):
    """Slot pointers that are not 4-byte aligned take the byte path although Ws % 4 == 0: the same bits."""
    name = 'x0-mod-4-dword-slots'
    Hs, Ws, Hp, Wp, _ = CASES[name]
    for shift in (1, 2, 3):
        for binarize in (True, False):
            got = run_kernels(lib, dev, *case_data(name), Hp, Wp, 'plain', binarize, shift=shift)
            check_outputs(got, case_want(name, binarize), (name, binarize, shift))


# every way of not fitting for a 10 x 12 image in a 12 x 16 slot with an 8 x 8 view: (h, w, (y0, x0, ch, cw))
DOES_NOT_FIT = {
    'ch < 1': (10, 12, (2, 2, 0, 4)), 'cw < 1': (10, 12, (2, 2, 4, 0)), 'ch negative': (10, 12, (2, 2, -4, 4)),
    'y0 < 0': (10, 12, (-1, 2, 4, 4)), 'x0 < 0': (10, 12, (2, -1, 4, 4)),
    'y0 + ch > h': (10, 12, (7, 2, 4, 4)), 'x0 + cw > w': (10, 12, (2, 9, 4, 4)),
    'ch > Hp': (10, 12, (0, 2, 9, 4)), 'cw > Wp': (10, 12, (2, 0, 4, 9)),
    'h > Hs': (13, 12, (2, 2, 4, 4)), 'w > Ws': (10, 17, (2, 2, 4, 4)),
    'y0 + ch overflows': (10, 12, (2 ** 31 - 2, 2, 4, 4)), 'x0 + cw overflows': (10, 12, (2, 2 ** 31 - 2, 4, 4)),
}


def check_rects_that_do_not_fit(lib, dev, layout='plain'):
    """A batch of three -- a served image, an empty slot, a rect that does not fit -- for each way of not fitting: the compose writes zeros for
    that image and the paste its whole slot as 0, nothing out of bounds, the image beside them is served."""
    Hs, Ws, Hp, Wp = 12, 16, 8, 8
    good = (10, 12, (1, 3, 7, 5))
    for why, bad in DOES_NOT_FIT.items():
        img, msk = np.full((3, Hs, Ws, 3), 200, np.uint8), np.full((3, Hs, Ws), 255, np.uint8)
        img[0, :10, :12], msk[0, :10, :12] = _image(10, 12, 4), _mask(10, 12, 4)
        ssz = np.array([good[:2], (0, 0), bad[:2]], np.int32)
        rects = np.array([good[2], (0, 0, 0, 0), bad[2]], np.int32)
        pred = _pred(Hp, Wp, 7)[None].repeat(3, 0)
        for binarize in (True, False):
            comp, paste = run_kernels(lib, dev, img, msk, ssz, rects, pred, Hp, Wp, layout, binarize)
            assert not comp[1:].view(np.uint32).any() and not paste[1:].any(), (why, binarize)
            assert _same_bits(comp[0], crop_compose_ref(img[0, :10, :12], msk[0, :10, :12], good[2], Hp, Wp, binarize)), why
            want = np.zeros((Hs, Ws, 3), np.uint8)
            want[:10, :12] = crop_paste_ref(img[0, :10, :12], msk[0, :10, :12], good[2], pred[0], binarize)
            assert np.array_equal(paste[0], want), why


def check_non_finite(lib, dev):
    """A NaN sample quantises to 0 under the mask; +-inf and +-1e38 saturate to 255 / 0 with mask > 0 -- and a fractional mask whose other term is
    finite does the same; no sample is read (so none is seen) where the mask byte is 0 or outside the window."""
    img, msk = np.full((1, 8, 8, 3), 9, np.uint8), np.zeros((1, 8, 8), np.uint8)
    msk[0, :, 1:] = 255
    msk[0, 3, 3] = 128
    ssz, rects = np.array([[8, 8]], np.int32), np.array([[2, 0, 4, 8]], np.int32)
    for val, want in ((np.nan, 0), (np.inf, 255), (-np.inf, 0), (1e38, 255), (-1e38, 0)):
        pred = np.full((1, 3, 8, 8), val, F32)
        for binarize in (True, False):
            comp, paste = run_kernels(lib, dev, img, msk, ssz, rects, pred, 8, 8, 'plain', binarize)
            assert (paste[0, 2:6, 1:] == want).all(), (val, binarize)
            assert (paste[0, :, 0] == 9).all() and (paste[0, :2] == 9).all() and (paste[0, 6:] == 9).all(), (val, binarize)
            assert np.array_equal(paste[0], crop_paste_ref(img[0], msk[0], rects[0], pred[0], binarize))
            assert np.array_equal(paste, entry_want(lib, dev, img, msk, ssz, rects, pred, 8, 8, binarize)[1])


def check_refusals(lib, dev):
    """Every LAMA_ERR_* case of both entries returns its code and launches nothing: the canary-filled outputs stay as they are."""
    name = 'x0-mod-4-dword-slots'
    Hs, Ws, Hp, Wp, _ = CASES[name]
    img, msk, ssz, rects, pred = case_data(name)
    B = len(ssz)
    t = [torch.from_numpy(a.copy()).to(dev) for a in (img, msk, ssz, rects)]
    out = F32View(B, 4, Hp, Wp, 'plain', dev)
    prd = F32View(B, 3, Hp, Wp, 'plain', dev, data=pred)
    f_out, t_out = u8_at(img, dev, fill=CANARY)
    stream = _stream(dev)
    good = [x.data_ptr() for x in t]
    bad, uns = L.ERR_BAD_ARG, L.ERR_UNSUPPORTED

    def mod(view, **kw):
        w = L.Tensor4(view.ptr, view.batch_stride, view.C, view.H, view.W, view.dtype)
        for k, val in kw.items():
            setattr(w, k, val)
        return w

    def compose(ptrs=good, Hs=Hs, Ws=Ws, v=out.view, batch=B):
        rc = lib._l.lama_crop_compose_u8_fwd(stream, *ptrs, Hs, Ws, None if v is None else C.byref(v), batch, 1)
        _sync(dev)
        assert out.unchanged(), 'a refused compose wrote'
        return rc

    def paste(ptrs=good, Hs=Hs, Ws=Ws, v=prd.view, o=t_out.data_ptr(), batch=B):
        rc = lib._l.lama_crop_paste_u8_fwd(stream, *ptrs, Hs, Ws, None if v is None else C.byref(v), o, batch, 1)
        _sync(dev)
        assert bool((f_out == CANARY).all()), 'a refused paste wrote'
        return rc

    for call, view, ch in ((compose, out.view, 4), (paste, prd.view, 3)):
        for k in range(4):                                    # each null operand pointer
            a = list(good)
            a[k] = None
            assert call(ptrs=a) == bad, (call.__name__, k)
        assert call(v=None) == bad and call(v=mod(view, ptr=None)) == bad
        assert call(batch=0) == bad and call(batch=-1) == bad
        assert call(Hs=0) == bad and call(Ws=0) == bad and call(Hs=-8) == bad and call(Ws=-8) == bad
        assert call(v=mod(view, C=ch + 1)) == bad and call(v=mod(view, C=1)) == bad            # not [., C, H, W]
        assert call(v=mod(view, H=0)) == bad and call(v=mod(view, W=0)) == bad and call(v=mod(view, H=-8)) == bad
        assert call(v=mod(view, batch_stride=ch * Hp * Wp - 1)) == bad
        assert call(v=mod(view, ptr=view.ptr + 2)) == bad                                      # a view pointer that is not 4-byte aligned
        assert call(v=mod(view, dtype=L.DT_F16)) == uns and call(v=mod(view, dtype=L.DT_SPLIT16)) == uns
        # index ranges of 2^30 and beyond (the geometry alone decides: nothing is launched, nothing is touched)
        assert call(v=mod(view, H=2 ** 16, W=2 ** 16, batch_stride=2 ** 40)) == uns
    assert paste(o=None) == bad
    assert paste(o=good[0]) == bad                                                             # in place
    assert paste(Hs=2 ** 30, Ws=8) == uns                                                      # 2^31 work items per slot (the item-wise form)
    assert paste(Hs=2 ** 31 - 1, Ws=4096) == uns                                               # 5 * 2^31 workgroups (the row-wise form)
    # ... and the binding reports them as LamaError with the code
    for fn, args in ((lib.crop_compose_u8, (mod(out.view, dtype=L.DT_F16),)), (lib.crop_paste_u8, (mod(prd.view, dtype=L.DT_F16), t_out))):
        try:
            fn(*t, *args, B, stream=stream)
        except L.LamaError as e:
            assert e.code == uns
        else:
            raise AssertionError('not refused')
    # the same calls, unmodified, are served
    assert lib._l.lama_crop_compose_u8_fwd(stream, *good, Hs, Ws, C.byref(out.view), B, 1) == 0
    assert lib._l.lama_crop_paste_u8_fwd(stream, *good, Hs, Ws, C.byref(prd.view), t_out.data_ptr(), B, 1) == 0
    _sync(dev)
    check_outputs((out.read()[0], t_out.cpu().numpy()), case_want(name, True), 'after the refusals')
    assert out.read()[1] and guards_intact(f_out, t_out)


# ---- crop_rect -------------------------------------------------------------------------------------------------------------------------------
def check_rect_properties(mask: np.ndarray, margin: int, step: int, pad_mod: int):
    h, w = mask.shape
    y0, x0, ch, cw, Hp, Wp = P.crop_rect(mask, margin, step, pad_mod)
    ys, xs = np.flatnonzero((mask > 0).any(1)), np.flatnonzero((mask > 0).any(0))
    if ys.size:                                               # the window encloses the box ...
        assert y0 <= ys[0] and ys[-1] < y0 + ch and x0 <= xs[0] and xs[-1] < x0 + cw
    assert 0 <= y0 and y0 + ch <= h and 0 <= x0 and x0 + cw <= w and ch >= 1 and cw >= 1        # ... and lies inside the image
    assert ch % step == 0 or ch == h
    assert cw % step == 0 or cw == w
    assert Hp % pad_mod == 0 and Wp % pad_mod == 0 and ch <= Hp < ch + pad_mod and cw <= Wp < cw + pad_mod
    assert all(isinstance(v, int) for v in (y0, x0, ch, cw, Hp, Wp))
    return y0, x0, ch, cw, Hp, Wp


# ---- HostFedStep, the loop and the CLI --------------------------------------------------------------------------------------------------------
MARGIN, STEP, PAD_MOD = 4, 16, 8
# (h, w), the mask's box (y, x, height, width) -> the window crop_rect gives it with the options above
PAIRS = [((40, 56), (10, 20, 8, 12)),     # window (6, 10, 16, 32): the 16 x 32 bucket
         ((48, 48), (30, 5, 8, 8)),       # window (26, 1, 16, 16): the 16 x 16 bucket
         ((33, 61), (28, 50, 5, 8))]      # window (17, 45, 16, 16), clamped to the bottom and right edges: the 16 x 16 bucket
WINDOWS = [(6, 10, 16, 32, 16, 32), (26, 1, 16, 16, 16, 16), (17, 45, 16, 16, 16, 16)]


def write_pairs(root, seed=3, pairs=None):
    """The three PNG pairs (or those of ``pairs``); each mask is a box of 255 with one pixel of 1 in its corner (any non-zero pixel is hole) and
    zeros."""
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    for i, ((h, w), (by, bx, bh, bw)) in enumerate(PAIRS if pairs is None else pairs):
        mask = np.zeros((h, w), np.uint8)
        mask[by:by + bh, bx:bx + bw] = 255
        mask[by, bx] = 1
        Image.fromarray(_image(h, w, seed + i)).save(os.path.join(root, f'im{i}.png'))
        Image.fromarray(mask).save(os.path.join(root, f'im{i}_mask.png'))
    return P.list_dataset(root if root.endswith(os.sep) else root + os.sep, '.png')


def item_rects(items, windows=None):
    rects = [P.crop_rect(P.load_item_u8(*it)[1], MARGIN, STEP, PAD_MOD) for it in items]
    assert rects == (WINDOWS if windows is None else windows), rects
    return rects


def batches_of(rects, batch_size, pairs=None):
    """[(bucket (Hp, Wp), source slot (Hs, Ws), [item index lists])] in the order of the loop (plan_rounds: the largest bucket first)."""
    rounds = P.plan_rounds([r[4:] for r in rects], batch_size, 1)
    out = []
    for rd in rounds:
        if not out or out[-1][0] != rd['shape']:
            out.append((rd['shape'], None, []))
        out[-1][2].append(rd['batches'][0])
    sizes = [hw for hw, _ in (PAIRS if pairs is None else pairs)]
    return [(shape, (max(sizes[i][0] for b in bs for i in b), max(sizes[i][1] for b in bs for i in b)), bs) for shape, _, bs in out]


def run_step(hs, rows):
    """Feed host set 0 (``rows`` = one ``put`` argument tuple per slot; the rest of the batch: empty slots), run one step."""
    for j in range(hs.n):
        hs.put(0, j, *(rows[j] if j < len(rows) else (None, None)))
    hs.prime(0)
    hs.launch(0)
    hs.wait(0)
    hs.flush(0)


def cropped_want(model, items, rects, batch_size, device, mode, pairs=None):
    """The definition: per bucket and batch the EXISTING u8 HostFedStep, fed the host-cropped pairs in the same slots of the same batch size,
    its [:ch, :cw] results pasted into the decoded sources by numpy slicing -> one source-size u8 image per item."""
    u8 = [P.load_item_u8(*it) for it in items]
    want = [None] * len(items)
    for (Hp, Wp), _, batches in batches_of(rects, batch_size, pairs):
        hs = P.HostFedStep(model, batch_size, Hp, Wp, device, drain=True, mode=mode)
        assert hs.u8_input
        for batch in batches:
            run_step(hs, [(u8[i][0][rects[i][0]:rects[i][0] + rects[i][2], rects[i][1]:rects[i][1] + rects[i][3]],
                           u8[i][1][rects[i][0]:rects[i][0] + rects[i][2], rects[i][1]:rects[i][1] + rects[i][3]]) for i in batch])
            res = hs.result(0).copy()
            for j, i in enumerate(batch):
                y0, x0, ch, cw = rects[i][:4]
                want[i] = u8[i][0].copy()
                want[i][y0:y0 + ch, x0:x0 + cw] = res[j, :ch, :cw]
    return want


def result_raises(hs) -> bool:
    """``result()`` of a step that ends with an encoder: the u8 images are not downloaded."""
    try:
        hs.result(0)
    except L.LamaError:
        return True
    return False


def check_step(model, items, rects, device, mode, want, batch_size, encode_png=False, encode_jpeg=False, jpeg_quality=95, jpeg_subsampling='420',
               pairs=None):
    """HostFedStep(crop=True) in ``mode`` per bucket: source-slot results equal to ``want``, zeros around each image and in the empty slots;
    ``encode_png``: the streams decode to the same pixels; ``encode_jpeg``: the scans are tests/jpeg_ref.py's scans of ``want``, byte for byte.
    ``pairs``: the table the items were written from (the default: PAIRS)."""
    from PIL import Image
    from tests import jpeg_ref
    pairs = PAIRS if pairs is None else pairs
    u8 = [P.load_item_u8(*it) for it in items]
    got = [None] * len(items)
    enc = dict(encode_jpeg=True, jpeg_quality=jpeg_quality, jpeg_subsampling=jpeg_subsampling) if encode_jpeg else {}
    for (Hp, Wp), src_hw, batches in batches_of(rects, batch_size, pairs):
        hs = P.HostFedStep(model, batch_size, Hp, Wp, device, drain=True, mode=mode, crop=True, src_hw=src_hw, encode_png=encode_png, **enc)
        assert hs.mode == mode and hs.crop and hs.out_hw == src_hw and tuple(hs.u8[0].shape) == (batch_size, *src_hw, 3)
        for batch in batches:
            run_step(hs, [(u8[i][0], u8[i][1], rects[i]) for i in batch])
            assert np.array_equal(hs.crop_sizes(0)[:len(batch)], [pairs[i][0] for i in batch]) and not hs.crop_sizes(0)[len(batch):].any()
            if encode_png:
                for j, i in enumerate(batch):
                    h, w = pairs[i][0]
                    got[i] = np.array(Image.open(io.BytesIO(P.png_from_zlib(h, w, 3, bytes(hs.result_png(0, j))))))
                assert all(len(hs.result_png(0, j)) == 0 for j in range(len(batch), batch_size)) and result_raises(hs)
                continue
            if encode_jpeg:
                for j, i in enumerate(batch):
                    got[i] = bytes(hs.result_jpeg(0, j))
                assert all(len(hs.result_jpeg(0, j)) == 0 for j in range(len(batch), batch_size)) and result_raises(hs)
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
        assert np.array_equal(g, w), (mode, i, encode_png)
        mask = u8[i][1]
        assert np.array_equal(g[mask == 0], u8[i][0][mask == 0]) and (g[mask != 0] != u8[i][0][mask != 0]).any()
    return got


def check_written_pngs(outdir, indir, items, want):
    """The loop's files: source size, the source pixels where the mask is 0, the definition everywhere."""
    from PIL import Image
    for j, (mask_path, img_path) in enumerate(items):
        rel = os.path.splitext(mask_path[len(indir):].lstrip(os.sep))[0] + '.png'
        got = np.array(Image.open(os.path.join(outdir, rel)))
        src, mask = np.array(Image.open(img_path).convert('RGB')), np.array(Image.open(mask_path).convert('L'))
        assert got.shape == src.shape, rel
        assert np.array_equal(got[mask == 0], src[mask == 0]), rel
        assert np.array_equal(got, want[j]), rel
        assert (got[mask != 0] != src[mask != 0]).any(), rel
