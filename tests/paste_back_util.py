"""Shared by tests/test_paste_back_emu.py and tests/test_paste_back_gpu.py: the numpy restatement of lama_paste_back_u8_fwd
(csrc/elementwise.hip) and the checks both suites run -- through the host SIMT emulator and on the GPU, through the same C ABI.

``paste_back`` has no counterpart in the reference (which writes the scaled image): ``paste_back_ref`` below IS the definition, and every
comparison with the kernel is byte for byte.  ``check_ref_against_torch`` holds the restatement itself to torch's bilinear interpolation."""
import ctypes as C
import functools
import os

import numpy as np
import torch

from lama_amd import _lib as L
from lama_amd import predict as P

F32 = np.float32
CANARY = 0xA5
GUARD = 64                  # bytes in front of and behind every output buffer (keeps the buffer 4-byte aligned)
FAR = 1.0e30                # what the low-resolution tensor holds outside [:dh, :dw]: one read of it saturates a byte


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _axis(n_out: int, n_in: int):
    """rf_bilin_src for every destination index: (i0, i1, l), every operation in float32."""
    scale = F32(n_in) / F32(n_out)
    s = (np.arange(n_out, dtype=F32) + F32(0.5)) * scale - F32(0.5)
    s = np.where(s < F32(0), F32(0), s).astype(F32)
    i0 = np.minimum(s.astype(np.int32), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (s - i0.astype(F32)).astype(F32)


def bilinear_ref(lowres: np.ndarray, dsize, size) -> np.ndarray:
    """lowres [3, >= dh, >= dw] float32 -> [3, h, w]: (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11), each operation
    rounded to float32 on its own."""
    (dh, dw), (h, w) = dsize, size
    low = np.ascontiguousarray(lowres[:, :dh, :dw], dtype=F32)
    y0, y1, ly = _axis(h, dh)
    x0, x1, lx = _axis(w, dw)
    ly, lx = ly[None, :, None], lx[None, None, :]
    hy, hx = F32(1) - ly, F32(1) - lx
    top, bot = low[:, y0], low[:, y1]
    with np.errstate(invalid='ignore', over='ignore'):        # (non-finite operands are legal: they quantise as the blend kernel's do)
        a = hx * top[:, :, x0] + lx * top[:, :, x1]
        b = hx * bot[:, :, x0] + lx * bot[:, :, x1]
        v = hy * a + ly * b
    assert v.dtype == F32
    return v


def _quantize(r: np.ndarray) -> np.ndarray:
    """clip(r * 255, 0, 255) truncated, a NaN -> 0 (fmaxf returns its other operand), as lama_blend_quantize_u8_fwd does it."""
    with np.errstate(invalid='ignore', over='ignore'):
        t = r * F32(255)
        return np.fmin(np.fmax(t, F32(0)), F32(255)).astype(np.uint8)


def paste_back_ref(image_u8: np.ndarray, mask_u8: np.ndarray, lowres_f32: np.ndarray, dsize, binarize) -> np.ndarray:
    """image [h, w, 3] u8, mask [h, w] u8, lowres [3, >= dh, >= dw] float32 -> [h, w, 3] u8.  The sample is not read where the mask byte is 0
    (as lama_blend_quantize_u8_fwd does not read the prediction there): it counts as 0, and the blend then gives the source byte back."""
    h, w = mask_u8.shape
    v = np.transpose(bilinear_ref(lowres_f32, dsize, (h, w)), (1, 2, 0))
    hole = (mask_u8 != 0)[:, :, None]
    v = np.where(hole, v, F32(0)).astype(F32)
    img = image_u8.astype(F32) / F32(255)
    if binarize:
        m = hole.astype(F32)
    else:
        m = (mask_u8.astype(F32) / F32(255))[:, :, None]
    with np.errstate(invalid='ignore', over='ignore'):
        if binarize:
            r = np.where(hole, v, img).astype(F32)           # masked: the sample; unmasked: (k / 255.f) * 255.f truncates to k
        else:
            r = m * v + (F32(1) - m) * img
    assert r.dtype == F32
    return _quantize(r)


def check_ref_against_torch(size, dsize, seed=0):
    """The restatement against F.interpolate(mode='bilinear', align_corners=False) + blend + truncation: within one level everywhere (the two
    may contract differently), and the source byte wherever the mask is 0."""
    import torch.nn.functional as TF
    (h, w), (dh, dw) = size, dsize
    image, mask, low = _image(h, w, seed), _mask(h, w, 'random', seed), _lowres(dh, dw, seed)
    up = TF.interpolate(torch.from_numpy(low)[None], size=(h, w), mode='bilinear', align_corners=False)[0].permute(1, 2, 0).numpy()
    for binarize in (True, False):
        m = (mask > 0).astype(F32) if binarize else mask.astype(F32) / F32(255)
        blend = m[:, :, None] * up + (1 - m[:, :, None]) * (image.astype(F32) / F32(255))
        want = np.clip(blend * 255, 0, 255).astype(np.uint8)
        got = paste_back_ref(image, mask, low, dsize, binarize)
        assert got.shape == want.shape == (h, w, 3)
        assert np.abs(got.astype(int) - want.astype(int)).max() <= 1, (size, dsize, binarize)
        assert np.array_equal(got[mask == 0], image[mask == 0]), (size, dsize, binarize)
        assert (got[mask != 0] != image[mask != 0]).any()


# ---- kernel cases ---------------------------------------------------------------------------------------------------------------------------
# name: (Hs, Ws, [(h, w, dh, dw) or None per image])
CASES = {
    'dword-8x8-half': (8, 8, [(8, 8, 4, 4)]),
    'bytes-9x7-third': (9, 7, [(9, 7, 3, 2)]),
    'smaller-than-slot-5x6': (8, 12, [(5, 6, 4, 5)]),
    'lowres-1x1': (6, 8, [(6, 8, 1, 1)]),
    'lowres-1x4': (6, 8, [(6, 8, 1, 4)]),
    'shrink-4x4-from-6x6': (4, 4, [(4, 4, 6, 6)]),
    'batch-of-three-one-empty': (8, 12, [(8, 12, 4, 6), None, (7, 5, 4, 3)]),
    'rows-1030x1028': (1030, 1028, [(1030, 1028, 258, 257)]),
    # (beyond the issue's table) the byte path of the row-wise form: a row of more than one workgroup whose last work item is partial
    'rows-bytes-13x1027': (13, 1027, [(13, 1027, 4, 257)]),
    # the row-wise form's workgroup decode (chunk / row group / image) on a batch: 193 items per row, two row groups per slot (the second one
    # partial), an empty slot between two images, the last image smaller than its slot -- in the dword form and, at Ws = 771, in the byte form
    'rows-batch-one-empty': (6, 772, [(6, 772, 3, 386), None, (5, 770, 2, 385)]),
    'rows-bytes-batch-one-empty': (6, 771, [(6, 771, 3, 386), None, (5, 770, 2, 385)]),
}
MASKS = ('random', 'zero', 'full')
LAYOUTS = ('plain', 'view')


def _image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _mask(h, w, kind, seed):
    if kind == 'zero':
        return np.zeros((h, w), np.uint8)
    if kind == 'full':
        return np.full((h, w), 255, np.uint8)
    # about 30 % hole, with the values 1 and 128 beside 255 so that mask > 0 and mask / 255 differ
    return np.random.RandomState(seed + 1000).choice(np.array([0, 1, 128, 255], np.uint8), size=(h, w), p=[0.7, 0.1, 0.1, 0.1])


def _lowres(dh, dw, seed):
    """[3, dh, dw] in [-0.1, 1.1]: the clip is hit at both ends."""
    return (np.random.RandomState(seed + 2000).rand(3, dh, dw) * 1.2 - 0.1).astype(F32)


@functools.lru_cache(maxsize=None)
def case_data(name: str, mask_kind: str):
    """(image slots [B,Hs,Ws,3], mask slots [B,Hs,Ws], src sizes, dst sizes, [lowres [3,dh,dw] or None per image]).  The slots outside an image
    hold 77 in image AND mask: a kernel that used them would paste there."""
    Hs, Ws, images = CASES[name]
    B = len(images)
    img, msk = np.full((B, Hs, Ws, 3), 77, np.uint8), np.full((B, Hs, Ws), 77, np.uint8)
    ssz, dsz, lows = np.zeros((B, 2), np.int32), np.zeros((B, 2), np.int32), []
    for j, it in enumerate(images):
        if it is None:
            lows.append(None)
            continue
        h, w, dh, dw = it
        img[j, :h, :w], msk[j, :h, :w] = _image(h, w, 10 * j + h), _mask(h, w, mask_kind, 10 * j + w)
        ssz[j], dsz[j] = (h, w), (dh, dw)
        lows.append(_lowres(dh, dw, 10 * j + dh))
    return img, msk, ssz, dsz, lows


@functools.lru_cache(maxsize=None)
def case_want(name: str, mask_kind: str, binarize: bool) -> np.ndarray:
    """The expected output slots: zeros outside h x w and in an empty slot.  Computed once per case; both layouts and both suites share it."""
    img, msk, ssz, dsz, lows = case_data(name, mask_kind)
    want = np.zeros_like(img)
    for j, low in enumerate(lows):
        if low is not None:
            (h, w), (dh, dw) = ssz[j], dsz[j]
            want[j, :h, :w] = paste_back_ref(img[j, :h, :w], msk[j, :h, :w], low, (dh, dw), binarize)
    want.setflags(write=False)
    return want


def lowres_tensor(lows, dsz, layout, dev):
    """The low-resolution operand on ``dev``: 'plain' = a contiguous [B,3,max dh,max dw] tensor; 'view' = [B,3,max dh + 3,max dw + 5] with a
    padded batch stride inside a larger buffer.  Everything outside each image's [:dh, :dw] holds FAR.  Returns (keep-alive, L.Tensor4)."""
    B = len(lows)
    Hp, Wp = max(1, int(dsz[:, 0].max())), max(1, int(dsz[:, 1].max()))
    pad_b = 0
    if layout == 'view':
        Hp, Wp, pad_b = Hp + 3, Wp + 5, 7
    bs = 3 * Hp * Wp + pad_b
    flat = np.full((16 + B * bs + 16,), FAR, F32)
    for j, low in enumerate(lows):
        if low is not None:
            dh, dw = dsz[j]
            flat[16 + j * bs:16 + j * bs + 3 * Hp * Wp].reshape(3, Hp, Wp)[:, :dh, :dw] = low
    t = torch.from_numpy(flat).to(dev)
    return t, L.Tensor4(t.data_ptr() + 4 * 16, bs, 3, Hp, Wp, L.DT_F32)


def guarded_out(B, Hs, Ws, dev, shift=0):
    """A canary-filled u8 buffer with the [B,Hs,Ws,3] output ``shift`` bytes behind its 4-byte aligned middle: (flat, out view)."""
    n = B * Hs * Ws * 3
    flat = torch.full((GUARD + shift + n + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    return flat, flat[GUARD + shift:GUARD + shift + n].view(B, Hs, Ws, 3)


def guards_intact(flat, out) -> bool:
    n, off = out.numel(), out.storage_offset()
    return bool((flat[:off] == CANARY).all()) and bool((flat[off + n:] == CANARY).all())


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream if torch.device(dev).type == 'cuda' else 0


def _sync(dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize(dev)


def run_kernel(lib, dev, img, msk, ssz, dsz, lows, layout, binarize, shift=0):
    """One launch on copies of the operands -> (out [B,Hs,Ws,3] numpy, guards intact, inputs unchanged)."""
    B, Hs, Ws = msk.shape
    t_img, t_msk, t_ssz, t_dsz = (torch.from_numpy(a.copy()).to(dev) for a in (img, msk, ssz, dsz))
    keep, view = lowres_tensor(lows, dsz, layout, dev)
    low0 = keep.clone()
    flat, out = guarded_out(B, Hs, Ws, dev, shift)
    assert out.is_contiguous()
    lib.paste_back_u8(t_img, t_msk, t_ssz, t_dsz, view, out, B, binarize=binarize, stream=_stream(dev))
    _sync(dev)
    same = (torch.equal(t_img.cpu(), torch.from_numpy(img)) and torch.equal(t_msk.cpu(), torch.from_numpy(msk))
            and torch.equal(t_ssz.cpu(), torch.from_numpy(ssz)) and torch.equal(t_dsz.cpu(), torch.from_numpy(dsz))
            and torch.equal(keep.view(torch.int32), low0.view(torch.int32)))            # (bit patterns: a NaN operand equals itself)
    return out.cpu().numpy(), guards_intact(flat, out), same


def check_case(lib, dev, name, mask_kind, binarize, layout):
    """The kernel against the restatement, byte for byte; canaries around the output; the inputs as they were."""
    img, msk, ssz, dsz, lows = case_data(name, mask_kind)
    want = case_want(name, mask_kind, binarize)
    got, guards, same = run_kernel(lib, dev, img, msk, ssz, dsz, lows, layout, binarize)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, mask_kind, binarize, layout, len(bad), bad[:4].tolist())
    assert guards and same
    if mask_kind == 'zero':                                   # nothing to paste: the source bytes, and zeros around them
        for j, low in enumerate(lows):
            if low is not None:
                h, w = ssz[j]
                assert np.array_equal(got[j, :h, :w], img[j, :h, :w])


def check_misaligned_slots(lib, dev):
    """Slot pointers that are not 4-byte aligned take the byte path although Ws % 4 == 0: the same bytes."""
    img, msk, ssz, dsz, lows = case_data('dword-8x8-half', 'random')
    for shift in (1, 2):
        got, guards, same = run_kernel(lib, dev, img, msk, ssz, dsz, lows, 'plain', True, shift=shift)
        assert np.array_equal(got, case_want('dword-8x8-half', 'random', True)) and guards and same


def check_sizes_that_do_not_fit(lib, dev):
    """h > Hs, dw > Wp, dh = 0 with h > 0: each an all-zero slot, nothing out of bounds; the image beside them is served."""
    Hs = Ws = 8
    img, msk = np.full((4, Hs, Ws, 3), 200, np.uint8), np.full((4, Hs, Ws), 255, np.uint8)
    ssz = np.array([[9, 8], [8, 8], [8, 8], [8, 8]], np.int32)
    dsz = np.array([[4, 4], [4, 10], [0, 4], [4, 4]], np.int32)        # (10: wider than the padded 4 + 5 view too)
    low = _lowres(4, 4, 5)
    for layout in LAYOUTS:
        # (lowres_tensor sizes the view by the largest dst size: state the 4 x 4 view by hand)
        keep, view = lowres_tensor([low] * 4, np.full((4, 2), 4, np.int32), layout, dev)
        t = [torch.from_numpy(a).to(dev) for a in (img, msk, ssz, dsz)]
        for binarize in (True, False):
            flat, out = guarded_out(4, Hs, Ws, dev)
            lib.paste_back_u8(t[0], t[1], t[2], t[3], view, out, 4, binarize=binarize, stream=_stream(dev))
            _sync(dev)
            got = out.cpu().numpy()
            assert not got[:3].any() and guards_intact(flat, out)
            assert np.array_equal(got[3], paste_back_ref(img[3], msk[3], low, (4, 4), binarize))


def check_non_finite(lib, dev):
    """A NaN sample quantises to 0 under the mask (an infinite tap times a zero weight is one); +-1e38 saturate to 255 / 0; no sample is read
    (so none is seen) where the mask byte is 0."""
    img, msk = np.full((1, 4, 4, 3), 9, np.uint8), np.zeros((1, 4, 4), np.uint8)
    msk[0, :, 1:] = 255
    ssz = dsz = np.array([[4, 4]], np.int32)
    for val, want in ((np.nan, 0), (np.inf, 0), (-np.inf, 0), (1e38, 255), (-1e38, 0)):
        low = np.full((3, 4, 4), val, F32)
        for binarize in (True, False):
            got, guards, same = run_kernel(lib, dev, img, msk, ssz, dsz, [low], 'plain', binarize)
            assert guards and same
            assert (got[0, :, 1:] == want).all() and (got[0, :, 0] == 9).all(), (val, binarize)
            assert np.array_equal(got[0], paste_back_ref(img[0], msk[0], low, (4, 4), binarize))


def check_refusals(lib, dev):
    """Every LAMA_ERR_* case returns its code and launches nothing: the output keeps its canaries."""
    img, msk, ssz, dsz, lows = case_data('dword-8x8-half', 'random')
    t = [torch.from_numpy(a.copy()).to(dev) for a in (img, msk, ssz, dsz)]
    keep, view = lowres_tensor(lows, dsz, 'plain', dev)
    flat, out = guarded_out(1, 8, 8, dev)
    raw = lib._l.lama_paste_back_u8_fwd
    stream = _stream(dev)

    def call(ptrs=None, Hs=8, Ws=8, v=view, o=None, batch=1):
        a = [x.data_ptr() for x in t] if ptrs is None else ptrs
        rc = raw(stream, a[0], a[1], a[2], a[3], Hs, Ws, None if v is None else C.byref(v), out.data_ptr() if o is None else o, batch, 1)
        _sync(dev)
        assert bool((flat == CANARY).all()), 'a refused call wrote'
        return rc

    def mod(**kw):
        w = L.Tensor4(view.ptr, view.batch_stride, view.C, view.H, view.W, view.dtype)
        for k, val in kw.items():
            setattr(w, k, val)
        return w

    bad, uns = L.ERR_BAD_ARG, L.ERR_UNSUPPORTED
    good = [x.data_ptr() for x in t]
    for k in range(4):                                        # each null operand pointer
        a = list(good)
        a[k] = None
        assert call(ptrs=a) == bad, k
    assert call(v=None) == bad
    assert call(v=mod(ptr=None)) == bad
    assert raw(stream, *good, 8, 8, C.byref(view), None, 1, 1) == bad
    assert call(batch=0) == bad and call(batch=-1) == bad
    assert call(Hs=0) == bad and call(Ws=0) == bad and call(Hs=-8) == bad
    assert call(v=mod(C=4)) == bad and call(v=mod(C=1)) == bad            # not [., 3, H, W]
    assert call(v=mod(H=0)) == bad and call(v=mod(W=0)) == bad
    assert call(v=mod(batch_stride=3 * 4 * 4 - 1)) == bad
    assert call(o=good[0]) == bad                                          # in place
    assert call(v=mod(dtype=L.DT_F16)) == uns and call(v=mod(dtype=L.DT_SPLIT16)) == uns
    # ... and the binding reports them as LamaError with the code
    try:
        lib.paste_back_u8(t[0], t[1], t[2], t[3], mod(dtype=L.DT_F16), out, 1, stream=stream)
    except L.LamaError as e:
        assert e.code == uns
    else:
        raise AssertionError('not refused')
    assert raw(stream, *good, 8, 8, C.byref(view), out.data_ptr(), 1, 1) == 0     # the same call, unmodified, is served
    _sync(dev)
    assert np.array_equal(out.cpu().numpy(), case_want('dword-8x8-half', 'random', True)) and guards_intact(flat, out)


# ---- HostFedStep and the CLI ----------------------------------------------------------------------------------------------------------------
FACTOR = 0.5
# three source sizes of ONE bucket at 0.5, none of them the source slot's size (x.5 rounds to even):
SHAPES = [(21, 30), (22, 31), (20, 32)]             # scaled 10 x 15, 11 x 16, 10 x 16: the 16 x 16 bucket of the emulator tests
SHAPES_GPU = [(190, 238), (191, 239), (189, 240)]   # scaled 95 x 119, 96 x 120, 94 x 120: the 96 x 120 bucket of the other GPU step tests


def geometry(shapes):
    """(bucket = the padded scaled size all of them share, source slot = the largest source height and width)."""
    buckets = {tuple(P.ceil_modulo(v, 8) for v in P.scaled_size(h, w, FACTOR)) for h, w in shapes}
    assert len(buckets) == 1, buckets
    return buckets.pop(), (max(h for h, _ in shapes), max(w for _, w in shapes))


def write_pairs(root, shapes, seed=3):
    """PNG pairs of the given sizes; the mask has a block of 255, a pixel of 1 (any non-zero pixel is hole) and zeros."""
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    for i, (h, w) in enumerate(shapes):
        image = _image(h, w, seed + i)
        mask = np.zeros((h, w), np.uint8)
        mask[h // 4:h // 2 + 2, w // 3:2 * w // 3] = 255
        mask[1, 2] = 1
        Image.fromarray(image).save(os.path.join(root, f'im{i}.png'))
        Image.fromarray(mask).save(os.path.join(root, f'im{i}_mask.png'))
    return P.list_dataset(root if root.endswith(os.sep) else root + os.sep, '.png')


def pasted_want(model, items, batch_size, device='cpu'):
    """The expected source-size results: ``paste_back_ref`` applied to the fp32 ``inpainted`` of the existing scale_factor step, taken from its
    fp32 form -- ``load_item``'s host-scaled, padded tensors through the model as HostFedStep(u8_input=False) runs them (bin/predict.py:84-86),
    in the batches the step under test forms: ``batch_size`` images at a time, a partial batch filled with empty (all-zero) slots."""
    host = [P.load_item(m, i, 8, FACTOR) for m, i in items]
    want = []
    keep = model.keep_predicted_image
    model.keep_predicted_image = False
    try:
        for b0 in range(0, len(items), batch_size):
            part = host[b0:b0 + batch_size]
            image = np.zeros((batch_size,) + part[0][0].shape, F32)
            mask = np.zeros((batch_size,) + part[0][1].shape, F32)
            for j, it in enumerate(part):
                image[j], mask[j] = it[0], it[1]
            with torch.no_grad():
                mk = torch.from_numpy(mask).to(device)
                out = model(dict(image=torch.from_numpy(image).to(device), mask=(mk > 0) * 1))['inpainted'].float().cpu().numpy()
            for j, it in enumerate(part):
                src, msk, _ = P.load_item_u8(*items[b0 + j])
                want.append(paste_back_ref(src, msk, out[j], tuple(it[2]), True))
    finally:
        model.keep_predicted_image = keep
    return want


def one_step(hs, items):
    """Feed host set 0 with the decoded pairs (the rest of the batch: empty slots), run one step, return the result set."""
    u8 = [P.load_item_u8(m, i) for m, i in items]
    for j in range(hs.n):
        hs.put(0, j, *(u8[j][:2] if j < len(u8) else (None, None)))
    hs.prime(0)
    hs.launch(0)
    hs.wait(0)
    hs.flush(0)
    return hs.result(0).copy()


def check_step(model, items, shapes, device, mode, want):
    """HostFedStep(scale_factor=0.5, paste_back=True) in ``mode``, a batch of the pairs and one empty slot: source-slot results equal to the
    restatement (``want`` = pasted_want(..., batch_size=len(items) + 1)), zeros around each image and in the empty slot."""
    bucket, src_hw = geometry(shapes)
    n = len(items) + 1
    hs = P.HostFedStep(model, n, *bucket, device, drain=True, mode=mode, scale_factor=FACTOR, src_hw=src_hw, paste_back=True)
    assert hs.mode == mode and tuple(hs.u8[0].shape) == (n, *src_hw, 3) == tuple(hs.h_u8[0].shape)
    got = one_step(hs, items)
    for j, w in enumerate(want):
        h, wd = w.shape[:2]
        assert (h, wd) == tuple(shapes[j])
        assert np.array_equal(got[j, :h, :wd], w), (mode, j)
        assert not got[j, h:].any() and not got[j, :, wd:].any()
    assert not got[len(items)].any()
    return got


def check_written_pngs(outdir, indir, items, want):
    """The CLI's files: source size, the source pixels where the mask is 0, the restatement everywhere."""
    from PIL import Image
    for j, (mask_path, img_path) in enumerate(items):
        rel = os.path.splitext(mask_path[len(indir):].lstrip(os.sep))[0] + '.png'
        got = np.array(Image.open(os.path.join(outdir, rel)))
        src, mask = np.array(Image.open(img_path).convert('RGB')), np.array(Image.open(mask_path).convert('L'))
        assert got.shape == src.shape, rel
        assert np.array_equal(got[mask == 0], src[mask == 0]), rel
        assert np.array_equal(got, want[j]), rel
        assert (got[mask != 0] != src[mask != 0]).any(), rel
