"""Shared by tests/test_png_emu.py and tests/test_png_gpu.py: the cases and checks of lama_png_deflate_u8_fwd (csrc/png.hip) against the
restatement tests/png_ref.py::deflate_ref, byte for byte, and of HostFedStep(encode_png=True) / the CLI's device_png on top of it."""
import ctypes as C
import functools
import io
import os
import zlib

import numpy as np
import torch

from lama_amd import _lib as L
from lama_amd import predict as P
from tests import png_ref as R

CANARY, GUARD = 0xA5, 64


# ---- images ---------------------------------------------------------------------------------------------------------------------------------
def photo(h, w, c=3, seed=0):
    """Photo-like: smooth gradients and waves under a few levels of noise."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[:h, :w].astype(np.float64)
    base = (128 + 60 * np.sin(x / 9.0) + 50 * np.cos(y / 7.0))[..., None] + np.arange(c) * 10.0
    return np.clip(base + rs.randn(h, w, c) * 6, 0, 255).astype(np.uint8)


def hole(h, w, c=3, seed=0):
    """The same with a flat rectangle in it, as an inpainted region of one colour would be."""
    a = photo(h, w, c, seed)
    a[h // 4:3 * h // 4, w // 3:2 * w // 3] = 200
    return a


def noise(h, w, c=3, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, c)).astype(np.uint8)


def skewed_counts(n_symbols):
    """Byte counts of a Fibonacci-type series (w[k+2] = w[k+1] + w[k]: 1, 1, 3, 4, 7, 11, 18, ... beside symbol 256's own 1) that the two-queue
    merge with its leaf-first tie rule turns into ONE chain: every leaf is larger than the sum of all leaves but its predecessor, so it is
    merged with the node that holds all smaller ones."""
    leaves = [1, 1, 1]                          # two byte values and symbol 256
    while len(leaves) < n_symbols + 1:
        leaves.append(sum(leaves[:-1]) + 1)
    return [1, 1] + leaves[3:]


def skewed_image(w, n_symbols=17):
    """One row of ``w`` RGB pixels whose FILTERED bytes (the filter type byte included) have ``skewed_counts``: a Huffman tree deeper than 15
    before the limiting rule.  The byte values are spread so that the (count, symbol) order is not the symbol order."""
    counts = skewed_counts(n_symbols)
    values = [(37 * k + 1) % 256 for k in range(n_symbols)]           # value 1 (k = 0) has count 1: the filter type byte itself
    assert len(set(values)) == n_symbols and values[0] == 1
    body = np.concatenate([np.full(n, v, np.uint8) for v, n in zip(values[1:], counts[1:])])
    assert body.size <= 3 * w, (body.size, 3 * w)
    body = np.concatenate([body, np.full(3 * w - body.size, values[-1], np.uint8)])      # the rest of the row: more of the most frequent value
    np.random.RandomState(5).shuffle(body)
    img = np.cumsum(body.reshape(w, 3).astype(np.int64), axis=0).astype(np.uint8)[None]    # undo the Sub filter: pixel = filtered + pixel to the left
    raw = R.filtered(img, 1, w)
    cnt = np.bincount(raw.ravel(), minlength=257)
    cnt[256] = 1
    assert max(R._depths([int(v) for v in cnt]).values()) > 15, 'the case does not reach the limiting rule'
    return img


# name: (Hs, Ws, c, chunk_bytes, [image [h,w,c] or None per slot], size condition against zlib?)
@functools.lru_cache(maxsize=None)
def case(name):
    def one(img, Hs=None, Ws=None, cb=256, sized=False):
        h, w, c = img.shape
        return (Hs or h, Ws or w, c, cb, [img], sized)
    if name == '1x1':
        return one(noise(1, 1, seed=1))
    if name == '1x5':
        return one(noise(1, 5, seed=2))
    if name == '3x7':
        return one(photo(3, 7, seed=3))
    if name == '3x7-in-4x8':                                    # a row of 24 slot bytes: dword loads
        return one(photo(3, 7, seed=3), 4, 8)
    if name == '37x53-in-40x64':                                # row stride != row, 16-byte loads, R = 1 row... chunk 512 = 3 rows of 160, a short last chunk
        return one(photo(37, 53, seed=4), 40, 64, cb=512, sized=True)
    if name == 'hole-37x53-in-40x64':
        return one(hole(37, 53, seed=5), 40, 64, cb=1024, sized=True)
    if name == 'one-row-per-chunk':                             # chunk_bytes < 2 rows (row = 160)
        return one(photo(9, 53, seed=6), cb=300, sized=True)
    if name == 'row-longer-than-chunk':                         # chunk_bytes < 1 row: R = max(1, 0)
        return one(photo(3, 53, seed=7), cb=64)
    if name == 'flat':                                          # two used symbols (the colour's first pixel aside) of one bit
        return one(np.full((16, 24, 3), 9, np.uint8))
    if name == 'flat-zero':                                     # filtered bytes 1 and 0 only
        return one(np.zeros((16, 24, 3), np.uint8))
    if name == 'noise-stored':                                  # stored fallback in every chunk
        return one(noise(20, 30, seed=8), cb=512)
    if name == 'mixed-stored':                                  # only some chunks fall back
        a = photo(24, 30, seed=9)
        a[6:12] = noise(6, 30, seed=10)
        a[20:] = noise(4, 30, seed=11)
        return one(a, cb=546)                                   # 6 rows of 91
    if name == 'depth-limit':                                   # one row of w = 2047: 6142 raw bytes, one chunk
        return one(skewed_image(2047), cb=8192)
    if name == 'gray':
        return one(photo(19, 31, c=1, seed=12), 24, 32, cb=256, sized=True)
    if name == 'gray-odd':
        return one(hole(11, 13, c=1, seed=13), cb=64)
    if name == 'batch-of-4':                                    # mixed sizes and one empty slot
        return (24, 32, 3, 512, [photo(24, 32, seed=14), None, hole(17, 5, seed=15), noise(1, 32, seed=16)], False)
    if name == 'chunks-beyond-one-tile':                        # 300 chunks: the assembly's second tile of 256
        return one(photo(300, 3, seed=17), cb=64)
    raise KeyError(name)


CASES = ('1x1', '1x5', '3x7', '3x7-in-4x8', '37x53-in-40x64', 'hole-37x53-in-40x64', 'one-row-per-chunk', 'row-longer-than-chunk', 'flat',
         'flat-zero', 'noise-stored', 'mixed-stored', 'depth-limit', 'gray', 'gray-odd', 'batch-of-4', 'chunks-beyond-one-tile')


@functools.lru_cache(maxsize=None)
def case_want(name):
    """The restatement's stream per slot (b'' for an empty one): computed once, shared by both suites."""
    Hs, Ws, c, cb, images, _ = case(name)
    return tuple(b'' if im is None else R.deflate_ref(im, im.shape[0], im.shape[1], cb) for im in images)


def slots_of(name, fill=77):
    """(slots [B,Hs,Ws,c] u8 with ``fill`` outside each image, sizes [B,2] int32)."""
    Hs, Ws, c, cb, images, _ = case(name)
    slots = np.full((len(images), Hs, Ws, c), fill, np.uint8)
    sizes = np.zeros((len(images), 2), np.int32)
    for j, im in enumerate(images):
        if im is not None:
            slots[j, :im.shape[0], :im.shape[1]] = im
            sizes[j] = im.shape[:2]
    return slots, sizes


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream if torch.device(dev).type == 'cuda' else 0


def _sync(dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize(dev)


def shifted(a: np.ndarray, dev, shift=0):
    """``a`` on ``dev``, ``shift`` bytes behind a 16-byte aligned address: (keep-alive, view)."""
    flat = torch.zeros(a.size + shift + 32, dtype=torch.uint8, device=dev)
    off = (-flat.data_ptr()) % 16 + shift
    v = flat[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return flat, v


def run(lib, dev, slots, sizes, chunk_bytes, *, shift=0, pad=3, workspace=None):
    """One call -> (streams [bytes per slot], out_bytes, canaries intact: around the buffer and behind every stream's end, workspace)."""
    B, Hs, Ws, c = slots.shape
    keep, img = shifted(slots, dev, shift)
    t_sizes = torch.from_numpy(sizes.copy()).to(dev)
    stride = lib.png_deflate_bound(Hs, Ws, c, chunk_bytes) + pad                # (pad 3: slots at odd byte offsets)
    assert stride - pad == R.bound(Hs, Ws, c, chunk_bytes or R.DEFAULT_CHUNK)
    flat = torch.full((GUARD + B * stride + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    out = flat[GUARD:GUARD + B * stride]
    n_out = torch.full((B,), -7, dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = torch.empty(lib.png_deflate_workspace_bytes(B, Hs, Ws, c, chunk_bytes), dtype=torch.uint8, device=dev)
    lib.png_deflate_u8(img, t_sizes, out, stride, n_out, workspace, B, chunk_bytes=chunk_bytes, stream=_stream(dev))
    _sync(dev)
    assert torch.equal(img.cpu(), torch.from_numpy(slots)) and torch.equal(t_sizes.cpu(), torch.from_numpy(sizes))      # the operands as they were
    host, lens = flat.cpu().numpy(), n_out.cpu().numpy()
    intact = bool((host[:GUARD] == CANARY).all() and (host[GUARD + B * stride:] == CANARY).all())
    streams = []
    for j in range(B):
        n = int(lens[j])
        assert 0 <= n <= stride - pad, (j, n)
        slot = host[GUARD + j * stride:GUARD + (j + 1) * stride]
        streams.append(slot[:n].tobytes())
        intact = intact and bool((slot[n:] == CANARY).all())
    return streams, lens, intact, workspace


def decode_png(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


def check_case(lib, dev, name, shift=0):
    """The kernel's bytes are the restatement's, out_bytes is exact, nothing behind a stream's end is touched, a second call (on the used
    workspace) gives the same bytes; zlib and PIL decode the stream to the filtered bytes and the pixels."""
    Hs, Ws, c, cb, images, sized = case(name)
    want = case_want(name)
    slots, sizes = slots_of(name)
    got, lens, intact, ws = run(lib, dev, slots, sizes, cb, shift=shift)
    for j, im in enumerate(images):
        assert lens[j] == len(want[j]), (name, j, int(lens[j]), len(want[j]))
        if got[j] != want[j]:
            k = next(i for i in range(len(want[j])) if got[j][i] != want[j][i])
            raise AssertionError((name, j, 'first difference at byte', k, got[j][k:k + 8].hex(), want[j][k:k + 8].hex()))
        if im is None:
            continue
        h, w = im.shape[:2]
        raw = R.filtered(im, h, w).tobytes()
        assert zlib.decompress(got[j]) == raw
        assert np.array_equal(decode_png(P.png_from_zlib(h, w, c, got[j])).reshape(h, w, c), im)
        if sized:                                           # held against zlib, not against the code under test
            ho = R.huffman_only_len(raw)
            assert len(got[j]) <= ho + 160 * R.n_chunks(h, w, c, cb) + 0.01 * ho, (name, len(got[j]), ho)
    assert intact
    again, lens2, intact2, _ = run(lib, dev, slots, sizes, cb, shift=shift, workspace=ws)
    assert again == got and np.array_equal(lens, lens2) and intact2
    return got


def check_default_chunk(lib, dev):
    """chunk_bytes = 0 is 24576: a 96 x 128 photo-like image in 2 chunks (66 rows of 385 bytes, then 30), and the size condition at the default."""
    im = photo(96, 128, seed=20)
    got, lens, intact, _ = run(lib, dev, im[None], np.array([[96, 128]], np.int32), 0)
    assert got[0] == R.deflate_ref(im, 96, 128) and intact and R.n_chunks(96, 128, 3) == 2
    ho = R.huffman_only_len(R.filtered(im, 96, 128).tobytes())
    assert len(got[0]) <= ho + 160 * 2 + 0.01 * ho


def check_sizes_that_do_not_fit(lib, dev):
    """h > Hs, w > Ws, negative sizes: out_bytes 0 and nothing else touched, the image beside them is served."""
    im = photo(8, 8, seed=21)
    slots = np.repeat(im[None], 4, 0)
    sizes = np.array([[9, 8], [8, 9], [-1, 8], [8, 8]], np.int32)
    got, lens, intact, _ = run(lib, dev, slots, sizes, 256)
    assert list(lens[:3]) == [0, 0, 0] and got[3] == R.deflate_ref(im, 8, 8, 256) and intact


def check_refusals(lib, dev):
    """Every refusal code, with nothing launched: the output keeps its canaries and out_bytes its sentinel."""
    im = photo(8, 8, seed=22)
    keep, img = shifted(im[None], dev)
    sizes = torch.tensor([[8, 8]], dtype=torch.int32, device=dev)
    stride = lib.png_deflate_bound(8, 8, 3, 256)
    out = torch.full((stride + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    n_out = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.png_deflate_workspace_bytes(1, 8, 8, 3, 256), dtype=torch.uint8, device=dev)
    raw = lib._l.lama_png_deflate_u8_fwd
    good = dict(image=img.data_ptr(), sizes=sizes.data_ptr(), Hs=8, Ws=8, c=3, batch=1, cb=256, out=out.data_ptr(), stride=stride, n=n_out.data_ptr(),
                ws=ws.data_ptr(), wsb=ws.numel())

    def call(**kw):
        a = dict(good, **kw)
        rc = raw(_stream(dev), a['image'], a['sizes'], a['Hs'], a['Ws'], a['c'], a['batch'], a['cb'], a['out'], a['stride'], a['n'], a['ws'], a['wsb'])
        _sync(dev)
        assert bool((out == CANARY).all()) and int(n_out[0]) == -7, ('a refused call wrote', kw)
        return rc

    bad, uns = L.ERR_BAD_ARG, L.ERR_UNSUPPORTED
    for k in ('image', 'sizes', 'out', 'n', 'ws'):
        assert call(**{k: None}) == bad, k
    assert call(c=2) == bad and call(c=4) == bad and call(c=0) == bad
    assert call(cb=63) == bad and call(cb=32769) == bad and call(cb=-1) == bad
    assert call(stride=stride - 1) == bad
    assert call(batch=0) == bad and call(Hs=0) == bad and call(Ws=-8) == bad
    assert call(Ws=21845) == uns                                             # a row of 1 + 3 * 21845 = 65536 bytes (refused before the bound is looked at)
    assert call(wsb=ws.numel() - 1) == L.ERR_WORKSPACE
    n = C.c_size_t(5)
    wsq = lib._l.lama_png_deflate_workspace_bytes
    assert wsq(1, 8, 8, 2, 256, C.byref(n)) == bad and wsq(1, 8, 8, 3, 256, None) == bad and wsq(1, 8, 21845, 3, 256, C.byref(n)) == uns and n.value == 5
    assert lib.png_deflate_bound(8, 8, 2, 256) == 0 and lib.png_deflate_bound(0, 8, 3, 256) == 0 and lib.png_deflate_bound(8, 8, 3, 63) == 0
    assert lib.png_deflate_bound(1, 21845, 1, 64) == 21846 + 5 + 11
    try:
        lib.png_deflate_u8(img, sizes, out, stride - 1, n_out, ws, 1, chunk_bytes=256, stream=_stream(dev))
    except L.LamaError as e:
        assert e.code == bad
    else:
        raise AssertionError('not refused')
    g = good                                                                 # the same call, unmodified, is served
    assert raw(_stream(dev), g['image'], g['sizes'], 8, 8, 3, 1, 256, g['out'], stride, g['n'], g['ws'], g['wsb']) == 0
    _sync(dev)
    want = R.deflate_ref(im, 8, 8, 256)
    assert int(n_out[0]) == len(want) and out[:len(want)].cpu().numpy().tobytes() == want and bool((out[len(want):] == CANARY).all())


# ---- HostFedStep and the CLI ----------------------------------------------------------------------------------------------------------------
def feed(hs, p, u8_pairs):
    for j in range(hs.n):
        hs.put(p, j, *(u8_pairs[j][:2] if j < len(u8_pairs) else (None, None)))


def one_step(hs, u8_pairs):
    feed(hs, 0, u8_pairs)
    hs.prime(0)
    hs.launch(0)
    hs.wait(0)
    hs.flush(0)


def check_step(model, items, device, mode, bucket, **form):
    """HostFedStep(encode_png=True) in ``mode``, the pairs and one empty slot: every stream decodes to the u8 result of the same step with
    the option off, byte for byte, and is the restatement's stream of it; the lengths are exact."""
    pairs = [P.load_item_u8(m, i) for m, i in items]
    n = len(items) + 1
    ref = P.HostFedStep(model, n, *bucket, device, drain=True, mode=mode, **form)
    one_step(ref, pairs)
    want = ref.result(0).copy()
    hs = P.HostFedStep(model, n, *bucket, device, drain=True, mode=mode, encode_png=True, **form)
    assert hs.mode == mode and hs.encode_png and hs.h_u8 is None
    one_step(hs, pairs)
    assert tuple(hs.out_hw) == tuple(want.shape[1:3])
    crops = hs.crop_sizes(0)
    for j in range(n):
        data = bytes(hs.result_png(0, j))
        if j == len(items):
            assert data == b'' and tuple(crops[j]) == (0, 0)
            continue
        h, w = (int(v) for v in crops[j])
        assert h > 0 and w > 0
        assert data == R.deflate_ref(want[j], h, w), (mode, form, j)
        assert np.array_equal(decode_png(P.png_from_zlib(h, w, 3, data)), want[j, :h, :w]), (mode, form, j)
    return hs


def check_same_pngs(dir_a, dir_b):
    """The same file names, and every pair of PNGs decodes (PIL) to identical pixels."""
    from PIL import Image
    names = sorted(os.path.relpath(os.path.join(d, f), dir_a) for d, _, fs in os.walk(dir_a) for f in fs)
    assert names and names == sorted(os.path.relpath(os.path.join(d, f), dir_b) for d, _, fs in os.walk(dir_b) for f in fs)
    for nm in names:
        a, b = np.array(Image.open(os.path.join(dir_a, nm))), np.array(Image.open(os.path.join(dir_b, nm)))
        assert a.shape == b.shape and np.array_equal(a, b), nm
    return names
