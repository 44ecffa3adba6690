"""The device PNG encoder (lama_png_deflate_u8_fwd, csrc/png.hip; HostFedStep(encode_png=True) / the CLI's device_png on top of it), driven through
the host SIMT emulator (tests/hipemu).  The checks live in tests/png_util.py and run on the GPU too (tests/test_png_gpu.py).  The stream is
this engine's own definition: every comparison with the restatement tests/png_ref.py::deflate_ref is byte for byte, and the size condition is
held against zlib's own Z_HUFFMAN_ONLY stream of the same filtered bytes."""
import os
import zlib

import numpy as np
import pytest

from lama_amd import _lib as L
from lama_amd import predict as P
from tests import paste_back_util as PB
from tests import png_ref as R
from tests import png_util as U
from tests.emu import emu_lib


# ---- the restatement, before any kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', U.CASES)
def test_restatement_is_a_zlib_stream_of_the_filtered_bytes(name):
    """zlib.decompress(ref) is the filtered bytes, PIL decodes png_from_zlib(ref) to the pixels, no stream is longer than the bound."""
    Hs, Ws, c, cb, images, sized = U.case(name)
    for im, ref in zip(images, U.case_want(name)):
        if im is None:
            assert ref == b''
            continue
        h, w = im.shape[:2]
        raw = R.filtered(im, h, w).tobytes()
        assert zlib.decompress(ref) == raw and zlib.adler32(raw) == int.from_bytes(ref[-4:], 'big')
        assert np.array_equal(U.decode_png(P.png_from_zlib(h, w, c, ref)).reshape(h, w, c), im)
        assert len(ref) <= R.bound(h, w, c, cb) <= R.bound(Hs, Ws, c, cb)
        if sized:
            ho = R.huffman_only_len(raw)
            assert len(ref) <= ho + 160 * R.n_chunks(h, w, c, cb) + 0.01 * ho


@pytest.mark.parametrize('kind', ['photo', 'hole', 'smooth'])
@pytest.mark.parametrize('hw', [(64, 96), (101, 67), (256, 256)])
def test_restatement_meets_the_size_condition_at_the_default_chunk(kind, hw):
    h, w = hw
    im = U.hole(h, w, seed=h) if kind == 'hole' else U.photo(h, w, seed=w)
    if kind == 'smooth':
        im = (np.add.outer(np.arange(h), np.arange(w))[..., None] // 3 + np.arange(3)).astype(np.uint8)
    ref = R.deflate_ref(im, h, w)
    ho = R.huffman_only_len(R.filtered(im, h, w).tobytes())
    assert len(ref) <= ho + 160 * R.n_chunks(h, w, 3) + 0.01 * ho, (len(ref), ho)


def test_restatement_limits_the_code_lengths_to_15():
    counts = np.zeros(257, np.int64)
    for v, n in zip(range(40, 80), U.skewed_counts(22)):
        counts[v] = n
    counts[256] = 1
    assert max(R._depths([int(v) for v in counts]).values()) == 22
    lens = R.code_lengths(counts)
    assert max(lens) <= 15 and sum(2.0 ** -l for l in lens if l) == 1.0          # a complete code
    assert [l > 0 for l in lens] == [bool(v) for v in counts]
    # ... and the stored / dynamic choice: a chunk of all 256 values once is stored, 00 LEN ~LEN + raw
    raw = bytes(range(256))
    assert R.chunk_ref(raw) == b'\x00\x00\x01\xff\xfe' + raw


def test_png_from_zlib_wraps_any_zlib_stream():
    im = U.photo(5, 9, c=1, seed=1)[..., 0]
    data = P.png_from_zlib(5, 9, 1, zlib.compress(R.filtered(im, 5, 9).tobytes()))
    assert np.array_equal(U.decode_png(data), im) and data[:8] == b'\x89PNG\r\n\x1a\n' and data[-12:] == P.encode_png(im)[-12:]
    with pytest.raises(L.LamaError):
        P.png_from_zlib(5, 9, 2, b'')


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', U.CASES)
def test_kernel_is_the_restatement_byte_for_byte(name):
    U.check_case(emu_lib(), 'cpu', name)


@pytest.mark.parametrize('shift', [1, 4])
def test_misaligned_slots_take_the_narrower_loads(shift):
    """The 40 x 64 slot (192-byte rows) at a pointer 1 / 4 bytes behind a 16-byte boundary: byte / dword loads, the same stream."""
    U.check_case(emu_lib(), 'cpu', '37x53-in-40x64', shift=shift)


def test_default_chunk_bytes():
    U.check_default_chunk(emu_lib(), 'cpu')


def test_sizes_that_do_not_fit_yield_no_stream():
    U.check_sizes_that_do_not_fit(emu_lib(), 'cpu')


def test_refusals_return_their_code_and_launch_nothing():
    U.check_refusals(emu_lib(), 'cpu')


# ---- the step and the loop ------------------------------------------------------------------------------------------------------------------
BUCKET, SRC_HW = PB.geometry(PB.SHAPES)
FORMS = {'scale_factor': dict(scale_factor=PB.FACTOR, src_hw=SRC_HW),
         'scale_factor+paste_back': dict(scale_factor=PB.FACTOR, src_hw=SRC_HW, paste_back=True)}


@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    from tests.test_dist_gloo import _build_model
    root = tmp_path_factory.mktemp('png')
    items = PB.write_pairs(str(root / 'in') + os.sep, PB.SHAPES)
    same = PB.write_pairs(str(root / 'same') + os.sep, [(13, 16), (16, 11), (16, 16)], seed=9)      # three sizes of the plain 16 x 16 bucket
    return dict(model=_build_model()[0], indir=str(root / 'in') + os.sep, items=items, plain_dir=str(root / 'same') + os.sep, plain=same)


@pytest.mark.parametrize('form', ['plain', 'predicted_image', 'scale_factor', 'scale_factor+paste_back'])
def test_host_fed_step_streams_decode_to_the_u8_results(pairs, form):
    """(the emulator's device offers one mode; two pairs of different sizes and an empty slot)"""
    if form in FORMS:
        hs = U.check_step(pairs['model'], pairs['items'][:2], 'cpu', 'replay', BUCKET, **FORMS[form])
    else:
        hs = U.check_step(pairs['model'], pairs['plain'][:2], 'cpu', 'replay', (16, 16), **(dict(out_key='predicted_image') if form == 'predicted_image' else {}))
    assert hs.png[0].numel() == hs.n * hs.png_slot + 4 * hs.n and hs.png_slot % 16 == 0
    assert hs.png_slot >= emu_lib().png_deflate_bound(*hs.out_hw, 3, 0)
    with pytest.raises(L.LamaError):
        hs.result(0)


def test_host_fed_step_without_the_option_is_unchanged(pairs):
    """encode_png=False (the default): the u8 result sets, no stream buffers; the fp32 input form refuses the option."""
    hs = P.HostFedStep(pairs['model'], 2, 16, 16, 'cpu')
    assert not hs.encode_png and hs.h_u8 is not None and hs.d_out is hs.u8 and hs.h_out is hs.h_u8 and not hasattr(hs, 'png')
    with pytest.raises(L.LamaError):
        P.HostFedStep(pairs['model'], 2, 16, 16, 'cpu', u8_input=False, encode_png=True)


@pytest.mark.parametrize('form', ['plain', 'scale_factor+paste_back'])
def test_predict_loop_writes_the_same_pixels(pairs, tmp_path, form):
    """predict(device_png=True) against device_png=False, batches of two (a full and a partial round): the same names, the same pixels."""
    kw = dict(scale_factor=PB.FACTOR, paste_back=True) if form != 'plain' else {}
    items, indir = (pairs['items'], pairs['indir']) if form != 'plain' else (pairs['plain'], pairs['plain_dir'])
    outs = []
    for on in (False, True):
        outs.append(str(tmp_path / f'out{int(on)}'))
        assert P.predict(pairs['model'], items, indir, outs[-1], pad_mod=8, batch_size=2, device='cpu', io_threads=2, device_png=on, **kw) == 3
    assert len(U.check_same_pngs(*outs)) == 3
    with pytest.raises(L.LamaError):
        P.predict(pairs['model'], items, indir, os.devnull, device='cpu', out_ext='.jpg', device_png=True)


def test_cli_key_and_its_two_refusals(monkeypatch):
    base = ['model.path=/m', 'indir=i', 'outdir=o']
    assert P.parse_overrides(base)['device_png'] is False and P.DEFAULTS['device_png'] is False
    assert 'device_png' in P.KNOWN_KEYS and 'device_png' in P.BOOL_KEYS
    assert P.parse_overrides(base + ['device_png=true'])['device_png'] is True
    assert P.parse_overrides(base + ['device_png=true', 'dataset.scale_factor=0.25', 'paste_back=true'])['device_png'] is True

    def no_launch(*a, **k):
        raise AssertionError('the refusal came after the model was loaded')
    monkeypatch.setattr(P.trainers, 'load_checkpoint', no_launch)
    for extra, word in ((['device_png=true', 'out_ext=.jpg'], 'out_ext'), (['device_png=true', 'refine=true'], 'refine')):
        with pytest.raises(SystemExit) as e:
            P.main(base + extra)
        assert 'device_png' in str(e.value) and word in str(e.value), extra
    with pytest.raises(SystemExit):
        P.parse_overrides(base + ['device_png=maybe'])
