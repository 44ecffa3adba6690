"""The device JPEG encoder (lama_jpeg_scan_u8_fwd, csrc/jpeg.hip; HostFedStep(encode_jpeg=True) / the CLI's device_jpeg on top of it), driven
through the host SIMT emulator (tests/hipemu).  The checks live in tests/jpeg_util.py and run on the GPU too (tests/test_jpeg_gpu.py).  The scan
is this engine's own definition: every comparison with the restatement tests/jpeg_ref.py::scan_ref is byte for byte, and the restatement itself
is held against things that are not the code under test -- PIL's tables, PIL's decoder, an fp64 DCT and PIL's own file of the same structure.

Measured against PIL (Pillow 12.2 on libjpeg-turbo; restart_marker_rows=1, optimize=False) on the inputs of test_restatement_against_pil, length gap in
per cent of PIL's file / PSNR deficit in dB:
                        q75 4:4:4        q75 4:2:0        q95 4:4:4        q95 4:2:0
    photo 37 x 53    +0.000 / +0.0001  +0.000 / +0.0100  +0.126 / -0.0051  -0.362 / +0.0284
    hole  37 x 53    +0.000 / -0.0029  +0.000 / -0.0014  +0.084 / +0.0028  -0.175 / +0.0244
    photo 96 x 128   -0.038 / -0.0007  -0.090 / -0.0086  +0.028 / +0.0072  -0.051 / -0.0040
    hole  96 x 128   +0.039 / -0.0009  -0.185 / -0.0069  -0.117 / +0.0014  +0.294 / -0.0012
The bars of tests/jpeg_util.py are the largest of each plus half of it again: 0.442 % and 0.0426 dB."""
import io
import os

import numpy as np
import pytest

from lama_amd import _lib as L
from lama_amd import jpeg as J
from lama_amd import predict as P
from tests import jpeg_ref as R
from tests import jpeg_util as U
from tests import paste_back_util as PB
from tests.emu import emu_lib


# ---- the restatement, against things that are not the code under test -----------------------------------------------------------------------
@pytest.mark.parametrize('ss', [R.J444, R.J420])
@pytest.mark.parametrize('quality', [1, 50, 75, 95, 100])
def test_tables_are_the_ones_pil_writes(quality, ss):
    """The DQT and DHT segments of jpeg_from_scan equal PIL's for the same quality and subsampling, byte for byte, and the rest of the header
    has PIL's structure."""
    im = U.photo(16, 16, seed=1)
    ours = U.segments(P.jpeg_from_scan(16, 16, quality, ss, R.scan_ref(im, 16, 16, quality, ss)))
    pil = U.segments(U.pil_jpeg(im, quality, ss))
    for marker in (0xdb, 0xc4):
        assert [b for m, b in ours if m == marker] == [b for m, b in pil if m == marker] and sum(m == marker for m, _ in ours) == (2 if marker == 0xdb else 4)
    assert [m for m, _ in ours] == [m for m, _ in pil] == [0xe0, 0xdb, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xdd, 0xda]
    assert dict(ours)[0xc0] == dict(pil)[0xc0] and dict(ours)[0xdd] == dict(pil)[0xdd] and dict(ours)[0xda] == dict(pil)[0xda]
    if quality == 95:
        assert list(J.quant_table(J.QUANT_LUMA, 95)[:8]) == [2, 1, 1, 2, 2, 4, 5, 6]


@pytest.mark.parametrize('name', U.CASES)
def test_restatement_decodes(name):
    """PIL opens and decodes jpeg_from_scan(scan_ref(...)): the right size, mode RGB, the expected quantisation tables; no scan is longer than
    the bound; every case reaches the mechanism it is there for (asserted in case_want)."""
    from PIL import Image
    import io
    Hs, Ws, q, ss, images, _ = U.case(name)
    for im, ref in zip(images, U.case_want(name)):
        if im is None:
            assert ref == b''
            continue
        h, w = im.shape[:2]
        pim = Image.open(io.BytesIO(P.jpeg_from_scan(h, w, q, ss, ref)))
        pim.load()
        assert pim.size == (w, h) and pim.mode == 'RGB'
        zz = list(J.ZIGZAG)
        want_q = {0: [int(v) for v in J.quant_table(J.QUANT_LUMA, q)], 1: [int(v) for v in J.quant_table(J.QUANT_CHROMA, q)]}
        got_q = {k: list(v) for k, v in pim.quantization.items()}
        assert got_q == want_q or got_q == {k: [v[i] for i in zz] for k, v in want_q.items()}      # (Pillow has reported either order over its versions)
        assert len(ref) <= R.bound(h, w, ss) <= R.bound(Hs, Ws, ss)
        assert ref.count(b'\xff') == sum(ref[i + 1] == 0 or 0xd0 <= ref[i + 1] <= 0xd7 for i in range(len(ref) - 1) if ref[i] == 0xff)


def test_restatement_levels_against_an_fp64_dct():
    """The integer DCT (coefficients times 8) against the fp64 orthonormal DCT of the same integer samples: within DCT_BOUND; a level differs from
    round(fp64 / Q) by at most 1, and only where fp64 / Q lies within DCT_BOUND / Q of a rounding boundary."""
    rs = np.random.RandomState(3)
    y, cb, cr = R.ycc_planes(np.concatenate([U.noise(64, 64, seed=1), U.photo(64, 64, seed=2), U.blocks8(64, 64, 1), U.blocks8(64, 64)], 1), R.J444)
    blocks = np.concatenate([R.blocks_of(p).reshape(-1, 8, 8) for p in (y, cb, cr)] + [rs.choice([0, 255], (64, 8, 8))])
    C = R.dct_matrix_f64()
    real = np.einsum('vy,byx,ux->bvu', C, blocks.astype(np.float64) - 128, C)
    got = R.fdct(blocks)
    assert np.abs(got / 8.0 - real).max() < R.DCT_BOUND
    assert np.abs(got).max() <= 8 * 1024 + 4
    for q in (50, 95, 100):
        Q = J.quant_table(J.QUANT_LUMA, q).reshape(8, 8)
        lev = R.quantise(got, Q.ravel())
        ideal = real / Q
        want = np.sign(ideal) * np.floor(np.abs(ideal) + 0.5)
        diff = lev - want.reshape(-1, 64)[:, list(J.ZIGZAG)]
        assert np.abs(diff).max() <= 1
        frac = np.abs(np.abs(ideal) + 0.5 - np.round(np.abs(ideal) + 0.5))          # distance of |ideal| from a rounding boundary
        near = (frac <= R.DCT_BOUND / Q).reshape(-1, 64)[:, list(J.ZIGZAG)]
        assert not (diff != 0)[~near].any()


@pytest.mark.parametrize('ss', [R.J444, R.J420])
@pytest.mark.parametrize('quality', [75, 95])
@pytest.mark.parametrize('kind', ['photo', 'hole'])
@pytest.mark.parametrize('hw', [(37, 53), (96, 128)])
def test_restatement_against_pil(hw, kind, quality, ss):
    """File length and PSNR of the PIL-decoded file against the source, held to PIL's own file of the same structure."""
    im = (U.hole if kind == 'hole' else U.photo)(*hw)
    ours = P.jpeg_from_scan(*hw, quality, ss, R.scan_ref(im, *hw, quality, ss))
    pil = U.pil_jpeg(im, quality, ss)
    gap_len = (len(ours) - len(pil)) / len(pil)
    gap_db = U.psnr(U.decode_jpeg(pil), im) - U.psnr(U.decode_jpeg(ours), im)
    print(f'{kind} {hw} q{quality} ss{ss}: length {len(ours)} / {len(pil)} ({100 * gap_len:+.3f} %), PSNR deficit {gap_db:+.4f} dB')
    assert gap_len <= U.LENGTH_BAR and gap_db <= U.PSNR_BAR


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', U.CASES)
def test_kernel_is_the_restatement_byte_for_byte(name):
    U.check_case(emu_lib(), 'cpu', name)


@pytest.mark.parametrize('ss', ['444', '420'])
@pytest.mark.parametrize('shift', [1, 2, 3])
def test_misaligned_slots_take_the_narrow_loads(shift, ss):
    """The 40 x 64 slot (192-byte rows) at a pointer 1 / 2 / 3 bytes behind a 16-byte boundary: single-byte loads, the same scan."""
    U.check_case(emu_lib(), 'cpu', f'37x53-in-40x64@{ss}', shift=shift)


def test_sizes_that_do_not_fit_yield_no_scan():
    U.check_sizes_that_do_not_fit(emu_lib(), 'cpu')


def test_a_scan_longer_than_its_slot_reports_the_bytes_needed():
    U.check_overflow(emu_lib(), 'cpu')


def test_refusals_return_their_code_and_launch_nothing():
    U.check_refusals(emu_lib(), 'cpu')


# ---- the step and the loop ------------------------------------------------------------------------------------------------------------------
BUCKET, SRC_HW = PB.geometry(PB.SHAPES)
FORMS = {'scale_factor': dict(scale_factor=PB.FACTOR, src_hw=SRC_HW),
         'scale_factor+paste_back': dict(scale_factor=PB.FACTOR, src_hw=SRC_HW, paste_back=True)}


@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    from tests.test_dist_gloo import _build_model
    root = tmp_path_factory.mktemp('jpeg')
    items = PB.write_pairs(str(root / 'in') + os.sep, PB.SHAPES)
    same = PB.write_pairs(str(root / 'same') + os.sep, [(13, 16), (16, 11), (16, 16)], seed=9)      # three sizes of the plain 16 x 16 bucket
    return dict(model=_build_model()[0], indir=str(root / 'in') + os.sep, items=items, plain_dir=str(root / 'same') + os.sep, plain=same)


@pytest.fixture(scope='module')
def png_runs(pairs, tmp_path_factory):
    """The PNG runs the JPEG files are held against, once per form."""
    done = {}

    def get(form):
        if form not in done:
            kw = dict(scale_factor=PB.FACTOR, paste_back=True) if form != 'plain' else {}
            items, indir = (pairs['items'], pairs['indir']) if form != 'plain' else (pairs['plain'], pairs['plain_dir'])
            out = str(tmp_path_factory.mktemp('png_run'))
            assert P.predict(pairs['model'], items, indir, out, pad_mod=8, batch_size=2, device='cpu', io_threads=2, **kw) == len(items)
            done[form] = (items, indir, kw, out)
        return done[form]
    return get


@pytest.mark.parametrize('form', ['plain', 'predicted_image-444-q50', 'scale_factor', 'scale_factor+paste_back'])
def test_host_fed_step_scans_are_the_restatement_of_the_u8_results(pairs, form):
    """(the emulator's device offers one mode; three pairs and an empty slot)"""
    if form in FORMS:
        U.check_step(pairs['model'], pairs['items'][:3], 'cpu', 'replay', BUCKET, **FORMS[form])
    elif form == 'plain':
        U.check_step(pairs['model'], pairs['plain'], 'cpu', 'replay', (16, 16))
    else:
        U.check_step(pairs['model'], pairs['plain'], 'cpu', 'replay', (16, 16), quality=50, subsampling='444', out_key='predicted_image')


def test_host_fed_step_reports_a_scan_that_does_not_fit(pairs):
    U.check_step_overflow(pairs['model'], pairs['plain'][:2], 'cpu', 'replay', (16, 16))


def test_host_fed_step_without_the_option_is_unchanged(pairs):
    """encode_jpeg=False (the default): the u8 result sets, no scan buffers; the option excludes encode_png and the fp32 input form."""
    loaded = [P.load_item_u8(m, i) for m, i in pairs['plain'][:2]]
    hs = P.HostFedStep(pairs['model'], 2, 16, 16, 'cpu')
    off = P.HostFedStep(pairs['model'], 2, 16, 16, 'cpu', encode_jpeg=False, jpeg_quality=50, jpeg_subsampling='444')
    U.one_step(hs, loaded)
    U.one_step(off, loaded)
    assert hs.result(0).shape == off.result(0).shape == (2, 16, 16, 3) and np.array_equal(hs.result(0), off.result(0)) and hs.result(0).any()
    assert np.array_equal(hs.crop_sizes(0), off.crop_sizes(0)) and not off.encode_jpeg and off.h_out is off.h_u8 and not hasattr(off, 'jpeg')
    assert not hs.encode_jpeg and not hs.encode_png and hs.h_u8 is not None and hs.d_out is hs.u8 and hs.h_out is hs.h_u8 and not hasattr(hs, 'jpeg')
    for bad in (dict(u8_input=False), dict(encode_png=True), dict(jpeg_quality=0), dict(jpeg_subsampling='422')):
        with pytest.raises(L.LamaError):
            P.HostFedStep(pairs['model'], 2, 16, 16, 'cpu', encode_jpeg=True, **bad)


@pytest.mark.parametrize('form', ['plain', 'scale_factor+paste_back'])
def test_predict_loop_writes_the_restatement_files(pairs, png_runs, tmp_path, form):
    """predict(device_jpeg=True, out_ext='.jpg') against the PNG run (and, 'plain', the option off), batches of two (a full and a partial round)."""
    items, indir, kw, png = png_runs(form)
    on, off = str(tmp_path / 'on'), None
    assert P.predict(pairs['model'], items, indir, on, pad_mod=8, batch_size=2, device='cpu', io_threads=2, out_ext='.jpg', device_jpeg=True, **kw) == len(items)
    if form == 'plain':
        off = str(tmp_path / 'off')
        assert P.predict(pairs['model'], items, indir, off, pad_mod=8, batch_size=2, device='cpu', io_threads=2, out_ext='.jpg', **kw) == len(items)
        for bad in (dict(out_ext='.png'), dict(out_ext='.jpg', device_png=True)):
            with pytest.raises(L.LamaError):
                P.predict(pairs['model'], items, indir, os.devnull, device='cpu', device_jpeg=True, **bad)
    assert len(U.check_cli_outputs(png, on, dir_off=off)) == len(items)


def test_predict_loop_takes_the_host_fallback_for_a_slot_that_overflows(pairs, png_runs, tmp_path, monkeypatch):
    """Scan slots as long as the shortest scan (the test hook; 4:4:4 at quality 80): the larger images overflow and are computed again and
    encoded on the host, the shortest keeps the device's bytes; every file is a valid JPEG of its image."""
    from PIL import Image
    items, indir, kw, png = png_runs('plain')
    jpg, q, ss = str(tmp_path / 'jpg'), 80, R.J444
    sizes = {}
    for nm in U.files_of(png):
        src = np.array(Image.open(os.path.join(png, nm)))
        sizes[os.path.splitext(nm)[0]] = len(R.scan_ref(src, *src.shape[:2], q, ss))
    stride = min(sizes.values())                           # the shortest scan fits exactly, the longer ones do not
    assert len(set(sizes.values())) >= 2
    monkeypatch.setattr(P, 'JPEG_OUT_STRIDE', stride)
    assert P.predict(pairs['model'], items, indir, jpg, pad_mod=8, batch_size=2, device='cpu', out_ext='.JPEG', device_jpeg=True, jpeg_quality=q,
                     jpeg_subsampling='444') == 3
    assert [os.path.splitext(n)[0] for n in U.files_of(jpg)] == sorted(sizes) and all(n.endswith('.JPEG') for n in U.files_of(jpg))
    n_host = 0
    for nm in U.files_of(jpg):
        stem = os.path.splitext(nm)[0]
        src = np.array(Image.open(os.path.join(png, stem + '.png')))
        with open(os.path.join(jpg, nm), 'rb') as f:
            data = f.read()
        dec = U.decode_jpeg(data)
        assert dec.shape == src.shape and U.psnr(dec, src) >= U.psnr(U.decode_jpeg(U.pil_jpeg(src, q, ss)), src) - 1.0      # (a valid file of THIS image)
        device_made = data == P.jpeg_from_scan(*src.shape[:2], q, ss, R.scan_ref(src, *src.shape[:2], q, ss))
        assert device_made == (sizes[stem] <= stride), nm
        n_host += not device_made
    assert n_host == sum(v > stride for v in sizes.values()) >= 1


def test_predict_loop_fallback_over_several_batches_with_paste_back(pairs, png_runs, tmp_path, monkeypatch):
    """Scan slots of 16 bytes with scale_factor + paste_back and batches of two: every image overflows, the fallback step runs twice (a full and a
    partial batch) in the source-slot form, and every file decodes to its image as PIL's own file of the PNG run's pixels does."""
    from PIL import Image
    items, indir, kw, png = png_runs('scale_factor+paste_back')
    jpg = str(tmp_path / 'jpg')
    monkeypatch.setattr(P, 'JPEG_OUT_STRIDE', 16)
    assert len(items) == 3
    assert P.predict(pairs['model'], items, indir, jpg, pad_mod=8, batch_size=2, device='cpu', out_ext='.jpg', device_jpeg=True, **kw) == 3
    assert [os.path.splitext(n)[0] for n in U.files_of(jpg)] == [os.path.splitext(n)[0] for n in U.files_of(png)]
    for nm in U.files_of(jpg):
        src = np.array(Image.open(os.path.join(png, os.path.splitext(nm)[0] + '.png')))
        with open(os.path.join(jpg, nm), 'rb') as f:
            data = f.read()
        b = io.BytesIO()
        Image.fromarray(src).save(b, 'JPEG', quality=95, subsampling=2)
        assert data == b.getvalue(), nm                    # the host fallback's own bytes: libjpeg at the same quality and subsampling


def test_cli_keys_and_refusals(monkeypatch):
    base = ['model.path=/m', 'indir=i', 'outdir=o']
    cfg = P.parse_overrides(base)
    assert cfg['device_jpeg'] is False and cfg['jpeg_quality'] == 95 and cfg['jpeg_subsampling'] == '420'
    assert {'device_jpeg', 'jpeg_quality', 'jpeg_subsampling'} <= P.KNOWN_KEYS
    assert 'device_jpeg' in P.BOOL_KEYS and 'jpeg_quality' in P.INT_KEYS and 'jpeg_subsampling' in P.STRING_KEYS
    cfg = P.parse_overrides(base + ['device_jpeg=true', 'out_ext=.JPG', 'jpeg_quality=80', 'jpeg_subsampling=444', 'dataset.scale_factor=0.25', 'paste_back=true'])
    assert cfg['device_jpeg'] is True and cfg['jpeg_quality'] == 80 and cfg['jpeg_subsampling'] == '444'
    assert P.parse_overrides(base + ['device_jpeg=true', 'out_ext=.jpeg'])['device_jpeg'] is True
    assert P.parse_overrides(base + ['out_ext=.jpg'])['device_jpeg'] is False               # a .jpg without the option stays PIL's

    def no_launch(*a, **k):
        raise AssertionError('the refusal came after the model was loaded')
    monkeypatch.setattr(P.trainers, 'load_checkpoint', no_launch)
    on = ['device_jpeg=true', 'out_ext=.jpg']
    for extra, words in ((['device_jpeg=true'], ('device_jpeg', 'out_ext')), (['device_jpeg=true', 'out_ext=.png'], ('device_jpeg', 'out_ext')),
                         (on + ['refine=true'], ('device_jpeg', 'refine')), (['device_jpeg=true', 'device_png=true'], ('device_png',)),
                         (on + ['device_png=true'], ('device_png',)), (on + ['jpeg_quality=0'], ('jpeg_quality',)),
                         (on + ['jpeg_quality=101'], ('jpeg_quality',)), (on + ['jpeg_subsampling=422'], ('jpeg_subsampling',)),
                         (['out_ext=.jpg', 'jpeg_quality=90'], ('jpeg_quality', 'device_jpeg'))):
        with pytest.raises(SystemExit) as e:
            P.main(base + extra)
        assert all(wd in str(e.value) for wd in words), (extra, str(e.value))
    with pytest.raises(SystemExit):
        P.parse_overrides(base + ['device_jpeg=maybe'])
