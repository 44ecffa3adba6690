"""``crop_to_mask`` (lama_crop_compose_u8_fwd / lama_crop_paste_u8_fwd, csrc/elementwise.hip; ``crop_rect``, HostFedStep(crop=True), the loop and
the CLI keys on top of them), driven through the host SIMT emulator (tests/hipemu).  The checks live in tests/crop_util.py and run on the GPU too
(tests/test_crop_gpu.py).  Every comparison is bit for bit (fp32) or byte for byte (u8): the output is the engine's own definition -- the existing
u8 step on the cropped arrays, pasted by slicing -- and the reference has none like it."""
import os

import numpy as np
import pytest

from lama_amd import _lib as L
from lama_amd import predict as P
from tests import crop_util as U
from tests.emu import emu_lib


# ---- the restatement's own arithmetic -------------------------------------------------------------------------------------------------------
def test_fma32_rounds_once():
    """Against exact rational arithmetic: operands whose product needs all 48 bits and whose sum lies close to a float32 tie."""
    from fractions import Fraction
    rs = np.random.RandomState(0)
    a = rs.rand(4000).astype(np.float32)
    b = (rs.rand(4000) * 1.2 - 0.1).astype(np.float32)
    c = rs.rand(4000).astype(np.float32)
    a[:8], b[:8], c[:8] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24) * np.arange(8, dtype=np.float32)
    got = U.fma32(a, b, c)
    for x, y, z, g in zip(a[:600], b[:600], c[:600], got[:600]):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        assert abs(Fraction(float(g)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    assert np.array_equal(U.fma32(np.float32(1), b, np.float32(0) * c), b) and np.array_equal(U.fma32(np.float32(0), b, c), c)


def test_quantising_a_source_byte_over_255_gives_the_byte_back():
    """The byte copy where the mask is 0 is the blend formula, not an exception to it."""
    k = np.arange(256, dtype=np.uint8)
    img = np.stack([k, k, k], -1)[None]
    for binarize in (True, False):
        assert np.array_equal(U.crop_paste_ref(img, np.zeros((1, 256), np.uint8), (0, 0, 1, 256), np.full((3, 1, 256), np.nan, np.float32), binarize), img)


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', U.LAYOUTS)
@pytest.mark.parametrize('binarize', [True, False], ids=['binarize', 'fractional'])
@pytest.mark.parametrize('name', list(U.CASES))
def test_kernels_are_the_u8_step_on_the_crop_bit_for_bit(name, binarize, layout):
    U.check_case(emu_lib(), 'cpu', name, binarize, layout)


def test_misaligned_slots_take_the_byte_path():
    U.check_misaligned_slots(emu_lib(), 'cpu')


@pytest.mark.parametrize('layout', U.LAYOUTS)
def test_rects_that_do_not_fit_behave_as_empty_slots(layout):
    U.check_rects_that_do_not_fit(emu_lib(), 'cpu', layout)


def test_non_finite_samples_quantise_as_the_blend_does():
    U.check_non_finite(emu_lib(), 'cpu')


def test_refusals_return_their_code_and_launch_nothing():
    U.check_refusals(emu_lib(), 'cpu')


# ---- crop_rect ------------------------------------------------------------------------------------------------------------------------------
def _box(h, w, y, x, bh, bw):
    m = np.zeros((h, w), np.uint8)
    m[y:y + bh, x:x + bw] = 255
    return m


def test_crop_rect_known_answers():
    # a box at the top-left corner: the window is clamped to the corner
    assert P.crop_rect(_box(100, 120, 0, 0, 10, 12), 8, 16, 8) == (0, 0, 32, 32, 32, 32)
    # ... and at the bottom-right corner
    assert P.crop_rect(_box(100, 120, 90, 108, 10, 12), 8, 16, 8) == (68, 88, 32, 32, 32, 32)
    # centred: a 10 x 12 box at (40, 50) wants 26 x 28 -> 32 x 32, (32 - 10) // 2 = 11 above and (32 - 12) // 2 = 10 to the left
    assert P.crop_rect(_box(100, 120, 40, 50, 10, 12), 8, 16, 8) == (29, 40, 32, 32, 32, 32)
    # a box larger than the image minus the margins: the window spans both axes and is padded as the whole image is
    assert P.crop_rect(_box(100, 120, 5, 5, 90, 110), 8, 16, 8) == (0, 0, 100, 120, 104, 120)
    # it spans one axis only
    assert P.crop_rect(_box(100, 120, 5, 50, 90, 12), 8, 16, 8) == (0, 40, 100, 32, 104, 32)
    # an empty mask: the empty box at the origin
    assert P.crop_rect(np.zeros((100, 120), np.uint8), 8, 16, 8) == (0, 0, 16, 16, 16, 16)
    assert P.crop_rect(np.zeros((100, 120), np.uint8), 0, 16, 8) == (0, 0, 16, 16, 16, 16)
    # an image smaller than the step
    assert P.crop_rect(_box(13, 11, 4, 4, 2, 2), 8, 128, 8) == (0, 0, 13, 11, 16, 16)
    # any non-zero byte is hole, whatever binarize will say
    m = np.zeros((64, 64), np.uint8)
    m[3, 60] = 1
    assert P.crop_rect(m, 4, 16, 8) == (0, 48, 16, 16, 16, 16)
    # without padding (pad_mod 1) a spanning window keeps the image's size
    assert P.crop_rect(_box(13, 11, 4, 4, 2, 2), 8, 128, 1) == (0, 0, 13, 11, 13, 11)


def test_crop_rect_refuses_bad_options():
    m = _box(32, 32, 4, 4, 2, 2)
    for margin, step, pad_mod in ((4, 0, 8), (4, -16, 8), (4, 12, 8), (-1, 16, 8)):
        with pytest.raises(L.LamaError):
            P.crop_rect(m, margin, step, pad_mod)
    with pytest.raises(L.LamaError):
        P.crop_rect(np.zeros((0, 4), np.uint8), 4, 16, 8)


def test_crop_rect_sweep_of_random_masks():
    rs = np.random.RandomState(7)
    for _ in range(200):
        h, w = rs.randint(1, 90, 2)
        pad_mod = int(rs.choice([1, 2, 8]))
        step = pad_mod * int(rs.randint(1, 6))
        mask = np.zeros((h, w), np.uint8)
        for _ in range(rs.randint(0, 4)):                     # up to three blobs of any non-zero value
            y, x = rs.randint(0, h), rs.randint(0, w)
            mask[y:y + rs.randint(1, 20), x:x + rs.randint(1, 20)] = rs.randint(1, 256)
        U.check_rect_properties(mask, int(rs.randint(0, 12)), step, pad_mod)


# ---- the step and the loop ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    """The three PNG pairs and, computed once, the definition of their results: the existing u8 step on the host-cropped pairs, pasted by numpy
    (batches of three for the step test, of two for the loop test)."""
    from tests.test_dist_gloo import _build_model
    indir = str(tmp_path_factory.mktemp('crop') / 'in') + os.sep
    items = U.write_pairs(indir)
    model = _build_model()[0]
    rects = U.item_rects(items)
    return dict(model=model, indir=indir, items=items, rects=rects, want3=U.cropped_want(model, items, rects, 3, 'cpu', 'replay'),
                want2=U.cropped_want(model, items, rects, 2, 'cpu', 'replay'))


def test_host_fed_step_is_the_u8_step_on_the_crop_pasted_by_slicing(pairs):
    U.check_step(pairs['model'], pairs['items'], pairs['rects'], 'cpu', 'replay', pairs['want3'], 3)


def test_host_fed_step_with_encode_png_decodes_to_the_same_pixels(pairs):
    U.check_step(pairs['model'], pairs['items'], pairs['rects'], 'cpu', 'replay', pairs['want3'], 3, encode_png=True)


def test_host_fed_step_refusals(pairs):
    model = pairs['model']
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, 16, 16, 'cpu', crop=True)                                                     # no source slot size
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, 16, 16, 'cpu', crop=True, src_hw=(40, 56), scale_factor=0.5)
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, 16, 16, 'cpu', crop=True, src_hw=(40, 56), out_key='predicted_image')
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, 16, 16, 'cpu', crop=True, src_hw=(40, 56), u8_input=False)
    assert not P.HostFedStep(model, 2, 16, 16, 'cpu').crop                                                    # the default
    hs = P.HostFedStep(model, 2, 16, 16, 'cpu', crop=True, src_hw=(40, 56))
    image, mask = np.zeros((40, 56, 3), np.uint8), np.zeros((40, 56), np.uint8)
    hs.put(0, 0, image, mask, (6, 16, 16, 16))
    assert hs.h_rects[0].numpy()[0].tolist() == [6, 16, 16, 16] and hs.h_sizes[0].numpy()[0].tolist() == [40, 56]
    hs.put(0, 1, None, None)
    assert hs.h_rects[0].numpy()[1].tolist() == [0, 0, 0, 0] and hs.h_sizes[0].numpy()[1].tolist() == [0, 0]
    for rect in (None, (6, 16, 17, 16), (6, 16, 16, 17), (-1, 16, 16, 16), (6, -1, 16, 16), (25, 16, 16, 16), (6, 41, 16, 16), (6, 16, 0, 16),
                 (6, 16, 16, 0)):
        with pytest.raises(L.LamaError):
            hs.put(0, 0, image, mask, rect)
    with pytest.raises(L.LamaError):
        hs.put(0, 0, np.zeros((41, 56, 3), np.uint8), np.zeros((41, 56), np.uint8), (6, 16, 16, 16))          # larger than the source slot
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, 16, 16, 'cpu').put(0, 0, image[:16, :16], mask[:16, :16], (0, 0, 16, 16))     # a window without the crop form


def test_predict_loop_writes_source_size_pngs(pairs, tmp_path):
    """predict(crop_to_mask=True), batches of two (the 16 x 16 bucket: one full round; the 16 x 32 bucket: a partial one): source-size PNGs equal to
    the definition, and the pre-pass is on the loop's clock."""
    out = str(tmp_path / 'out')
    P.LOOP_TIMES.pop('crop_prepass', None)
    n = P.predict(pairs['model'], pairs['items'], pairs['indir'], out, pad_mod=U.PAD_MOD, batch_size=2, device='cpu', io_threads=2,
                  crop_to_mask=True, crop_margin=U.MARGIN, crop_step=U.STEP)
    assert n == 3 and P.LOOP_TIMES['crop_prepass'] > 0
    U.check_written_pngs(out, pairs['indir'], pairs['items'], pairs['want2'])


def test_predict_loop_with_device_png_writes_the_same_pixels(pairs, tmp_path):
    out = str(tmp_path / 'out')
    assert P.predict(pairs['model'], pairs['items'], pairs['indir'], out, pad_mod=U.PAD_MOD, batch_size=2, device='cpu', io_threads=2,
                     crop_to_mask=True, crop_margin=U.MARGIN, crop_step=U.STEP, device_png=True) == 3
    U.check_written_pngs(out, pairs['indir'], pairs['items'], pairs['want2'])


def test_predict_loop_with_the_option_off_writes_todays_bytes(pairs, tmp_path):
    """crop_to_mask=False (the default), spelled out or left out: the files of the loop as it is -- the plain u8 step on the whole images."""
    from PIL import Image
    model = pairs['model']
    indir = str(tmp_path / 'in') + os.sep                     # (whole images through the emulated generator: two small ones of one bucket)
    os.makedirs(indir)
    for i, (h, w) in enumerate(((16, 16), (14, 15))):
        mask = np.zeros((h, w), np.uint8)
        mask[4:9, 5:11] = 255
        Image.fromarray(U._image(h, w, 20 + i)).save(os.path.join(indir, f'im{i}.png'))
        Image.fromarray(mask).save(os.path.join(indir, f'im{i}_mask.png'))
    items = P.list_dataset(indir, '.png')
    out_default, out_off = str(tmp_path / 'default'), str(tmp_path / 'off')
    assert P.predict(model, items, indir, out_default, pad_mod=U.PAD_MOD, batch_size=2, device='cpu', io_threads=2) == 2
    assert P.predict(model, items, indir, out_off, pad_mod=U.PAD_MOD, batch_size=2, device='cpu', io_threads=2, crop_to_mask=False,
                     crop_margin=U.MARGIN, crop_step=U.STEP) == 2
    # ... which are the whole-image u8 step's: both images in the one batch of their 16 x 16 bucket
    u8 = [P.load_item_u8(*it) for it in items]
    hs = P.HostFedStep(model, 2, 16, 16, 'cpu', drain=True, mode='replay')
    U.run_step(hs, [(u8[0][0], u8[0][1]), (u8[1][0], u8[1][1])])
    for i, (mask_path, _) in enumerate(items):
        rel = os.path.splitext(mask_path[len(indir):])[0] + '.png'
        with open(os.path.join(out_default, rel), 'rb') as a, open(os.path.join(out_off, rel), 'rb') as b:
            assert a.read() == b.read(), rel
        h, w = u8[i][2]
        assert np.array_equal(np.array(Image.open(os.path.join(out_off, rel))), hs.result(0)[i, :h, :w]), rel


def test_predict_refuses_the_combinations_the_step_does_not_serve(pairs):
    model, items, indir = pairs['model'], pairs['items'], pairs['indir']
    for kw in (dict(scale_factor=0.5), dict(out_key='predicted_image'), dict(crop_step=12), dict(crop_step=0), dict(crop_margin=-1)):
        with pytest.raises(L.LamaError):
            P.predict(model, items, indir, os.devnull, pad_mod=8, device='cpu', crop_to_mask=True, **kw)       # before anything is opened


def test_cli_keys_and_their_four_refusals(monkeypatch):
    base = ['model.path=/m', 'indir=i', 'outdir=o']
    cfg = P.parse_overrides(base)
    assert cfg['crop_to_mask'] is False and cfg['crop_margin'] == 128 and cfg['crop_step'] == 128
    assert P.DEFAULTS['crop_to_mask'] is False and P.DEFAULTS['crop_margin'] == 128 and P.DEFAULTS['crop_step'] == 128
    assert 'crop_to_mask' in P.BOOL_KEYS and {'crop_margin', 'crop_step'} <= P.INT_KEYS and {'crop_to_mask', 'crop_margin', 'crop_step'} <= P.KNOWN_KEYS
    cfg = P.parse_overrides(base + ['crop_to_mask=true', 'crop_margin=32', 'crop_step=64'])
    assert cfg['crop_to_mask'] is True and cfg['crop_margin'] == 32 and cfg['crop_step'] == 64
    assert P.parse_overrides(base + ['crop_to_mask=false'])['crop_to_mask'] is False
    # it composes with the device encoders
    assert P.parse_overrides(base + ['crop_to_mask=true', 'device_png=true'])['device_png'] is True
    assert P.parse_overrides(base + ['crop_to_mask=true', 'device_jpeg=true', 'out_ext=.jpg'])['device_jpeg'] is True
    assert P.parse_overrides(base + ['crop_to_mask=true', 'crop_step=24', 'dataset.pad_out_to_modulo=12'])['crop_step'] == 24

    def no_launch(*a, **k):
        raise AssertionError('the refusal came after the model was loaded')
    monkeypatch.setattr(P.trainers, 'load_checkpoint', no_launch)
    for extra, word in ((['crop_to_mask=true', 'dataset.scale_factor=0.5'], 'dataset.scale_factor'),
                        (['crop_to_mask=true', 'refine=true'], 'refine'),
                        (['crop_to_mask=true', 'out_key=predicted_image'], 'predicted_image'),
                        (['crop_to_mask=true', 'crop_step=100'], 'crop_step'),
                        (['crop_to_mask=true', 'crop_step=0'], 'crop_step'),
                        (['crop_to_mask=true', 'crop_step=-128'], 'crop_step'),
                        (['crop_to_mask=true', 'crop_step=16', 'dataset.pad_out_to_modulo=32'], 'crop_step')):
        with pytest.raises(SystemExit) as e:
            P.main(base + extra)
        assert 'crop_to_mask' in str(e.value) and word in str(e.value), extra
    for extra in (['crop_to_mask=maybe'], ['crop_step=a'], ['crop_margin=1.5']):
        with pytest.raises(SystemExit):
            P.parse_overrides(base + extra)
