"""``crop_max_side`` (lama_crop_shrink_compose_u8_fwd / lama_crop_shrink_paste_u8_fwd, csrc/elementwise.hip; ``crop_rect_limited``,
HostFedStep(crop=True, crop_shrink=True), the loop and the CLI key on top of them), driven through the host SIMT emulator (tests/hipemu).  The
checks live in tests/crop_shrink_util.py and run on the GPU too (tests/test_crop_shrink_gpu.py).  Every comparison is bit for bit (fp32) or byte
for byte (u8): the output is the engine's own definition and the reference has none like it."""
import os

import numpy as np
import pytest

from lama_amd import _lib as L
from lama_amd import predict as P
from tests import crop_shrink_util as U
from tests.emu import emu_lib


# ---- the restatement's own arithmetic -------------------------------------------------------------------------------------------------------
def test_the_restatement_is_the_hosts_integer_shrink_where_k_divides_the_window():
    """``shrink_ref`` against ``predict._resize_area(C / 255, 1.0 / k)`` for k = 1 .. 16, bit for bit, and 1.0 / (1.0 / k) == k in fp64."""
    for k in range(1, 17):
        assert 1.0 / (1.0 / k) == k
        c = U.CU._image(3 * k, 2 * k, k)
        S, mu = U.shrink_ref(c, np.zeros(c.shape[:2], np.uint8), k)
        assert U._same_bits(S, P._resize_area(c.astype(np.float32) / np.float32(255), 1.0 / k)) and not mu.any()


def test_the_mask_of_a_box_is_its_max_cut_boxes_included():
    m = np.zeros((5, 7), np.uint8)
    m[4, 6], m[0, 1], m[2, 2] = 3, 200, 9
    _, mu = U.shrink_ref(np.zeros((5, 7, 3), np.uint8), m, 2)
    assert mu.tolist() == [[200, 0, 0, 0], [0, 9, 0, 0], [0, 0, 0, 3]]


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', U.LAYOUTS)
@pytest.mark.parametrize('binarize', [True, False], ids=['binarize', 'fractional'])
@pytest.mark.parametrize('name', list(U.CASES))
def test_kernels_are_the_definition_bit_for_bit(name, binarize, layout):
    U.check_case(emu_lib(), 'cpu', name, binarize, layout)


def test_k1_is_the_crop_entries():
    U.check_k1_is_the_crop(emu_lib(), 'cpu')


def test_one_pixel_strokes_stay_holes_and_are_replaced():
    U.check_one_pixel_strokes(emu_lib(), 'cpu')


def test_misaligned_slots_take_the_byte_path():
    U.check_misaligned_slots(emu_lib(), 'cpu')


@pytest.mark.parametrize('layout', U.LAYOUTS)
def test_rects_that_do_not_fit_behave_as_empty_slots(layout):
    U.check_rects_that_do_not_fit(emu_lib(), 'cpu', layout)


def test_non_finite_samples_quantise_as_the_paste_back_does():
    U.check_non_finite(emu_lib(), 'cpu')


def test_refusals_return_their_code_and_launch_nothing():
    U.check_refusals(emu_lib(), 'cpu')


# ---- crop_rect_limited ----------------------------------------------------------------------------------------------------------------------
def _box(h, w, y, x, bh, bw):
    m = np.zeros((h, w), np.uint8)
    m[y:y + bh, x:x + bw] = 255
    return m


def test_crop_rect_limited_known_answers():
    """margin = step = 128, pad_mod 8, crop_max_side 512."""
    got = P.crop_rect_limited(_box(2048, 2048, 900, 800, 200, 300), 128, 128, 8, 512)
    assert got[2:] == (768, 1024, 2, 384, 512, 384, 512)                                   # 300 x 200 box: k = 2, window 1024 x 768
    assert P.crop_rect_limited(_box(2048, 2048, 600, 500, 700, 900), 128, 128, 8, 512) == (0, 0, 2048, 2048, 4, 512, 512, 512, 512)
    assert P.crop_rect_limited(_box(3000, 4000, 0, 1000, 3000, 1500), 128, 128, 8, 512)[2:] == (3000, 3072, 6, 500, 512, 504, 512)
    assert P.crop_rect_limited(np.full((8192, 8192), 255, np.uint8), 128, 128, 8, 512) == (0, 0, 8192, 8192, 16, 512, 512, 512, 512)
    with pytest.raises(L.LamaError) as e:
        P.crop_rect_limited(np.full((9000, 9000), 255, np.uint8), 128, 128, 8, 512)
    assert '9000' in str(e.value) and 'crop_max_side=512' in str(e.value)
    small = _box(2048, 2048, 900, 800, 100, 100)                                           # k = 1: crop_rect's own window
    assert P.crop_rect_limited(small, 128, 128, 8, 512) == (758, 658, 384, 384, 1, 384, 384, 384, 384)
    assert P.crop_rect(small, 128, 128, 8) == (758, 658, 384, 384, 384, 384)
    with pytest.raises(L.LamaError):
        P.crop_rect_limited(small, 128, 128, 8, 512, kmax=17)


def test_crop_rect_limited_sweep_of_random_masks():
    rs = np.random.RandomState(11)
    served = refused = shrunk = 0
    for _ in range(300):
        h, w = rs.randint(1, 400, 2)
        pad_mod = int(rs.choice([1, 2, 8]))
        step = pad_mod * int(rs.randint(1, 4))
        margin = int(rs.randint(0, 6))
        least = (2 * margin + step + step - 1) // step * step
        max_side = -(-(least + int(rs.randint(0, 24))) // pad_mod) * pad_mod
        mask = np.zeros((h, w), np.uint8)
        for _ in range(rs.randint(0, 4)):
            y, x = rs.randint(0, h), rs.randint(0, w)
            mask[y:y + rs.randint(1, 200), x:x + rs.randint(1, 200)] = rs.randint(1, 256)
        got = U.check_limited_properties(mask, margin, step, pad_mod, max_side)
        served, refused, shrunk = served + (got is not None), refused + (got is None), shrunk + (got is not None and got[4] > 1)
    assert served > 100 and refused > 5 and shrunk > 50, (served, refused, shrunk)


def test_crop_max_side_option_checks():
    for max_side, margin, step, pad_mod in ((0, 128, 128, 8), (384, 128, 128, 8), (512, 128, 128, 8), (32, 4, 16, 8), (33, 4, 16, 1)):
        P.check_crop_max_side(max_side, margin, step, pad_mod)
    for max_side, margin, step, pad_mod in ((-8, 4, 16, 8), (36, 4, 16, 8), (24, 4, 16, 8), (256, 128, 128, 8), (376, 128, 128, 8), (16, 4, 16, 8)):
        with pytest.raises(L.LamaError):
            P.check_crop_max_side(max_side, margin, step, pad_mod)
    P.check_crop_options(4, 16, 8)                                                          # (its callers keep their behaviour: no new argument)
    with pytest.raises(L.LamaError):
        P.crop_rect_limited(_box(64, 64, 4, 4, 8, 8), 4, 16, 8, 0)                          # no limit is no window rule


def test_cli_key_and_its_refusals(monkeypatch):
    base = ['model.path=/m', 'indir=i', 'outdir=o']
    assert P.parse_overrides(base)['crop_max_side'] == 0 and P.DEFAULTS['crop_max_side'] == 0
    assert 'crop_max_side' in P.INT_KEYS and 'crop_max_side' in P.KNOWN_KEYS
    cfg = P.parse_overrides(base + ['crop_to_mask=true', 'crop_max_side=512'])
    assert cfg['crop_max_side'] == 512 and cfg['crop_margin'] == 128
    assert P.parse_overrides(base + ['crop_to_mask=true', 'crop_max_side=0'])['crop_max_side'] == 0
    assert P.parse_overrides(base + ['crop_to_mask=true', 'crop_max_side=512', 'device_png=true'])['device_png'] is True

    def no_launch(*a, **k):
        raise AssertionError('the refusal came after the model was loaded')
    monkeypatch.setattr(P.trainers, 'load_checkpoint', no_launch)
    for extra, word in ((['crop_max_side=512'], 'crop_to_mask'),
                        (['crop_to_mask=false', 'crop_max_side=512'], 'crop_to_mask'),
                        (['crop_to_mask=true', 'crop_max_side=500'], 'crop_max_side'),
                        (['crop_to_mask=true', 'crop_max_side=256'], 'crop_max_side'),
                        (['crop_to_mask=true', 'crop_max_side=-512'], 'crop_max_side'),
                        (['crop_to_mask=true', 'crop_max_side=512', 'dataset.scale_factor=0.5'], 'dataset.scale_factor'),
                        (['crop_to_mask=true', 'crop_max_side=512', 'refine=true'], 'refine')):
        with pytest.raises(SystemExit) as e:
            P.main(base + extra)
        assert word in str(e.value), extra
    with pytest.raises(SystemExit):
        P.parse_overrides(base + ['crop_max_side=1.5'])


# ---- the step and the loop ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    """The three PNG pairs (k = 1, 2, 3) and, computed once, the definition of their results in batches of two (the shrunk 32 x 32 bucket holds
    the k = 2 and the k = 3 window in one batch)."""
    from tests.test_dist_gloo import _build_model
    indir = str(tmp_path_factory.mktemp('crop_shrink') / 'in') + os.sep
    items = U.write_pairs(indir)
    model = _build_model()[0]
    wins = U.item_windows(items)
    return dict(model=model, indir=indir, items=items, wins=wins, want=U.definition_want(model, items, wins, 'cpu', 2))


def test_host_fed_step_is_the_definition(pairs):
    U.check_step(pairs['model'], pairs['items'], pairs['wins'], 'cpu', 'replay', pairs['want'], 2)


def test_host_fed_step_with_encode_png_decodes_to_the_same_pixels(pairs):
    U.check_step(pairs['model'], pairs['items'], pairs['wins'], 'cpu', 'replay', pairs['want'], 2, encode_png=True)


def test_host_fed_step_refusals(pairs):
    model = pairs['model']
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, 16, 16, 'cpu', crop_shrink=True)                                              # not without the crop form
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, 16, 16, 'cpu', crop=True, crop_shrink=True)                                   # no source slot size
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, 16, 16, 'cpu', crop=True, crop_shrink=True, src_hw=(40, 56), scale_factor=0.5)
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, 16, 16, 'cpu', crop=True, crop_shrink=True, src_hw=(40, 56), out_key='predicted_image')
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, 16, 16, 'cpu', crop=True, crop_shrink=True, src_hw=(40, 56), u8_input=False)
    assert not P.HostFedStep(model, 2, 16, 16, 'cpu', crop=True, src_hw=(40, 56)).crop_shrink                 # the default
    hs = P.HostFedStep(model, 2, 16, 16, 'cpu', crop=True, crop_shrink=True, src_hw=(40, 56))
    image, mask = np.zeros((40, 56, 3), np.uint8), np.zeros((40, 56), np.uint8)
    hs.put(0, 0, image, mask, (6, 16, 32, 31, 2))
    assert hs.h_rects[0].numpy()[0].tolist() == [6, 16, 32, 31] and hs.h_shrinks[0].numpy()[0] == 2 and hs.h_sizes[0].numpy()[0].tolist() == [40, 56]
    hs.put(0, 1, None, None)
    assert hs.h_rects[0].numpy()[1].tolist() == [0, 0, 0, 0] and hs.h_shrinks[0].numpy()[1] == 0 and hs.h_sizes[0].numpy()[1].tolist() == [0, 0]
    for rect in (None, (6, 16, 32, 32), (6, 16, 33, 32, 2), (6, 16, 32, 33, 2), (6, 16, 32, 32, 0), (6, 16, 32, 32, 17), (6, 16, 32, 32, -1),
                 (-1, 16, 32, 32, 2), (6, -1, 32, 32, 2), (9, 16, 32, 32, 2), (6, 25, 32, 32, 2), (6, 16, 0, 32, 2), (6, 16, 32, 0, 2), (6, 16, 17, 16, 1)):
        with pytest.raises(L.LamaError):
            hs.put(0, 0, image, mask, rect)
    with pytest.raises(L.LamaError):
        hs.put(0, 0, np.zeros((41, 56, 3), np.uint8), np.zeros((41, 56), np.uint8), (6, 16, 32, 32, 2))      # larger than the source slot


def test_predict_loop_writes_the_definition_and_keeps_the_k1_file(pairs, tmp_path):
    """predict(crop_to_mask=True, crop_max_side=32), batches of two: the 16 x 32 bucket of the k = 1 window (the crop step as it is) and the
    shrunk 32 x 32 bucket.  Source-size PNGs equal to the definition, the source pixels where the mask is 0; the k = 1 item's file is
    byte-identical to a run without the key."""
    model, items, indir = pairs['model'], pairs['items'], pairs['indir']
    out, plain = str(tmp_path / 'out'), str(tmp_path / 'plain')
    kw = dict(pad_mod=U.PAD_MOD, batch_size=2, device='cpu', io_threads=2, crop_to_mask=True, crop_margin=U.MARGIN, crop_step=U.STEP)
    assert P.predict(model, items, indir, out, crop_max_side=U.MAX_SIDE, **kw) == 3
    U.check_written_pngs(out, indir, items, pairs['want'])
    assert P.predict(model, items[:1], indir, plain, **kw) == 1
    with open(os.path.join(out, 'im0_mask.png'), 'rb') as a, open(os.path.join(plain, 'im0_mask.png'), 'rb') as b:
        assert a.read() == b.read()


def test_predict_loop_with_device_png_writes_the_same_pixels(pairs, tmp_path):
    out = str(tmp_path / 'out')
    assert P.predict(pairs['model'], pairs['items'], pairs['indir'], out, pad_mod=U.PAD_MOD, batch_size=2, device='cpu', io_threads=2,
                     crop_to_mask=True, crop_margin=U.MARGIN, crop_step=U.STEP, crop_max_side=U.MAX_SIDE, device_png=True) == 3
    U.check_written_pngs(out, pairs['indir'], pairs['items'], pairs['want'])


def test_predict_loop_names_the_file_whose_window_cannot_fit(pairs, tmp_path):
    from PIL import Image
    indir = str(tmp_path / 'in') + os.sep
    os.makedirs(indir)
    Image.fromarray(U.CU._image(600, 40, 1)).save(os.path.join(indir, 'tall.png'))
    Image.fromarray(np.full((600, 40), 255, np.uint8)).save(os.path.join(indir, 'tall_mask.png'))
    items = P.list_dataset(indir, '.png')
    with pytest.raises(L.LamaError) as e:
        P.predict(pairs['model'], items, indir, str(tmp_path / 'out'), pad_mod=8, batch_size=2, device='cpu', io_threads=2, crop_to_mask=True,
                  crop_margin=4, crop_step=16, crop_max_side=32)
    assert 'tall_mask.png' in str(e.value) and 'crop_max_side' in str(e.value) and 'dataset.scale_factor' in str(e.value)
    for kw in (dict(crop_max_side=20), dict(crop_max_side=16), dict(crop_max_side=-32)):
        with pytest.raises(L.LamaError):
            P.predict(pairs['model'], items, indir, os.devnull, pad_mod=8, device='cpu', crop_to_mask=True, crop_margin=4, crop_step=16, **kw)
