"""``dataset.scale_factor`` on the device (lama_resize_u8_fwd, csrc/elementwise.hip), driven through the host SIMT emulator (tests/hipemu).

The kernel is held to lama_amd.predict's host restatement of cv2.resize (``scale_image`` -- tests/test_scale_factor.py holds that one to its
known answers) followed by ``pad_img_to_modulo`` and ``mask > 0``.  Every bar is bit-equality: the kernel performs the same IEEE operations in
the same order, so nothing else is acceptable."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from lama_amd import _lib as L
from lama_amd import predict as P
from tests import scale_device_util as U
from tests.emu import emu_lib


@pytest.mark.parametrize('case', U.REGIME_CASES, ids=U.case_id)
def test_regime_table_is_bit_equal_to_the_host_chain(case):
    factor, (h, w) = case
    pair = U.random_pair(h, w, seed=h * 100 + w)
    Hp, Wp = U.padded_scaled(h, w, factor)
    want_i, want_m = U.host_chain(*pair, factor)
    got_i, got_m = U.device_resize(emu_lib(), [pair], factor, h, w, Hp, Wp)
    assert got_i.shape == (1,) + want_i.shape and got_m.shape == (1,) + want_m.shape
    assert np.array_equal(got_i[0], want_i)
    assert np.array_equal(got_m[0], want_m)


def test_padding_larger_than_the_scaled_side():
    """5 x 7 at 0.5 scales to 2 x 4 and is padded to 8 x 8: np.pad(mode='symmetric') is periodic, a single reflection is not enough."""
    pair = U.random_pair(5, 7, seed=9)
    assert P.scaled_size(5, 7, 0.5) == (2, 4) and U.padded_scaled(5, 7, 0.5) == (8, 8)
    want_i, want_m = U.host_chain(*pair, 0.5)
    got_i, got_m = U.device_resize(emu_lib(), [pair], 0.5, 5, 7, 8, 8)
    assert np.array_equal(got_i[0], want_i) and np.array_equal(got_m[0], want_m)
    assert np.array_equal(want_i[:, 4:6, :4], want_i[:, 0:2, :4])          # the reference really wraps: rows 4, 5 repeat rows 0, 1


@pytest.mark.parametrize('factor', [0.75, 0.5, 1.25])
def test_batch_of_different_source_sizes_and_an_empty_slot(factor):
    """Two images of different source size whose scaled sizes share one padded shape, and an empty slot between them, in source slots larger
    than both: every image is resized from its own (h, w), the empty slot yields zeros, nothing outside an image is read."""
    a, b = {0.75: ((37, 50), (40, 51)), 0.5: ((61, 75), (59, 78)), 1.25: ((23, 29), (20, 31))}[factor]
    Hp, Wp = U.padded_scaled(*a, factor)
    assert U.padded_scaled(*b, factor) == (Hp, Wp) and P.scaled_size(*a, factor) != P.scaled_size(*b, factor)
    pa, pb = U.random_pair(*a, seed=1), U.random_pair(*b, seed=2)
    Hs, Ws = max(a[0], b[0]) + 5, max(a[1], b[1]) + 3
    got_i, got_m = U.device_resize(emu_lib(), [pa, None, pb], factor, Hs, Ws, Hp, Wp)
    for j, pr in ((0, pa), (2, pb)):
        want_i, want_m = U.host_chain(*pr, factor)
        assert np.array_equal(got_i[j], want_i) and np.array_equal(got_m[j], want_m), j
    assert not got_i[1].any() and not got_m[1].any()


@pytest.mark.parametrize('case', [(0.75, (37, 50)), (0.5, (9, 11)), (1.5, (9, 11))], ids=U.case_id)
def test_mask_without_binarisation_stays_mask_over_255(case):
    factor, (h, w) = case
    pair = U.random_pair(h, w, seed=4)
    Hp, Wp = U.padded_scaled(h, w, factor)
    want_i, want_m = U.host_chain(*pair, factor, binarize=False)
    assert set(np.unique(want_m)) == {np.float32(0), np.float32(100) / np.float32(255), np.float32(200) / np.float32(255)}
    got_i, got_m = U.device_resize(emu_lib(), [pair], factor, h, w, Hp, Wp, binarize=False)
    assert np.array_equal(got_i[0], want_i) and np.array_equal(got_m[0], want_m)


def test_bad_arguments():
    lib = emu_lib()
    img, msk = torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    ssz = torch.tensor([[8, 8]], dtype=torch.int32)
    dsz = torch.tensor([[4, 4]], dtype=torch.int32)
    oi, om = torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 8, 8)

    def code(fn):
        with pytest.raises(L.LamaError) as e:
            fn()
        return e.value.code

    for factor in (0.0, -0.5, float('nan')):
        assert code(lambda: lib.resize_u8(img, msk, ssz, dsz, factor, L.view(oi), L.view(om), 1)) == -1         # LAMA_ERR_BAD_ARG
    vi, vm = L.view(oi), L.view(om)
    raw = lib._l.lama_resize_u8_fwd
    ptr = [img.data_ptr(), msk.data_ptr(), ssz.data_ptr(), dsz.data_ptr()]
    for k in range(4):                                                        # each null pointer
        a = list(ptr)
        a[k] = None
        assert raw(0, *a, 8, 8, 0.5, C.byref(vi), C.byref(vm), 1, 1) == -1
    assert raw(0, *ptr, 8, 8, 0.5, None, C.byref(vm), 1, 1) == -1
    assert raw(0, *ptr, 8, 8, 0.5, C.byref(vi), None, 1, 1) == -1
    assert raw(0, *ptr, 0, 8, 0.5, C.byref(vi), C.byref(vm), 1, 1) == -1        # no source slot
    assert raw(0, *ptr, 8, 8, 0.5, C.byref(vi), C.byref(vm), 0, 1) == -1        # no batch
    small = torch.zeros(1, 1, 8, 4)
    assert code(lambda: lib.resize_u8(img, msk, ssz, dsz, 0.5, vi, L.view(small), 1)) == -1          # mask view of another size
    assert code(lambda: lib.resize_u8(img, msk, ssz, dsz, 0.5, L.view(torch.zeros(1, 4, 8, 8)), vm, 1)) == -1   # not a 3-channel image view
    half = torch.zeros(1, 3, 8, 8, dtype=torch.float16)
    assert code(lambda: lib.resize_u8(img, msk, ssz, dsz, 0.5, L.view(half), vm, 1)) == -2            # LAMA_ERR_UNSUPPORTED: fp32 outputs only
    assert raw(0, *ptr, 8, 8, 0.5, C.byref(vi), C.byref(vm), 1, 1) == 0


def test_sizes_that_do_not_fit_yield_zeros_not_out_of_bounds_reads():
    """The per-image sizes are device data, so the entry cannot refuse them: a destination size beyond the output view, or a source size beyond
    the slot, is written as zeros like an empty slot."""
    lib = emu_lib()
    img, msk = torch.full((2, 8, 8, 3), 200, dtype=torch.uint8), torch.full((2, 8, 8), 255, dtype=torch.uint8)
    ssz = torch.tensor([[8, 8], [9, 8]], dtype=torch.int32)                  # image 1: taller than its slot
    dsz = torch.tensor([[16, 16], [4, 4]], dtype=torch.int32)                # image 0: larger than the 8 x 8 view
    oi, om = torch.full((2, 3, 8, 8), float('nan')), torch.full((2, 1, 8, 8), float('nan'))
    lib.resize_u8(img, msk, ssz, dsz, 0.5, L.view(oi), L.view(om), 2)
    assert not oi.numpy().any() and not om.numpy().any()


# ---- the step and the loop ----------------------------------------------------------------------------------------------------------------------

def _model():
    from tests.test_dist_gloo import _build_model
    return _build_model()[0]


def _write_pairs(root, shapes, seed=3):
    from PIL import Image
    paths = []
    for i, (h, w) in enumerate(shapes):
        image, mask = U.random_pair(h, w, seed + i)
        mask = np.where(mask > 100, 255, 0).astype('uint8')
        mask[1, 2] = 1                                                       # any non-zero pixel is "hole"
        Image.fromarray(image).save(os.path.join(root, f'im{i}.png'))
        Image.fromarray(mask).save(os.path.join(root, f'im{i}_mask.png'))
        paths.append((os.path.join(root, f'im{i}_mask.png'), os.path.join(root, f'im{i}.png')))
    return paths


def _one_step(hs, put):
    put(0)
    hs.prime(0)
    hs.launch(0)
    hs.wait(0)
    hs.flush(0)
    return hs.result(0).copy()


FACTOR, SHAPES = 0.75, [(21, 30), (20, 31)]      # scaled 16 x 22 and 15 x 23: one 16 x 24 bucket whose source slot (21, 31) is neither image's size


@pytest.fixture(scope='module')
def scaled_pair(tmp_path_factory):
    """Two PNG pairs and, computed once, the u8 results of HostFedStep(u8_input=False) fed with ``load_item``'s host-scaled, padded fp32 tensors."""
    indir = str(tmp_path_factory.mktemp('scaled') / 'in') + os.sep
    os.makedirs(indir)
    _write_pairs(indir, SHAPES)
    items = P.list_dataset(indir, '.png')
    model = _model()
    Hp, Wp = U.padded_scaled(*SHAPES[0], FACTOR)
    assert (Hp, Wp) == (16, 24) == U.padded_scaled(*SHAPES[1], FACTOR)
    host = [P.load_item(m, i, 8, FACTOR) for m, i in items]
    assert [it[2] for it in host] == [(16, 22), (15, 23)] and all(it[0].shape == (3, Hp, Wp) for it in host)
    ref = P.HostFedStep(model, 2, Hp, Wp, 'cpu', drain=True, u8_input=False)
    want = _one_step(ref, lambda p: [ref.put(p, j, host[j][0], host[j][1]) for j in range(2)])
    assert want.any()
    return dict(model=model, indir=indir, items=items, want=want, sizes=[it[2] for it in host], shape=(Hp, Wp))


def test_host_fed_step_with_scale_factor_equals_the_fp32_form(scaled_pair):
    """HostFedStep(scale_factor=0.75) fed with two decoded u8 originals of different size against HostFedStep(u8_input=False) fed with
    ``load_item``'s host-scaled, padded fp32 tensors of the same two images: the same u8 results, bitwise."""
    model, (Hp, Wp) = scaled_pair['model'], scaled_pair['shape']
    hs = P.HostFedStep(model, 2, Hp, Wp, 'cpu', drain=True, scale_factor=FACTOR, src_hw=(21, 31))
    assert not hs.u8_input and hs.h_img[0].shape == (2, 21, 31, 3) and hs.h_img[0].dtype == torch.uint8
    u8 = [P.load_item_u8(m, i) for m, i in scaled_pair['items']]
    got = _one_step(hs, lambda p: [hs.put(p, j, u8[j][0], u8[j][1]) for j in range(2)])
    assert np.array_equal(got, scaled_pair['want'])
    with pytest.raises(L.LamaError):
        hs.put(0, 0, np.zeros((22, 31, 3), np.uint8), np.zeros((22, 31), np.uint8))       # does not fit the source slot
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, Hp, Wp, 'cpu', scale_factor=FACTOR)                      # no source slot size


def test_predict_loop_with_scale_factor_writes_the_host_scaled_bytes(scaled_pair, tmp_path, monkeypatch):
    """``predict(..., scale_factor=0.75)`` -- u8 decode, buckets by the padded scaled size, source slots of the bucket's largest image, the rescale
    on the device, crops to the scaled size -- writes the PNG bytes of a loop whose step is fed ``load_item``'s host-scaled fp32 tensors, and
    never calls the host rescale."""
    indir, items = scaled_pair['indir'], scaled_pair['items']

    def no_host_rescale(*a, **k):
        raise AssertionError('scale_image called on the predict path')
    monkeypatch.setattr(P, 'scale_image', no_host_rescale)
    out = str(tmp_path / 'out')
    assert P.predict(scaled_pair['model'], items, indir, out, pad_mod=8, batch_size=2, device='cpu', io_threads=2, scale_factor=FACTOR) == len(items)
    for j, (mask_path, _) in enumerate(items):
        h, w = scaled_pair['sizes'][j]
        rel = os.path.splitext(mask_path[len(indir):])[0] + '.png'
        with open(os.path.join(out, rel), 'rb') as f:
            assert f.read() == P.encode_png(scaled_pair['want'][j, :h, :w]), rel
