"""``paste_back`` (lama_paste_back_u8_fwd, csrc/elementwise.hip; HostFedStep / the CLI on top of it), driven through the host SIMT emulator
(tests/hipemu).  The checks live in tests/paste_back_util.py and run on the GPU too (tests/test_paste_back_gpu.py).  Every comparison with the
numpy restatement ``paste_back_ref`` is byte for byte: this output is the engine's own definition, the reference writes the scaled image."""
import os

import numpy as np
import pytest

from lama_amd import _lib as L
from lama_amd import predict as P
from tests import paste_back_util as U
from tests.emu import emu_lib


@pytest.mark.parametrize('size,dsize', [((8, 8), (4, 4)), ((9, 7), (3, 2)), ((6, 8), (1, 1)), ((6, 8), (1, 4)), ((4, 4), (6, 6)),
                                        ((61, 75), (30, 38)), ((128, 96), (32, 24))])
def test_restatement_is_torch_bilinear_within_one_level(size, dsize):
    U.check_ref_against_torch(size, dsize)


def test_quantising_a_source_byte_over_255_gives_the_byte_back():
    """The byte copy where the mask is 0 is the blend formula, not an exception to it: (k / 255.f) * 255.f truncates to k."""
    k = np.arange(256, dtype=np.uint8)
    assert np.array_equal(U._quantize(k.astype(np.float32) / np.float32(255)), k)
    img = np.stack([k, k, k], -1)[None]
    for binarize in (True, False):
        assert np.array_equal(U.paste_back_ref(img, np.zeros((1, 256), np.uint8), np.full((3, 1, 1), np.nan, np.float32), (1, 1), binarize), img)


@pytest.mark.parametrize('layout', U.LAYOUTS)
@pytest.mark.parametrize('binarize', [True, False], ids=['binarize', 'fractional'])
@pytest.mark.parametrize('mask_kind', U.MASKS)
@pytest.mark.parametrize('name', list(U.CASES))
def test_kernel_is_the_restatement_byte_for_byte(name, mask_kind, binarize, layout):
    U.check_case(emu_lib(), 'cpu', name, mask_kind, binarize, layout)


def test_misaligned_slots_take_the_byte_path():
    U.check_misaligned_slots(emu_lib(), 'cpu')


def test_sizes_that_do_not_fit_yield_zero_slots():
    U.check_sizes_that_do_not_fit(emu_lib(), 'cpu')


def test_non_finite_samples_quantise_as_the_blend_does():
    U.check_non_finite(emu_lib(), 'cpu')


def test_refusals_return_their_code_and_launch_nothing():
    U.check_refusals(emu_lib(), 'cpu')


BUCKET, SRC_HW = U.geometry(U.SHAPES)


# ---- the step and the loop ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    """Three PNG pairs of different source sizes and, computed once, the restatement of their pasted results from the fp32 ``inpainted`` of the
    existing scale_factor step."""
    from tests.test_dist_gloo import _build_model
    indir = str(tmp_path_factory.mktemp('paste') / 'in') + os.sep
    items = U.write_pairs(indir, U.SHAPES)
    model = _build_model()[0]
    assert U.geometry(U.SHAPES) == ((16, 16), (22, 32)) and [P.scaled_size(h, w, U.FACTOR) for h, w in U.SHAPES] == [(10, 15), (11, 16), (10, 16)]
    # (the step test runs the three pairs and an empty slot as one batch, the loop test batches of two)
    return dict(model=model, indir=indir, items=items, want4=U.pasted_want(model, items, 4), want2=U.pasted_want(model, items, 2))


def test_host_fed_step_pastes_the_scaled_result_into_the_source(pairs):
    got = U.check_step(pairs['model'], pairs['items'], U.SHAPES, 'cpu', 'replay', pairs['want4'])
    assert got.any()


def test_host_fed_step_without_paste_back_is_unchanged(pairs):
    """paste_back=False (the default): the scaled-size result sets and bytes of the step as it was -- those of the fp32 form."""
    model, items = pairs['model'], pairs['items']
    host = [P.load_item(m, i, 8, U.FACTOR) for m, i in items]
    ref = P.HostFedStep(model, 3, *BUCKET, 'cpu', drain=True, u8_input=False)
    for j in range(3):
        ref.put(0, j, host[j][0], host[j][1])
    ref.prime(0)
    ref.launch(0)
    ref.wait(0)
    ref.flush(0)
    hs = P.HostFedStep(model, 3, *BUCKET, 'cpu', drain=True, scale_factor=U.FACTOR, src_hw=SRC_HW, paste_back=False)
    assert not hs.paste_back and tuple(hs.u8[0].shape) == (3, *BUCKET, 3)
    assert not P.HostFedStep(model, 3, *BUCKET, 'cpu', scale_factor=U.FACTOR, src_hw=SRC_HW).paste_back                 # the default
    assert np.array_equal(U.one_step(hs, items), ref.result(0))


def test_host_fed_step_refuses_paste_back_without_its_conditions(pairs):
    model = pairs['model']
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, *BUCKET, 'cpu', paste_back=True)                                               # no scale_factor
    with pytest.raises(L.LamaError):
        P.HostFedStep(model, 2, *BUCKET, 'cpu', scale_factor=U.FACTOR, src_hw=SRC_HW, paste_back=True, out_key='predicted_image')
    with pytest.raises(L.LamaError):
        P.predict(model, pairs['items'], pairs['indir'], os.devnull, device='cpu', paste_back=True)              # before anything is opened


def test_predict_loop_writes_source_size_pngs(pairs, tmp_path):
    """predict(scale_factor=0.5, paste_back=True), batches of two (a full and a partial round): source-size PNGs, the source pixels where the
    mask is 0, the restatement everywhere."""
    out = str(tmp_path / 'out')
    n = P.predict(pairs['model'], pairs['items'], pairs['indir'], out, pad_mod=8, batch_size=2, device='cpu', io_threads=2, scale_factor=U.FACTOR,
                  paste_back=True)
    assert n == 3
    U.check_written_pngs(out, pairs['indir'], pairs['items'], pairs['want2'])


def test_cli_key_and_its_three_refusals(monkeypatch):
    base = ['model.path=/m', 'indir=i', 'outdir=o']
    assert P.parse_overrides(base)['paste_back'] is False and P.DEFAULTS['paste_back'] is False
    assert 'paste_back' in P.KNOWN_KEYS and 'paste_back' in P.BOOL_KEYS
    cfg = P.parse_overrides(base + ['dataset.scale_factor=0.25', 'paste_back=true'])
    assert cfg['paste_back'] is True and cfg['dataset.scale_factor'] == 0.25
    assert P.parse_overrides(base + ['dataset.scale_factor=0.25', 'paste_back=false'])['paste_back'] is False

    def no_launch(*a, **k):
        raise AssertionError('the refusal came after the model was loaded')
    monkeypatch.setattr(P.trainers, 'load_checkpoint', no_launch)
    for extra, word in ((['paste_back=true'], 'dataset.scale_factor'),
                        (['dataset.scale_factor=0.5', 'paste_back=true', 'refine=true'], 'refine'),
                        (['dataset.scale_factor=0.5', 'paste_back=true', 'out_key=predicted_image'], 'predicted_image')):
        with pytest.raises(SystemExit) as e:
            P.main(base + extra)
        assert 'paste_back' in str(e.value) and word in str(e.value), extra
    with pytest.raises(SystemExit):
        P.parse_overrides(base + ['paste_back=maybe'])
