"""The device PNG encoder on the MI355X: lama_png_deflate_u8_fwd through the C ABI of the shipped library, HostFedStep(encode_png=True) in every
mode and input form, and the CLI with device_png on and off.  The checks are those of tests/test_png_emu.py (tests/png_util.py): byte for
byte against the restatement tests/png_ref.py::deflate_ref."""
import os

import numpy as np
import pytest
import torch

from tests import paste_back_util as PB
from tests import png_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from lama_amd import _lib as L
    return L.get_lib()          # raises if liblama_hip.so was not built: no fallback


@pytest.mark.parametrize('name', U.CASES)
def test_kernel_is_the_restatement_byte_for_byte(lib, name):
    U.check_case(lib, 'cuda', name)


@pytest.mark.parametrize('shift', [1, 4])
def test_misaligned_slots_take_the_narrower_loads(lib, shift):
    U.check_case(lib, 'cuda', '37x53-in-40x64', shift=shift)


def test_default_chunk_bytes(lib):
    U.check_default_chunk(lib, 'cuda')


def test_sizes_that_do_not_fit_yield_no_stream(lib):
    U.check_sizes_that_do_not_fit(lib, 'cuda')


def test_refusals_return_their_code_and_launch_nothing(lib):
    U.check_refusals(lib, 'cuda')


def test_full_size_slots_many_workgroups(lib):
    """2 x 512 x 512 at the default chunk (33 chunks per image, 16 rows of 1537 bytes each but the last): more workgroups than one round, a
    photo-like and a random image side by side -- the dynamic and the stored form in one launch."""
    from tests import png_ref as R
    slots = np.stack([U.photo(512, 512, seed=30), U.noise(512, 512, seed=31)])
    sizes = np.array([[512, 512], [509, 511]], np.int32)
    got, lens, intact, _ = U.run(lib, 'cuda', slots, sizes, 0)
    assert intact
    for j in range(2):
        h, w = sizes[j]
        assert got[j] == R.deflate_ref(slots[j], h, w), j


# ---- the step and the CLI -------------------------------------------------------------------------------------------------------------------
PLAIN_SHAPES = [(95, 119), (96, 120), (94, 120)]        # three sizes of the 96 x 120 bucket of the other GPU step tests


@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    from tests.test_paste_back_gpu import _small_model
    root = tmp_path_factory.mktemp('png')
    items = PB.write_pairs(str(root / 'in') + os.sep, PB.SHAPES_GPU)
    plain = PB.write_pairs(str(root / 'plain') + os.sep, PLAIN_SHAPES, seed=9)
    model, sd, train_config = _small_model()
    return dict(model=model, sd=sd, train_config=train_config, indir=str(root / 'in') + os.sep, items=items, plain_dir=str(root / 'plain') + os.sep,
                plain=plain)


@pytest.mark.parametrize('form', ['plain', 'predicted_image', 'scale_factor', 'scale_factor+paste_back'])
@pytest.mark.parametrize('mode', ['host', 'replay', 'streams', 'graph'])
def test_host_fed_step_streams_decode_to_the_u8_results(pairs, mode, form):
    """In 'graph' the two launches are two more kernel nodes of the captured step."""
    bucket, src_hw = PB.geometry(PB.SHAPES_GPU)
    if form.startswith('scale_factor'):
        U.check_step(pairs['model'], pairs['items'], 'cuda', mode, bucket, scale_factor=PB.FACTOR, src_hw=src_hw, paste_back=form.endswith('paste_back'))
    else:
        U.check_step(pairs['model'], pairs['plain'], 'cuda', mode, (96, 120), **(dict(out_key='predicted_image') if form == 'predicted_image' else {}))


def test_host_fed_step_double_buffered_rounds(pairs):
    """Three rounds through both parities (mode 'host'): every round's streams are those of its own batch."""
    from lama_amd import predict as P
    from tests import png_ref as R
    loaded = [P.load_item_u8(m, i) for m, i in pairs['plain']]
    batches = [loaded[:2], loaded[1:], loaded[::-1][:2]]
    ref = P.HostFedStep(pairs['model'], 2, 96, 120, 'cuda', mode='host')
    hs = P.HostFedStep(pairs['model'], 2, 96, 120, 'cuda', mode='host', encode_png=True)
    results = []
    for step in (ref, hs):
        got = []

        def take(p):
            got.append(step.result(p).copy() if step is ref else [bytes(step.result_png(p, j)) for j in range(2)])
        U.feed(step, 0, batches[0])
        step.prime(0)
        for k in range(3):                     # the round loop of predict: launch k downloads round k - 1, which wait(k - 1's parity) at k + 1 covers
            p = k & 1
            if k + 1 < 3:
                U.feed(step, 1 - p, batches[k + 1])
            step.launch(p)
            if k >= 1:
                step.wait(1 - p)
                if k >= 2:
                    take(p)
        step.wait(0)
        take(1)
        step.flush(0)
        take(0)
        results.append(got)
    for k in range(3):
        for j in range(2):
            h, w = batches[k][j][2]
            assert results[1][k][j] == R.deflate_ref(results[0][k][j], h, w), (k, j)


def _model_dir(pairs, tmp_path):
    import yaml
    mdir = tmp_path / 'model'
    os.makedirs(mdir / 'models')
    with open(mdir / 'config.yaml', 'w') as f:
        yaml.safe_dump(pairs['train_config'], f)
    torch.save(dict(state_dict=pairs['sd']), str(mdir / 'models' / 'best.ckpt'))
    return mdir


@pytest.mark.parametrize('form', ['plain', 'scale_factor+paste_back'])
def test_cli_writes_the_same_pixels_with_the_option_on_and_off(pairs, tmp_path, form):
    """lama_amd.predict's main on a small synthetic checkpoint directory, device_png=false and true: the same file names, and every pair of PNGs
    decodes (PIL) to identical pixels; with the option off the bytes are encode_png's."""
    from PIL import Image
    from lama_amd import predict as P
    mdir = _model_dir(pairs, tmp_path)
    indir = pairs['plain_dir'] if form == 'plain' else pairs['indir']
    extra = [] if form == 'plain' else ['dataset.scale_factor=0.5', 'paste_back=true']
    outs = []
    for on in ('false', 'true'):
        outs.append(str(tmp_path / f'out_{on}'))
        assert P.main([f'model.path={mdir}', f'indir={indir}', f'outdir={outs[-1]}', 'batch_size=2', f'device_png={on}'] + extra) == 0
    names = U.check_same_pngs(*outs)
    assert len(names) == 3
    for nm in names:
        with open(os.path.join(outs[0], nm), 'rb') as f:
            assert f.read() == P.encode_png(np.array(Image.open(os.path.join(outs[0], nm))))
