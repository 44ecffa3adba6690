"""The device JPEG encoder on the MI355X: lama_jpeg_scan_u8_fwd through the C ABI of the shipped library, HostFedStep(encode_jpeg=True) in every
mode and input form, and the CLI with device_jpeg on and off.  The checks are those of tests/test_jpeg_emu.py (tests/jpeg_util.py): byte for
byte against the restatement tests/jpeg_ref.py::scan_ref."""
import os

import numpy as np
import pytest
import torch

from tests import jpeg_ref as R
from tests import jpeg_util as U
from tests import paste_back_util as PB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from lama_amd import _lib as L
    return L.get_lib()          # raises if liblama_hip.so was not built: no fallback


@pytest.mark.parametrize('name', U.CASES)
def test_kernel_is_the_restatement_byte_for_byte(lib, name):
    U.check_case(lib, 'cuda', name)


@pytest.mark.parametrize('ss', ['444', '420'])
@pytest.mark.parametrize('shift', [1, 2, 3])
def test_misaligned_slots_take_the_narrow_loads(lib, shift, ss):
    U.check_case(lib, 'cuda', f'37x53-in-40x64@{ss}', shift=shift)


def test_sizes_that_do_not_fit_yield_no_scan(lib):
    U.check_sizes_that_do_not_fit(lib, 'cuda')


def test_a_scan_longer_than_its_slot_reports_the_bytes_needed(lib):
    U.check_overflow(lib, 'cuda')


def test_refusals_return_their_code_and_launch_nothing(lib):
    U.check_refusals(lib, 'cuda')


@pytest.mark.parametrize('ss', [R.J444, R.J420])
def test_many_workgroups_side_by_side(lib, ss):
    """2 x 200 x 600 (25 / 13 MCU rows of two segments each, more workgroups than one image's): a photo-like and a random image in one launch,
    the second smaller than its slot."""
    slots = np.stack([U.photo(200, 600, seed=30), U.noise(200, 600, seed=31)])
    sizes = np.array([[200, 600], [197, 599]], np.int32)
    got, lens, intact, _ = U.run(lib, 'cuda', slots, sizes, 95, ss)
    assert intact
    for j in range(2):
        h, w = sizes[j]
        U._same(got[j], R.scan_ref(slots[j], h, w, 95, ss), j)


# ---- the step and the CLI -------------------------------------------------------------------------------------------------------------------
PLAIN_SHAPES = [(95, 119), (96, 120), (94, 120)]        # three sizes of the 96 x 120 bucket of the other GPU step tests


@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    from tests.test_paste_back_gpu import _small_model
    root = tmp_path_factory.mktemp('jpeg')
    items = PB.write_pairs(str(root / 'in') + os.sep, PB.SHAPES_GPU)
    plain = PB.write_pairs(str(root / 'plain') + os.sep, PLAIN_SHAPES, seed=9)
    model, sd, train_config = _small_model()
    return dict(model=model, sd=sd, train_config=train_config, indir=str(root / 'in') + os.sep, items=items, plain_dir=str(root / 'plain') + os.sep,
                plain=plain)


@pytest.mark.parametrize('form', ['plain', 'predicted_image', 'scale_factor', 'scale_factor+paste_back'])
@pytest.mark.parametrize('mode', ['host', 'replay', 'streams', 'graph'])
def test_host_fed_step_scans_are_the_restatement_of_the_u8_results(pairs, mode, form):
    """In 'graph' the three launches are three more kernel nodes of the captured step.  ('predicted_image': 4:4:4 at quality 50.)"""
    bucket, src_hw = PB.geometry(PB.SHAPES_GPU)
    if form.startswith('scale_factor'):
        U.check_step(pairs['model'], pairs['items'], 'cuda', mode, bucket, scale_factor=PB.FACTOR, src_hw=src_hw, paste_back=form.endswith('paste_back'))
    elif form == 'plain':
        U.check_step(pairs['model'], pairs['plain'], 'cuda', mode, (96, 120))
    else:
        U.check_step(pairs['model'], pairs['plain'], 'cuda', mode, (96, 120), quality=50, subsampling='444', out_key='predicted_image')


def test_host_fed_step_reports_a_scan_that_does_not_fit(pairs):
    U.check_step_overflow(pairs['model'], pairs['plain'][:2], 'cuda', 'host', (96, 120))


def _model_dir(pairs, tmp_path):
    import yaml
    mdir = tmp_path / 'model'
    os.makedirs(mdir / 'models')
    with open(mdir / 'config.yaml', 'w') as f:
        yaml.safe_dump(pairs['train_config'], f)
    torch.save(dict(state_dict=pairs['sd']), str(mdir / 'models' / 'best.ckpt'))
    return mdir


@pytest.mark.parametrize('form', ['plain', 'scale_factor+paste_back'])
def test_cli_writes_the_restatement_files(pairs, tmp_path, form, monkeypatch):
    """lama_amd.predict's main on a small synthetic checkpoint directory: the PNG run, out_ext=.jpg with device_jpeg off and on -- the same file
    names, every device file byte for byte jpeg_from_scan(scan_ref(the PNG run's pixels)); then ('plain') with scan slots as long as the shortest scan:
    the host fallback still writes a valid file for the others."""
    from PIL import Image
    from lama_amd import predict as P
    mdir = _model_dir(pairs, tmp_path)
    indir = pairs['plain_dir'] if form == 'plain' else pairs['indir']
    extra = [] if form == 'plain' else ['dataset.scale_factor=0.5', 'paste_back=true']
    base = [f'model.path={mdir}', f'indir={indir}', 'batch_size=2'] + extra
    outs = {tag: str(tmp_path / tag) for tag in ('png', 'off', 'on', 'small')}
    assert P.main(base + [f"outdir={outs['png']}"]) == 0
    assert P.main(base + [f"outdir={outs['off']}", 'out_ext=.jpg']) == 0
    assert P.main(base + [f"outdir={outs['on']}", 'out_ext=.jpg', 'device_jpeg=true']) == 0
    names = U.check_cli_outputs(outs['png'], outs['on'], dir_off=outs['off'])
    assert len(names) == 3
    if form != 'plain':
        return
    sizes = [os.path.getsize(os.path.join(outs['on'], nm)) for nm in names]
    header = len(P.jpeg_from_scan(8, 8, 95, '420', b''))
    monkeypatch.setattr(P, 'JPEG_OUT_STRIDE', min(sizes) - header)
    assert P.main(base + [f"outdir={outs['small']}", 'out_ext=.jpg', 'device_jpeg=true']) == 0
    assert U.files_of(outs['small']) == names
    n_host = 0
    for nm, size in zip(names, sizes):
        with open(os.path.join(outs['small'], nm), 'rb') as f, open(os.path.join(outs['on'], nm), 'rb') as g:
            data, dev = f.read(), g.read()
        src = np.array(Image.open(os.path.join(outs['png'], os.path.splitext(nm)[0] + '.png')))
        dec = U.decode_jpeg(data)
        assert dec.shape == src.shape and U.psnr(dec, src) >= U.psnr(U.decode_jpeg(dev), src) - 1.0
        assert (data == dev) == (size == min(sizes)), nm
        n_host += data != dev
    assert n_host >= 1
