"""``crop_max_side`` on the MI355X: lama_crop_shrink_compose_u8_fwd / lama_crop_shrink_paste_u8_fwd through the C ABI of the shipped library,
HostFedStep(crop=True, crop_shrink=True) in its modes and the CLI end to end.  The checks are those of tests/test_crop_shrink_emu.py
(tests/crop_shrink_util.py): bit for bit / byte for byte against the numpy restatement and against the existing entries on host-cropped slots."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import crop_shrink_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from lama_amd import _lib as L
    return L.get_lib()          # raises if liblama_hip.so was not built: no fallback


@pytest.mark.parametrize('layout', U.LAYOUTS)
@pytest.mark.parametrize('binarize', [True, False], ids=['binarize', 'fractional'])
@pytest.mark.parametrize('name', list(U.CASES))
def test_kernels_are_the_definition_bit_for_bit(lib, name, binarize, layout):
    U.check_case(lib, 'cuda', name, binarize, layout)


def test_k1_is_the_crop_entries(lib):
    U.check_k1_is_the_crop(lib, 'cuda')


def test_one_pixel_strokes_stay_holes_and_are_replaced(lib):
    U.check_one_pixel_strokes(lib, 'cuda')


def test_misaligned_slots_take_the_byte_path(lib):
    U.check_misaligned_slots(lib, 'cuda')


@pytest.mark.parametrize('layout', U.LAYOUTS)
def test_rects_that_do_not_fit_behave_as_empty_slots(lib, layout):
    U.check_rects_that_do_not_fit(lib, 'cuda', layout)


def test_non_finite_samples_quantise_as_the_paste_back_does(lib):
    U.check_non_finite(lib, 'cuda')


def test_refusals_return_their_code_and_launch_nothing(lib):
    U.check_refusals(lib, 'cuda')


# ---- the step and the CLI -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    from tests.test_crop_gpu import _small_model
    indir = str(tmp_path_factory.mktemp('crop_shrink') / 'in') + os.sep
    items = U.write_pairs(indir)
    model, sd, train_config = _small_model()
    wins = U.item_windows(items)
    return dict(model=model, sd=sd, train_config=train_config, indir=indir, items=items, wins=wins,
                want=U.definition_want(model, items, wins, 'cuda', 2))


def test_host_fed_step_host_replay_and_graph_are_the_definition(pairs):
    """Modes 'host', 'replay' and 'graph' (the compose and the paste are two more kernel nodes of the captured step) against the definition;
    the three agree with one another."""
    m, it, w = pairs['model'], pairs['items'], pairs['wins']
    host = U.check_step(m, it, w, 'cuda', 'host', pairs['want'], 2)
    replay = U.check_step(m, it, w, 'cuda', 'replay', pairs['want'], 2)
    graph = U.check_step(m, it, w, 'cuda', 'graph', pairs['want'], 2)
    for a, b, c in zip(host, replay, graph):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_host_fed_step_with_encode_png_decodes_to_the_same_pixels(pairs):
    U.check_step(pairs['model'], pairs['items'], pairs['wins'], 'cuda', 'host', pairs['want'], 2, encode_png=True)


def test_cli_end_to_end_writes_source_size_pngs(pairs, tmp_path):
    """python -m lama_amd.predict crop_to_mask=true crop_max_side=32 in a process of its own, and once more without the key for the k = 1 item:
    that file is byte-identical."""
    import yaml
    mdir = tmp_path / 'model'
    os.makedirs(mdir / 'models')
    with open(mdir / 'config.yaml', 'w') as f:
        yaml.safe_dump(pairs['train_config'], f)
    torch.save(dict(state_dict=pairs['sd']), str(mdir / 'models' / 'best.ckpt'))
    out, plain = str(tmp_path / 'out'), str(tmp_path / 'plain')
    one = str(tmp_path / 'one') + os.sep
    os.makedirs(one)
    for name in ('im0.png', 'im0_mask.png'):
        os.symlink(os.path.join(pairs['indir'], name), os.path.join(one, name))
    common = ['batch_size=2', 'crop_to_mask=true', f'crop_margin={U.MARGIN}', f'crop_step={U.STEP}', f'dataset.pad_out_to_modulo={U.PAD_MOD}']
    for indir, outdir, extra in ((pairs['indir'], out, [f'crop_max_side={U.MAX_SIDE}']), (one, plain, [])):
        r = subprocess.run([sys.executable, '-m', 'lama_amd.predict', f'model.path={mdir}', f'indir={indir}', f'outdir={outdir}', *common, *extra],
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    U.check_written_pngs(out, pairs['indir'], pairs['items'], pairs['want'])
    with open(os.path.join(out, 'im0_mask.png'), 'rb') as a, open(os.path.join(plain, 'im0_mask.png'), 'rb') as b:
        assert a.read() == b.read()
