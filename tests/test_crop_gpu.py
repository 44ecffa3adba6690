"""``crop_to_mask`` on the MI355X: lama_crop_compose_u8_fwd / lama_crop_paste_u8_fwd through the C ABI of the shipped library, HostFedStep(crop=True)
in its modes and the CLI end to end.  The checks are those of tests/test_crop_emu.py (tests/crop_util.py): bit for bit / byte for byte against the
numpy restatement and against the existing u8 entries and the existing u8 step on host-cropped operands."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import crop_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from lama_amd import _lib as L
    return L.get_lib()          # raises if liblama_hip.so was not built: no fallback


@pytest.mark.parametrize('layout', U.LAYOUTS)
@pytest.mark.parametrize('binarize', [True, False], ids=['binarize', 'fractional'])
@pytest.mark.parametrize('name', list(U.CASES))
def test_kernels_are_the_u8_step_on_the_crop_bit_for_bit(lib, name, binarize, layout):
    U.check_case(lib, 'cuda', name, binarize, layout)


def test_misaligned_slots_take_the_byte_path(lib):
    U.check_misaligned_slots(lib, 'cuda')


@pytest.mark.parametrize('layout', U.LAYOUTS)
def test_rects_that_do_not_fit_behave_as_empty_slots(lib, layout):
    U.check_rects_that_do_not_fit(lib, 'cuda', layout)


def test_non_finite_samples_quantise_as_the_blend_does(lib):
    U.check_non_finite(lib, 'cuda')


def test_refusals_return_their_code_and_launch_nothing(lib):
    U.check_refusals(lib, 'cuda')


# ---- the step and the CLI -------------------------------------------------------------------------------------------------------------------
def _small_model():
    """The small synthetic model of the other GPU step tests (tests/test_paste_back_gpu.py), as the CLI sets it up."""
    from lama_amd import trainers
    from oracle import lama_oracle as O
    cfg = O.small_config(ngf=16, n_blocks=2)
    sd = {'generator.' + k: v for k, v in O.make_synthetic_state_dict(cfg, seed=3, calib_hw=32).items()}
    train_config = dict(generator=dict(kind='ffc_resnet', **cfg))
    model = trainers.DefaultInpaintingTrainingModule(train_config)
    model.load_state_dict(sd, strict=True)
    model.freeze().cuda()
    model.generator.use_graph = True
    return model, sd, train_config


@pytest.fixture(scope='module')
def pairs(tmp_path_factory):
    indir = str(tmp_path_factory.mktemp('crop') / 'in') + os.sep
    items = U.write_pairs(indir)
    model, sd, train_config = _small_model()
    rects = U.item_rects(items)
    # (the step tests run each bucket as one batch of three, the CLI batches of two; the definition is computed once per mode)
    return dict(model=model, sd=sd, train_config=train_config, indir=indir, items=items, rects=rects,
                want3=U.cropped_want(model, items, rects, 3, 'cuda', 'host'), want2=U.cropped_want(model, items, rects, 2, 'cuda', 'host'))


def test_host_fed_step_host_replay_and_graph_are_the_u8_step_on_the_crop(pairs):
    """Modes 'host', 'replay' and 'graph' (the compose and the paste are two more kernel nodes of the captured step), each against the existing u8
    step on the host-cropped pairs in the same mode where it differs, pasted by numpy."""
    m, it, rc = pairs['model'], pairs['items'], pairs['rects']
    host = U.check_step(m, it, rc, 'cuda', 'host', pairs['want3'], 3)
    replay = U.check_step(m, it, rc, 'cuda', 'replay', U.cropped_want(m, it, rc, 3, 'cuda', 'replay'), 3)
    graph = U.check_step(m, it, rc, 'cuda', 'graph', U.cropped_want(m, it, rc, 3, 'cuda', 'graph'), 3)
    for a, b, c in zip(host, replay, graph):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_host_fed_step_with_encode_png_decodes_to_the_same_pixels(pairs):
    U.check_step(pairs['model'], pairs['items'], pairs['rects'], 'cuda', 'host', pairs['want3'], 3, encode_png=True)


def test_cli_end_to_end_writes_source_size_pngs(pairs, tmp_path):
    """python -m lama_amd.predict crop_to_mask=true in a process of its own."""
    import yaml
    mdir = tmp_path / 'model'
    os.makedirs(mdir / 'models')
    with open(mdir / 'config.yaml', 'w') as f:
        yaml.safe_dump(pairs['train_config'], f)
    torch.save(dict(state_dict=pairs['sd']), str(mdir / 'models' / 'best.ckpt'))
    out = str(tmp_path / 'out')
    r = subprocess.run([sys.executable, '-m', 'lama_amd.predict', f'model.path={mdir}', f'indir={pairs["indir"]}', f'outdir={out}',
                        'batch_size=2', 'crop_to_mask=true', f'crop_margin={U.MARGIN}', f'crop_step={U.STEP}',
                        f'dataset.pad_out_to_modulo={U.PAD_MOD}'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    U.check_written_pngs(out, pairs['indir'], pairs['items'], pairs['want2'])
