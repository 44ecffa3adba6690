"""``paste_back`` on the MI355X: lama_paste_back_u8_fwd through the C ABI of the shipped library, HostFedStep in its modes and the CLI end to
end.  The checks are those of tests/test_paste_back_emu.py (tests/paste_back_util.py): byte for byte against the numpy restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import paste_back_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from lama_amd import _lib as L
    return L.get_lib()          # raises if liblama_hip.so was not built: no fallback


@pytest.mark.parametrize('layout', U.LAYOUTS)
@pytest.mark.parametrize('binarize', [True, False], ids=['binarize', 'fractional'])
@pytest.mark.parametrize('mask_kind', U.MASKS)
@pytest.mark.parametrize('name', list(U.CASES))
def test_kernel_is_the_restatement_byte_for_byte(lib, name, mask_kind, binarize, layout):
    U.check_case(lib, 'cuda', name, mask_kind, binarize, layout)


def test_misaligned_slots_take_the_byte_path(lib):
    U.check_misaligned_slots(lib, 'cuda')


def test_sizes_that_do_not_fit_yield_zero_slots(lib):
    U.check_sizes_that_do_not_fit(lib, 'cuda')


def test_non_finite_samples_quantise_as_the_blend_does(lib):
    U.check_non_finite(lib, 'cuda')


def test_refusals_return_their_code_and_launch_nothing(lib):
    U.check_refusals(lib, 'cuda')


# ---- the step and the CLI -------------------------------------------------------------------------------------------------------------------
def _small_model():
    """The small synthetic model of the other GPU step tests (tests/test_scale_device_gpu.py), as the CLI sets it up."""
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
    indir = str(tmp_path_factory.mktemp('paste') / 'in') + os.sep
    items = U.write_pairs(indir, U.SHAPES_GPU)
    model, sd, train_config = _small_model()
    assert U.geometry(U.SHAPES_GPU) == ((96, 120), (191, 240))
    # (the step test runs the three pairs and an empty slot as one batch, the CLI batches of two)
    return dict(model=model, sd=sd, train_config=train_config, indir=indir, items=items, want4=U.pasted_want(model, items, 4, 'cuda'),
                want2=U.pasted_want(model, items, 2, 'cuda'))


def test_host_fed_step_graph_equals_host_equals_the_restatement(pairs):
    """The captured step ('graph': the paste is one more kernel node) against the host-synchronised one, both against the restatement."""
    host = U.check_step(pairs['model'], pairs['items'], U.SHAPES_GPU, 'cuda', 'host', pairs['want4'])
    graph = U.check_step(pairs['model'], pairs['items'], U.SHAPES_GPU, 'cuda', 'graph', pairs['want4'])
    assert np.array_equal(host, graph)


def test_cli_end_to_end_writes_source_size_pngs(pairs, tmp_path):
    """python -m lama_amd.predict dataset.scale_factor=0.5 paste_back=true in a process of its own."""
    import yaml
    mdir = tmp_path / 'model'
    os.makedirs(mdir / 'models')
    with open(mdir / 'config.yaml', 'w') as f:
        yaml.safe_dump(pairs['train_config'], f)
    torch.save(dict(state_dict=pairs['sd']), str(mdir / 'models' / 'best.ckpt'))
    out = str(tmp_path / 'out')
    r = subprocess.run([sys.executable, '-m', 'lama_amd.predict', f'model.path={mdir}', f'indir={pairs["indir"]}', f'outdir={out}',
                        'batch_size=2', 'dataset.scale_factor=0.5', 'paste_back=true'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    U.check_written_pngs(out, pairs['indir'], pairs['items'], pairs['want2'])
