"""GPU tests of the local Fourier unit (enable_lfu=True): the two kernels of lama_amd/csrc/lfu.hip bit for bit against their torch
restatement, the modules and the small generator against tests/golden/lfu.npz, and FFCResnetBlock(512) with the LFU at the bottleneck plane
(64 x 64 one-buffer FFT, Winograd local conv, 32 x 32 LFU planes) against tests/golden/lfu_block512.npz -- all recorded from the reference's
own classes (tests/golden/make_golden_lfu.py).  Bars: the ones tests/test_generator_gpu.py holds the non-LFU goldens to (tests/lfu_util.py)."""
import numpy as np
import os
import pytest
import torch

from lama_amd import _lib as L
from lama_amd import ffc as F
from tests import lfu_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')


def _prepare(m):
    return m.cuda()


@pytest.fixture(scope='module')
def small():
    return U.small_generator(_prepare)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['f32', 'f16'])
@pytest.mark.parametrize('B,C,h,layout', U.KERNEL_SHAPES, ids=['2x8x6-scalar', '1x16x8-slice', '3x8x64-wide', '1x4x130'])
def test_kernels_bit_for_bit(B, C, h, layout, dtype):
    U.check_kernels(L.get_lib(), DEV, B, C, h, layout, dtype)


def test_kernel_refusals_leave_the_outputs_alone():
    U.check_refusals(L.get_lib(), DEV)


@pytest.mark.parametrize('prec', list(U.PRECS), ids=list(U.PRECS))
def test_units_match_reference_goldens(prec):
    U.check_units(_prepare, DEV, U.PRECS[prec])


@pytest.mark.parametrize('prec', list(U.PRECS), ids=list(U.PRECS))
@pytest.mark.parametrize('case', list(U.GEN_CASES))
def test_small_generator_matches_reference_golden(small, case, prec):
    gen, sd, g = small
    U.check_generator_golden(gen, g, DEV, U.PRECS[prec], case)


def test_small_generator_graph_split_keys_and_refused_plane(small):
    gen, sd, g = small
    U.check_generator_plans(gen, sd, DEV, graph=True)


def test_probe_rows_and_refusals(small):
    gen, sd, g = small
    U.check_probe_and_refusals(gen, DEV)


@pytest.mark.parametrize('prec', list(U.PRECS), ids=list(U.PRECS))
def test_block512_with_lfu_at_the_production_routes(prec):
    g = np.load(os.path.join(U.GOLDEN, 'lfu_block512.npz'))
    blk = F.FFCResnetBlock(512, **U.BLOCK_KW)
    blk.load_state_dict(U.block512_state_dict(blk, U.stored_stats(g, 'blk')), strict=True)
    blk.cuda().set_precision(U.PRECS[prec])
    U.check_block512(blk, DEV, U.PRECS[prec])


def test_predict_cli_serves_an_lfu_checkpoint(small, tmp_path):
    """python -m lama_amd.predict on a checkpoint directory whose config.yaml has enable_lfu: True in resnet_conv_kwargs: square inputs with a
    side that is a multiple of 16 are served (the u8 results within one level of the module's own forward, quantised as bin/predict.py does),
    any other shape is refused with the LFU's message."""
    import yaml
    from PIL import Image
    from lama_amd import predict as P
    from lama_amd import trainers
    gen, sd, g = small
    cfg = U.small_lfu_config()
    raw = dict(training_model=dict(kind='default', concat_mask=True), generator=dict(kind='ffc_resnet', **cfg))
    mdir = tmp_path / 'model'
    os.makedirs(mdir / 'models')
    with open(mdir / 'config.yaml', 'w') as f:
        yaml.safe_dump(raw, f)
    sdg = {'generator.' + k: v for k, v in sd.items()}
    torch.save({'state_dict': sdg}, mdir / 'models' / 'best.ckpt')
    rng = np.random.RandomState(5)

    def write(d, name, h, w):
        os.makedirs(d, exist_ok=True)
        img = rng.randint(0, 256, (h, w, 3)).astype('uint8')
        m = np.zeros((h, w), 'uint8')
        m[h // 3: 2 * h // 3, w // 4: w // 2] = 255
        Image.fromarray(img).save(d / f'{name}.png')
        Image.fromarray(m).save(d / f'{name}_mask001.png')
        return img, m

    indir, out = tmp_path / 'in', tmp_path / 'out'
    items = {name: write(indir, name, s, s) for name, s in (('a', 64), ('b', 80))}
    assert P.main([f'model.path={mdir}', f'indir={indir}', f'outdir={out}', 'batch_size=1']) == 0
    model = trainers.DefaultInpaintingTrainingModule(dict(generator=dict(kind='ffc_resnet', **cfg)))
    model.load_state_dict(sdg, strict=True)
    model.freeze().cuda()
    for name, (img, m) in items.items():
        batch = dict(image=torch.from_numpy(img).permute(2, 0, 1)[None].float().div(255).cuda(),
                     mask=(torch.from_numpy(m)[None, None] > 0).float().cuda())
        want = np.clip(model(batch)['inpainted'][0].permute(1, 2, 0).cpu().numpy() * 255, 0, 255).astype('uint8')
        got = np.array(Image.open(out / f'{name}_mask001.png'))
        assert got.shape == want.shape and np.abs(got.astype(int) - want.astype(int)).max() <= 1, name
    bad = tmp_path / 'in_bad'
    write(bad, 'c', 64, 96)
    with pytest.raises(L.LamaError, match='h // 2'):
        P.main([f'model.path={mdir}', f'indir={bad}', f'outdir={tmp_path / "out_bad"}', 'batch_size=1'])
