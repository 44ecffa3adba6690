"""GPU tests of the pix2pixhd_global generator (big-lama-regular / lama-regular, lama_amd.pix2pixhd): the golden vectors of the
reference's own GlobalGenerator / ResnetBlock through the C ABI, the full models against an fp32 torch restatement built from the same
weights, graph replay, the fp16-split range watch, the predict CLI, and the Winograd conv at 512 output rows (four row groups)."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as tF

from lama_amd import _lib as L
from lama_amd import pix2pixhd as P
from lama_amd.modules import make_generator
from tests import regular_util as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PRECS = {'f32': L.PREC_F32, 'f16x3': L.PREC_F16X3, 'bf16x3': L.PREC_BF16X3}
BAR = 2e-4          # max-abs, the fp32-class precisions (as tests/test_generator_gpu.py)


@pytest.fixture(autouse=True, scope='module')
def _exact_torch():
    keep = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = keep


def _gen(cfg, sd, prec):
    gen = make_generator(None, kind='pix2pixhd_global', **cfg)
    gen.load_state_dict(sd, strict=True)
    return gen.cuda().set_precision(prec)


def _cuda(sd):
    return {k: v.cuda() for k, v in sd.items()}


# ---- golden vectors of the reference's classes ----------------------------------------------------------------------------------

@pytest.mark.parametrize('prec', list(PRECS), ids=list(PRECS))
def test_small_generator_matches_golden(prec):
    g = np.load(os.path.join(GOLDEN, 'regular_small.npz'))
    cfg = R.small_config(ngf=int(g['ngf'][0]), n_blocks=int(g['n_blocks'][0]))
    sd = R.make_state_dict(cfg, seed=int(g['seed'][0]), calib_hw=32)
    assert abs(sum(float(v.double().sum()) for v in sd.values() if v.is_floating_point()) - float(g['sd_checksum'][0])) < 1e-6 * max(1.0, abs(float(g['sd_checksum'][0])))
    gen = _gen(cfg, sd, PRECS[prec])
    for name in ('a', 'b'):
        x = torch.from_numpy(g[f'{name}_input']).cuda()
        y = gen(x)
        torch.cuda.synchronize()
        err = float((y.cpu() - torch.from_numpy(g[f'{name}_output'])).abs().max())
        assert err <= BAR, (prec, name, err)


@pytest.mark.parametrize('prec', list(PRECS), ids=list(PRECS))
def test_block512_matches_golden(prec):
    g = np.load(os.path.join(GOLDEN, 'regular_block512.npz'))
    sd = R.block_state_dict(512, seed=int(g['seed'][0]))
    blk = P.ResnetBlock(512, 'reflect', 'bn')
    blk.load_state_dict(sd, strict=True)
    blk.cuda().set_precision(PRECS[prec])
    x = R.block_input(2, 512, 64, seed=int(g['x_seed'][0]))
    assert abs(float(x.double().sum()) - float(g['x_checksum'][0])) < 1e-3
    x = x.cuda()
    lib = L.get_lib()
    ws = torch.empty(lib.winograd_workspace_bytes(2, 512, 64, 64) // 4, device='cuda') if PRECS[prec] != L.PREC_F32 else None
    st, t = x.clone(), torch.empty_like(x)
    with blk._exec.range_scope(st, blk.precision):
        paths = blk.run(st, t, st, ws)                  # in place over the block input, as the generator's plan runs it
    assert paths == ((True, True) if ws is not None else (False, False))
    y = blk(x)                                          # the stand-alone forward: direct kernel, separate output
    torch.cuda.synchronize()
    for out in (st, y):
        err = float((R.sample(out).cpu() - torch.from_numpy(g['y_sample'])).abs().max())
        assert err <= BAR * max(1.0, float(g['y_stat'][2])), (prec, err)
        s = out.double()
        assert abs(float(s.mean()) - float(g['y_stat'][0])) < 1e-5 and abs(float(s.std()) - float(g['y_stat'][1])) < 1e-5


# ---- the full published layouts ---------------------------------------------------------------------------------------------------

_SD = {}


def _sd(name):
    if name not in _SD:
        cfg = R.BIG_LAMA_REGULAR if name == 'big-lama-regular' else R.LAMA_REGULAR
        _SD[name] = (cfg, R.make_state_dict(cfg, seed=11, calib_hw=32))
    return _SD[name]


@pytest.mark.parametrize('shape', [(8, 512, 512), (1, 1000, 1504)], ids=['8x512', '1x1000x1504'])
@pytest.mark.parametrize('name', ['big-lama-regular', 'lama-regular'])
def test_full_model_matches_torch_restatement(name, shape):
    cfg, sd = _sd(name)
    B, H, W = shape
    x = R.calib_input(B, H, W, seed=31).cuda()
    ref = R.forward(_cuda(sd), cfg, x)
    gen = _gen(cfg, sd, L.PREC_F16X3)
    y = gen(x)
    torch.cuda.synchronize()
    err = float((y - ref).abs().max())
    assert err <= BAR, (name, shape, err)
    paths = gen.conv_paths(x.shape, x.device)
    assert len(paths) == 2 * cfg['n_blocks']
    lib = L.get_lib()
    h, w = H // 8, W // 8
    assert paths == ['winograd' if lib.winograd_preferred(B, 512, 512, h, w, L.PREC_F16X3) else 'direct'] * len(paths)
    if shape[0] == 8:
        assert paths[0] == 'winograd'            # the exact 64 x 64 geometry
        # graph replay: bit-identical to the eager launches
        gen.use_graph = True
        y2 = gen(x)
        y3 = gen(x)
        torch.cuda.synchronize()
        assert torch.equal(y2, y) and torch.equal(y3, y)
        gen.use_graph = False
        # bf16x3 and the direct kernel (Winograd off) on the same input
        gen.set_precision(L.PREC_BF16X3)
        assert float((gen(x) - ref).abs().max()) <= BAR
        gen._exec.winograd = False
        try:
            gen.set_precision(L.PREC_F16X3)
            yd = gen(x)
            assert gen.conv_paths(x.shape, x.device) == ['direct'] * len(paths)
            assert float((yd - ref).abs().max()) <= BAR
        finally:
            gen._exec.winograd = True
    gen.drop_plan(x.shape, x.device)


def test_exact_f32_path():
    cfg, sd = _sd('lama-regular')
    x = R.calib_input(2, 256, 256, seed=32).cuda()
    ref = R.forward(_cuda(sd), cfg, x)
    gen = _gen(cfg, sd, L.PREC_F32)
    y = gen(x)
    assert float((y - ref).abs().max()) <= BAR
    assert gen.conv_paths(x.shape, x.device) == ['direct'] * 18
    with pytest.raises(NotImplementedError):
        gen.set_precision(L.PREC_F16)


def test_plan_cache_eviction():
    cfg = R.small_config(ngf=16, n_blocks=1)
    gen = _gen(cfg, R.make_state_dict(cfg, seed=2), L.PREC_F16X3)
    gen.max_plans = 2
    for h in (64, 72, 80, 64):
        gen(R.calib_input(1, h, 64, seed=h).cuda())
    assert [k[0][2] for k in gen._plans] == [80, 64]


def test_f16_split_overflow_falls_back_to_bf16x3():
    cfg = R.small_config(ngf=16, n_blocks=2)
    sd = R.make_state_dict(cfg, seed=4)
    sd['model.2.bias'] = sd['model.2.bias'].clone()
    sd['model.2.bias'][3] = 2e5                          # one stem channel far beyond 65504: the first downsampling conv splits it
    x = R.calib_input(2, 64, 64, seed=9).cuda()
    for deferred in (False, True):
        gen = _gen(cfg, sd, L.PREC_F16X3)
        gen.defer_range_check = deferred
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            y = gen(x)
            if deferred:
                assert gen.precision == L.PREC_F16X3
                assert gen.check_range() is False        # the caller re-runs
                y = gen(x)
                assert gen.check_range() is True
        assert gen.precision == L.PREC_BF16X3 and any('bf16' in str(m.message) for m in w)
        assert bool(torch.isfinite(y).all())
        ref_gen = _gen(cfg, sd, L.PREC_BF16X3)
        assert torch.equal(y, ref_gen(x))
    gen = _gen(cfg, sd, L.PREC_F16X3)
    gen.auto_fallback = False
    with pytest.raises(L.LamaRangeError):
        gen(x)


# ---- predict CLI --------------------------------------------------------------------------------------------------------------------

def test_predict_cli_regular_model_dir(tmp_path):
    """python -m lama_amd.predict's main() on a model directory of the big-lama-regular layout (config.yaml with an ${env:...} entry,
    models/best.ckpt with foreign keys): PNGs within 1 u8 level of the restatement's predict step."""
    import yaml
    from PIL import Image
    from lama_amd import predict as PR
    from oracle import lama_oracle as O
    cfg, sd = _sd('big-lama-regular')
    raw = dict(run_title='', generator=dict(kind='pix2pixhd_global', **cfg),
               training_model=dict(kind='default', visualize_each_iters=1000, concat_mask=True, store_discr_outputs_for_vis=True),
               losses=dict(l1=dict(weight_missing=0, weight_known=10), resnet_pl=dict(weight=30, weights_path='${env:TORCH_HOME}')))
    mdir = tmp_path / 'model'
    os.makedirs(mdir / 'models')
    with open(mdir / 'config.yaml', 'w') as f:
        yaml.safe_dump(raw, f)
    torch.save({'state_dict': {**{'generator.' + k: v for k, v in sd.items()}, 'discriminator.model0.0.weight': torch.zeros(2),
                               'val_evaluator.x': torch.zeros(1)}}, mdir / 'models' / 'best.ckpt')
    rng = np.random.RandomState(5)
    indir = tmp_path / 'in'
    os.makedirs(indir)
    for i, (h, w) in enumerate([(100, 136), (128, 128), (100, 136)]):
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype('uint8')).save(indir / f'im{i}.png')
        m = np.zeros((h, w), 'uint8')
        m[h // 3: 2 * h // 3, w // 4: w // 2] = 255
        Image.fromarray(m).save(indir / f'im{i}_mask001.png')
    out = tmp_path / 'out'
    assert PR.main([f'model.path={mdir}', f'indir={indir}', f'outdir={out}', 'batch_size=2']) == 0
    sdc = _cuda(sd)
    for mask_path, img_path in PR.list_dataset(str(indir) + os.sep, '.png'):
        rel = os.path.splitext(os.path.basename(mask_path))[0] + '.png'
        got = np.array(Image.open(out / rel))
        image, mask = O.load_image(img_path, 'RGB'), O.load_image(mask_path, 'L')
        h, w = image.shape[1:]
        img = torch.from_numpy(O.pad_img_to_modulo(image, 8))[None].cuda()
        msk = (torch.from_numpy(O.pad_img_to_modulo(mask[None], 8))[None].cuda() > 0).float()
        pred = R.forward(sdc, cfg, torch.cat([img * (1 - msk), msk], 1))
        cur = (msk * pred + (1 - msk) * img)[0].permute(1, 2, 0).cpu().numpy()[:h, :w]
        u8 = np.clip(cur * 255, 0, 255).astype('uint8')
        assert got.shape == u8.shape
        assert np.abs(got.astype(int) - u8.astype(int)).max() <= 1, rel
    with pytest.raises(NotImplementedError):
        PR.main([f'model.path={mdir}', f'indir={indir}', f'outdir={tmp_path / "out_refine"}', 'refine=True'])


# ---- the Winograd conv at 512 output rows (MG = 4) ----------------------------------------------------------------------------------

WINO512 = [
    dict(B=8, H=64, W=64),        # the exact 64 x 64 geometry (GEO 1), 8 x 512^2
    dict(B=1, H=64, W=64),        # ... split-K of a small batch
    dict(B=1, H=32, W=32),        # the exact 32 x 32 geometry, split-K
    dict(B=1, H=135, W=240),      # the any-size geometry: 1080 x 1920
    dict(B=2, H=125, W=188),      # ... 1000 x 1504
]


@pytest.mark.parametrize('prec', ['f16x3', 'bf16x3'])
@pytest.mark.parametrize('case', WINO512, ids=lambda c: f"b{c['B']}_{c['H']}x{c['W']}")
def test_winograd_512_kernel(case, prec):
    """lama_winograd_conv3x3_fwd at cout = cin = 512: bias + ReLU into a fresh tensor, then bias + residual written IN PLACE over the
    residual (y aliasing resid), against torch fp32 and against the direct kernel."""
    lib = L.get_lib()
    p = PRECS[prec]
    B, H, W = case['B'], case['H'], case['W']
    g = torch.Generator().manual_seed(B * H + W)
    x = torch.randn(B, 512, H, W, generator=g).abs().cuda()
    w = (torch.randn(512, 512, 3, 3, generator=g) / 68.0).cuda()
    scale = (0.5 + torch.rand(512, generator=g)).cuda()
    bias = (0.1 * torch.randn(512, generator=g)).cuda()
    assert lib.winograd_supported(512, 512, H, W, p)
    wp = lib.pack_winograd_weight(w, scale, p)
    wd = lib.pack_conv_weight(w, scale, precision=p)
    ws = torch.empty(lib.winograd_workspace_bytes(B, 512, H, W) // 4, device='cuda')
    ref0 = tF.conv2d(tF.pad(x, (1, 1, 1, 1), mode='reflect'), w * scale.view(-1, 1, 1, 1)) + bias.view(1, -1, 1, 1)
    y = torch.full_like(x, 7.0)
    lib.winograd_conv3x3(L.view(x), wp, L.view(y), B, ws, bias, L.ACT_RELU, None, precision=p)
    yd = torch.empty_like(x)
    lib.conv2d(L.view(x), wd, L.view(yd), B, 3, 1, 1, L.PAD_REFLECT, False, bias, L.ACT_RELU, None, precision=p)
    torch.cuda.synchronize()
    ref = torch.relu(ref0)
    tol = 3e-4 * float(ref.abs().max())
    assert float((y - ref).abs().max()) <= tol and float((yd - ref).abs().max()) <= tol
    st = x.clone()
    lib.winograd_conv3x3(L.view(x), wp, L.view(st), B, ws, bias, L.ACT_NONE, L.view(st), precision=p)
    sd_ = x.clone()
    lib.conv2d(L.view(x), wd, L.view(sd_), B, 3, 1, 1, L.PAD_REFLECT, False, bias, L.ACT_NONE, L.view(sd_), precision=p)
    torch.cuda.synchronize()
    ref = x + ref0
    tol = 3e-4 * float(ref.abs().max())
    assert float((st - ref).abs().max()) <= tol and float((sd_ - ref).abs().max()) <= tol
    assert float((st - sd_).abs().max()) <= tol
