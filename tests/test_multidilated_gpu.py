"""GPU tests of the pix2pixhd_multidilated generator (lama-dilated, lama_amd.pix2pixhd.MultiDilatedGlobalGenerator): the golden vectors of the
reference's own MultiDilatedGlobalGenerator / MultidilatedResnetBlock through the C ABI, the multi-dilated kernel at 512 channels against
torch fp32, the range watch, the full model against an fp32 torch restatement built from the same weights, graph replay and the predict CLI."""
import os

import numpy as np
import pytest
import torch

from lama_amd import _lib as L
from lama_amd import pix2pixhd as P
from lama_amd.modules import make_generator
from tests import multidilated_util as M

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
    gen = make_generator(None, kind='pix2pixhd_multidilated', **cfg)
    gen.load_state_dict(sd, strict=True)
    return gen.cuda().set_precision(prec)


def _cuda(sd):
    return {k: v.cuda() for k, v in sd.items()}


# ---- golden vectors of the reference's classes ----------------------------------------------------------------------------------

@pytest.mark.parametrize('prec', list(PRECS), ids=list(PRECS))
def test_small_generator_matches_golden(prec):
    g = np.load(os.path.join(GOLDEN, 'multidilated_small.npz'))
    cfg = M.small_config(ngf=int(g['ngf'][0]), n_blocks=int(g['n_blocks'][0]))
    sd = M.make_state_dict(cfg, seed=int(g['seed'][0]))
    assert abs(sum(float(v.double().sum()) for v in sd.values() if v.is_floating_point()) - float(g['sd_checksum'][0])) < 1e-6 * max(1.0, abs(float(g['sd_checksum'][0])))
    gen = _gen(cfg, sd, PRECS[prec])
    for name in ('a', 'b'):
        x = torch.from_numpy(g[f'{name}_input']).cuda()
        y = gen(x)
        torch.cuda.synchronize()
        err = float((y.cpu() - torch.from_numpy(g[f'{name}_output'])).abs().max())
        print(f'small generator {name} {prec}: max abs error {err:.3g}')
        assert err <= BAR, (prec, name, err)
        assert gen.conv_paths(x.shape, x.device) == ['multidilated'] * 4
    with pytest.raises(L.LamaError, match='72'):
        gen(torch.zeros(1, 4, 64, 96, device='cuda'))


@pytest.mark.parametrize('prec', list(PRECS), ids=list(PRECS))
def test_block512_matches_golden(prec):
    g = np.load(os.path.join(GOLDEN, 'multidilated_block512.npz'))
    sd = M.block_state_dict(512, seed=int(g['seed'][0]))
    import functools
    blk = P.MultidilatedResnetBlock(512, 'reflect', functools.partial(P.MultidilatedConv, comb_mode='cat_in', dilation_num=4), 'bn')
    blk.load_state_dict(sd, strict=True)
    blk.cuda().set_precision(PRECS[prec])
    x = M.block_input(2, 512, 64, seed=int(g['x_seed'][0]))
    assert abs(float(x.double().sum()) - float(g['x_checksum'][0])) < 1e-3
    x = x.cuda()
    st, t = x.clone(), torch.empty_like(x)
    with blk._exec.range_scope(st, blk.precision):
        paths = blk.run(st, t, st)                      # in place over the block input, as the generator's plan runs it
    assert paths == ('multidilated', 'multidilated')
    y = blk(x)                                          # the stand-alone forward: separate output
    torch.cuda.synchronize()
    for out in (st, y):
        err = float((M.sample(out).cpu() - torch.from_numpy(g['y_sample'])).abs().max())
        print(f'block512 {prec}: max abs error of the samples {err:.3g} (absmax {float(g["y_stat"][2]):.3g})')
        assert err <= BAR * max(1.0, float(g['y_stat'][2])), (prec, err)
        s = out.double()
        assert abs(float(s.mean()) - float(g['y_stat'][0])) < 1e-5 and abs(float(s.std()) - float(g['y_stat'][1])) < 1e-5


# ---- the kernel at Cin = Cout = 512, four dilations -----------------------------------------------------------------------------------

PLANES = [(8, 64, 64), (1, 64, 64), (1, 135, 240), (2, 125, 188), (1, 9, 9), (1, 16, 24)]


@pytest.mark.parametrize('prec', list(PRECS), ids=list(PRECS))
@pytest.mark.parametrize('plane', PLANES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_multidilated_512_kernel(plane, prec):
    """lama_multidilated_conv3x3_fwd at cout = cin = 512, G = 4: bias + ReLU into a fresh tensor pre-filled with 7.0, then bias + residual written
    IN PLACE over the residual (y aliasing resid), against torch fp32 per group: 3e-4 max|ref|, the bar test_winograd_512_kernel holds the same
    K at the same arithmetic to."""
    lib = L.get_lib()
    p = PRECS[prec]
    B, H, W = plane
    g = torch.Generator().manual_seed(B * H + W)
    x = torch.randn(B, 512, H, W, generator=g).abs().cuda()
    ws = [(torch.randn(512, 128, 3, 3, generator=g) / 68.0).cuda() for _ in range(4)]
    scale = (0.5 + torch.rand(512, generator=g)).cuda()
    bias = (0.1 * torch.randn(512, generator=g)).cuda()
    wsc = [w * scale.view(-1, 1, 1, 1) for w in ws]
    wp = lib.pack_conv_weight(torch.cat(ws, 1), scale, precision=p)
    y = torch.full_like(x, 7.0)
    lib.multidilated_conv3x3(L.view(x), wp, L.view(y), B, 4, 1, bias, L.ACT_RELU, None, precision=p)
    torch.cuda.synchronize()
    ref = M.mdconv_ref(x, wsc, bias, relu=True)
    tol = 3e-4 * float(ref.abs().max())
    err = float((y - ref).abs().max())
    print(f'mdconv {plane} {prec} relu: max abs error {err:.3g}, bar {tol:.3g}')
    assert err <= tol
    st = x.clone()
    lib.multidilated_conv3x3(L.view(x), wp, L.view(st), B, 4, 1, bias, L.ACT_NONE, L.view(st), precision=p)
    torch.cuda.synchronize()
    ref = M.mdconv_ref(x, wsc, bias, resid=x)
    tol = 3e-4 * float(ref.abs().max())
    err = float((st - ref).abs().max())
    print(f'mdconv {plane} {prec} resid in place: max abs error {err:.3g}, bar {tol:.3g}')
    assert err <= tol


@pytest.mark.parametrize('prec', list(PRECS), ids=list(PRECS))
@pytest.mark.parametrize('plane', [(1, 64, 64), (2, 125, 188), (1, 9, 9)], ids=lambda s: 'x'.join(str(v) for v in s))
def test_one_group_is_the_plain_conv(plane, prec):
    """G = 1 (dilation 1) against lama_conv2d_fwd on the same operands and against torch, within the same bar."""
    lib = L.get_lib()
    p = PRECS[prec]
    B, H, W = plane
    g = torch.Generator().manual_seed(B * H + W + 1)
    x = torch.randn(B, 512, H, W, generator=g).abs().cuda()
    w = (torch.randn(512, 512, 3, 3, generator=g) / 68.0).cuda()
    bias = (0.1 * torch.randn(512, generator=g)).cuda()
    wp = lib.pack_conv_weight(w, None, precision=p)
    y, yd = torch.full_like(x, 7.0), torch.empty_like(x)
    lib.multidilated_conv3x3(L.view(x), wp, L.view(y), B, 1, 1, bias, L.ACT_RELU, None, precision=p)
    lib.conv2d(L.view(x), wp, L.view(yd), B, 3, 1, 1, L.PAD_REFLECT, False, bias, L.ACT_RELU, None, precision=p)
    torch.cuda.synchronize()
    ref = M.mdconv_ref(x, [w], bias, relu=True)
    tol = 3e-4 * float(ref.abs().max())
    assert float((y - ref).abs().max()) <= tol and float((y - yd).abs().max()) <= tol


def test_range_flag():
    lib = L.get_lib()
    x = torch.randn(1, 512, 16, 24, generator=torch.Generator().manual_seed(1)).cuda()
    wp = lib.pack_conv_weight(torch.zeros(512, 512, 3, 3, device='cuda'), None, precision=L.PREC_F16X3)
    y, flag = torch.empty_like(x), torch.zeros(1, dtype=torch.int32, device='cuda')
    lib.multidilated_conv3x3(L.view(x), wp, L.view(y), 1, 4, 1, precision=L.PREC_F16X3, range_flag=flag)
    assert int(flag.item()) == 0
    x[0, 300, 7, 11] = 1e5
    lib.multidilated_conv3x3(L.view(x), wp, L.view(y), 1, 4, 1, precision=L.PREC_F16X3, range_flag=flag)
    assert int(flag.item()) == 1
    flag.zero_()
    lib.multidilated_conv3x3(L.view(x), lib.pack_conv_weight(torch.zeros(512, 512, 3, 3, device='cuda'), None, precision=L.PREC_BF16X3), L.view(y),
                             1, 4, 1, precision=L.PREC_BF16X3, range_flag=flag)
    assert int(flag.item()) == 0
    with pytest.raises(L.LamaError) as e:                  # an 8 x 12 plane has no reflect padding of 8
        lib.multidilated_conv3x3(L.view(x[:, :, :8, :12].contiguous()), wp, L.view(y[:, :, :8, :12].contiguous()), 1, 4, 1, precision=L.PREC_F16X3)
    assert e.value.code == L.ERR_UNSUPPORTED


# ---- the full published layout --------------------------------------------------------------------------------------------------------

_SD = {}


def _sd():
    if not _SD:
        _SD['sd'] = M.make_state_dict(M.LAMA_DILATED, seed=11)
    return M.LAMA_DILATED, _SD['sd']


@pytest.mark.parametrize('shape', [(8, 512, 512), (1, 1000, 1504)], ids=['8x512', '1x1000x1504'])
def test_full_model_matches_torch_restatement(shape):
    cfg, sd = _sd()
    B, H, W = shape
    x = M.calib_input(B, H, W, seed=31).cuda()
    ref = M.forward(_cuda(sd), cfg, x)
    gen = _gen(cfg, sd, L.PREC_F16X3)
    y = gen(x)
    torch.cuda.synchronize()
    err = float((y - ref).abs().max())
    print(f'lama-dilated {shape} f16x3: max abs error {err:.3g}')
    assert err <= BAR, (shape, err)
    assert gen.conv_paths(x.shape, x.device) == ['multidilated'] * 18
    if shape[0] == 8:
        gen.use_graph = True                     # graph replay: bit-identical to the eager launches
        y2 = gen(x)
        y3 = gen(x)
        torch.cuda.synchronize()
        assert torch.equal(y2, y) and torch.equal(y3, y)
        gen.use_graph = False
        gen.set_precision(L.PREC_BF16X3)
        err = float((gen(x) - ref).abs().max())
        print(f'lama-dilated {shape} bf16x3: max abs error {err:.3g}')
        assert err <= BAR
    gen.drop_plan(x.shape, x.device)


def test_exact_f32_path():
    cfg, sd = _sd()
    x = M.calib_input(2, 256, 256, seed=32).cuda()
    ref = M.forward(_cuda(sd), cfg, x)
    gen = _gen(cfg, sd, L.PREC_F32)
    y = gen(x)
    err = float((y - ref).abs().max())
    print(f'lama-dilated 2 x 256^2 f32: max abs error {err:.3g}')
    assert err <= BAR
    assert gen.conv_paths(x.shape, x.device) == ['multidilated'] * 18
    with pytest.raises(NotImplementedError):
        gen.set_precision(L.PREC_F16)


# ---- predict CLI --------------------------------------------------------------------------------------------------------------------

def test_predict_cli_dilated_model_dir(tmp_path):
    """python -m lama_amd.predict's main() on a model directory of the lama-dilated layout (config.yaml with the nested multidilation_kwargs
    and an ${env:...} entry, models/best.ckpt with foreign keys): PNGs within 1 u8 level of the restatement's predict step."""
    import yaml
    from PIL import Image
    from lama_amd import predict as PR
    from oracle import lama_oracle as O
    cfg, sd = _sd()
    raw = dict(run_title='', generator=dict(kind='pix2pixhd_multidilated', **cfg),
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
        pred = M.forward(sdc, cfg, torch.cat([img * (1 - msk), msk], 1))
        cur = (msk * pred + (1 - msk) * img)[0].permute(1, 2, 0).cpu().numpy()[:h, :w]
        u8 = np.clip(cur * 255, 0, 255).astype('uint8')
        assert got.shape == u8.shape
        assert np.abs(got.astype(int) - u8.astype(int)).max() <= 1, rel
    with pytest.raises(NotImplementedError):
        PR.main([f'model.path={mdir}', f'indir={indir}', f'outdir={tmp_path / "out_refine"}', 'refine=True'])
