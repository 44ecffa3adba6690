"""CPU tests of the pix2pixhd_global generator (lama_amd.pix2pixhd): the reference's state-dict layout, checkpoint loading, the options
that are refused, and the launch plan driven through the host SIMT emulator (tests/hipemu) against the reference-generated golden
vectors -- with the Winograd conv at 512 output rows (four row groups) among the emulated kernels."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as tF
import yaml

from lama_amd import _lib as L
from lama_amd import config as lcfg
from lama_amd import ffc as F
from lama_amd import pix2pixhd as P
from lama_amd import trainers
from lama_amd.modules import make_generator
from tests import regular_util as R
from tests.emu import emu_lib


def _keys(golden_dir, name):
    g = np.load(os.path.join(golden_dir, 'regular_keys.npz'))
    return {k: tuple(int(d) for d in s.split(',') if d) for k, s in zip(g[name + '_keys'], g[name + '_shapes'])}


@pytest.mark.parametrize('name,cfg', [('big', R.BIG_LAMA_REGULAR), ('regular', R.LAMA_REGULAR)], ids=['big-lama-regular', 'lama-regular'])
def test_state_dict_matches_reference_layout(golden_dir, name, cfg):
    gen = make_generator(None, kind='pix2pixhd_global', **cfg)
    assert isinstance(gen, P.GlobalGenerator)
    want = _keys(golden_dir, name)
    got = {k: tuple(v.shape) for k, v in gen.state_dict().items()}
    assert got == want
    assert list(gen.state_dict().keys()) == list(want.keys())
    assert 'model.13.conv_block.1.weight' in got and 'model.13.conv_block.2.running_mean' in got
    assert R.state_dict_keys(cfg) == want          # the layout the synthetic weights of the tests are generated from


def test_synthetic_checkpoint_with_foreign_keys_loads(tmp_path):
    """A big-lama-regular checkpoint (generator + discriminator / evaluator keys) through trainers.load_checkpoint: strict=False drops the
    foreign keys, strict=True refuses them, a missing generator key is an error."""
    raw = dict(run_title='', generator=dict(kind='pix2pixhd_global', **R.BIG_LAMA_REGULAR),
               training_model=dict(kind='default', visualize_each_iters=1000, concat_mask=True, store_discr_outputs_for_vis=True),
               losses=dict(resnet_pl=dict(weight=30, weights_path='${env:TORCH_HOME}')))
    with open(tmp_path / 'config.yaml', 'w') as f:
        yaml.safe_dump(raw, f)
    cfg = lcfg.load_train_config(str(tmp_path / 'config.yaml'))
    keys = R.state_dict_keys(R.BIG_LAMA_REGULAR)
    g = torch.Generator().manual_seed(0)
    sd = {'generator.' + k: (torch.randn(s, generator=g) if s else torch.tensor(0)) for k, s in keys.items()}
    sd['generator.model.2.running_var'] = sd['generator.model.2.running_var'].abs()
    ckpt = tmp_path / 'best.ckpt'
    torch.save({'state_dict': {**sd, 'discriminator.model0.0.weight': torch.zeros(3), 'val_evaluator.x': torch.zeros(1)}}, ckpt)
    model = trainers.load_checkpoint(cfg, str(ckpt), strict=False, map_location='cpu')
    assert isinstance(model.generator, P.GlobalGenerator) and len(model.generator.model) == 13 + 15 + 12
    assert torch.equal(model.generator.model[13].conv_block[5].bias, sd['generator.model.13.conv_block.5.bias'])
    with pytest.raises(RuntimeError):
        trainers.load_checkpoint(cfg, str(ckpt), strict=True, map_location='cpu')
    torch.save({'state_dict': sd}, ckpt)
    trainers.load_checkpoint(cfg, str(ckpt), strict=True, map_location='cpu')
    del sd['generator.model.20.conv_block.6.running_mean']
    torch.save({'state_dict': sd}, ckpt)
    with pytest.raises(RuntimeError):
        trainers.load_checkpoint(cfg, str(ckpt), strict=False, map_location='cpu')


@pytest.mark.parametrize('kw', [dict(dilated_blocks_n=2), dict(dilated_blocks_n_start=1), dict(dilated_blocks_n_middle=1), dict(ffc_positions=[1]),
                                dict(is_resblock_depthwise=True), dict(conv_kind='depthwise'), dict(affine=True), dict(padding_type='zero'),
                                dict(norm_layer='in'), dict(up_norm_layer=nn.InstanceNorm2d), dict(dilation=2), dict(second_dilation=2)],
                         ids=lambda kw: next(iter(kw)))
def test_unsupported_options_raise(kw):
    with pytest.raises(NotImplementedError):
        make_generator(None, kind='pix2pixhd_global', **{**R.small_config(ngf=4, n_blocks=1), **kw})


def test_multidilated_stays_unsupported_and_f16_refused():
    with pytest.raises(NotImplementedError):
        make_generator(None, kind='pix2pixhd_multidilated', input_nc=4, output_nc=3)
    gen = make_generator(None, kind='pix2pixhd_global', **R.small_config(ngf=4, n_blocks=1))
    with pytest.raises(NotImplementedError):
        gen.set_precision(L.PREC_F16)
    assert gen.tune_split((8, 4, 512, 512), 'cpu') == 1 and gen.split_batch == 1


def test_refine_refuses_regular_generator():
    from lama_amd.refinement import refine_predict
    model = trainers.DefaultInpaintingTrainingModule(dict(generator=dict(kind='pix2pixhd_global', **R.small_config(ngf=4, n_blocks=1))))
    batch = dict(image=torch.zeros(1, 3, 64, 64), mask=torch.zeros(1, 1, 64, 64), unpad_to_size=[torch.tensor([64]), torch.tensor([64])])
    with pytest.raises(NotImplementedError, match='ffc_resnet'):
        refine_predict(batch, model, gpu_ids='0,', modulo=8, n_iters=1, lr=0.002, min_side=64, max_scales=1, px_budget=10 ** 6)


@pytest.fixture(scope='module')
def small(golden_dir):
    g = np.load(os.path.join(golden_dir, 'regular_small.npz'))
    cfg = R.small_config(ngf=int(g['ngf'][0]), n_blocks=int(g['n_blocks'][0]))
    sd = R.make_state_dict(cfg, seed=int(g['seed'][0]), calib_hw=32)
    ck = float(g['sd_checksum'][0])
    assert abs(sum(float(v.double().sum()) for v in sd.values() if v.is_floating_point()) - ck) < 1e-6 * max(1.0, abs(ck))
    gen = make_generator(None, kind='pix2pixhd_global', **cfg)
    gen.load_state_dict(sd, strict=True)
    gen.set_exec(F._Exec(emu_lib()))
    return g, cfg, sd, gen


@pytest.mark.parametrize('prec', [L.PREC_F16X3, L.PREC_BF16X3, L.PREC_F32], ids=['f16x3', 'bf16x3', 'f32'])
def test_small_generator_matches_golden_emulated(small, prec):
    g, cfg, sd, gen = small
    gen.set_precision(prec)
    x = torch.from_numpy(g['b_input'])                 # 2 x 56 x 72: a 7 x 9 bottleneck plane (the any-size Winograd geometry)
    y = gen(x)
    assert float((y - torch.from_numpy(g['b_output'])).abs().max()) <= 2e-4
    paths = gen.conv_paths(x.shape, x.device)
    lib = gen._exec.lib
    want = 'winograd' if prec != L.PREC_F32 and lib.winograd_preferred(2, 128, 128, 7, 9, prec) else 'direct'
    assert paths == [want] * 4
    if prec == L.PREC_F16X3:
        ex = gen._exec
        ex.winograd = False                             # the direct kernel for every block conv: the same function
        try:
            gen._invalidate()
            yd = gen(x)
            assert gen.conv_paths(x.shape, x.device) == ['direct'] * 4
            assert float((yd - y).abs().max()) <= 2e-4
        finally:
            ex.winograd = True
            gen._invalidate()


def test_layerwise_forward_matches_plan_emulated(small):
    g, cfg, sd, gen = small
    gen.set_precision(L.PREC_F16X3)
    x = torch.from_numpy(g['a_input'][:, :, :32, :40]).contiguous()
    y = gen(x)
    assert float((gen.model(x) - y).abs().max()) <= 1e-5          # generator.model as the reference's nn.Sequential, layer by layer
    assert float((y - R.forward(sd, cfg, x)).abs().max()) <= 2e-4


# the Winograd F(2x2, 3x3) conv at cout = 512 (four 128-row groups, MG = 4): bias + ReLU into a fresh tensor and bias + residual written in
# place over the residual, the exact geometries (W = 32 / 64) and the any-size one, both split precisions
WINO512 = [dict(B=1, cin=32, H=16, W=32), dict(B=1, cin=32, H=8, W=64), dict(B=2, cin=64, H=5, W=9)]


@pytest.mark.parametrize('prec', [L.PREC_F16X3, L.PREC_BF16X3], ids=['f16x3', 'bf16x3'])
@pytest.mark.parametrize('case', WINO512, ids=lambda c: f"b{c['B']}c{c['cin']}_{c['H']}x{c['W']}")
def test_winograd_cout512_emulated(case, prec):
    lib = emu_lib()
    B, cin, H, W = case['B'], case['cin'], case['H'], case['W']
    g = torch.Generator().manual_seed(H * W + cin)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(512, cin, 3, 3, generator=g) * 0.1
    scale, bias = torch.rand(512, generator=g) + 0.5, torch.randn(512, generator=g)
    resid = torch.randn(B, 512, H, W, generator=g)
    ref = tF.conv2d(tF.pad(x, (1, 1, 1, 1), mode='reflect'), w * scale.view(-1, 1, 1, 1)) + bias.view(1, -1, 1, 1)
    assert lib.winograd_supported(512, cin, H, W, prec)
    wp = lib.pack_winograd_weight(w, scale, prec)
    ws = torch.zeros(lib.winograd_workspace_bytes(B, 512, H, W) // 4)
    tol = dict(atol=1.2e-3, rtol=4e-4) if prec == L.PREC_BF16X3 else dict(atol=3e-4, rtol=1e-4)
    y = torch.full((B, 512, H, W), 7.0)
    lib.winograd_conv3x3(L.view(x), wp, L.view(y), B, ws, bias, L.ACT_RELU, None, precision=prec)
    assert torch.allclose(y, ref.relu(), **tol), float((y - ref.relu()).abs().max())
    st = resid.clone()                                                    # y aliasing resid
    lib.winograd_conv3x3(L.view(x), wp, L.view(st), B, ws, bias, L.ACT_NONE, L.view(st), precision=prec)
    assert torch.allclose(st, ref + resid, **tol), float((st - ref - resid).abs().max())
    sd_ = resid.clone()                                                   # ... and the direct kernel, in place as well
    lib.conv2d(L.view(x), lib.pack_conv_weight(w, scale, precision=prec), L.view(sd_), B, 3, 1, 1, L.PAD_REFLECT, False, bias, L.ACT_NONE,
               L.view(sd_), precision=prec)
    assert torch.allclose(sd_, ref + resid, **tol)


# ---- lama_winograd_preferred: the cost model of the any-size geometry (conv_split3.inc), restated ------------------------------------------

def _wg_bands(H, W):
    """(generic, bands) of wg_shape."""
    if W in (32, 64, 128, 256):
        tcl = (W // 2).bit_length() - 1
        rb = 128 >> tcl
        if H >= 2 * rb and H % (2 * rb) == 0:
            return 0, H // (2 * rb)
    qw, tr = (W + 3) >> 2, (H + 1) >> 1
    best, best_cost = 0, 0
    for qr in (32, 16, 8):
        nseg = 1 if qw <= qr else (qw - 1 + qr - 2) // (qr - 1)
        if not best or nseg * qr < best_cost:
            best, best_cost = qr, nseg * qr
    nseg = 1 if qw <= best else (qw - 1 + best - 2) // (best - 1)
    return 1, -(-(tr * nseg) // (64 // best))


def _ksplit(units):
    if units <= 256:
        return 1 if units >= 128 else (2 if units >= 64 else 4)
    best, best_t = 1, 0.0
    for ks in (1, 2, 4):
        t = ((units * ks + 255) // 256) * (8.0 + 45.0 / ks) + 5.0 * (ks - 1)
        if ks == 1 or t < best_t - 1e-9:
            best, best_t = ks, t
    return best


def _preferred(B, cout, H, W, refit=True):
    generic, bands = _wg_bands(H, W)
    if not generic:
        return True
    mg = cout // 128
    units = B * bands * 4 * mg
    ks = _ksplit(units)
    px = B * H * W / 32768.0
    tiles = 0
    for tl in (5, 4, 3):
        nt = B * -(-W // (1 << tl)) * -(-H // (128 >> tl))
        if not tiles or (nt + 255) // 256 < (tiles + 255) // 256:
            tiles = nt
    rounds_d = (tiles * mg + 255) // 256
    if mg > 1 and refit:
        return ((units * ks + 255) // 256) * (8.0 + 52.0 / ks) + px * (14.0 + 5.0 * (ks - 1)) < rounds_d * 88.0
    return ((units * ks + 255) // 256) * (8.0 + 45.0 / ks) + px * (14.0 + 5.0 * (ks - 1)) < 0.92 * rounds_d * 92.0


def test_winograd_preferred_cost_model():
    """cout = 128 (the FFC local conv) keeps the round-6 answers; cout = 512 (four row groups) follows the constants refitted on the hardware
    timings of profiles/regular_conv512.txt -- which differ from the 128-row ones on real plane shapes."""
    lib = emu_lib()
    planes = [(h, w) for h in (5, 9, 17, 32, 45, 64, 67, 100, 125, 135, 168, 191) for w in (8, 23, 32, 40, 64, 94, 100, 125, 168, 188, 240, 256)]
    differ = []
    for B in (1, 2, 3, 4, 8):
        for H, W in planes:
            for prec in (L.PREC_F16X3, L.PREC_BF16X3):
                assert bool(lib.winograd_preferred(B, 128, 512, H, W, prec)) == _preferred(B, 128, H, W), (B, H, W)
                assert bool(lib.winograd_preferred(B, 512, 512, H, W, prec)) == _preferred(B, 512, H, W), (B, H, W)
            if _preferred(B, 512, H, W) != _preferred(B, 512, H, W, refit=False):
                differ.append((B, H, W))
    assert differ
    # the 12 shapes timed on hardware: Winograd was faster on every one of them
    for B, H, W in ((8, 64, 64), (1, 64, 64), (1, 32, 32), (8, 32, 32), (1, 135, 240), (2, 135, 240), (8, 135, 240), (1, 125, 188), (2, 125, 188),
                    (8, 125, 188), (1, 168, 168), (4, 100, 100)):
        assert lib.winograd_preferred(B, 512, 512, H, W, L.PREC_F16X3)
