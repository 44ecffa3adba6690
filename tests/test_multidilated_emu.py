"""CPU tests of the pix2pixhd_multidilated generator (lama_amd.pix2pixhd.MultiDilatedGlobalGenerator, the lama-dilated checkpoint): the
reference's state-dict layout, checkpoint loading, the options that are refused, the planes that have no reflect padding, and the launch plan
and the multi-dilated kernel driven through the host SIMT emulator (tests/hipemu) against the reference-generated golden vectors."""
import os

import numpy as np
import pytest
import torch
import yaml

from lama_amd import _lib as L
from lama_amd import config as lcfg
from lama_amd import ffc as F
from lama_amd import pix2pixhd as P
from lama_amd import trainers
from lama_amd.modules import make_generator
from tests import multidilated_util as M
from tests.emu import emu_lib


def _keys(golden_dir):
    g = np.load(os.path.join(golden_dir, 'multidilated_keys.npz'))
    return {k: tuple(int(d) for d in s.split(',') if d) for k, s in zip(g['dilated_keys'], g['dilated_shapes'])}


def test_abi_version_and_entry():
    lib = emu_lib()
    assert L.ABI_VERSION == 112 and lib._l.lama_version() == 112
    assert lib._l.lama_multidilated_conv3x3_fwd.argtypes is not None


def test_state_dict_matches_reference_layout(golden_dir):
    gen = make_generator(None, kind='pix2pixhd_multidilated', **M.LAMA_DILATED)
    assert isinstance(gen, P.MultiDilatedGlobalGenerator) and isinstance(gen, P.GlobalGenerator)
    want = _keys(golden_dir)
    got = {k: tuple(v.shape) for k, v in gen.state_dict().items()}
    assert got == want
    assert list(gen.state_dict().keys()) == list(want.keys())
    assert got['model.13.conv_block.0.convs.3.weight'] == (512, 128, 3, 3) and 'model.13.conv_block.4.running_mean' in got
    assert M.state_dict_keys(M.LAMA_DILATED) == want          # the layout the synthetic weights of the tests are generated from
    assert gen.min_input_side == 72 and gen.split_batch == 1 and gen.tune_split((8, 4, 512, 512), 'cpu') == 1
    with pytest.raises(NotImplementedError):
        gen.set_precision(L.PREC_F16)


def test_synthetic_checkpoint_with_foreign_keys_loads(tmp_path):
    """A lama-dilated model directory's config.yaml (nested multidilation_kwargs) + a checkpoint with discriminator / evaluator keys through
    trainers.load_checkpoint."""
    raw = dict(run_title='', generator=dict(kind='pix2pixhd_multidilated', **M.LAMA_DILATED),
               training_model=dict(kind='default', visualize_each_iters=1000, concat_mask=True, store_discr_outputs_for_vis=True),
               losses=dict(resnet_pl=dict(weight=30, weights_path='${env:TORCH_HOME}')))
    with open(tmp_path / 'config.yaml', 'w') as f:
        yaml.safe_dump(raw, f)
    cfg = lcfg.load_train_config(str(tmp_path / 'config.yaml'))
    keys = M.state_dict_keys(M.LAMA_DILATED)
    g = torch.Generator().manual_seed(0)
    sd = {'generator.' + k: (torch.randn(s, generator=g) if s else torch.tensor(0)) for k, s in keys.items()}
    ckpt = tmp_path / 'best.ckpt'
    torch.save({'state_dict': {**sd, 'discriminator.model0.0.weight': torch.zeros(3), 'val_evaluator.x': torch.zeros(1)}}, ckpt)
    model = trainers.load_checkpoint(cfg, str(ckpt), strict=False, map_location='cpu')
    assert isinstance(model.generator, P.MultiDilatedGlobalGenerator) and len(model.generator.model) == 13 + 9 + 12
    assert torch.equal(model.generator.model[13].conv_block[3].convs[2].bias, sd['generator.model.13.conv_block.3.convs.2.bias'])
    assert [c.dilation for c in model.generator.model[21].conv_block[0].convs] == [(1, 1), (2, 2), (4, 4), (8, 8)]
    with pytest.raises(RuntimeError):
        trainers.load_checkpoint(cfg, str(ckpt), strict=True, map_location='cpu')
    del sd['generator.model.20.conv_block.0.convs.1.weight']
    torch.save({'state_dict': sd}, ckpt)
    with pytest.raises(RuntimeError):
        trainers.load_checkpoint(cfg, str(ckpt), strict=False, map_location='cpu')


@pytest.mark.parametrize('kw', [dict(multidilation_kwargs=dict(comb_mode='sum', dilation_num=4)), dict(multidilation_kwargs=dict(comb_mode='cat_out', dilation_num=4)),
                                dict(multidilation_kwargs=dict(comb_mode='cat_both', dilation_num=4)), dict(multidilation_kwargs={}),
                                dict(multidilation_kwargs=dict(comb_mode='cat_in', dilation_num=4, equal_dim=False)),
                                dict(multidilation_kwargs=dict(comb_mode='cat_in', dilation_num=4, shared_weights=True)),
                                dict(multidilation_kwargs=dict(comb_mode='cat_in', dilation_num=4, shuffle_in_channels=True)),
                                dict(multidilation_kwargs=dict(comb_mode='cat_in', dilation_num=4, use_depthwise=True)),
                                dict(multidilation_kwargs=dict(comb_mode='cat_in', dilation_num=4, min_dilation=2)),
                                dict(deconv_kind='bilinear'), dict(ffc_positions=[1]), dict(affine=True), dict(norm_layer='in'), dict(padding_type='zero')],
                         ids=['sum', 'cat_out', 'cat_both', 'default_kwargs', 'equal_dim', 'shared_weights', 'shuffle_in_channels', 'use_depthwise',
                              'min_dilation', 'deconv_kind', 'ffc_positions', 'affine', 'norm_layer', 'padding_type'])
def test_unsupported_options_raise(kw):
    with pytest.raises(NotImplementedError):
        make_generator(None, kind='pix2pixhd_multidilated', **{**M.small_config(ngf=16, n_blocks=1), **kw})


def test_refine_refuses_multidilated_generator():
    from lama_amd.refinement import refine_predict
    model = trainers.DefaultInpaintingTrainingModule(dict(generator=dict(kind='pix2pixhd_multidilated', **M.small_config(ngf=16, n_blocks=1))))
    batch = dict(image=torch.zeros(1, 3, 96, 96), mask=torch.zeros(1, 1, 96, 96), unpad_to_size=[torch.tensor([96]), torch.tensor([96])])
    with pytest.raises(NotImplementedError, match='ffc_resnet'):
        refine_predict(batch, model, gpu_ids='0,', modulo=8, n_iters=1, lr=0.002, min_side=96, max_scales=1, px_budget=10 ** 6)


@pytest.fixture(scope='module')
def small(golden_dir):
    g = np.load(os.path.join(golden_dir, 'multidilated_small.npz'))
    cfg = M.small_config(ngf=int(g['ngf'][0]), n_blocks=int(g['n_blocks'][0]))
    sd = M.make_state_dict(cfg, seed=int(g['seed'][0]))
    ck = float(g['sd_checksum'][0])
    assert abs(sum(float(v.double().sum()) for v in sd.values() if v.is_floating_point()) - ck) < 1e-6 * max(1.0, abs(ck))
    gen = make_generator(None, kind='pix2pixhd_multidilated', **cfg)
    gen.load_state_dict(sd, strict=True)
    gen.set_exec(F._Exec(emu_lib()))
    return g, cfg, sd, gen


def test_small_plane_is_refused(small):
    """A 64 x 96 input has an 8 x 12 bottleneck plane: no reflect padding of 8 (the reference raises 'Padding size should be less than the
    corresponding input dimension'); the generator names the minimum side, the C entry returns LAMA_ERR_UNSUPPORTED."""
    g, cfg, sd, gen = small
    with pytest.raises(L.LamaError, match='72'):
        gen(torch.zeros(1, 4, 64, 96))
    lib = emu_lib()
    x, y = torch.zeros(1, 64, 8, 12), torch.zeros(1, 32, 8, 12)
    wp = lib.pack_conv_weight(torch.zeros(32, 64, 3, 3), None, precision=L.PREC_F16X3)
    with pytest.raises(L.LamaError) as e:
        lib.multidilated_conv3x3(L.view(x), wp, L.view(y), 1, 4, 1, precision=L.PREC_F16X3)
    assert e.value.code == L.ERR_UNSUPPORTED
    lib.multidilated_conv3x3(L.view(x), wp, L.view(y), 1, 2, 1, precision=L.PREC_F16X3)          # d_max = 2 fits
    with pytest.raises(L.LamaError) as e:                                                         # Cin / G not a multiple of 16
        lib.multidilated_conv3x3(L.view(torch.zeros(1, 32, 9, 12)), wp, L.view(torch.zeros(1, 32, 9, 12)), 1, 4, 1, precision=L.PREC_F16X3)
    assert e.value.code == L.ERR_UNSUPPORTED


@pytest.mark.parametrize('prec', [L.PREC_F16X3, L.PREC_BF16X3, L.PREC_F32], ids=['f16x3', 'bf16x3', 'f32'])
def test_small_generator_matches_golden_emulated(small, prec):
    g, cfg, sd, gen = small
    gen.set_precision(prec)
    x = torch.from_numpy(g['b_input'])                 # 2 x 72 x 88: a 9 x 11 bottleneck plane, reflection at pad 8 = H - 1
    y = gen(x)
    err = float((y - torch.from_numpy(g['b_output'])).abs().max())
    print(f'small generator, precision {prec}: max abs error {err:.3g}')
    assert err <= 2e-4
    assert gen.conv_paths(x.shape, x.device) == ['multidilated'] * 4


def test_layerwise_forward_matches_plan_emulated(small):
    g, cfg, sd, gen = small
    gen.set_precision(L.PREC_F16X3)
    x = torch.from_numpy(g['a_input'][:, :, :72, :80]).contiguous()
    y = gen(x)
    assert float((gen.model(x) - y).abs().max()) <= 1e-5          # generator.model as the reference's nn.Sequential, layer by layer
    assert float((y - M.forward(sd, cfg, x)).abs().max()) <= 2e-4


# the kernel alone: bias + ReLU into a fresh tensor and bias + residual written in place over the residual.  K = 9 * Cin <= 1152 products of
# O(1) operands: the 3-term split leaves 2^-22 (f16) / 2^-16 (bf16) per product relative to max|ref|, the bars of test_winograd_cout512_emulated
KERNEL = [dict(G=1, cpg=32, cout=64, B=1, H=3, W=7), dict(G=2, cpg=32, cout=160, B=2, H=5, W=20), dict(G=4, cpg=16, cout=32, B=1, H=9, W=11),
          dict(G=4, cpg=32, cout=128, B=1, H=17, W=9)]


@pytest.mark.parametrize('prec', [L.PREC_F16X3, L.PREC_BF16X3, L.PREC_F32], ids=['f16x3', 'bf16x3', 'f32'])
@pytest.mark.parametrize('case', KERNEL, ids=lambda c: f"g{c['G']}c{c['cpg']}o{c['cout']}_{c['B']}x{c['H']}x{c['W']}")
def test_multidilated_kernel_emulated(case, prec):
    lib = emu_lib()
    G, cpg, cout, B, H, W = (case[k] for k in ('G', 'cpg', 'cout', 'B', 'H', 'W'))
    g = torch.Generator().manual_seed(G * 100 + H * W)
    x = torch.randn(B, G * cpg, H, W, generator=g)
    ws = [torch.randn(cout, cpg, 3, 3, generator=g) * 0.1 for _ in range(G)]
    scale, bias = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    resid = torch.randn(B, cout, H, W, generator=g)
    wsc = [w * scale.view(-1, 1, 1, 1) for w in ws]
    wp = lib.pack_conv_weight(torch.cat(ws, 1), scale, precision=prec)
    tol = dict(atol=1.2e-3, rtol=4e-4) if prec == L.PREC_BF16X3 else dict(atol=3e-4, rtol=1e-4)
    y = torch.full((B, cout, H, W), 7.0)
    lib.multidilated_conv3x3(L.view(x), wp, L.view(y), B, G, 1, bias, L.ACT_RELU, None, precision=prec)
    ref = M.mdconv_ref(x, wsc, bias, relu=True)
    assert torch.allclose(y, ref, **tol), float((y - ref).abs().max())
    st = resid.clone()                                                    # y aliasing resid
    lib.multidilated_conv3x3(L.view(x), wp, L.view(st), B, G, 1, bias, L.ACT_NONE, L.view(st), precision=prec)
    ref = M.mdconv_ref(x, wsc, bias, resid=resid)
    assert torch.allclose(st, ref, **tol), float((st - ref).abs().max())
    if G == 1:                                                            # one group of dilation 1 is the plain 3x3 reflect conv
        yd = resid.clone()
        lib.conv2d(L.view(x), wp, L.view(yd), B, 3, 1, 1, L.PAD_REFLECT, False, bias, L.ACT_NONE, L.view(yd), precision=prec)
        assert torch.allclose(st, yd, **tol)


def test_range_flag_emulated():
    lib = emu_lib()
    x = torch.randn(1, 64, 9, 9, generator=torch.Generator().manual_seed(1))
    wp = lib.pack_conv_weight(torch.zeros(32, 64, 3, 3), None, precision=L.PREC_F16X3)
    y, flag = torch.zeros(1, 32, 9, 9), torch.zeros(1, dtype=torch.int32)
    lib.multidilated_conv3x3(L.view(x), wp, L.view(y), 1, 4, 1, precision=L.PREC_F16X3, range_flag=flag)
    assert int(flag) == 0
    x[0, 50, 4, 4] = 1e5
    lib.multidilated_conv3x3(L.view(x), wp, L.view(y), 1, 4, 1, precision=L.PREC_F16X3, range_flag=flag)
    assert int(flag) == 1
