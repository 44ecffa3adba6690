"""GPU tests of batched refinement: the explicit reverse pass (lama_amd/backward.py) at batch 3 against three batch-1 runs,
refine_predict_batch against the oracle and the big-lama golden, and ``refine=True refiner.batch_size=N`` of the predict CLI."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from lama_amd import _lib as L
from lama_amd import refinement as RF
from lama_amd import trainers
from lama_amd.backward import RearPass
from lama_amd.modules import make_generator
from oracle import lama_oracle as O
from oracle import refine_oracle as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def big2():
    """big-lama channel counts, two resnet blocks (as test_refinement_gpu.py's fixture of the same name)."""
    cfg = dict(O.BIG_LAMA)
    cfg['n_blocks'] = 2
    sd = O.make_synthetic_state_dict(cfg, seed=2, calib_hw=64)
    gen = make_generator(None, kind='ffc_resnet', **cfg)
    gen.load_state_dict(sd, strict=True)
    gen.cuda().set_precision(L.PREC_F32)
    return cfg, gen


@pytest.mark.parametrize('hw,precs,bar', [((2048, 2048), (L.PREC_F32, L.PREC_F32), 5e-5), ((1000, 1504), (L.PREC_F32, L.PREC_F32), 5e-5),
                                           ((256, 256), (L.PREC_F16X3, L.PREC_BF16X3), 3e-4)],
                         ids=['planes256_masked_fft', 'planes125x188', 'planes32_winograd_dgrad_default_precisions'])
def test_rear_pass_batch3_equals_three_batch1_runs(big2, hw, precs, bar):
    """RearPass forward + reverse at batch 3 (three different images) against the same three images one by one: 256 x 256 planes (the
    masked-transform entries of the reverse pass) and a plane with a large prime (mixed-radix transforms, ragged dgrad tiles) in exact
    fp32 with the bars of test_rear_gradients_strict_* (relative L2 5e-5, 2.5e-4 of the largest element per image); 32 x 32 planes in the
    default precisions (the zero-pad Winograd dgrad + frame, whose split-K geometry follows the launch size) with the default-precision bar
    of test_rear_gradients_18_blocks_strict (3e-4, 5x that for the largest element)."""
    cfg, gen = big2
    fri = R.first_resblock_index(cfg)
    H, W = hw
    gen.set_precision(precs[0])
    try:
        _rear_pass_batch3(cfg, gen, fri, H, W, precs[1], bar)
    finally:
        gen.set_precision(L.PREC_F32)


def _rear_pass_batch3(cfg, gen, fri, H, W, bwd_prec, bar):
    batch = O.make_synthetic_batch(3, H, W, seed=12)
    x = torch.cat([batch['image'] * (1 - batch['mask']), batch['mask']], 1).cuda()
    with torch.no_grad():
        z = RF._state_buffer(gen.model[0:fri](x))
    assert tuple(z.shape) == (3, 512, H // 8, W // 8)
    gw = (torch.randn((3, 3, H, W), generator=torch.Generator().manual_seed(7)) / (3 * H * W)).cuda()
    rear = RearPass(gen, fri, bwd_precision=bwd_prec)
    pred3 = rear.forward(z).clone()
    g3 = rear.backward(gw.contiguous()).clone()
    if H == 2048:
        assert rear._plan['sh'].get('fft_mask', True) is True
    for b in range(3):
        pred1 = rear.forward(z[b:b + 1].contiguous()).clone()
        g1 = rear.backward(gw[b:b + 1].contiguous()).clone()
        perr = float((pred3[b:b + 1] - pred1).abs().max())
        rel = float((g3[b:b + 1] - g1).norm() / g1.norm())
        mx = float((g3[b:b + 1] - g1).abs().max() / g1.abs().max())
        print(f'{H} x {W}, image {b}: pred max-abs {perr:.2e}, gradient rel L2 {rel:.2e} (max / gmax {mx:.2e})', flush=True)
        assert perr < 1e-4, (b, perr)
        assert rel < bar and mx < 5 * bar, (b, rel, mx)


def test_refine_predict_batch_small_generator_against_oracle():
    """refine_predict_batch on three images of one size (2 scales, small generator, fp32 forward, bf16x3 reverse pass) against the oracle's
    batch-1 refinement of each image: test_refine_predict_end_to_end's bars, and every image's loss falls."""
    cfg = O.small_config(ngf=16, n_blocks=2)
    sd = O.make_synthetic_state_dict(cfg, seed=21, calib_hw=32)
    model = trainers.DefaultInpaintingTrainingModule(dict(generator=dict(kind='ffc_resnet', **cfg)))
    model.load_state_dict({'generator.' + k: v for k, v in sd.items()}, strict=True)
    model.freeze().cuda()
    g = torch.Generator().manual_seed(5)
    B, Hh, Ww = 3, 250, 300
    image = torch.rand(B, 3, 256, 304, generator=g)
    mask = torch.zeros(B, 1, 256, 304)
    mask[0, :, 40:200, 50:250] = 1.0
    mask[1, :, 90:150, 120:180] = 1.0
    mask[2, :, 20:120, 150:290] = 1.0
    batch = dict(image=image.cuda(), mask=mask.cuda(), unpad_to_size=[torch.tensor([Hh] * B), torch.tensor([Ww] * B)])
    trace = []
    kw = dict(modulo=8, n_iters=5, lr=0.002, min_side=125, max_scales=2, px_budget=10 ** 7)
    out = RF.refine_predict_batch(batch, model, gpu_ids='0,', trace=trace, **kw)
    assert out.shape == (B, 3, Hh, Ww) and len(trace) == 2
    losses = np.asarray(trace[1]['loss'])
    assert losses.shape == (5, B)
    for b in range(B):
        ref = R.refine_predict(image[b:b + 1], mask[b:b + 1], (Hh, Ww), sd, cfg, **kw)
        d = (out[b:b + 1] - ref).abs()
        print(f'image {b}: max-abs {float(d.max()):.2e} mean-abs {float(d.mean()):.2e}; loss {losses[0, b]:.5f} -> {losses[-1, b]:.5f}', flush=True)
        assert float(d.max()) < 1e-2 and float(d.mean()) < 3e-4, b
        assert losses[-1, b] < losses[0, b], b


@pytest.fixture(scope='module')
def biglama_module():
    cfg = dict(O.BIG_LAMA)
    sd = O.make_synthetic_state_dict(cfg, seed=0, calib_hw=64)
    model = trainers.DefaultInpaintingTrainingModule(dict(generator=dict(kind='ffc_resnet', **cfg)))
    model.load_state_dict({'generator.' + k: v for k, v in sd.items()}, strict=True)
    model.freeze().cuda()
    checksum = sum(float(v.double().sum()) for v in sd.values() if v.is_floating_point())
    return model, checksum


def test_biglama_golden_in_slot0_of_a_batch_of_two(biglama_module, golden_dir):
    """The refine_biglama_1024 golden case (full big-lama, 2 scales, default precisions) in slot 0 of a batch of two whose slot 1 holds another
    image and mask: slot 0 meets exactly test_refine_predict_biglama_golden's bars -- a neighbour does not move an image's trajectory beyond the
    algorithm's own sensitivity."""
    g = np.load(os.path.join(golden_dir, 'refine_biglama_1024.npz'))
    model, checksum = biglama_module
    assert abs(checksum - float(g['sd_checksum'][0])) < 1e-3 * abs(checksum), 'seeded weights drifted from the golden run'
    spec = importlib.util.spec_from_file_location('make_golden_refine', os.path.join(golden_dir, 'make_golden_refine.py'))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    image0, mask0 = mk.make_case(res=1024, seed=int(g['seed_img'][0]))
    other = O.make_synthetic_batch(1, 1024, 1024, seed=31)
    image1, mask1 = other['image'], other['mask']
    assert not torch.equal(mask0, mask1)
    batch = dict(image=torch.cat([image0, image1]).cuda(), mask=torch.cat([mask0, mask1]).cuda(),
                 unpad_to_size=[torch.tensor([1024, 1024]), torch.tensor([1024, 1024])])
    trace = []
    out = RF.refine_predict_batch(batch, model, gpu_ids='0,', modulo=8, n_iters=int(g['n_iters'][0]), lr=0.002, min_side=512, max_scales=2,
                                  px_budget=1800000, trace=trace)
    assert out.shape == (2, 3, 1024, 1024) and len(trace) == 2
    for s in range(2):
        ref_loss = g[f'loss{s}']
        got = np.asarray(trace[s].get('loss', []), dtype=np.float64)
        assert len(got) == len(ref_loss)
        if len(ref_loss):
            assert got.shape == (len(ref_loss), 2)
            got0 = got[:, 0]
            rel = np.abs(got0 - ref_loss) / ref_loss
            self_rel = float(g[f'self{s}'][2]) if f'self{s}' in g.files else 0.0
            print(f'scale {s}: slot 0 max loss rel err {rel.max():.2e}; slot 1 loss {got[0, 1]:.5f} -> {got[-1, 1]:.5f}', flush=True)
            assert rel.max() < max(1e-4, 4 * self_rel), (s, got0, ref_loss)
            assert np.all(np.diff(got0) < 0)
        o = trace[s]['out'][0:1]
        st = o.shape[-1] // g[f'out{s}_sample'].shape[-1]
        d = o[:, :, ::st, ::st].numpy() - g[f'out{s}_sample']
        self_mean, self_max = (float(g[f'self{s}'][0]), float(g[f'self{s}'][1])) if f'self{s}' in g.files else (0.0, 0.0)
        print(f'scale {s}: slot 0 out mean-abs {np.abs(d).mean():.2e} max-abs {np.abs(d).max():.2e} (oracle self {self_mean:.2e} / {self_max:.2e})',
              flush=True)
        assert np.abs(d).mean() < max(3e-4, 2 * self_mean) and np.abs(d).max() < max(5e-3, 2 * self_max), s
    st = int(g['sample_stride'][0])
    moved = float(np.abs(out[0:1, :, ::st, ::st].numpy() - g['plain_sample']).mean())
    assert moved > 0.3 * float(g['refine_minus_plain_meanabs'][0]), (moved, g['refine_minus_plain_meanabs'])


def test_predict_cli_refiner_batch_size(tmp_path):
    """``refine=True refiner.batch_size=4`` on six images of two sizes against ``refiner.batch_size=1``: the same files, and every image
    within the bars of test_refine_predict_batch_small_generator_against_oracle in u8 levels (+1 level of quantisation)."""
    import yaml
    from PIL import Image
    from lama_amd import predict as P
    cfg = O.small_config(ngf=16, n_blocks=2)
    sd = O.make_synthetic_state_dict(cfg, seed=5, calib_hw=32)
    raw = dict(training_model=dict(kind='default', concat_mask=True),
               generator=dict(kind='ffc_resnet', **{k: v for k, v in cfg.items() if not isinstance(v, dict)},
                              init_conv_kwargs=dict(ratio_gin=0, ratio_gout=0, enable_lfu=False),
                              downsample_conv_kwargs=dict(ratio_gin=0, ratio_gout=0, enable_lfu=False),
                              resnet_conv_kwargs=dict(ratio_gin=0.75, ratio_gout=0.75, enable_lfu=False)))
    mdir = tmp_path / 'model'
    os.makedirs(mdir / 'models')
    with open(mdir / 'config.yaml', 'w') as f:
        yaml.safe_dump(raw, f)
    torch.save({'state_dict': {'generator.' + k: v for k, v in sd.items()}}, mdir / 'models' / 'best.ckpt')
    rng = np.random.RandomState(4)
    indir = tmp_path / 'in'
    os.makedirs(indir)
    shapes = [(200, 248), (160, 200), (200, 248), (200, 248), (160, 200), (200, 248)]
    for i, (h, w) in enumerate(shapes):
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype('uint8')).save(indir / f'im{i}.png')
        m = np.zeros((h, w), 'uint8')
        y0, x0 = rng.randint(10, h // 3), rng.randint(10, w // 3)
        m[y0:y0 + h // (2 + i % 3), x0:x0 + w // (2 + i % 2)] = 255
        Image.fromarray(m).save(indir / f'im{i}_mask001.png')
    common = [f'model.path={mdir}', f'indir={indir}', 'refine=True', 'refiner.min_side=80', 'refiner.max_scales=2', 'refiner.n_iters=5']
    out1, out4 = tmp_path / 'out1', tmp_path / 'out4'
    assert P.main(common + [f'outdir={out1}']) == 0
    assert P.main(common + [f'outdir={out4}', 'refiner.batch_size=4']) == 0
    files1 = sorted(os.listdir(out1))
    assert files1 == sorted(os.listdir(out4)) and len(files1) == 6
    for name in files1:
        a = np.asarray(Image.open(out1 / name)).astype(int)
        b = np.asarray(Image.open(out4 / name)).astype(int)
        assert a.shape == b.shape
        d = np.abs(a - b)
        print(f'{name}: u8 max-abs {d.max()} mean-abs {d.mean():.4f}', flush=True)
        assert d.max() <= 1e-2 * 255 + 1 and d.mean() <= 3e-4 * 255 + 0.05, name
