"""CPU tests of batched refinement (lama_amd.refinement.refine_predict_batch, the per-image masked-L1 kernels of v111 and the
``refiner.batch_size`` option) through the host SIMT emulator, against numpy and the CPU oracle (oracle/refine_oracle.py)."""
import numpy as np
import pytest
import torch

from lama_amd import _lib as L
from lama_amd import ffc as F
from lama_amd import refinement as RF
from lama_amd import trainers
from lama_amd._lib import LamaError
from oracle import lama_oracle as O
from oracle import refine_oracle as R
from tests.emu import emu_lib


@pytest.fixture(scope='module')
def setup():
    cfg = O.small_config(ngf=8, n_blocks=2)
    sd = O.make_synthetic_state_dict(cfg, seed=21, calib_hw=32)
    model = trainers.DefaultInpaintingTrainingModule(dict(generator=dict(kind='ffc_resnet', **cfg)))
    model.load_state_dict({'generator.' + k: v for k, v in sd.items()}, strict=True)
    model.freeze()
    model.generator.set_exec(F._Exec(emu_lib()))
    model.generator.set_precision(L.PREC_F32)
    RF._lib_of.override = emu_lib()
    yield cfg, sd, model
    RF._lib_of.override = None


def _np_terms(pred, target, mask, select_ge):
    m = np.broadcast_to(mask, pred.shape)
    sel = (m >= 1e-8) if select_ge else (m < 1e-8)
    d = (pred - target).astype(np.float64)
    return [(float(np.abs(d[b][sel[b]]).sum()), float(sel[b].sum())) for b in range(pred.shape[0])], sel


PER_IMAGE_MASK_C = [1, 3]
PER_IMAGE_SELECT_GE = [False, True]


def _sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


def check_l1_masked_per_image_kernels_against_numpy(lib, mask_c, select_ge, dev='cpu'):
    """The body of the test below; tests/test_refine_kernels_gpu.py reruns it through the production library (``dev='cuda'``)."""
    g = torch.Generator().manual_seed(40 + mask_c + 2 * select_ge)
    B, H, W = 3, 11, 17
    pred, target = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    target[0, :, 2, 3] = pred[0, :, 2, 3]                          # d == 0 on selected elements: sign(0) = 0
    mask = torch.zeros(B, mask_c, H, W)
    mask[0, :, 1:9, 2:14] = 1.0                                    # large selection
    mask[1, :, 4:6, 5:8] = 1.0                                     # small one
    if select_ge:
        pass                                                       # image 2: mask all 0 -> nothing >= thr: empty selection
    else:
        mask[2] = 1.0                                              # image 2: mask all 1 -> nothing < thr: empty selection
    terms, sel = _np_terms(pred.numpy(), target.numpy(), mask.numpy(), select_ge)
    assert terms[2][1] == 0 and terms[0][1] != terms[1][1]
    predd, targetd, maskd = pred.to(dev), target.to(dev), mask.to(dev)
    accd = torch.zeros(B, 2, dtype=torch.float64, device=dev)
    lib.l1_masked_per_image(L.view(predd), L.view(targetd), L.view(maskd), 1e-8, select_ge, accd, B)
    _sync(dev)
    acc = accd.cpu()
    for b in range(B):
        assert acc[b, 1].item() == terms[b][1]
        assert abs(acc[b, 0].item() - terms[b][0]) <= 1e-9 * max(1.0, terms[b][0])
    sgn = np.sign(pred.numpy() - target.numpy()) * sel
    scale = np.array([np.float32(1.0 / n) if n else np.float32(0.0) for _, n in terms], dtype=np.float32)
    want = (sgn * scale[:, None, None, None]).astype(np.float32)
    gbuf = torch.full((B, 3, H, W), 5.0, device=dev)
    lib.l1_masked_per_image_bwd(L.view(predd), L.view(targetd), L.view(maskd), 1e-8, select_ge, accd, False, L.view(gbuf), B)
    _sync(dev)
    assert np.array_equal(gbuf.cpu().numpy(), want)
    assert float(gbuf[2].abs().max()) == 0.0                       # the empty selection contributes 0 (and overwrites)
    base = torch.randn(B, 3, H, W, generator=g)
    gacc = base.clone().to(dev)
    lib.l1_masked_per_image_bwd(L.view(predd), L.view(targetd), L.view(maskd), 1e-8, select_ge, accd, True, L.view(gacc), B)
    _sync(dev)
    assert np.array_equal(gacc.cpu().numpy(), (base.numpy() + want).astype(np.float32))
    # batch 1: bit-identical to lama_l1_masked_bwd with the host's float(1 / n)
    for b in range(B):
        one = torch.zeros(1, 2, dtype=torch.float64, device=dev)
        pb, tb, mb = predd[b:b + 1].contiguous(), targetd[b:b + 1].contiguous(), maskd[b:b + 1].contiguous()
        lib.l1_masked_per_image(L.view(pb), L.view(tb), L.view(mb), 1e-8, select_ge, one, 1)
        old = torch.zeros(2, dtype=torch.float64, device=dev)
        lib.l1_masked(L.view(pb), L.view(tb), L.view(mb), 1e-8, select_ge, old, 1)
        _sync(dev)
        assert torch.equal(one[0].cpu(), old.cpu())
        n = float(old[1])
        g_old, g_new = torch.zeros(1, 3, H, W, device=dev), torch.zeros(1, 3, H, W, device=dev)
        lib.l1_masked_bwd(L.view(pb), L.view(tb), L.view(mb), 1e-8, select_ge, (1.0 / n) if n else 0.0, False, L.view(g_old), 1)
        lib.l1_masked_per_image_bwd(L.view(pb), L.view(tb), L.view(mb), 1e-8, select_ge, one, False, L.view(g_new), 1)
        _sync(dev)
        assert torch.equal(g_old.cpu(), g_new.cpu())


@pytest.mark.parametrize('mask_c', PER_IMAGE_MASK_C)
@pytest.mark.parametrize('select_ge', PER_IMAGE_SELECT_GE)
def test_l1_masked_per_image_kernels_against_numpy(mask_c, select_ge):
    check_l1_masked_per_image_kernels_against_numpy(emu_lib(), mask_c, select_ge)


def _case(B, seed, Hp=96, Wp=104):
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(B, 3, Hp, Wp, generator=g)
    mask = torch.zeros(B, 1, Hp, Wp)
    boxes = [(10, 80, 12, 90), (30, 62, 30, 66), (20, 50, 40, 90), (8, 88, 8, 96)]
    for b in range(B):
        y0, y1, x0, x1 = boxes[b % len(boxes)]
        mask[b, :, y0:y1, x0:x1] = 1.0
    return image, mask


KW = dict(gpu_ids='0,', modulo=8, n_iters=3, lr=0.002, min_side=45, max_scales=2, px_budget=10 ** 6)


def test_refine_predict_batch_of_one_equals_refine_predict(setup):
    _, _, model = setup
    Hh, Ww = 90, 100
    image, mask = _case(1, 5)
    batch = dict(image=image, mask=mask, unpad_to_size=[torch.tensor([Hh]), torch.tensor([Ww])])
    tr1, trb = [], []
    out1 = RF.refine_predict(dict(batch), model, trace=tr1, **KW)
    outb = RF.refine_predict_batch(dict(batch), model, trace=trb, **KW)
    assert outb.shape == (1, 3, Hh, Ww)
    assert torch.equal(out1, outb)
    assert len(trb) == len(tr1) == 2
    for a, b in zip(tr1, trb):
        assert torch.equal(a['out'], b['out'])
        assert np.allclose(np.asarray(a.get('loss', [])).reshape(-1, 1), np.asarray(b.get('loss', [])).reshape(-1, 1), rtol=1e-9)


def test_refine_predict_batch_images_are_separate_optimisations(setup):
    """Three images of one size whose mask areas differ by more than 4x: each image's loss curve and output are those of its own batch-1
    refinement through the oracle (normalising an L1 term over the whole batch would mix the balance of the two terms across images)."""
    cfg, sd, model = setup
    Hh, Ww = 90, 100
    B = 3
    image, mask = _case(B, 7)
    areas = [float(mask[b].sum()) for b in range(B)]
    assert max(areas) > 4 * min(areas)
    batch = dict(image=image, mask=mask, unpad_to_size=[torch.tensor([Hh] * B), torch.tensor([Ww] * B)])
    trace = []
    out = RF.refine_predict_batch(batch, model, trace=trace, **KW)
    assert out.shape == (B, 3, Hh, Ww) and len(trace) == 2
    losses = np.asarray(trace[1]['loss'])
    assert losses.shape == (KW['n_iters'], B)
    assert trace[1]['out'].shape == (B, 3, Hh, Ww)
    for b in range(B):
        tr = []
        ref = R.refine_predict(image[b:b + 1], mask[b:b + 1], (Hh, Ww), sd, cfg, modulo=8, n_iters=KW['n_iters'], lr=KW['lr'],
                               min_side=KW['min_side'], max_scales=KW['max_scales'], px_budget=KW['px_budget'], trace=tr)
        assert np.allclose(losses[:, b], tr[1]['loss'], rtol=2e-4, atol=1e-6), (b, losses[:, b], tr[1]['loss'])
        err = float((out[b:b + 1] - ref).abs().max())
        assert err < 2e-3, (b, err)


def test_refine_predict_batch_refuses_mixed_sizes_and_regular_generators(setup):
    _, _, model = setup
    image, mask = _case(2, 3)
    batch = dict(image=image, mask=mask, unpad_to_size=[torch.tensor([90, 96]), torch.tensor([100, 100])])
    with pytest.raises(LamaError, match='unpad_to_size'):
        RF.refine_predict_batch(batch, model, **KW)
    from tests import regular_util as RU
    reg = trainers.DefaultInpaintingTrainingModule(dict(generator=dict(kind='pix2pixhd_global', **RU.small_config(ngf=4, n_blocks=1))))
    reg.freeze()
    batch = dict(image=image, mask=mask, unpad_to_size=[torch.tensor([90, 90]), torch.tensor([100, 100])])
    with pytest.raises(NotImplementedError, match='ffc_resnet'):
        RF.refine_predict_batch(batch, reg, **KW)


def test_refiner_batch_size_option():
    from lama_amd import predict as P
    base = ['model.path=/m', 'indir=/i', 'outdir=/o']
    assert P.parse_overrides(base)['refiner.batch_size'] == 1
    cfg = P.parse_overrides(base + ['refiner.batch_size=4'])
    assert cfg['refiner.batch_size'] == 4 and isinstance(cfg['refiner.batch_size'], int)
    with pytest.raises(SystemExit):
        P.parse_overrides(base + ['refiner.batch_size=four'])
