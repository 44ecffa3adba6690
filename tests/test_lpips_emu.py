"""CPU: LPIPS (VGG-16, net-lin).  The fp64 restatement (tests/lpips_ref.py) against the reference-generated vectors, the two new kernels
(lama_lpips_scale_fwd, lama_lpips_layer_fwd) on the host emulator against that restatement, and the host logic of lama_amd.evaluation
(state-dict keys, loaders, refusals, LPIPSScore bookkeeping)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lpips_ref as R  # noqa: E402
import lpips_util as U  # noqa: E402
from emu import emu_lib  # noqa: E402
from lama_amd import _lib as L  # noqa: E402
from lama_amd import evaluation as EV  # noqa: E402
from lama_amd.ffc import _Exec  # noqa: E402

GOLD = np.load(U.GOLDEN)
UNIT = float(GOLD['unit'])
F32_EPS = 2.0 ** -24                     # one fp32 rounding, relative


@pytest.fixture(scope='module')
def backbone():
    return U.backbone_state_dict()


@pytest.fixture(scope='module')
def heads():
    return U.heads_state_dict(GOLD)


# ---- the fp64 restatement reproduces the reference -----------------------------------------------------------------------------

@pytest.mark.parametrize('tag', U.CASES)
def test_ref_reproduces_reference_vectors(tag, backbone):
    """Bar: the reference's own fp32-vs-fp64 distance recorded with the vectors (`unit`; case h: its own `h_rel32`), + 1e-10 for the
    summation order of two fp64 computations.  Against the reference's fp64 value the restatement agrees to 1e-12."""
    pred, target, normalize = U.case_inputs(GOLD, tag)
    val, levels = R.lpips_ref(pred, target, backbone, [torch.from_numpy(GOLD[f'lin{k}']) for k in range(5)], normalize)
    v64, v32 = GOLD[f'{tag}_value64'], GOLD[f'{tag}_value'].astype(np.float64)
    if tag == 'd':
        assert float(val.abs().max()) == 0.0 and float(np.abs(v32).max()) == 0.0
        return
    assert np.abs(val.numpy() - v64).max() <= 1e-12 * np.abs(v64).max()
    bar = (float(GOLD['h_rel32']) if tag == 'h' else UNIT) + 1e-10
    assert (np.abs(val.numpy() - v32) / np.abs(v64)).max() <= bar
    lv32 = GOLD[f'{tag}_levels'].astype(np.float64)
    assert np.abs(levels.numpy() - lv32).max() <= 4 * max(bar, UNIT) * np.abs(v64).max()      # per-level terms are fp32 too: a few units of the value


# ---- the kernels on the emulator --------------------------------------------------------------------------------------------------

def _half(t, i, B):
    return EV._DistModel._half(t, i, B)


@pytest.mark.parametrize('B,H,W,normalize', [(1, 16, 16, True), (3, 5, 7, True), (2, 37, 50, False), (1, 33, 32, True)])
def test_scale_kernel(B, H, W, normalize):
    """Three fp32 roundings (2x - 1, - shift, / scale) of values below 2.7, the first two amplified by 1 / scale = 2.2: 4.5e-7 absolute at most."""
    lib = emu_lib()
    g = torch.Generator().manual_seed(B * 1000 + H)
    x0, x1 = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    if not normalize:
        x0, x1 = 2 * x0 - 1, 2 * x1 - 1
    y = torch.full((2 * B, 3, H, W), float('nan'))
    lib.lpips_scale(L.view(x0), L.view(x1), L.view(y), B, U.SHIFT, U.SCALE, normalize=normalize)
    ref = R.scale_ref(torch.cat([x0, x1]), normalize)
    assert float((y.double() - ref).abs().max()) <= 5e-7


LAYER_SHAPES = [(3, 1, 1), (3, 2, 3), (64, 5, 7), (64, 16, 16), (512, 1, 1), (512, 2, 3), (64, 9, 32), (3, 16, 16), (512, 5, 7)]


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C,H,W,pool', [(c, h, w, pool) for c, h, w in LAYER_SHAPES for pool in (False, True) if not (pool and min(h, w) < 2)])
def test_layer_kernel(C, H, W, pool, B):
    """The distance term against the fp64 restatement: the kernel sums in fp64 and rounds once to fp32 when it adds the term to acc (= 0 before),
    so 2^-24 relative (+ 1e-12 for the fp64 order).  The pooled maps are exact (a maximum of four fp32 values)."""
    lib = emu_lib()
    g = torch.Generator().manual_seed(C * 100 + H * 10 + W + B)
    f = torch.relu(torch.randn(2 * B, C, H, W, generator=g) + 0.3)          # ReLU features: a share of exact zeros
    w = torch.rand(C, generator=g) + 0.01
    acc = torch.zeros(B)
    ws = torch.empty(max(1, lib.lpips_layer_workspace_bytes(B, C, H, W) // 8), dtype=torch.float64)
    p = torch.full((2 * B, C, H // 2, W // 2), float('nan')) if pool else None
    lib.lpips_layer(_half(f, 0, B), _half(f, 1, B), B, w, acc, ws, None if p is None else _half(p, 0, B), None if p is None else _half(p, 1, B))
    ref = R.layer_ref(f[:B], f[B:], w)
    assert float(((acc.double() - ref).abs() / ref).max()) <= F32_EPS + 1e-12
    if pool:
        assert torch.equal(p, torch.nn.functional.max_pool2d(f, 2, 2))
    # accumulation: a second launch adds the same term to what acc holds
    lib.lpips_layer(_half(f, 0, B), _half(f, 1, B), B, w, acc, ws)
    assert float(((acc.double() - 2 * ref).abs() / ref).max()) <= 3 * F32_EPS


@pytest.mark.parametrize('C,H,W', [(3, 5, 7), (64, 16, 16), (512, 2, 3)])
def test_layer_kernel_identical_pair_is_exactly_zero(C, H, W):
    lib = emu_lib()
    g = torch.Generator().manual_seed(7)
    h = torch.relu(torch.randn(2, C, H, W, generator=g))
    f = torch.cat([h, h.clone()])
    acc = torch.zeros(2)
    ws = torch.empty(max(1, lib.lpips_layer_workspace_bytes(2, C, H, W) // 8), dtype=torch.float64)
    lib.lpips_layer(_half(f, 0, 2), _half(f, 1, 2), 2, torch.rand(C, generator=g), acc, ws)
    assert acc.tolist() == [0.0, 0.0]


def test_layer_kernel_near_identical_does_not_cancel():
    """f1 = f0 (1 + 1e-4 noise): the value is 1e-8 of the expansion's terms; fp64 sums of exact fp32 products keep 2^-53 of the TERMS, i.e. 1e-8
    relative to such a value at worst -- bar: one fp32 rounding + 1e-7."""
    lib = emu_lib()
    g = torch.Generator().manual_seed(9)
    f0 = torch.relu(torch.randn(1, 64, 6, 10, generator=g) + 0.5)
    f = torch.cat([f0, f0 * (1 + 1e-4 * torch.randn(f0.shape, generator=g))])
    w, acc = torch.rand(64, generator=g), torch.zeros(1)
    ws = torch.empty(max(1, lib.lpips_layer_workspace_bytes(1, 64, 6, 10) // 8), dtype=torch.float64)
    lib.lpips_layer(_half(f, 0, 1), _half(f, 1, 1), 1, w, acc, ws)
    ref = R.layer_ref(f[:1], f[1:], w)
    assert float(ref) < 1e-6
    assert float(((acc.double() - ref).abs() / ref).max()) <= F32_EPS + 1e-7


def test_kernel_argument_checks():
    lib = emu_lib()
    f, w, acc = torch.zeros(2, 4, 3, 3), torch.ones(4), torch.zeros(1)
    ws = torch.empty(8, dtype=torch.float64)
    p = torch.zeros(2, 4, 1, 1)
    with pytest.raises(L.LamaError) as e:                          # one pooled map only
        lib.lpips_layer(_half(f, 0, 1), _half(f, 1, 1), 1, w, acc, ws, _half(p, 0, 1), None)
    assert e.value.code == L.ERR_BAD_ARG
    with pytest.raises(L.LamaError) as e:                          # workspace too small
        lib.lpips_layer(_half(f, 0, 1), _half(f, 1, 1), 1, w, acc, torch.empty(0, dtype=torch.float64))
    assert e.value.code == L.ERR_WORKSPACE
    bad = torch.zeros(2, 4, 2, 2)
    with pytest.raises(L.LamaError) as e:                          # pooled map of the wrong size
        lib.lpips_layer(_half(f, 0, 1), _half(f, 1, 1), 1, w, acc, ws, _half(bad, 0, 1), _half(bad, 1, 1))
    assert e.value.code == L.ERR_BAD_ARG
    x, y = torch.zeros(1, 3, 4, 4), torch.zeros(2, 3, 4, 5)
    with pytest.raises(L.LamaError) as e:
        lib.lpips_scale(L.view(x), L.view(x), L.view(y), 1, U.SHIFT, U.SCALE)
    assert e.value.code == L.ERR_BAD_ARG


# ---- host logic -----------------------------------------------------------------------------------------------------------------------

def _loss(backbone, heads, **kw):
    return EV.PerceptualLoss(model_path=heads, backbone=backbone, **kw).set_exec(_Exec(emu_lib()))


def test_state_dict_keys_are_the_references(backbone, heads):
    keys = set(_loss(backbone, heads).state_dict().keys())
    want = {'model.net.scaling_layer.shift', 'model.net.scaling_layer.scale'}
    want |= {f'model.net.lin{k}.model.1.weight' for k in range(5)}
    for sl, idxs in {1: (0, 2), 2: (5, 7), 3: (10, 12, 14), 4: (17, 19, 21), 5: (24, 26, 28)}.items():
        want |= {f'model.net.net.slice{sl}.{i}.{n}' for i in idxs for n in ('weight', 'bias')}
    assert keys == want


def test_loaders(backbone, heads, tmp_path):
    a = _loss(backbone, heads)
    sd = {k: v.clone() for k, v in a.state_dict().items()}
    # a reference-keyed state dict loads strictly, and serves as backbone= as it is
    other = U.backbone_state_dict(seed=5)
    b = _loss(other, heads)
    assert not torch.equal(b.state_dict()['model.net.net.slice3.12.weight'], sd['model.net.net.slice3.12.weight'])
    b.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in b.state_dict().items())
    c = _loss(sd, heads)
    assert torch.equal(c.state_dict()['model.net.net.slice5.28.bias'], backbone['features.28.bias'])
    # torchvision-keyed file (with the classifier tensors a real vgg16 file carries) and a heads file, both by path
    tv = dict(backbone)
    tv['classifier.0.weight'] = torch.zeros(2, 2)
    torch.save(tv, tmp_path / 'vgg16.pth')
    torch.save(heads, tmp_path / 'heads.pth')
    d = EV.PerceptualLoss(model_path=str(tmp_path / 'heads.pth'), backbone=str(tmp_path / 'vgg16.pth'))
    assert torch.equal(d.state_dict()['model.net.net.slice1.0.weight'], backbone['features.0.weight'])
    assert torch.equal(d.state_dict()['model.net.lin4.model.1.weight'], heads['lin4.model.1.weight'])
    # heads load with strict=False: foreign keys are ignored, a missing head is an error that names it
    EV.PerceptualLoss(model_path=dict(heads, extra=torch.zeros(1)), backbone=backbone)
    with pytest.raises(EV.LamaError, match='lin2'):
        EV.PerceptualLoss(model_path={k: v for k, v in heads.items() if not k.startswith('lin2')}, backbone=backbone)
    with pytest.raises(EV.LamaError, match='features.7|slice2.7'):
        EV.PerceptualLoss(model_path=heads, backbone={k: v for k, v in backbone.items() if not k.startswith('features.7.')})


def test_missing_files_raise(backbone, heads, tmp_path, monkeypatch):
    with pytest.raises(EV.LamaError, match='model_path'):
        EV.PerceptualLoss(model_path=None, backbone=backbone)
    with pytest.raises(EV.LamaError, match='not found'):
        EV.PerceptualLoss(model_path=str(tmp_path / 'nope.pth'), backbone=backbone)
    monkeypatch.setattr(torch.hub, 'get_dir', lambda: str(tmp_path))          # an empty hub cache: nothing is downloaded
    with pytest.raises(EV.LamaError, match='backbone='):
        EV.PerceptualLoss(model_path=heads, backbone=None)
    with pytest.raises(EV.LamaError, match='not found'):
        EV.PerceptualLoss(model_path=heads, backbone=str(tmp_path / 'nope.pth'))
    os.makedirs(tmp_path / 'checkpoints')
    torch.save(backbone, tmp_path / 'checkpoints' / 'vgg16-397923af.pth')     # backbone=None finds torchvision's file in the hub cache
    m = EV.PerceptualLoss(model_path=heads, backbone=None)
    assert torch.equal(m.state_dict()['model.net.net.slice4.19.weight'], backbone['features.19.weight'])


@pytest.mark.parametrize('kw', [dict(net='alex'), dict(net='squeeze'), dict(model='net'), dict(model='L2'), dict(model='SSIM'),
                                dict(spatial=True), dict(colorspace='Lab')])
def test_refusals(kw, backbone, heads):
    with pytest.raises(NotImplementedError):
        EV.PerceptualLoss(model_path=heads, backbone=backbone, **kw)


def test_cpu_tensor_and_bad_shapes_raise(backbone, heads):
    m = EV.PerceptualLoss(model_path=heads, backbone=backbone)                 # the default exec: the real library, device tensors only
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(EV.LamaError, match='GPU'):
        m(x, x)
    e = _loss(backbone, heads)
    with pytest.raises(EV.LamaError):
        e(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 18))
    with pytest.raises(EV.LamaError, match='16 x 16'):
        e(torch.rand(1, 3, 15, 16), torch.rand(1, 3, 15, 16))
    with pytest.raises(NotImplementedError):
        m.train()


def test_lpips_score_bookkeeping(backbone, heads):
    """forward appends the flattened batch values; get_value = mean / std (population) overall and per group, or over `states`."""
    s = EV.LPIPSScore(model_path=heads, backbone=backbone)
    assert isinstance(s.score, EV.PerceptualLoss) and not s.score.training
    fake = [torch.tensor([0.1, 0.4, 0.2]), torch.tensor([0.3, 0.5])]
    it = iter(fake)
    s.score.forward = lambda pred, target: next(it).view(-1, 1, 1, 1)         # the bookkeeping alone (the metric itself: the tests around)
    for v in fake:
        out = s(None, None)
        assert out.shape == v.shape and torch.equal(out, v)
    allv = np.hstack([[]] + [v.numpy() for v in fake])           # the reference stacks onto an empty list: float64
    assert np.array_equal(s.individual_values, allv)
    total, groups = s.get_value()
    assert groups is None and total == {'mean': allv.mean(), 'std': allv.std()}
    labels = [2, 7, 2, 7, 7]
    total, groups = s.get_value(groups=labels)
    assert set(groups) == {2, 7}
    for lab in (2, 7):
        sel = allv[[i for i, v in enumerate(labels) if v == lab]]
        assert groups[lab] == {'mean': sel.mean(), 'std': sel.std()}
    total, _ = s.get_value(states=[torch.tensor([1.0, 3.0]), torch.tensor([5.0])])
    assert total['mean'] == 3.0 and abs(total['std'] - np.std([1.0, 3.0, 5.0])) < 1e-7
    s.reset()
    assert len(s.individual_values) == 0


# The whole module does NOT run here: thirteen MFMA convolutions at 16 x 16 take twenty minutes on the emulator (measured once: cases a and g
# came out 0.28 and 1.0 units from fp64 with exact-fp32 convs).  tests/test_lpips_gpu.py runs it on the hardware.
