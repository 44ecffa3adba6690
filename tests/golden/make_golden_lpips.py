"""Golden vectors of the LPIPS evaluator, produced by the REFERENCE's own PerceptualLoss(model='net-lin', net='vgg') (run in the build container
only; /root/reference does not exist on the GPU box).  usage: python tests/golden/make_golden_lpips.py  ->  tests/golden/lpips.npz

The reference module is loaded by file path with stubs for the imports it does not need here; its torchvision vgg16 is a plain-torch Sequential of
the standard layout holding the SEEDED backbone of tests/lpips_util.py (the pretrained one is a download); the linear heads are the real ones.
Recorded: the inputs (uint8), the reference's fp32 value and per-level terms, its own fp64 value, the fp32-vs-fp64 relative distance of the
reference per case (`<tag>_rel32`), and `unit` = the largest of them over the cases -- the unit of the test bars.  The near-identical case h (a value
of 2e-5, where the reference's own fp32 result is 20 times further from fp64 than anywhere else) does NOT enter `unit`: it would loosen the bar
of every other case; it is measured in units of its own `h_rel32` instead."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lpips_util as U  # noqa: E402

REF = '/root/reference'
SD = U.backbone_state_dict()


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _FakeVGG(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.features = U.features_sequential(SD)


_stub('skimage')
_stub('skimage.metrics', structural_similarity=None)
_stub('pytorch_lightning')
_stub('tqdm', tqdm=lambda it, **kw: it)
_stub('saicinpainting')
_stub('saicinpainting.utils', get_shape=None)
tvm = _stub('torchvision.models', vgg16=lambda pretrained=False, **kw: _FakeVGG())
_stub('torchvision', models=tvm)
spec = importlib.util.spec_from_file_location('ref_lpips', os.path.join(REF, 'saicinpainting/evaluation/losses/lpips.py'))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

heads_path = os.path.join(REF, 'models/lpips_models/vgg.pth')
loss32 = ref.PerceptualLoss(model='net-lin', net='vgg', model_path=heads_path, use_gpu=False).eval()
loss64 = ref.PerceptualLoss(model='net-lin', net='vgg', model_path=heads_path, use_gpu=False).eval().double()

# the reference adds the levels IN PLACE into res[0] (val = res[0]; val += res[l]), so the first entry of retPerLayer comes back as the total:
# the level-0 term is taken from the output of lin0 itself (its spatial mean, the same call the reference makes)
_lin0 = {}
loss32.model.net.lin0.model.register_forward_hook(lambda mod, inp, outp: _lin0.__setitem__('map', outp.detach().clone()))

g = torch.Generator().manual_seed(20261018)


def u8(*shape):
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


def inpainted(t, y0, y1, x0, x1):
    p = t.clone()
    p[:, :, y0:y1, x0:x1] = u8(t.shape[0], 3, y1 - y0, x1 - x0)
    return p


t64 = u8(1, 3, 64, 48)
near = (t64.int() + torch.randint(-1, 2, t64.shape, generator=g)).clamp(0, 255).to(torch.uint8)
t32 = u8(1, 3, 32, 32)
cases = dict(a=(u8(2, 3, 16, 16), u8(2, 3, 16, 16), True),            # smallest plane that survives four pools (relu5_3 is 1 x 1)
             b=(u8(2, 3, 37, 50), u8(2, 3, 37, 50), True),            # odd sizes: floor pooling at every level
             c=(inpainted(t64, 20, 44, 10, 30), t64, True),           # equals the target outside a rectangle
             d=(t32.clone(), t32, True),                              # identical pair: exactly 0
             f=(u8(1, 3, 64, 48), t64, True),                         # independent random images of the size of c / h
             g=(u8(2, 3, 16, 16), u8(2, 3, 16, 16), False),           # normalize=False: inputs already in [-1, 1]
             h=(near, t64, True))                                     # near-identical: +-1 grey level of noise
assert tuple(cases) == U.CASES
out = {f'lin{k}': torch.load(heads_path, map_location='cpu')[f'lin{k}.model.1.weight'].reshape(-1).numpy() for k in range(5)}
unit = 0.0
for tag, (pred, target, normalize) in cases.items():
    out[f'{tag}_pred'], out[f'{tag}_target'], out[f'{tag}_normalize'] = pred.numpy(), target.numpy(), np.array(normalize)
    p, t, _ = U.case_inputs(out, tag)
    with torch.no_grad():
        if not normalize:
            v32, l32 = loss32.model(t, p, retPerLayer=True)
            v64 = loss64.model(t.double(), p.double())
        else:
            v32 = loss32(p, t, normalize=True)
            _, l32 = loss32.model(2 * t - 1, 2 * p - 1, retPerLayer=True)
            v64 = loss64(p.double(), t.double(), normalize=True)
    v32, v64 = v32.flatten(), v64.flatten()
    out[f'{tag}_value'] = v32.numpy()
    l32 = [ref.spatial_average(_lin0['map'], keepdim=True)] + list(l32[1:])
    out[f'{tag}_levels'] = torch.stack([l.flatten() for l in l32]).numpy()
    out[f'{tag}_value64'] = v64.numpy()
    rel = float(((v32.double() - v64).abs() / v64.abs().clamp_min(1e-300)).max()) if float(v64.abs().max()) > 0 else 0.0
    out[f'{tag}_rel32'] = np.array(rel)
    if tag != 'h':
        unit = max(unit, rel)
    print(tag, tuple(pred.shape), v32.tolist(), 'fp32 vs fp64 rel', rel)
assert float(np.abs(out['d_value']).max()) == 0.0
out['unit'] = np.array(unit)
np.savez_compressed(U.GOLDEN, **out)
print('unit', unit, 'bytes', os.path.getsize(U.GOLDEN))
