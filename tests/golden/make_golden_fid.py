"""Golden vectors of the FID evaluator, produced by the REFERENCE's own InceptionV3 / FIDScore / calculate_frechet_distance on the CPU (run where a
checkout of the reference exists; the tests read only what this writes).
usage: python tests/golden/make_golden_fid.py <reference root>  ->  tests/golden/fid.npz

The reference modules are imported from their files through stub packages.  Its ``torchvision.models`` is the plain-torch restatement of
tests/inception_util.py (the reference subclasses InceptionA / C / E and patches their forwards itself), and ``load_state_dict_from_url`` is a stub
that returns the seeded synthetic state dict: both are in place before the module is executed, and sockets are disabled for the whole run.

Recorded: the calibrated BatchNorm statistics of the synthetic network (one pass in training mode with momentum 1 over noise images: every
layer's output stays O(1) through all 94 layers), the u8 inputs of four cases, the reference's fp32 and ``.double()`` pool3 activations, `unit` =
the largest fp32-vs-fp64 distance (max-abs over max-abs) over the cases, four activation pairs with the reference's Frechet distance, a 12-item
FIDScore.get_value result (total and groups, one group of a single item) and the two integral values."""
import importlib
import os
import socket
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import inception_util as U  # noqa: E402

if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], 'saicinpainting')):
    sys.exit(__doc__)
REF = os.path.abspath(sys.argv[1])


def _no_network(*a, **kw):
    raise RuntimeError('make_golden_fid.py must not reach the network')


socket.socket = _no_network
socket.create_connection = _no_network


def _stub(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


# ---- the synthetic network: seeded weights, BatchNorm statistics calibrated once ------------------------------------------------------------
g = torch.Generator().manual_seed(20261020)


def u8(*shape):
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


net = U.seeded_network()
for m in U.basic_convs(net):
    m.bn.momentum = 1.0                       # running statistics = the statistics of the one calibration batch
net.train()
with torch.no_grad():
    calib = torch.cat([torch.nn.functional.interpolate(u8(6, 3, 64, 48).float() / 255, size=(299, 299), mode='bilinear', align_corners=False),
                       u8(2, 3, 299, 299).float() / 255])
    net.features(2 * calib - 1)
net.eval()
out = dict(bn_mean=torch.cat([m.bn.running_mean for m in U.basic_convs(net)]).numpy(),
           bn_var=torch.cat([m.bn.running_var for m in U.basic_convs(net)]).numpy())
SD = U.synthetic_state_dict(out)

# ---- the reference, on stubs ---------------------------------------------------------------------------------------------------------------
tv_inc = _stub('torchvision.models.inception', InceptionA=U.InceptionA, InceptionB=U.InceptionB, InceptionC=U.InceptionC, InceptionD=U.InceptionD,
               InceptionE=U.InceptionE)
tv_utils = _stub('torchvision.models.utils', load_state_dict_from_url=lambda url, **kw: {k: v.clone() for k, v in SD.items()})
tvm = _stub('torchvision.models', inception_v3=U.inception_v3, inception=tv_inc, utils=tv_utils)
_stub('torchvision', models=tvm)
import torch.utils.model_zoo  # noqa: E402
torch.utils.model_zoo.load_url = _no_network
for name in ('sklearn', 'sklearn.svm', 'cv2', 'skimage', 'pytorch_lightning'):
    _stub(name)
_stub('skimage.metrics', structural_similarity=None)
_stub('joblib', Parallel=None, delayed=None)
_stub('models')
_stub('models.ade20k', SegmentationModule=None, NUM_CLASS=150, segm_options=None)
_stub('saicinpainting', os.path.join(REF, 'saicinpainting'))
_stub('saicinpainting.utils', get_shape=None)
_stub('saicinpainting.evaluation', os.path.join(REF, 'saicinpainting/evaluation'))
_stub('saicinpainting.evaluation.utils', move_to_device=None)
_stub('saicinpainting.evaluation.losses', os.path.join(REF, 'saicinpainting/evaluation/losses'))
_stub('saicinpainting.evaluation.losses.fid', os.path.join(REF, 'saicinpainting/evaluation/losses/fid'))
_stub('saicinpainting.evaluation.losses.lpips', PerceptualLoss=None)
_stub('saicinpainting.evaluation.losses.ssim', SSIM=None)
import tqdm.auto  # noqa: E402,F401
ref_inc = importlib.import_module('saicinpainting.evaluation.losses.fid.inception')
ref_loss = importlib.import_module('saicinpainting.evaluation.losses.base_loss')
ref_eval = importlib.import_module('saicinpainting.evaluation.evaluator')

# ---- the network cases ---------------------------------------------------------------------------------------------------------------------
small = u8(1, 3, 64, 48)
big = torch.nn.functional.interpolate(small.float(), size=(320, 299), mode='nearest').to(torch.uint8)     # an upscaled image beside ...
c_img = u8(2, 3, 64, 48)
cases = dict(a=(u8(2, 3, 64, 48), u8(2, 3, 64, 48), True),
             b=(big, u8(1, 3, 320, 299), True),                     # ... a noise image: 320 rows shrink, 299 columns stay
             c=(c_img.clone(), c_img, True),                        # pred equal to target
             d=(u8(2, 3, 75, 75), u8(2, 3, 75, 75), False))         # resize_input=False: the smallest plane the network takes
assert tuple(cases) == U.CASES
unit = 0.0
for tag, (pred, target, resize) in cases.items():
    out[f'{tag}_pred'], out[f'{tag}_target'], out[f'{tag}_resize'] = pred.numpy(), target.numpy(), np.array(resize)
    m32 = ref_inc.InceptionV3([3], resize_input=resize).eval()
    m64 = ref_inc.InceptionV3([3], resize_input=resize).eval().double()
    p, t = U.case_inputs(out, tag)
    with torch.no_grad():
        x = torch.cat([p, t])
        a32 = m32(x)[0].flatten(1)
        a64 = m64(x.double())[0].flatten(1)
    out[f'{tag}_act32'], out[f'{tag}_act64'] = a32.numpy(), a64.numpy()
    rel = float((a32.double() - a64).abs().max() / a64.abs().max())
    own = float((U.restated_features(SD, x, resize) - a64).abs().max() / a64.abs().max())
    unit = max(unit, rel)
    print(tag, tuple(x.shape), 'max |a64|', float(a64.abs().max()), 'mean', float(a64.mean()), 'fp32 vs fp64', rel, 'restatement vs reference fp64', own)
    assert own <= 1e-12
out['unit'] = np.array(unit)

# ---- the Frechet distance ------------------------------------------------------------------------------------------------------------------
rng = np.random.default_rng(20261021)
for k, (D, N) in enumerate([(32, 96), (64, 200), (64, 40), (256, 24)]):
    spread = 0.5 + rng.random(D)                 # independent features of different spread: well-conditioned covariances where N > D
    ap = rng.standard_normal((N, D)) * spread + 0.1 * rng.standard_normal(D)
    at = rng.standard_normal((N, D)) * spread * 1.2 + 0.1 * rng.standard_normal(D)
    out[f'fd{k}_pred'], out[f'fd{k}_target'] = ap.astype(np.float32), at.astype(np.float32)
    out[f'fd{k}_value'] = np.array(ref_loss.calculate_frechet_distance(out[f'fd{k}_pred'], out[f'fd{k}_target']))
    print('frechet', D, N, float(out[f'fd{k}_value']))

# ---- FIDScore.get_value over recorded activations, the integrals ----------------------------------------------------------------------------
score = ref_loss.FIDScore.__new__(ref_loss.FIDScore)
torch.nn.Module.__init__(score)
score.eps = 1e-6
score.reset()
acts_p = (rng.standard_normal((12, 48)) @ (rng.standard_normal((48, 48)) / 7)).astype(np.float32)
acts_t = (rng.standard_normal((12, 48)) @ (rng.standard_normal((48, 48)) / 7) + 0.2).astype(np.float32)
groups = np.array([3, 0, 3, 5, 0, 3, 9, 5, 0, 3, 5, 0])             # label 9: a group of a single item
for lo in (0, 4, 8):
    score.activations_pred.append(torch.from_numpy(acts_p[lo:lo + 4]))
    score.activations_target.append(torch.from_numpy(acts_t[lo:lo + 4]))
total, per_group = score.get_value(groups=groups)
out['score_pred'], out['score_target'], out['score_groups'] = acts_p, acts_t, groups
out['score_total'] = np.array(total['mean'])
out['score_labels'] = np.array(sorted(per_group))
out['score_group_values'] = np.array([per_group[k]['mean'] for k in sorted(per_group)], dtype=np.float64)
assert np.isnan(out['score_group_values'][-1]) and np.isfinite(out['score_group_values'][:-1]).all()
metrics = {('ssim', 'total'): dict(mean=0.8731), ('lpips', 'total'): dict(mean=0.1234), ('fid', 'total'): dict(mean=17.25)}
out['integral_inputs'] = np.array([0.8731, 0.1234, 17.25])
out['integral_values'] = np.array([ref_eval.ssim_fid100_f1(metrics), ref_eval.lpips_fid100_f1(metrics)])
print('FIDScore', total, per_group, 'integrals', out['integral_values'])

np.savez_compressed(U.GOLDEN, **out)
print('unit', unit, 'bytes', os.path.getsize(U.GOLDEN))
