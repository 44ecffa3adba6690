#!/usr/bin/env python3
"""Golden vectors that pin oracle/refine_oracle.py to the REFERENCE's own ``saicinpainting/evaluation/refinement.py:86-174,228-314``.

Runs only where a checkout of the reference LaMa tree is available: ``make_golden_refine_pin.py <reference root>``.  The reference module is imported
UNMODIFIED.  What it cannot import is stubbed, and every stub is bound to a helper that is itself pinned by known-answer vectors
(tests/test_refine_helpers_known_answers.py):

  * ``kornia.filters.gaussian_blur2d``, ``kornia.geometry.transform.resize``, ``kornia.morphology.erosion`` -> the restated helpers
    of oracle/refine_oracle.py; ``cv2.getStructuringElement`` -> ``ellipse_kernel``; ``easydict`` -> dict subclass (never executed);
  * a package stub for ``saicinpainting.evaluation`` (its ``__init__`` pulls the evaluators and their downloads) whose ``__path__``
    is the real directory, so ``evaluation/data.py`` and ``evaluation/utils.py`` are the reference's own files;
  * ``torch.device('cuda:N')`` -> cpu inside the reference module only (it hard-codes cuda devices, refinement.py:265,277).

The generator the reference loop runs is the reference's own ``FFCResNetGenerator`` (reference factory, state dict loaded with
strict=True).  For every case of CASES it stores in refine_pin.npz what pins the reference's fp32 ``refine_predict`` output bit for
bit at a small size: its shape (``shape<i>``), the SHA-256 of its bytes (``sha256_<i>``, C order, little-endian fp32) and a strided
sample (``sample<i>``, every SAMPLE_STRIDE-th pixel, for the message when the digest differs).  tests/test_refine_oracle_pin.py runs
``oracle.refine_oracle.refine_predict`` on the same seeded inputs and weights and asks for the same bits (both sides execute the same
torch primitives in the same order).  The script checks that itself before it writes the file.  Both sides run on ONE intra-op thread, so the bits do not depend on the core count of the host.
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

N_ITERS, LR, SEED_SD = 6, 0.002, 11
SAMPLE_STRIDE = 8

# (h, w, kwargs of refine_predict, gray stroke): three scales; one scale boundary; a px-budget resize with a gray mask stroke
CASES = [
    (250, 300, dict(min_side=64, max_scales=3, px_budget=1800000), False),
    (256, 256, dict(min_side=128, max_scales=3, px_budget=1800000), False),
    (300, 420, dict(min_side=100, max_scales=3, px_budget=60000), True),
]


def digest(t):
    """SHA-256 of an fp32 tensor's bytes (C order, little-endian) as 32 uint8."""
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype='<f4')
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)


def sample(t):
    return t[..., ::SAMPLE_STRIDE, ::SAMPLE_STRIDE].numpy().astype(np.float32)


def config():
    from oracle import lama_oracle as O
    return O.small_config(ngf=8, n_blocks=3)


def make_case(h, w, gray_stroke=False):
    """The padded image / mask batch of one case (what the dataset hands refine_predict, + unpad_to_size = (h, w))."""
    from oracle import lama_oracle as O
    g = torch.Generator().manual_seed(h * 1000 + w)
    low = torch.rand(1, 3, max(h // 16, 2), max(w // 16, 2), generator=g)
    image = F.interpolate(low, size=(h, w), mode='bilinear', align_corners=False)
    image = (image + 0.05 * torch.rand(1, 3, h, w, generator=g)).clamp(0, 1)
    mask = torch.zeros(1, 1, h, w)
    mask[:, :, h // 5:h // 2, w // 4:(2 * w) // 3] = 1.0
    mask[:, :, (3 * h) // 5:(3 * h) // 5 + max(h // 40, 2), w // 8:(7 * w) // 8] = 0.5 if gray_stroke else 1.0
    ph, pw = O.ceil_modulo(h, 8), O.ceil_modulo(w, 8)
    image_p = F.pad(image, (0, pw - w, 0, ph - h), mode='reflect')
    mask_p = F.pad(mask, (0, pw - w, 0, ph - h), mode='reflect')
    return image_p, mask_p


class _TorchProxy:
    """``torch`` as the reference module sees it: everything forwarded, ``device(...)`` always the CPU."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def device(*a, **kw):
        return torch.device('cpu')


class _Bar:
    def __init__(self, it):
        self.it = it

    def __iter__(self):
        return iter(self.it)

    def set_description(self, *_a, **_kw):
        pass


class _Inpainter:
    """What refine_predict touches of DefaultInpaintingTrainingModule (refinement.py:262-289)."""
    training = False
    add_noise_kwargs = None
    concat_mask = True

    def __init__(self, generator):
        self.generator = generator


def import_reference(ref):
    """The reference's refinement module and generator factory, with the stubs above."""
    from oracle import refine_oracle as R

    def mod(name, **attrs):
        m = types.ModuleType(name)
        for a, v in attrs.items():
            setattr(m, a, v)
        sys.modules[name] = m
        return m

    def blur(x, kernel_size, sigma):
        assert tuple(kernel_size) == (5, 5) and tuple(sigma) == (1.0, 1.0)
        return R.gaussian_blur2d(x, 5, 1.0)

    def resize(x, size, interpolation='bilinear', align_corners=False):
        assert interpolation == 'bilinear' and align_corners is False
        return F.interpolate(x, size=size, mode='bilinear', align_corners=False)

    def get_se(shape, ksize):
        assert shape == 2 and tuple(ksize) == (15, 15)
        return R.ellipse_kernel(15).numpy().astype(np.uint8)

    k = mod('kornia')
    k.filters = mod('kornia.filters', gaussian_blur2d=blur)
    k.geometry = mod('kornia.geometry')
    k.geometry.transform = mod('kornia.geometry.transform', resize=resize,
                               rotate=lambda *a, **kw: (_ for _ in ()).throw(RuntimeError('stub')))
    k.morphology = mod('kornia.morphology', erosion=lambda x, kern: R.erosion(x, kern))
    mod('cv2', getStructuringElement=get_se, MORPH_ELLIPSE=2, INTER_AREA=3)
    mod('easydict', EasyDict=type('EasyDict', (dict,), {}))
    mod('pytorch_lightning', seed_everything=lambda *a, **kw: None)
    sys.path.insert(0, ref)
    import saicinpainting                                                            # the reference's (empty) top-level package
    ev = mod('saicinpainting.evaluation')
    ev.__path__ = [os.path.join(ref, 'saicinpainting', 'evaluation')]
    saicinpainting.evaluation = ev
    from saicinpainting.evaluation import refinement as ref_refinement               # UNMODIFIED reference file
    from saicinpainting.training.modules import make_generator
    assert os.path.realpath(ref_refinement.__file__).startswith(os.path.realpath(ref))
    ref_refinement.torch = _TorchProxy()
    ref_refinement.tqdm = lambda it, **kw: _Bar(it)
    return ref_refinement, make_generator


def main(ref):
    from oracle import lama_oracle as O
    from oracle import refine_oracle as R
    torch.set_num_threads(1)
    ref_refinement, make_generator = import_reference(ref)
    cfg = config()
    sd = O.make_synthetic_state_dict(cfg, seed=SEED_SD, calib_hw=32)
    gen = make_generator(None, kind='ffc_resnet', **cfg)
    res = gen.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    gen.eval()
    for p in gen.parameters():
        p.requires_grad_(False)                                                       # = LightningModule.freeze() (bin/predict.py:60)
    out = {}
    for i, (h, w, kw, gray) in enumerate(CASES):
        image_p, mask_p = make_case(h, w, gray)
        batch = {'image': image_p.clone(), 'mask': mask_p.clone(), 'unpad_to_size': [torch.tensor([h]), torch.tensor([w])]}
        want = ref_refinement.refine_predict(batch, _Inpainter(gen), gpu_ids='0,', modulo=8, n_iters=N_ITERS, lr=LR, **kw)
        got = R.refine_predict(image_p.clone(), mask_p.clone(), (h, w), sd, cfg, modulo=8, n_iters=N_ITERS, lr=LR, **kw)
        assert torch.equal(got, want), (i, float((got - want).abs().max()))
        assert want.dtype == torch.float32
        out[f'shape{i}'] = np.array(want.shape, dtype=np.int64)
        out[f'sha256_{i}'] = digest(want)
        out[f'sample{i}'] = sample(want)
        print(f'case {i} ({h}x{w}): reference output {tuple(want.shape)}, oracle equal', flush=True)
    np.savez_compressed(os.path.join(HERE, 'refine_pin.npz'), **out)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit('usage: make_golden_refine_pin.py <root of the reference LaMa checkout>')
    main(os.path.abspath(sys.argv[1]))
