#!/usr/bin/env python3
"""Golden vectors of the pix2pixhd_global generator (big-lama-regular / lama-regular) from the reference's own classes.

Runs only in the build container (needs the reference tree, see make_golden.py).  The reference ``GlobalGenerator`` and ``ResnetBlock``
(saicinpainting/training/modules/pix2pixhd.py) are instantiated UNMODIFIED; their weights are the seeded, BN-calibrated synthetic ones of
tests/regular_util.py (regenerated from the seed at test time; the checksums pin them).

  regular_keys.npz      state-dict key lists and shapes of the big-lama-regular (15 blocks) and lama-regular (9 blocks) generators
  regular_small.npz     inputs / outputs of a small generator (ngf=16: bottleneck 128, 2 blocks, sigmoid) on 1 x 64 x 64 and 2 x 56 x 72
  regular_block512.npz  strided samples ([:, :, 1::8, ::4]) + (mean, std, absmax) of one ResnetBlock(512) on a seeded [2, 512, 64, 64] state
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

SMALL_SEED, BLOCK_SEED, X_SEED = 7, 3, 21


def ref_pix2pixhd():
    from make_golden import import_reference
    import_reference()                                   # the stubs + the reference on sys.path
    from saicinpainting.training.modules import pix2pixhd
    return pix2pixhd


def checksum(sd):
    return np.array([sum(float(v.double().sum()) for v in sd.values() if v.is_floating_point())])


def stat(t):
    t = t.double()
    return np.array([t.mean().item(), t.std().item(), t.abs().max().item()])


def main():
    import torch.nn as nn
    from tests import regular_util as R
    ref = ref_pix2pixhd()
    keys = {}
    for name, cfg in (('big', R.BIG_LAMA_REGULAR), ('regular', R.LAMA_REGULAR)):
        gen = ref.GlobalGenerator(**{k: v for k, v in cfg.items()})
        sd = gen.state_dict()
        keys[name + '_keys'] = np.array(list(sd.keys()))
        keys[name + '_shapes'] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
    np.savez_compressed(os.path.join(HERE, 'regular_keys.npz'), **keys)

    cfg = R.small_config(ngf=16, n_blocks=2)
    sd = R.make_state_dict(cfg, seed=SMALL_SEED, calib_hw=32)
    gen = ref.GlobalGenerator(**cfg).eval()
    res = gen.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    out = dict(ngf=np.array([16]), n_blocks=np.array([2]), seed=np.array([SMALL_SEED]), sd_checksum=checksum(sd))
    for name, (b, h, w) in (('a', (1, 64, 64)), ('b', (2, 56, 72))):
        x = R.calib_input(b, h, w, seed=100 + h)
        with torch.no_grad():
            y = gen(x)
        assert float((y - R.forward(sd, cfg, x)).abs().max()) < 1e-5        # the restatement the GPU tests use agrees with the reference
        out[name + '_input'] = x.numpy()
        out[name + '_output'] = y.numpy()
    np.savez_compressed(os.path.join(HERE, 'regular_small.npz'), **out)

    bsd = R.block_state_dict(512, seed=BLOCK_SEED)
    blk = ref.ResnetBlock(512, padding_type='reflect', norm_layer=nn.BatchNorm2d).eval()
    res = blk.load_state_dict(bsd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    x = R.block_input(2, 512, 64, seed=X_SEED)
    with torch.no_grad():
        y = blk(x)
    assert float((y - R.block_forward(bsd, x)).abs().max()) < 1e-5
    np.savez_compressed(os.path.join(HERE, 'regular_block512.npz'), seed=np.array([BLOCK_SEED]), x_seed=np.array([X_SEED]),
                        sd_checksum=checksum(bsd), x_checksum=np.array([float(x.double().sum())]),
                        y_sample=R.sample(y).numpy(), y_stat=stat(y))
    for f in ('regular_keys.npz', 'regular_small.npz', 'regular_block512.npz'):
        print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == '__main__':
    main()
