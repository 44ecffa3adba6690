#!/usr/bin/env python3
"""Golden vectors of the pix2pixhd_multidilated generator (lama-dilated) from the reference's own classes.

Runs only in the build container (needs the reference tree, see make_golden.py).  The reference ``MultiDilatedGlobalGenerator`` and
``MultidilatedResnetBlock`` (saicinpainting/training/modules/pix2pixhd.py, multidilated_conv.py) are instantiated UNMODIFIED; their weights
are the seeded, BN-calibrated synthetic ones of tests/multidilated_util.py (regenerated from the seed at test time; the checksums pin them).

  multidilated_keys.npz      state-dict key list and shapes of the shipped config (pix2pixhd_multidilated_catin_4dil_9b.yaml)
  multidilated_small.npz     inputs / outputs of a small generator (ngf=16: bottleneck 128 = 4 x 32, 2 blocks, sigmoid) on 1 x 96 x 96 and
                             2 x 72 x 88 (a 9 x 11 bottleneck plane: reflection at pad 8 = H - 1)
  multidilated_block512.npz  strided samples ([:, :, 1::8, ::4]) + (mean, std, absmax) of one MultidilatedResnetBlock(512) on a seeded
                             [2, 512, 64, 64] state
"""
import functools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

SMALL_SEED, BLOCK_SEED, X_SEED = 11, 5, 23


def checksum(sd):
    return np.array([sum(float(v.double().sum()) for v in sd.values() if v.is_floating_point())])


def stat(t):
    t = t.double()
    return np.array([t.mean().item(), t.std().item(), t.abs().max().item()])


def main():
    import torch.nn as nn
    from make_golden_regular import ref_pix2pixhd
    from tests import multidilated_util as M
    ref = ref_pix2pixhd()
    from saicinpainting.training.modules.multidilated_conv import MultidilatedConv
    gen = ref.MultiDilatedGlobalGenerator(**M.LAMA_DILATED)
    sd = gen.state_dict()
    np.savez_compressed(os.path.join(HERE, 'multidilated_keys.npz'), dilated_keys=np.array(list(sd.keys())),
                        dilated_shapes=np.array([','.join(str(d) for d in v.shape) for v in sd.values()]))

    cfg = M.small_config(ngf=16, n_blocks=2)
    sd = M.make_state_dict(cfg, seed=SMALL_SEED)
    gen = ref.MultiDilatedGlobalGenerator(**cfg).eval()
    res = gen.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    out = dict(ngf=np.array([16]), n_blocks=np.array([2]), seed=np.array([SMALL_SEED]), sd_checksum=checksum(sd))
    for name, (b, h, w) in (('a', (1, 96, 96)), ('b', (2, 72, 88))):
        x = M.calib_input(b, h, w, seed=100 + h)
        with torch.no_grad():
            y = gen(x)
        assert float((y - M.forward(sd, cfg, x)).abs().max()) < 1e-5        # the restatement the GPU tests use agrees with the reference
        out[name + '_input'] = x.numpy()
        out[name + '_output'] = y.numpy()
    np.savez_compressed(os.path.join(HERE, 'multidilated_small.npz'), **out)

    bsd = M.block_state_dict(512, seed=BLOCK_SEED)
    conv_layer = functools.partial(MultidilatedConv, comb_mode='cat_in', dilation_num=4)
    blk = ref.MultidilatedResnetBlock(512, padding_type='reflect', conv_layer=conv_layer, norm_layer=nn.BatchNorm2d).eval()
    res = blk.load_state_dict(bsd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    x = M.block_input(2, 512, 64, seed=X_SEED)
    with torch.no_grad():
        y = blk(x)
    assert float((y - M.block_forward(bsd, x)).abs().max()) < 1e-5
    np.savez_compressed(os.path.join(HERE, 'multidilated_block512.npz'), seed=np.array([BLOCK_SEED]), x_seed=np.array([X_SEED]),
                        sd_checksum=checksum(bsd), x_checksum=np.array([float(x.double().sum())]),
                        y_sample=M.sample(y).numpy(), y_stat=stat(y))
    for f in ('multidilated_keys.npz', 'multidilated_small.npz', 'multidilated_block512.npz'):
        print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == '__main__':
    main()
