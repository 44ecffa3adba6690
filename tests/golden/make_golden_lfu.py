#!/usr/bin/env python3
"""Golden vectors of the local Fourier unit (enable_lfu=True) from the REFERENCE's own classes.

Runs only in the build container (needs the reference checkout).  The reference ``saicinpainting/training/modules/ffc.py`` is imported
unmodified with the two import stubs make_golden.py uses (restated here).  Weights are seeded by tests/lfu_util.py (the tests regenerate
them); the oracle does not know the LFU, so the running statistics of every ``lfu.bn`` are CALIBRATED here by one pass of the reference
module -- a forward pre-hook sets them to the mean / variance of the BatchNorm's input, which makes the LFU's spectrum O(1) and its
output comparable to x1 + fu(x1) -- and stored.  The script asserts that max|tile(xs)| is at least 10 % of max|x1 + fu(x1)| in every unit
case: a missing tile-add must not hide under the tolerances.

  lfu.npz            st8_y, st10_y             SpectralTransform(32, 32, enable_lfu=True) on [2, 32, 8, 8] and [2, 32, 10, 10] (5 x 5 LFU planes)
                     blk_*                     FFCResnetBlock(64, ratios 0.75, LFU) on 12 x 12 planes: block output, its conv1 (FFC_BN_ACT) output,
                                               the bare FFC of conv1, its SpectralTransform
                     gen_<case>_*              the small generator (ngf 8, two blocks, resnet_conv_kwargs.enable_lfu) on [1, 4, 64, 64],
                                               [2, 4, 80, 80], [1, 4, 96, 96]: output and per-layer taps
                     <tag>_bn_<key>            the calibrated lfu.bn statistics
  lfu_block512.npz   FFCResnetBlock(512, ratios 0.75, LFU) on [1, 512, 64, 64] (32 x 32 LFU planes): strided samples ([:, :, 1::8, ::4]) +
                     (mean, std, absmax) of block output, conv1 layer output, SpectralTransform output; the calibrated statistics
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, ROOT)


def import_reference():
    if 'kornia' not in sys.modules:
        k, kg, kt = types.ModuleType('kornia'), types.ModuleType('kornia.geometry'), types.ModuleType('kornia.geometry.transform')
        kt.rotate = lambda *a, **kw: (_ for _ in ()).throw(RuntimeError('stub'))
        k.geometry, kg.transform = kg, kt
        sys.modules.update({'kornia': k, 'kornia.geometry': kg, 'kornia.geometry.transform': kt})
    if 'pytorch_lightning' not in sys.modules:
        pl = types.ModuleType('pytorch_lightning')
        pl.seed_everything = lambda *a, **kw: None
        sys.modules['pytorch_lightning'] = pl
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from saicinpainting.training.modules import ffc as ref_ffc
    from saicinpainting.training.modules import make_generator
    return ref_ffc, make_generator


def observe(module, run, calibrate: bool = False):
    """One pass of ``run()``; returns, per SpectralTransform call, the share of the LFU term: max|tile(xs)| / max|x1 + fu(x1)| (ffc.py:161
    adds the three terms in front of conv2).  ``calibrate``: every lfu.bn first takes the statistics of its own input."""
    ref_ffc, _ = import_reference()
    hooks, shares = [], []

    def pre(bn, inp):
        x = inp[0]
        bn.running_mean.copy_(x.mean(dim=(0, 2, 3)))
        bn.running_var.copy_(x.var(dim=(0, 2, 3), unbiased=False))

    for m in module.modules():
        if isinstance(m, ref_ffc.SpectralTransform):
            if calibrate:
                hooks.append(m.lfu.bn.register_forward_pre_hook(pre))
            seen = {}
            for key, sub in (('x1', m.conv1), ('fu', m.fu), ('xs', m.lfu)):
                hooks.append(sub.register_forward_hook(lambda mod, i, o, seen=seen, key=key: seen.__setitem__(key, o.detach().clone())))
            hooks.append(m.conv2.register_forward_hook(
                lambda mod, i, o, seen=seen: shares.append(float(seen['xs'].abs().max() / (seen['x1'] + seen['fu']).abs().max()))))
    with torch.no_grad():
        run()
    for h in hooks:
        h.remove()
    return shares


def stat(t):
    t = t.double()
    return np.array([t.mean().item(), t.std().item(), t.abs().max().item()])


def main():
    from tests import lfu_util as U
    ref_ffc, make_generator = import_reference()
    out = {}

    # ---- SpectralTransform(32, 32, enable_lfu=True) ------------------------------------------------------------------------------------------
    st = ref_ffc.SpectralTransform(32, 32, enable_lfu=True).eval()
    st.load_state_dict(U.seeded_entries(st, 11), strict=True)
    shares = observe(st, lambda: st(U.unit_input('st8')), calibrate=True)
    for tag in U.ST_CASES:
        shares += observe(st, lambda tag=tag: out.__setitem__(tag + '_y', st(U.unit_input(tag)).numpy()))
    out.update({'st_bn_' + k: v.numpy() for k, v in U.lfu_bn_stats(st.state_dict()).items()})

    # ---- FFCResnetBlock(64) / FFC_BN_ACT / FFC / SpectralTransform with the LFU on 12 x 12 planes ----------------------------------------------
    blk = ref_ffc.FFCResnetBlock(U.BLOCK_DIM, **U.BLOCK_KW).eval()
    blk.load_state_dict(U.seeded_entries(blk, 13), strict=True)
    xl, xg = U.block_input()
    shares += observe(blk, lambda: blk((xl, xg)), calibrate=True)

    def units():
        yl, yg = blk((xl, xg))
        l1, g1 = blk.conv1((xl, xg))
        fl, fg = blk.conv1.ffc((xl, xg))
        stv = blk.conv1.ffc.convg2g(xg)
        out.update(blk_yl=yl.numpy(), blk_yg=yg.numpy(), blk_c1_l=l1.numpy(), blk_c1_g=g1.numpy(), blk_ffc_l=fl.numpy(), blk_ffc_g=fg.numpy(),
                   blk_st=stv.numpy())
    shares += observe(blk, units)
    out.update({'blk_bn_' + k: v.numpy() for k, v in U.lfu_bn_stats(blk.state_dict()).items()})
    assert min(shares) >= 0.1, shares
    print('LFU share of t, unit cases: min %.3f max %.3f' % (min(shares), max(shares)))

    # ---- the small generator ---------------------------------------------------------------------------------------------------------------
    gen = make_generator(None, kind='ffc_resnet', **U.small_lfu_config()).eval()
    res = gen.load_state_dict(U.small_lfu_state_dict(gen), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    gshares = observe(gen, lambda: gen(U.gen_input('b')), calibrate=True)
    for case in U.GEN_CASES:
        x = U.gen_input(case)
        with torch.no_grad():
            taps = {}
            z = x
            for i, layer in enumerate(gen.model):
                z = layer(z)
                taps[i] = z
        out[f'gen_{case}_y'] = z.numpy()
        for i in U.GEN_TAPS[case]:
            t = taps[i]
            if isinstance(t, tuple):
                out[f'gen_{case}_tap{i}_l'], out[f'gen_{case}_tap{i}_g'] = t[0].numpy(), t[1].numpy()
            else:
                out[f'gen_{case}_tap{i}'] = t.numpy()
    out.update({'gen_bn_' + k: v.numpy() for k, v in U.lfu_bn_stats(gen.state_dict()).items()})
    print('LFU share of t, generator (calibration pass):', ['%.3f' % s for s in gshares])
    path = os.path.join(HERE, 'lfu.npz')
    np.savez_compressed(path, **out)
    print('written', path, os.path.getsize(path), 'bytes')

    # ---- FFCResnetBlock(512) at the bottleneck shape ------------------------------------------------------------------------------------------
    blk = ref_ffc.FFCResnetBlock(512, **U.BLOCK_KW).eval()
    blk.load_state_dict(U.block512_state_dict(blk), strict=True)
    xl, xg = U.block512_input()
    s512 = observe(blk, lambda: blk((xl, xg)), calibrate=True)
    big = {}
    with torch.no_grad():
        yl, yg = blk((xl, xg))
        l1, g1 = blk.conv1((xl, xg))
        stv = blk.conv1.ffc.convg2g(xg)
    for name, t in dict(yl=yl, yg=yg, c1_l=l1, c1_g=g1, st=stv).items():
        big[name + '_sample'] = U.sample512(t)
        big[name + '_stat'] = stat(t)
    big.update({'blk_bn_' + k: v.numpy() for k, v in U.lfu_bn_stats(blk.state_dict()).items()})
    assert min(s512) >= 0.1, s512
    path = os.path.join(HERE, 'lfu_block512.npz')
    np.savez_compressed(path, **big)
    print('written', path, os.path.getsize(path), 'bytes; LFU share', ['%.3f' % s for s in s512])


if __name__ == '__main__':
    main()
