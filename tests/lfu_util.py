"""Shared by tests/test_lfu_emu.py, tests/test_lfu_gpu.py and tests/golden/make_golden_lfu.py: the torch restatement of the two LFU kernels,
the seeded weights of the LFU fixtures (tests/golden/lfu.npz, lfu_block512.npz store results and the calibrated BatchNorm statistics of the
``lfu.bn`` modules only; everything else is regenerated from seeds here) and the checks both test files run -- on the emulator and on the GPU."""
import copy
import math
import os

import numpy as np
import torch
import torch.nn as nn

from lama_amd import _lib as L
from lama_amd import ffc as F
from oracle import lama_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PRECS = {'f32': L.PREC_F32, 'bf16x3': L.PREC_BF16X3, 'f16x3': L.PREC_F16X3}
# the bars of tests/test_generator_gpu.py for the same kinds of tensors: test_reference_unit_goldens_on_hardware (units, max-abs), the small
# generator's output (TOLS) and per-layer taps (1e-3), test_reference_units_at_biglama_channel_counts_on_hardware (relative to max(1, absmax))
UNIT_TOL = {L.PREC_F32: 5e-5, L.PREC_F16X3: 5e-5, L.PREC_BF16X3: 1e-3}
GEN_TOL = {L.PREC_F32: 2e-4, L.PREC_F16X3: 2e-4, L.PREC_BF16X3: 5e-4}
TAP_TOL = 1e-3
BLOCK512_REL = {L.PREC_F32: 2e-5, L.PREC_F16X3: 2e-5, L.PREC_BF16X3: 4e-4}

ST_CASES = {'st8': (2, 32, 8), 'st10': (2, 32, 10)}           # SpectralTransform(32, 32): x [B, 32, h, h]; 10 x 10 gives 5 x 5 LFU planes
BLOCK_DIM, BLOCK_HW = 64, 12                                   # FFC_BN_ACT / FFCResnetBlock(64, ratios 0.75) on 12 x 12 planes
GEN_CASES = {'a': (1, 64), 'b': (2, 80), 'c': (1, 96)}         # the small generator: [B, 4, S, S]
GEN_TAPS = {'a': (4, 5, 6, 7, 10, 13), 'b': (4, 5, 6, 7), 'c': (4, 5, 6, 7)}
BLOCK_KW = dict(padding_type='reflect', norm_layer=nn.BatchNorm2d, activation_layer=nn.ReLU, ratio_gin=0.75, ratio_gout=0.75, enable_lfu=True)


# ---- the two kernels, restated with torch indexing ---------------------------------------------------------------------------------------
def gather_ref(x: torch.Tensor) -> torch.Tensor:
    """x [B, q, h, h] -> [B, 4q, h/2, h/2]: y[b, (2j + i) q + c, yy, xx] = x[b, c, i s + yy, j s + xx]."""
    B, q, h, _ = x.shape
    s = h // 2
    y = torch.empty(B, 4 * q, s, s, dtype=x.dtype, device=x.device)
    for j in range(2):
        for i in range(2):
            y[:, (2 * j + i) * q:(2 * j + i + 1) * q] = x[:, :, i * s:(i + 1) * s, j * s:(j + 1) * s]
    return y


def tile_add_ref(a: torch.Tensor, xs: torch.Tensor) -> torch.Tensor:
    """a + tile(xs): one add per element (fp16: torch widens, adds and rounds once)."""
    s = xs.shape[2]
    idx = torch.arange(a.shape[2], device=a.device) % s
    return a + xs[:, :, idx][:, :, :, idx]


# ---- seeded weights ------------------------------------------------------------------------------------------------------------------------
def seeded_entries(module: nn.Module, seed: int, only: str = '') -> dict:
    """Seeded values for the state-dict entries of ``module`` whose key contains ``only`` (the reference's classes and lama_amd's have the
    same keys and shapes): conv weights N(0, 1 / fan_in), BatchNorm weight U(0.5, 1.5), bias N(0, 0.04), mean N(0, 0.01), var U(0.5, 1.5)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    sd = module.state_dict()
    for k in sorted(sd):
        if only not in k:
            continue
        v = sd[k]
        if k.endswith('num_batches_tracked'):
            out[k] = torch.zeros_like(v)
        elif k.endswith('running_mean'):
            out[k] = torch.randn(v.shape, generator=g) * 0.1
        elif k.endswith('running_var'):
            out[k] = torch.rand(v.shape, generator=g) + 0.5
        elif k.endswith('.bias'):
            out[k] = torch.randn(v.shape, generator=g) * 0.2
        elif v.dim() == 1:
            out[k] = torch.rand(v.shape, generator=g) + 0.5
        else:
            out[k] = torch.randn(v.shape, generator=g) / math.sqrt(v[0].numel())
    return out


def lfu_bn_stats(sd: dict) -> dict:
    """The entries a golden file stores: the calibrated running statistics of every ``lfu.bn``."""
    return {k: v for k, v in sd.items() if '.lfu.bn.running_' in k or k.startswith('lfu.bn.running_')}


def stored_stats(g, tag: str) -> dict:
    return {k[len(tag) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(tag + '_bn_')}


def unit_input(tag: str) -> torch.Tensor:
    b, c, h = ST_CASES[tag]
    return torch.randn(b, c, h, h, generator=torch.Generator().manual_seed(100 + h))


def block_input():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, BLOCK_DIM, BLOCK_HW, BLOCK_HW, generator=g)
    return x[:, :16].contiguous(), x[:, 16:].contiguous()


def small_lfu_config() -> dict:
    cfg = copy.deepcopy(O.small_config(ngf=8, n_blocks=2))
    cfg['resnet_conv_kwargs']['enable_lfu'] = True
    return cfg


def small_lfu_state_dict(gen: nn.Module, stats: dict = None) -> dict:
    """The small LFU generator's weights: the seeded synthetic state dict of the same generator WITHOUT the LFU (the oracle does not know
    it), seeded ``lfu.*`` entries, and -- when given -- the stored statistics of the ``lfu.bn`` modules."""
    sd = dict(O.make_synthetic_state_dict(O.small_config(ngf=8, n_blocks=2), seed=7, calib_hw=32))
    sd.update(seeded_entries(gen, 31, only='.lfu.'))
    sd.update(stats or {})
    return sd


def gen_input(case: str) -> torch.Tensor:
    b, s = GEN_CASES[case]
    batch = O.make_synthetic_batch(b, s, s, seed=40 + s)
    return torch.cat([batch['image'] * (1 - batch['mask']), batch['mask']], 1)


def block512_state_dict(blk: nn.Module, stats: dict = None) -> dict:
    """FFCResnetBlock(512) with the LFU: seeded entries + the stored statistics of the two ``lfu.bn``."""
    bsd = seeded_entries(blk, 33)
    bsd.update(stats or {})
    return bsd


def block512_input():
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, 512, 64, 64, generator=g).abs()
    x[:, 130] *= 4.0
    return x[:, :128].contiguous(), x[:, 128:].contiguous()


def sample512(t: torch.Tensor) -> np.ndarray:
    return t[:, :, 1::8, ::4].contiguous().numpy()


# ---- kernel checks (the library under test is ``lib``; tensors live on ``dev``) ----------------------------------------------------------------
CANARY = 12288.0          # (exact in fp16)
KERNEL_SHAPES = [(2, 8, 6, 'plain'), (1, 16, 8, 'slice'), (3, 8, 64, 'plain'), (1, 4, 130, 'plain')]      # B, C, h


def _guarded(shape, dtype, dev, pad_c: int = 0, pad_b: int = 0):
    """A [B, C, H, W] view inside a canary-filled buffer: ``pad_c`` extra channels on either side (a channel slice) and ``pad_b`` extra
    elements per image (a padded batch_stride), plus a guard band in front of and behind everything.  Returns (flat buffer, L.Tensor4, view)."""
    B, C, H, W = shape
    ct = C + 2 * pad_c
    bs = ct * H * W + pad_b
    guard = 64
    flat = torch.full((guard + B * bs + guard,), CANARY, dtype=dtype, device=dev)
    off = guard + pad_c * H * W
    t = torch.as_strided(flat, (B, C, H, W), (bs, H * W, W, 1), off)
    v = L.Tensor4(flat.data_ptr() + flat.element_size() * off, bs, C, H, W, L.DT_F16 if dtype == torch.float16 else L.DT_F32)
    return flat, v, t


def _outside_untouched(flat, t):
    mask = torch.ones_like(flat, dtype=torch.bool)
    torch.as_strided(mask, t.shape, t.stride(), t.storage_offset()).fill_(False)
    return bool((flat[mask] == CANARY).all())


def check_kernels(lib, dev, B, C, h, layout, dtype):
    """Both entries against the restatement, bit for bit, with canaries around every output; the tile-add out of place and in place."""
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + h)
    s, q = h // 2, C // 4
    pad_c, pad_b = (4, 24) if layout == 'slice' else (0, 0)
    x1 = torch.randn(B, C, h, h, generator=g).to(dtype).to(dev)
    fx, vx, tx = _guarded((B, C, h, h), dtype, dev, pad_c, pad_b)
    tx.copy_(x1)
    # gather: the first quarter of x1's channels as a view with x1's batch stride
    vq = L.Tensor4(vx.ptr, vx.batch_stride, q, h, h, vx.dtype)
    fy, vy, ty = _guarded((B, 4 * q, s, s), dtype, dev, pad_c, pad_b)
    lib.lfu_gather(vq, vy, B)
    assert torch.equal(ty, gather_ref(x1[:, :q])), 'gather'
    assert _outside_untouched(fy, ty) and torch.equal(tx, x1)
    # tile-add, out of place then in place
    xs = torch.randn(B, C, s, s, generator=g).to(dtype).to(dev)
    fs, vs, ts = _guarded((B, C, s, s), dtype, dev, pad_c, pad_b)
    ts.copy_(xs)
    want = tile_add_ref(x1, xs)
    fo, vo, to = _guarded((B, C, h, h), dtype, dev, pad_c, pad_b)
    lib.lfu_tile_add(vx, vs, vo, B)
    assert torch.equal(to, want), 'tile_add'
    assert _outside_untouched(fo, to) and torch.equal(tx, x1) and torch.equal(ts, xs)
    lib.lfu_tile_add(vx, vs, vx, B)
    assert torch.equal(tx, want), 'tile_add in place'
    assert _outside_untouched(fx, tx) and _outside_untouched(fs, ts)


def check_refusals(lib, dev):
    """Every refusal returns its code and leaves the outputs as they were."""
    def t4(shape, dtype=torch.float32):
        return _guarded(shape, dtype, dev)

    fx, vx, _ = t4((2, 2, 8, 8))
    fy, vy, _ = t4((2, 8, 4, 4))
    fa, va, _ = t4((2, 8, 8, 8))
    fs, vs, _ = t4((2, 8, 4, 4))
    fo, vo, _ = t4((2, 8, 8, 8))
    outs = (fy, fo)

    def mod(v, **kw):
        w = L.Tensor4(v.ptr, v.batch_stride, v.C, v.H, v.W, v.dtype)
        for k, val in kw.items():
            setattr(w, k, val)
        return w

    def refused(code, fn, *a):
        try:
            fn(*a)
        except L.LamaError as e:
            assert e.code == code, (e.code, code, a)
        else:
            raise AssertionError('not refused')
        assert all(bool((f == CANARY).all()) for f in outs)

    bad, uns = L.ERR_BAD_ARG, L.ERR_UNSUPPORTED
    null = L.Tensor4(None, 0, 2, 8, 8, L.DT_F32)
    refused(bad, lib.lfu_gather, null, vy, 2)
    refused(bad, lib.lfu_gather, vx, vy, 0)
    refused(bad, lib.lfu_gather, vx, mod(vy, C=4), 2)                       # not 4 q channels
    refused(bad, lib.lfu_gather, vx, mod(vy, H=3), 2)
    refused(bad, lib.lfu_gather, mod(vx, batch_stride=2 * 64 - 1), vy, 2)
    refused(bad, lib.lfu_gather, vx, mod(vy, batch_stride=8 * 16 - 1), 2)
    refused(uns, lib.lfu_gather, mod(vx, W=6), vy, 2)                       # H != W
    refused(uns, lib.lfu_gather, mod(vx, H=7, W=7), mod(vy, H=3, W=3), 2)   # odd side
    refused(uns, lib.lfu_gather, mod(vx, dtype=L.DT_SPLIT16), mod(vy, dtype=L.DT_SPLIT16), 2)
    refused(uns, lib.lfu_gather, mod(vx, dtype=7), mod(vy, dtype=7), 2)
    refused(uns, lib.lfu_gather, vx, mod(vy, dtype=L.DT_F16), 2)            # mixed
    refused(bad, lib.lfu_tile_add, va, vs, null, 2)
    refused(bad, lib.lfu_tile_add, va, vs, vo, -1)
    refused(bad, lib.lfu_tile_add, va, mod(vs, C=4), vo, 2)
    refused(bad, lib.lfu_tile_add, va, mod(vs, H=2, W=2), vo, 2)
    refused(bad, lib.lfu_tile_add, va, vs, mod(vo, batch_stride=8 * 64 - 1), 2)
    refused(uns, lib.lfu_tile_add, mod(va, H=8, W=4), vs, mod(vo, H=8, W=4), 2)
    refused(uns, lib.lfu_tile_add, mod(va, H=6, W=6), mod(vs, H=3, W=3), mod(vo, H=6, W=6, dtype=L.DT_F16), 2)
    refused(uns, lib.lfu_tile_add, mod(va, dtype=L.DT_SPLIT16), mod(vs, dtype=L.DT_SPLIT16), mod(vo, dtype=L.DT_SPLIT16), 2)


# ---- module checks -------------------------------------------------------------------------------------------------------------------------
def _err(a: torch.Tensor, want: np.ndarray) -> float:
    return float(np.abs(a.float().cpu().numpy() - want).max())


def check_units(prepare, dev, prec):
    """SpectralTransformLFU, FFC_BN_ACT and FFCResnetBlock with the LFU against tests/golden/lfu.npz (the reference's own classes).
    ``prepare(module)`` moves a loaded module to the device / exec under test."""
    g = np.load(os.path.join(GOLDEN, 'lfu.npz'))
    tol = UNIT_TOL[prec]
    st = F.SpectralTransformLFU(32, 32)
    assert st.enable_lfu is True
    sd = seeded_entries(st, 11)
    sd.update(stored_stats(g, 'st'))
    st.load_state_dict(sd, strict=True)
    prepare(st).set_precision(prec)
    for tag in ST_CASES:
        e = _err(st(unit_input(tag).to(dev)), g[tag + '_y'])
        print(f'lfu unit {tag}: max-abs {e:.3e} (bar {tol:g})')
        assert e < tol, (tag, e)
    blk = F.FFCResnetBlock(BLOCK_DIM, **BLOCK_KW)
    assert isinstance(blk.conv1.ffc.convg2g, F.SpectralTransformLFU)
    sd = seeded_entries(blk, 13)
    sd.update(stored_stats(g, 'blk'))
    blk.load_state_dict(sd, strict=True)
    prepare(blk).set_precision(prec)
    xl, xg = (t.to(dev) for t in block_input())
    yl, yg = blk((xl, xg))
    l1, g1 = blk.conv1((xl, xg))
    fl, fg = blk.conv1.ffc((xl, xg))                                      # the bare FFC: no BatchNorm, no activation
    stv = blk.conv1.ffc.convg2g(xg)
    for a, key in ((yl, 'blk_yl'), (yg, 'blk_yg'), (l1, 'blk_c1_l'), (g1, 'blk_c1_g'), (fl, 'blk_ffc_l'), (fg, 'blk_ffc_g'), (stv, 'blk_st')):
        e = _err(a, g[key])
        print(f'lfu unit {key}: max-abs {e:.3e} (bar {tol:g})')
        assert e < tol, (key, e)
    yl2, yg2 = blk((xl, xg))          # the fused packing is restored after the stand-alone calls
    assert torch.equal(yl2, yl) and torch.equal(yg2, yg)
    for shape in ((1, 48, 8, 12), (1, 48, 7, 7)):                           # planes the reference's LFU does not take: refused before any launch
        try:
            blk.conv1.ffc.convg2g(torch.zeros(shape, device=dev))
        except F.LamaError as e:
            assert 'h // 2' in str(e) and f'{shape[2]} x {shape[3]}' in str(e)
        else:
            raise AssertionError('not refused')
    try:
        F.SpectralTransformLFU(36, 36)                                     # 18 channels: not a multiple of 4
    except NotImplementedError:
        pass
    else:
        raise AssertionError('C % 4 != 0 accepted')


def small_generator(prepare):
    from lama_amd.modules import make_generator
    g = np.load(os.path.join(GOLDEN, 'lfu.npz'))
    gen = make_generator(None, kind='ffc_resnet', **small_lfu_config())
    sd = small_lfu_state_dict(gen, stored_stats(g, 'gen'))
    res = gen.load_state_dict(sd, strict=True)                              # the reference's keys, convg2g.lfu.* included
    assert not res.missing_keys and not res.unexpected_keys
    assert any('.convg2g.lfu.conv_layer.weight' in k for k in sd) and any('.convg2g.lfu.bn.running_var' in k for k in sd)
    return prepare(gen), sd, g


def check_generator_golden(gen, g, dev, prec, case):
    gen.set_precision(prec)
    x = gen_input(case).to(dev)
    e = _err(gen(x), g[f'gen_{case}_y'])
    print(f'lfu generator {case}: output max-abs {e:.3e} (bar {GEN_TOL[prec]:g})')
    assert e < GEN_TOL[prec], (case, e)
    z = x
    for i, layer in enumerate(gen.model):
        z = layer(z)
        if i not in GEN_TAPS[case]:
            continue
        for part, zz in (('_l', z[0]), ('_g', z[1])) if isinstance(z, tuple) else (('', z),):
            e = _err(zz, g[f'gen_{case}_tap{i}{part}'])
            print(f'lfu generator {case}: tap {i}{part} max-abs {e:.3e} (bar {TAP_TOL:g})')
            assert e < TAP_TOL, (case, i, part, e)


def check_generator_plans(gen, sd, dev, graph: bool):
    """Eager against graph replay, the split plan against the one-part plan (bit for bit), strict loading, the refused plane."""
    from lama_amd.modules import make_generator
    gen.set_precision(L.PREC_F16X3)
    x = gen_input('b').to(dev)
    keep = (gen.use_graph, gen.split_batch, gen.verify_split)
    try:
        gen.use_graph, gen.split_batch, gen.verify_split = False, 1, False
        gen._plans.clear()
        ref = gen(x).clone()
        assert 'lfu' in next(iter(gen._plans.values()))['scratch']
        if graph:
            gen.use_graph = True
            gen._plans.clear()
            assert torch.equal(gen(x), ref) and torch.equal(gen(x), ref), 'graph replay'
        gen.split_batch = 2
        gen._plans.clear()
        assert torch.equal(gen(x), ref) and torch.equal(gen(x), ref), 'split plan'
        assert next(iter(gen._plans.values()))['nsplit'] == 2
    finally:
        gen.use_graph, gen.split_batch, gen.verify_split = keep
        gen._plans.clear()
    bare = {k: v for k, v in sd.items() if '.lfu.' not in k}
    other = make_generator(None, kind='ffc_resnet', **small_lfu_config())
    try:
        other.load_state_dict(bare, strict=True)
    except RuntimeError as e:
        assert 'lfu' in str(e)
    else:
        raise AssertionError('a state dict without lfu.* passed strict loading')
    launched = []
    real = gen._exec.lib.conv2d
    gen._exec.lib.conv2d = lambda *a, **kw: launched.append(1) or real(*a, **kw)
    try:
        gen(torch.zeros(1, 4, 64, 96, device=dev))
    except F.LamaError as e:
        assert 'h // 2' in str(e) and '8 x 12' in str(e)
    else:
        raise AssertionError('a 64 x 96 input was not refused')
    finally:
        gen._exec.lib.conv2d = real
    assert not launched, 'something was launched before the refusal'


def check_probe_and_refusals(gen, dev):
    from lama_amd import probe, refinement
    gen.set_precision(L.PREC_F16X3)
    rep = probe.probe_ranges(gen, gen_input('a').to(dev))
    names = rep.names()
    for lay in ('model.5.conv1', 'model.5.conv2', 'model.6.conv1', 'model.6.conv2'):
        p = lay + '.ffc.convg2g'
        for row in (p + '.lfu:in', p + '.lfu:spectrum', p + '.lfu:spectrum_out'):
            assert row in names, row
        assert names.index(p + '.fu:spectrum_out') < names.index(p + '.lfu:in') < names.index(p + ':t')
        assert rep[p + '.lfu:spectrum'].shape == (1, 48, 4, 3) and rep[p + '.lfu:in'].shape == (1, 24, 4, 4)
        assert rep[p + '.lfu:spectrum'].abs_max > 0 and not rep[p + '.lfu:spectrum'].bad

    class _Inpainter:
        training, concat_mask, generator = False, True, gen

    for fn in (refinement.refine_predict, refinement.refine_predict_batch):
        try:
            fn(dict(image=torch.zeros(1, 3, 64, 64, device=dev), mask=torch.zeros(1, 1, 64, 64, device=dev)), _Inpainter(), '0', 8, 1, 0.002, 32, 2, 10 ** 6)
        except NotImplementedError as e:
            assert 'lfu' in str(e).lower()
        else:
            raise AssertionError('refinement of an LFU generator was not refused')
    try:
        F.SpectralTransform(8, 8, enable_lfu=True)
    except NotImplementedError as e:
        assert 'SpectralTransformLFU' in str(e)
    else:
        raise AssertionError('a direct SpectralTransform(enable_lfu=True) was accepted')


def check_block512(blk, dev, prec):
    g = np.load(os.path.join(GOLDEN, 'lfu_block512.npz'))
    xl, xg = (t.to(dev) for t in block512_input())
    yl, yg = blk((xl, xg))
    l1, g1 = blk.conv1((xl, xg))
    st = blk.conv1.ffc.convg2g(xg)
    for a, key in ((yl, 'yl'), (yg, 'yg'), (l1, 'c1_l'), (g1, 'c1_g'), (st, 'st')):
        err = np.abs(sample512(a.float().cpu()) - g[key + '_sample']).max()
        bar = BLOCK512_REL[prec] * max(1.0, float(g[key + '_stat'][2]))
        print(f'lfu block512 {key}: max-abs {err:.3e} (bar {bar:.3e})')
        assert err < bar, (key, err)
