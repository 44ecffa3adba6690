"""Test helper of the LAMA_DT_SPLIT16 activations (include/lama_hip.h; tests/test_presplit_outer_emu.py, tests/test_presplit_outer_gpu.py):
the stem and the stride-2 convs launched through the C ABI with fp32 or pre-split tensors on guarded buffers, and the checks both modules
share.  ``dev`` is 'cpu' with the emulated library and 'cuda' with a GPU build.

Nothing here has a tolerance: a pre-split tensor must hold the bits ``rne16(y)`` / ``rne16(y - hi)`` of the fp32 run (torch's CPU conversions,
fp16 subnormals kept), and whatever is computed FROM it must equal the fp32-fed result with ``torch.equal``.  A launch with a split tensor has
no fallback behind the dedicated kernels (stem7_ws_kernel, the 4 x 1 conv_wr_kernel): anything else returns LAMA_ERR_UNSUPPORTED, which
``LamaLib.check`` raises -- so every successful launch below IS one of the two kernels."""
import functools

import torch

from lama_amd import _lib as L

PRECS = [L.PREC_F16X3, L.PREC_BF16X3]
PREC_ID = {L.PREC_F16X3: 'f16x3', L.PREC_BF16X3: 'bf16x3'}
GUARD = 64                      # fp32 words in front of and behind every output buffer
FILL = -1                       # int32 pattern of the fill: 0xffffffff = an fp32 NaN, two fp16 / bf16 NaNs


def _st(dev):
    return 0 if dev == 'cpu' else torch.cuda.current_stream().cuda_stream


def _sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


def guarded(shape, dev):
    """(flat int32 buffer filled with FILL, the fp32 [B, C, H, W] view behind GUARD words of it)."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    return flat, flat[GUARD:GUARD + n].view(torch.float32).view(shape)


def assert_guards(flat, what):
    h = flat.cpu()
    assert bool((h[:GUARD] == FILL).all()) and bool((h[-GUARD:] == FILL).all()), f'{what}: a byte outside the tensor was written'


def conv(lib, dev, x, w, bias, stride, pad, prec, x_split=False, y_split=False, pad_mode=L.PAD_REFLECT, act=L.ACT_RELU, scale=None):
    """One lama_conv2d_fwd launch.  ``x``: CPU fp32 [B, C, H, W], or (x_split) the LAMA_DT_SPLIT16 image of it (L.split16_pack).  Returns
    (the output as a CPU fp32-typed [B, M, Ho, Wo] tensor -- split parts if y_split --, range flag, flat guarded buffer)."""
    B, _, H, W = x.shape
    M, k = w.shape[0], w.shape[2]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xd = x.contiguous().to(dev)
    flat, y = guarded((B, M, Ho, Wo), dev)
    wp = lib.pack_conv_weight(w.to(dev), None if scale is None else scale.to(dev), stride=stride, precision=prec)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.conv2d(L.view_split(xd) if x_split else L.view(xd), wp, L.view_split(y) if y_split else L.view(y), B, k, stride, pad, pad_mode, False,
               None if bias is None else bias.to(dev), act, None, precision=prec, stream=_st(dev), range_flag=flag)
    _sync(dev)
    return y.cpu().clone(), int(flag.cpu()), flat


def bits(t):
    return t.contiguous().view(torch.int16)


def assert_split_of(ysplit, y32, prec, what):
    """The layout known-answer check: the unpacked planes are rne16(y) and rne16(y - hi) of the fp32 run, bit for bit."""
    hi, lo = L.split16_unpack(ysplit, prec)
    dt = hi.dtype
    want_hi = y32.to(dt)
    want_lo = (y32 - want_hi.float()).to(dt)
    assert not bool(torch.isnan(hi.float()).any()) and not bool(torch.isnan(lo.float()).any()), f'{what}: part of the tensor was not written'
    for name, got, want in (('hi', hi, want_hi), ('lo', lo, want_lo)):
        if not torch.equal(bits(got), bits(want)):
            bad = (bits(got) != bits(want)).nonzero()
            i = tuple(int(v) for v in bad[0])
            raise AssertionError(f'{what}: {len(bad)} {name} parts differ; first at {i}: got {float(got[i])!r}, want {float(want[i])!r}')
    # the exact-zero rule of the header
    z = (want_hi.float() == 0) | ((y32 - want_hi.float()) == 0)
    assert bool((bits(lo)[z] == 0).all()), f'{what}: a lo part that must be exactly zero is not'


@functools.lru_cache(None)
def stem_operands(B, H, W, seed=3, cout=64):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 4, H, W, generator=g) * 2 - 1
    w = torch.randn(cout, 4, 7, 7, generator=g) * 0.1
    bias = torch.randn(cout, generator=g) * 0.5            # the BatchNorm shift (the scale is folded into w by the packer)
    return x, w, bias


@functools.lru_cache(None)
def down_operands(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(cout, cin, 3, 3, generator=g) * (0.6 / (3.0 * cin ** 0.5)), torch.randn(cout, generator=g) * 0.2


def check_stem_layout(lib, dev, shape, prec):
    B, H, W = shape
    x, w, bias = stem_operands(B, H, W)
    y32, f32, g32 = conv(lib, dev, x, w, bias, 1, 3, prec)
    ys, fs, gs = conv(lib, dev, x, w, bias, 1, 3, prec, y_split=True)
    what = f'stem {B}x{H}x{W} {PREC_ID[prec]}'
    assert_guards(g32, what), assert_guards(gs, what)
    assert f32 == 0 and fs == 0, f'{what}: range_flag raised'
    assert bool((y32 > 0).any()) and bool((y32 == 0).any())          # ReLU on both sides
    assert_split_of(ys, y32, prec, what)


def check_chain(lib, dev, prec, B=2, H=64, W=96, chans=(64, 128, 256, 512)):
    """stem -> down1 -> down2 -> down3 with fp32 and with split intermediates: equal final outputs, every split intermediate the split of its
    fp32 twin."""
    x, w, bias = stem_operands(B, H, W, seed=5, cout=chans[0])
    ws = [(w, bias, 1, 3)] + [down_operands(chans[i], chans[i + 1], 40 + i) + (2, 1) for i in range(len(chans) - 1)]
    a32, a16 = x, x
    for i, (wi, bi, stride, pad) in enumerate(ws):
        last = i == len(ws) - 1
        n32, f32, g32 = conv(lib, dev, a32, wi, bi, stride, pad, prec)
        n16, f16, g16 = conv(lib, dev, a16, wi, bi, stride, pad, prec, x_split=i > 0, y_split=not last)
        what = f'chain layer {i} {PREC_ID[prec]}'
        assert_guards(g32, what), assert_guards(g16, what)
        assert f32 == 0 and f16 == 0, f'{what}: range_flag raised'
        if last:
            assert torch.equal(n16, n32), f'{what}: {int((n16 != n32).sum())} outputs of the split-fed chain differ from the fp32 chain'
        else:
            assert_split_of(n16, n32, prec, what)
        a32, a16 = n32, n16
    return a32


def check_down_alone(lib, dev, prec, cin, cout, H, W, pad_mode, y_split=False, B=1, seed=9):
    """One stride-2 conv on a tensor packed on the HOST from random fp32 against the same launch on the fp32 tensor."""
    g = torch.Generator().manual_seed(seed + cin + H)
    x = torch.randn(B, cin, H, W, generator=g)
    w, bias = down_operands(cin, cout, 70 + cin)
    y32, f32, g32 = conv(lib, dev, x, w, bias, 2, 1, prec, pad_mode=pad_mode)
    ys, fs, gs = conv(lib, dev, L.split16_pack(x, prec), w, bias, 2, 1, prec, x_split=True, y_split=y_split, pad_mode=pad_mode)
    what = f'down {cin}->{cout} {H}x{W} pad_mode {pad_mode} {PREC_ID[prec]}'
    assert_guards(g32, what), assert_guards(gs, what)
    assert f32 == 0 and fs == 0, f'{what}: range_flag raised'
    if y_split:
        assert_split_of(ys, y32, prec, what)
    else:
        assert torch.equal(ys, y32), f'{what}: {int((ys != y32).sum())} outputs differ'


# ---- range flag ----------------------------------------------------------------------------------------------------------------------------------
def stem_one_element(lib, dev, prec, H, W, x_val, w_val, at=None, nan_input=False):
    """The stem with ONE non-zero output element: image channel 0 is x_val at ``at`` (default: the last pixel of the plane), the centre tap of
    output channel 63 over channel 0 is w_val, everything else zero.  Returns (value of that element as the split stores it, flag)."""
    at = at or (H - 1, W - 1)
    x = torch.zeros(1, 4, H, W)
    x[0, 0, at[0], at[1]] = x_val
    if nan_input:
        x[0, 1, 0, 0] = float('nan')
    w = torch.zeros(64, 4, 7, 7)
    w[63, 0, 3, 3] = w_val
    ys, flag, flat = conv(lib, dev, x, w, torch.zeros(64), 1, 3, prec, y_split=True)
    assert_guards(flat, 'stem range case')
    hi, lo = L.split16_unpack(ys, prec)
    return float(hi[0, 63, at[0], at[1]].float()) + float(lo[0, 63, at[0], at[1]].float()), flag


def ragged_tile_case(lib, dev, prec, big_row):
    """A 4 x 1 stride-2 launch (64 -> 128, split output) on a 12 x 48 plane: 6 x 24 outputs in 32 x 4 tiles, so the second tile row has two rows
    of lanes outside the plane.  Only tap (ky, kx) = (0, 1) of input channel 0 is non-zero (300): output row oy reads input row 2 oy - 1, the
    out-of-plane row oy = 6 reads row 11.  ``big_row`` carries 300 in channel 0: row 11 is read by out-of-plane lanes ONLY (their 300 x 300 =
    90 000 is beyond the fp16 range and must not be watched or stored), row 9 by the last row inside the plane.  Returns (output parts, flag)."""
    x = torch.zeros(1, 64, 12, 48)
    x[0, 0, big_row, :] = 300.0
    w = torch.zeros(128, 64, 3, 3)
    w[:, 0, 0, 1] = 300.0
    ys, flag, flat = conv(lib, dev, x, w, None, 2, 1, prec, y_split=True)
    assert_guards(flat, 'ragged tile case')
    return ys, flag


# ---- generator -----------------------------------------------------------------------------------------------------------------------------------
def gen_config():
    """The smallest generator whose head has pre-split edges: 64 stem channels (the stem kernel takes 33 .. 64), two stride-2 convs of at least
    96 output channels (a0 and a1 become LAMA_DT_SPLIT16, the second conv writes the fp32 state), one residual block."""
    from oracle import lama_oracle as O
    return O.small_config(ngf=64, n_blocks=1, n_downsampling=2)


@functools.lru_cache(None)
def gen_state_dict(seed=21):
    from oracle import lama_oracle as O
    return O.make_synthetic_state_dict(gen_config(), seed=seed, calib_hw=32)


def make_model(ex_factory, dev, presplit, sd=None, head_only=False):
    """A predict-only training module around the small generator; ``ex_factory`` -> the _Exec (library) it runs on, None = the default.
    ``head_only`` (the emulator, where a 64-channel residual block takes minutes): the generator's plan ends behind the last stride-2 conv --
    ReflectionPad2d, stem, down1, down2 -- and its output is the fp32 (x_l | x_g) state; everything the plan builder does for the edges is in it."""
    from lama_amd import trainers
    sd = sd or gen_state_dict()
    m = trainers.DefaultInpaintingTrainingModule(dict(generator=dict(kind='ffc_resnet', **gen_config())))
    m.load_state_dict({'generator.' + k: v for k, v in sd.items()}, strict=True)
    m.freeze()
    if dev != 'cpu':
        m.to(dev)
    if ex_factory is not None:
        m.generator.set_exec(ex_factory())
    m.generator.presplit_outer = presplit
    if head_only:
        from lama_amd import ffc as F
        m.generator.model = F.LayerSequence(*list(m.generator.model)[:2 + gen_config()['n_downsampling']])
    return m


def split_names(gen):
    """Which buffers of the generator's plans are pre-split (whole-batch plans and the parts of split plans alike)."""
    out = []
    for plan in gen._plans.values():
        for pl in plan.get('parts', [plan]):
            out.append(sorted(pl['split']))
    return out


def check_generator_identity(ex_factory, dev, shape, graph=False, split_batch=None, reps=2, head_only=False):
    """presplit_outer on against off: the u8 'inpainted' output, the u8 'predicted_image' output and the generator's fp32 output, ``reps`` times
    each (the second call replays the cached plan / graph; the emulator runs one).  Equal bit for bit; on: a0 and a1 are split, off: nothing is
    and every buffer is fp32."""
    from oracle import lama_oracle as O
    B, H, W = shape
    g = torch.Generator().manual_seed(17)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    batch = O.make_synthetic_batch(B, H, W, seed=19)
    mask = (batch['mask'][:, 0] * 255).to(torch.uint8).contiguous().to(dev)
    x = torch.cat([batch['image'] * (1 - batch['mask']), batch['mask']], 1).to(dev)
    res = {}
    for presplit in (True, False):
        m = make_model(ex_factory, dev, presplit, head_only=head_only)
        gen = m.generator
        gen.auto_fallback = False
        gen.use_graph = graph
        gen.split_batch = split_batch
        gen.verify_split = False
        outs = []
        for _ in range(reps):
            if head_only:                   # (no image comes out of the truncated plan: the state three times)
                outs += [gen(x).cpu().clone() for _ in range(3)]
                continue
            outs.append(m.forward_u8(img, mask, None, torch.empty_like(img)).cpu().clone())
            outs.append(m.forward_u8(img, mask, None, torch.empty_like(img), out_key='predicted_image').cpu().clone())
            outs.append(gen(x).cpu().clone())
        names = split_names(gen)
        assert names and all(n == (['a0', 'a1'] if presplit else []) for n in names), names
        if split_batch:
            assert all('parts' in p and len(p['parts']) == split_batch for p in gen._plans.values())
        if not presplit:
            for plan in gen._plans.values():
                for pl in plan.get('parts', [plan]):
                    assert all(b.dtype == torch.float32 for b in pl['bufs'].values())
        for a, b in zip(outs[:3], outs[3:]):
            assert torch.equal(a, b), 'the cached plan does not repeat its first run'
        res[presplit] = outs[:3]
    for a, b, what in zip(res[True], res[False], ('inpainted u8', 'predicted_image u8', 'generator fp32')):
        assert torch.equal(a, b), f'{what}: presplit_outer on and off differ in {int((a != b).sum())} elements'


def check_generator_fallback(ex_factory, dev, head_only=False):
    """An activation beyond the fp16 range in a0 (every stem weight 600, image of ones: 4 x 49 x 600 = 117 600 before the BatchNorm of channel 0 is
    made the identity): the deferred check reports it with presplit_outer on as with it off, both generators fall back to bf16x3 and agree bit for bit."""
    import warnings
    from lama_amd import ffc as F
    sd = dict(gen_state_dict())
    w = sd['model.1.ffc.convl2l.weight'].clone()
    w[0] = 600.0
    sd['model.1.ffc.convl2l.weight'] = w
    for k, v in (('weight', 1.0), ('bias', 0.0), ('running_mean', 0.0), ('running_var', 1.0)):
        t = sd[f'model.1.bn_l.{k}'].clone()
        t[0] = v
        sd[f'model.1.bn_l.{k}'] = t
    x = torch.ones(1, 4, 32, 64).to(dev)
    outs = {}
    for presplit in (True, False):
        m = make_model(ex_factory, dev, presplit, sd=sd, head_only=head_only)
        gen = m.generator
        gen.defer_range_check = True
        assert gen.precision == L.PREC_F16X3
        gen(x)
        assert split_names(gen) == [['a0', 'a1'] if presplit else []]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            assert gen.check_range(x.device) is False, 'the deferred check did not see the activation beyond 65504'
        assert gen.precision == L.PREC_BF16X3
        y = gen(x).cpu().clone()
        assert gen.check_range(x.device) is True
        assert split_names(gen) == [['a0', 'a1'] if presplit else []]        # the bf16x3 plan holds bf16 parts
        assert bool(torch.isfinite(y).all())
        outs[presplit] = y
    assert torch.equal(outs[True], outs[False])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    """Every combination the header excludes returns LAMA_ERR_UNSUPPORTED, launches nothing and leaves the output buffer as it was."""
    import pytest
    g = torch.Generator().manual_seed(2)
    st = _st(dev)

    def buf(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    def refused(fn, y, what):
        before = y.clone()
        with pytest.raises(L.LamaError) as e:
            fn()
        _sync(dev)
        assert e.value.code == L.ERR_UNSUPPORTED, f'{what}: code {e.value.code}'
        assert torch.equal(y.view(torch.int32), before.view(torch.int32)), f'{what}: the output buffer changed'

    P = L.PREC_F16X3
    x64, y128 = buf(1, 64, 12, 16), buf(1, 128, 6, 8)
    w_s2 = lib.pack_conv_weight(buf(128, 64, 3, 3) * 0.05, None, stride=2, precision=P)
    cv = lambda xv, yv, **kw: lib.conv2d(xv, w_s2, yv, 1, 3, 2, 1, L.PAD_REFLECT, False, None, L.ACT_RELU, precision=P, stream=st, **kw)   # noqa: E731
    refused(lambda: cv(L.view_split(x64), L.view(y128), resid=L.view_split(y128)), y128, 'split resid')
    refused(lambda: cv(L.view(x64), L.view_split(y128), resid=L.view(buf(1, 128, 6, 8))), y128, 'split y with a residual')
    for prec, name in ((L.PREC_F32, 'f32'), (L.PREC_F16, 'f16')):
        wp = lib.pack_conv_weight(buf(128, 64, 3, 3) * 0.05, None, stride=2, precision=prec)
        refused(lambda: lib.conv2d(L.view_split(x64), wp, L.view(y128), 1, 3, 2, 1, L.PAD_REFLECT, False, None, L.ACT_RELU, precision=prec, stream=st),
                y128, f'split x under {name}')
        refused(lambda: lib.conv2d(L.view(x64), wp, L.view_split(y128), 1, 3, 2, 1, L.PAD_REFLECT, False, None, L.ACT_RELU, precision=prec, stream=st),
                y128, f'split y under {name}')
    # C % 8 != 0 (view_split refuses such a buffer itself: the raw struct)
    x60, y100 = buf(1, 60, 12, 16), buf(1, 100, 6, 8)
    w60 = lib.pack_conv_weight(buf(128, 60, 3, 3) * 0.05, None, stride=2, precision=P)
    w100 = lib.pack_conv_weight(buf(100, 64, 3, 3) * 0.05, None, stride=2, precision=P)
    raw = lambda t: L.Tensor4(t.data_ptr(), t[0].numel(), t.shape[1], t.shape[2], t.shape[3], L.DT_SPLIT16)          # noqa: E731
    refused(lambda: lib.conv2d(raw(x60), w60, L.view(y128), 1, 3, 2, 1, L.PAD_REFLECT, False, None, L.ACT_RELU, precision=P, stream=st), y128, 'x.C % 8')
    refused(lambda: lib.conv2d(L.view(x64), w100, raw(y100), 1, 3, 2, 1, L.PAD_REFLECT, False, None, L.ACT_RELU, precision=P, stream=st), y100, 'y.C % 8')
    # stride 1 (local conv, LDS-staged or weights in registers), 1 x 1, second operand, fused conv1
    y1 = buf(1, 128, 12, 16)
    w_s1 = lib.pack_conv_weight(buf(128, 64, 3, 3) * 0.05, None, precision=P)
    refused(lambda: lib.conv2d(L.view_split(x64), w_s1, L.view(y1), 1, 3, 1, 1, L.PAD_REFLECT, False, None, L.ACT_RELU, precision=P, stream=st), y1, 'stride-1 3x3')
    w_11 = lib.pack_conv_weight(buf(128, 64, 1, 1) * 0.05, None, precision=P)
    refused(lambda: lib.conv2d(L.view(x64), w_11, L.view_split(y1), 1, 1, 1, 0, L.PAD_ZERO, False, None, L.ACT_RELU, precision=P, stream=st), y1, '1x1')
    x2 = buf(1, 64, 12, 16)
    refused(lambda: lib.conv2d(L.view(x64), w_s1, L.view(y1), 1, 3, 1, 1, L.PAD_REFLECT, False, None, L.ACT_RELU, x2=L.view_split(x2), w2_packed=w_11,
                               precision=P, stream=st), y1, 'split x2')
    y384, x1 = buf(1, 384, 12, 16), buf(1, 192, 12, 16)
    w384 = lib.pack_conv_weight(buf(384, 64, 3, 3) * 0.05, None, precision=P)
    w2_384 = lib.pack_conv_weight(buf(384, 64, 1, 1) * 0.05, None, precision=P)
    wf1 = lib.pack_conv_weight(buf(192, 384, 1, 1) * 0.05, None, precision=P)
    refused(lambda: lib.conv2d(L.view(x64), w384, L.view(y384), 1, 3, 1, 1, L.PAD_REFLECT, False, None, L.ACT_RELU, x2=L.view(x2), w2_packed=w2_384,
                               precision=P, stream=st, fuse1=(wf1, buf(192), L.view_split(x1))), y384, 'split fuse1_y')
    # transposed conv, head, Winograd, FFT
    yt = buf(1, 64, 24, 32)
    wt = lib.pack_conv_weight(buf(64, 64, 3, 3) * 0.05, None, stride=2, transposed=True, precision=P)
    refused(lambda: lib.conv2d(L.view_split(x64), wt, L.view(yt), 1, 3, 2, 1, L.PAD_ZERO, True, None, L.ACT_RELU, precision=P, stream=st), yt, 'transposed')
    yh = buf(1, 3, 12, 16)
    wh = lib.pack_conv_weight(buf(3, 64, 7, 7) * 0.02, None, precision=P)
    refused(lambda: lib.conv2d(L.view_split(x64), wh, L.view(yh), 1, 7, 1, 3, L.PAD_REFLECT, False, None, L.ACT_SIGMOID, precision=P, stream=st), yh, 'head')
    ww = lib.pack_winograd_weight(buf(128, 64, 3, 3) * 0.05, None, P)
    ws = torch.empty(max(1, lib.winograd_workspace_bytes(1, 128, 12, 16) // 4), dtype=torch.float32, device=dev)
    refused(lambda: lib.winograd_conv3x3(L.view_split(x64), ww, L.view(y1), 1, ws, precision=P, stream=st), y1, 'Winograd')
    spec = buf(1, 128, 12, 9)
    refused(lambda: lib.rfft2(L.view_split(x64), L.view(spec), 1, stream=st), spec, 'rfft2')
    refused(lambda: lib.irfft2(L.view(spec), None, L.view_split(x64), 1, stream=st), x64, 'irfft2')
