"""Test helper of the fp16 range watch (``lama_conv2d_args.range_flag`` in include/lama_hip.h): positions, values, the bar
and the ``check_*(lib, case, ..., dev)`` functions that tests/test_range_watch_emu.py runs through the host emulator and
tests/test_range_watch_gpu.py on the MI355X.  ``dev`` is 'cpu' with the emulated library and 'cuda' with a GPU build.

The contract, for ONE launch with ``range_flag`` given, x random N(0, 1) except one planted value v at a position that at least one output reads
(asserted: the float64 reference changes when v is planted):
  1. LAMA_PREC_F16X3, v in RAISE = {7e4, -1e5, +inf, NaN}: flag == 1.
  2. v in QUIET = {65504, the float below 65520}: flag == 0, the output within the bar of the float64 reference, guard channels intact.
  3. v = 65520 (the tie between 65504 and inf): flag == 1, or the output within the bar -- an unflagged result is a correct one.
  4. no planted value: flag == 0; the NaN channels around the input view do not raise it.
  5. LAMA_PREC_BF16X3: flag == 0 for every v; for finite v the output is finite and within the bf16 bar.
  6. the flag is only ever ORed: a launch on in-range data with the word preset to 1 leaves 1.

The bar per output element: CONV_TOL[prec] (atol + rtol |ref|, tests/test_kernels_emu.py) + c (|x| (*) |w scale|), the same convolution on absolute
values in float64; c = 2^-20 for f16x3 (the split keeps 22 bits of each operand and drops lo * lo: three terms of 2^-22), 2^-14 for bf16x3 (16
bits).  Derived, not measured; an activation behind the sum is 1-Lipschitz (ReLU) or better (sigmoid), a residual is added exactly.

The fp16 floor (f16x3 only, ``SUB_LO``): c |x| |w| presumes that the split keeps 22 bits of every operand.  A packed weight w' = w scale below 2^-3 does
not: its lo word (|lo| <= 2^-11 |w'| < 2^-14) is an fp16 SUBNORMAL on the grid 2^-24, so w' carries an absolute error of up to 2^-25 however small
it is, and a tap contributes up to 2^-25 |x| (include/lama_hip.h, LAMA_PREC_F16X3).  The weights here are the suite's ordinary ones (0.2 N(0, 1) and
the like, most of them below 2^-3), so the bar carries that third, derived term: 2^-25 (|x| (*) [0 < |w'| < 2^-3]), the same convolution of |x| with the
0 / 1 mask of the affected taps.  What the two first terms alone give is printed beside it ('issue-bar' in the GPU lines): at 65504 up to 1.6
(multidilated), 2.8 (LDS-staged rows) and 6.6 (rect, whose weights are (cin kh kw)^-1/2 N(0, 1), about 0.02), flag 0, on the MI355X.

Positions of x [B, C, H, W]: first, last, (0, C-1, 0, W-1), (B-1, 0, H-1, 0), centre -- each with 7e4; the last one with the whole value list.

Every check prints one line per launch on the GPU ('[range-watch] family shape precision position value flag err/bar'); the collected lines of a
run are profiles/range_watch.txt."""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

from lama_amd import _lib as L
from tests import test_kernels_emu as KE
from tests import test_split_exact_emu as E

INF, NAN = float('inf'), float('nan')
BELOW_TIE = float(np.nextafter(np.float32(65520.0), np.float32(0.0)))        # rounds to 65504 in fp16
TIE = 65520.0                                                                # rounds to even: inf
RAISE = [7.0e4, -1.0e5, INF, NAN]
QUIET = [65504.0, BELOW_TIE]
C_BAR = {L.PREC_F16X3: 2.0 ** -20, L.PREC_BF16X3: 2.0 ** -14}
SUB_LO = 2.0 ** -25                 # half a step of the fp16 subnormal grid: the absolute error of a packed f16x3 weight below 2^-3
PRE, POST, SENT = E.PRE, E.POST, E.SENT
PREC_NAME = E.PREC_NAME
_st, _sync, _d = E._st, E._sync, E._d


def positions(shape):
    """[(name, index)] of the five planted positions of x [B, C, H, W]."""
    B, C, H, W = shape
    return [('first', (0, 0, 0, 0)), ('last', (B - 1, C - 1, H - 1, W - 1)), ('c-1,w-1', (0, C - 1, 0, W - 1)), ('b-1,h-1', (B - 1, 0, H - 1, 0)),
            ('centre', (B // 2, C // 2, H // 2, W // 2))]


def plan(shape, prec, thin=False, names=None):
    """[(position name, index, v)] of one case under ``prec``: None = the clean baseline.  ``thin`` (the emulator's large rows): first and last
    with 7e4, the tie and one quiet value at the last position."""
    pos = [p for p in positions(shape) if names is None or p[0] in names]
    last = dict(pos).get('last')
    out = [('-', None, None)]
    if prec == L.PREC_BF16X3:
        return out + [('last', last, v) for v in ((7.0e4, NAN) if thin else (7.0e4, -1.0e5, INF, NAN))]
    out += [(n, i, 7.0e4) for n, i in pos if not thin or n in ('first', 'last')]
    if names is None:
        out += [('last', last, v) for v in ((BELOW_TIE, TIE) if thin else RAISE[1:] + QUIET + [TIE])]
    return out


def sub_mask(wf):
    """The 0 / 1 mask of the folded weights whose lo word is an fp16 subnormal (module docstring)."""
    return ((wf.abs() < 2.0 ** -3) & (wf != 0)).to(wf.dtype)


def plant(x, idx, v):
    if idx is None:
        return x
    x = x.clone()
    x[idx] = v
    return x


def bar_of(ref, absconv, prec, tol=None, floor=True):
    """``absconv``: |x| (*) |w'|, or the pair (|x| (*) |w'|, |x| (*) sub_mask(w')); ``floor=False``: the two terms the issue states, without the fp16 floor."""
    tol = tol or KE.CONV_TOL[prec]
    absconv, sub = absconv if isinstance(absconv, tuple) else (absconv, None)
    bar = tol['atol'] + tol['rtol'] * ref.abs() + C_BAR[prec] * absconv
    return bar + SUB_LO * sub if (floor and sub is not None and prec == L.PREC_F16X3) else bar


class Worst:
    """The worst err / bar of a family and precision (printed on the GPU, recorded in profiles/range_watch.txt)."""
    seen = {}

    @classmethod
    def add(cls, family, prec, ratio):
        k = (family, PREC_NAME[prec])
        cls.seen[k] = max(cls.seen.get(k, 0.0), ratio)
        return cls.seen[k]


def judge(what, family, shape_id, prec, pname, v, flag, y, guards_ok, ref_fn, dev, preset=0):
    """The assertions of one launch.  ``y``: the output view on the host (float64), ``ref_fn()`` -> (ref, absconv) of the planted input."""
    name = f'{what} {PREC_NAME[prec]} {pname} v={v!r}'
    ratio = issue = float('nan')
    assert guards_ok, f'{name}: a channel outside the output view was written'
    must_raise = prec == L.PREC_F16X3 and v is not None and (math.isnan(v) or abs(v) > TIE)
    finite = v is None or math.isfinite(v)
    if preset:
        assert flag == 1, f'{name}: the flag was cleared'
    elif must_raise:
        assert flag == 1, f'{name}: not raised'
    elif prec == L.PREC_BF16X3 or v is None or abs(v) < TIE:
        assert flag == 0, f'{name}: raised'
    else:
        assert flag in (0, 1), f'{name}: flag {flag}'
    if finite and not (flag == 1 and not preset):
        ref, absconv = ref_fn()
        assert bool(torch.isfinite(y).all()), f'{name}: a non-finite output'
        r = (y - ref).abs() / bar_of(ref, absconv, prec)
        ratio, issue = float(r.max()), float(((y - ref).abs() / bar_of(ref, absconv, prec, floor=False)).max())
        i = tuple(int(t) for t in (r == r.max()).nonzero()[0])
        assert ratio <= 1.0, f'{name}: flag {flag} and err / bar = {ratio:.3f} at {i}: got {float(y[i])!r}, want {float(ref[i])!r}'
        Worst.add(family, prec, ratio)
        Worst.add(family + ' issue-bar', prec, issue)
    if dev != 'cpu':
        print(f'[range-watch] {family} {shape_id} {PREC_NAME[prec]} {pname} v={v!r} flag={flag} err/bar={ratio:.4f}' + (f' issue-bar={issue:.4f}' if ratio == ratio else ''))
    return ratio


def guards_intact(ybuf_host, cout):
    g = torch.cat([ybuf_host[:, :PRE], ybuf_host[:, PRE + cout:]], 1)
    return float(g.min()) == SENT == float(g.max())


FAM_NAME = {getattr(L, n): n[9:].lower() for n in dir(L) if n.startswith('CONV_FAM_')}


# ---- lama_conv2d_fwd ---------------------------------------------------------------------------------------------------------------------------
def _conv_lin(c):
    tr = c.get('transposed', False)
    if c['k'] == 7 and c['H'] * c['W'] > 4096:
        return lambda x, w: E.U.tap_conv2d(x, w, c['stride'], c['pad'], True)
    return lambda x, w: KE._conv_ref(x, w, c['stride'], c['pad'], True, tr, None, 0, None)


_ACT = {L.ACT_NONE: lambda t: t, L.ACT_RELU: torch.relu, L.ACT_SIGMOID: torch.sigmoid}


def _make_conv_operands(c, seed):
    """The operands of KE.test_conv2d_emulated (N(0, 1) input, 0.2 N(0, 1) weights, the row's bias / residual / activation / scale) and, as a function
    of x, the float64 reference with the two absolute-value convolutions of the bar (``bar_of``)."""
    g = torch.Generator().manual_seed(seed)
    B, cin, cout, k, tr = c.get('B', 2), c['cin'], c['cout'], c['k'], c.get('transposed', False)
    x = torch.randn(B, cin, c['H'], c['W'], generator=g)
    w = torch.randn((cin, cout, k, k) if tr else (cout, cin, k, k), generator=g) * 0.2
    scale = torch.rand(cout, generator=g) + 0.5 if c['scale'] else None
    bias = torch.randn(cout, generator=g) if c['bias'] else None
    lin = _conv_lin(c)
    wf = w.double() if scale is None else w.double() * (scale.double()[None, :, None, None] if tr else scale.double()[:, None, None, None])
    oshape = lin(torch.zeros(1, cin, c['H'], c['W'], dtype=torch.float64), wf).shape
    resid = torch.randn(B, *oshape[1:], generator=g) if c['resid'] else None

    def ref_fn(xx):
        xd = xx.double()
        y = lin(xd, wf)
        if bias is not None:
            y = y + bias.double().view(1, -1, 1, 1)
        y = _ACT[c['act']](y)
        if resid is not None:
            y = y + resid.double()
        return y, (lin(xd.abs(), wf.abs()), lin(xd.abs(), sub_mask(wf)))

    return types.SimpleNamespace(x=x, w=w, scale=scale, bias=bias, resid=resid, ref_fn=ref_fn, oshape=(B, *oshape[1:]), clean=ref_fn(x))


@functools.lru_cache(None)
def _conv_operands(key):
    c = dict(key)
    return _make_conv_operands(c, 9000 + sum(int(v) * (i + 1) for i, (_, v) in enumerate(key) if isinstance(v, (int, bool))))


_OPERAND_KEYS = ('cin', 'cout', 'k', 'stride', 'pad', 'H', 'W', 'B', 'act', 'bias', 'resid', 'scale', 'transposed')


def conv_operands(case):
    """Built once per geometry on the host, shared by every launch, precision and library of one process, never written to."""
    return _conv_operands(tuple(sorted((k, v) for k, v in case.items() if k in _OPERAND_KEYS)))


def conv_launch(lib, case, prec, o, x, dev, preset=0, route=None, production=False):
    """One lama_conv2d_fwd launch of ``x`` in a NaN-guarded buffer: (output view on the host as float64, guards intact, flag)."""
    c, tr = case, case.get('transposed', False)
    xbuf = E.guarded_input(x, dev)
    ybuf = torch.full((o.oshape[0], PRE + c['cout'] + POST, *o.oshape[2:]), SENT, device=dev)
    wp = lib.pack_conv_weight(o.w.to(dev), _d(o.scale, dev), stride=c['stride'], transposed=tr, precision=prec)
    bias, resid = _d(o.bias, dev), _d(o.resid, dev)
    flag = torch.full((1,), preset, dtype=torch.int32, device=dev)
    args = (L.view(xbuf, PRE, c['cin']), wp, L.view(ybuf, PRE, c['cout']), x.shape[0], c['k'], c['stride'], c['pad'],
            L.PAD_ZERO if tr else L.PAD_REFLECT, tr, bias, c['act'], None if resid is None else L.view(resid))
    kw = dict(precision=prec, cooperative=c.get('geo') == 3 and not production)      # the production library reads no geometry knob
    if route is not None:
        route(args, kw)
    lib.conv2d(*args, stream=_st(dev), range_flag=flag, **kw)
    _sync(dev)
    h = ybuf.cpu()
    return h[:, PRE:PRE + c['cout']].double(), guards_intact(h, c['cout']), int(flag.cpu())


def run_plan(what, family, o, launch, prec, dev, thin=False, names=None, assert_read=True):
    """Every launch of ``plan`` on the operands ``o`` (x, ref_fn(x) -> (ref, absconv), clean = ref_fn(o.x)); ``launch(x, preset)`` ->
    (output on the host as float64, guards intact, flag).  Then the never-cleared launch (6)."""
    clean_ref = o.clean[0]
    for pname, idx, v in plan(getattr(o, 'read_shape', o.x.shape), prec, thin, names):
        x = plant(o.x, idx, v)
        cache = o.__dict__.setdefault('planted_refs', {})          # shared by the precisions and libraries of one process

        def ref_fn():
            if idx is None:
                return o.clean
            if (idx, v) not in cache:
                cache[(idx, v)] = o.ref_fn(x)
            return cache[(idx, v)]
        if idx is not None and v == 7.0e4 and assert_read:
            assert not torch.equal(ref_fn()[0], clean_ref), f'{what} {pname}: no output reads the planted position'
        y, ok, flag = launch(x, 0)
        judge(what, family, what, prec, pname, v, flag, y, ok, ref_fn, dev)
    if prec == L.PREC_F16X3:
        y, ok, flag = launch(o.x, 1)
        judge(what, family, what, prec, 'preset', None, flag, y, ok, lambda: o.clean, dev, preset=1)


def check_conv(lib, case, prec, dev, production=False, thin=False, names=None, family=None, geometry=True, operands=None, assert_read=True):
    """``run_plan`` on one CONV_CASES-style row, the route asserted before the first launch (KE.assert_conv_route: the row must reach its family)."""
    o = operands or conv_operands(case)
    what, fam = E.CONV_ID(case), family or f"conv2d-{FAM_NAME[KE.expected_conv_route(case, prec, production)[0]]}"
    todo = [lambda args, kw: KE.assert_conv_route(lib, case, prec, args, kw, production=production, geometry=geometry)] if 'fam' in case else []
    run_plan(what, fam, o, lambda x, preset: conv_launch(lib, case, prec, o, x, dev, preset, route=todo.pop() if todo else None, production=production),
             prec, dev, thin, names, assert_read)


def single_unit_case(fam):
    """The single-unit launch of an output-side watcher (the three pointwise GEMMs: ``classf`` on the pre-activation sums): one image of 4 x 8 =
    32 pixels, ONE pixel tile (and one super-tile), on one row group, so that the planted element's unit is the first and the last one of its
    workgroup -- the dummy-epilogue special case of conv_ws_dev.inc (u == 0) with nothing behind it.  Bias, residual, ReLU and scale on."""
    base = dict(k=1, stride=1, pad=0, H=4, W=8, B=1, act=1, bias=True, resid=True, scale=True, fam=fam)
    if fam == L.CONV_FAM_GEMM1X1_WS:
        return dict(base, cin=192, cout=96)
    if fam == L.CONV_FAM_GEMM1X1_W4:
        return dict(base, cin=384, cout=96, w4_slots=0)
    assert fam == L.CONV_FAM_GEMM1X1_WK
    return dict(base, cin=384, cout=384, resid=False, wk_slots=0)


SINGLE_UNIT_CASES = [single_unit_case(f) for f in (L.CONV_FAM_GEMM1X1_WS, L.CONV_FAM_GEMM1X1_W4, L.CONV_FAM_GEMM1X1_WK)]


# ---- the fused second operand --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _fused_operands(idx):
    c = E.FUSED_CASES[idx]
    g = torch.Generator().manual_seed(9100 + idx)
    B, cl, cg, half, H, W = 2, c['cl'], c['cg'], c['half'], c['H'], c['W']
    x, x2 = torch.randn(B, cl, H, W, generator=g), torch.randn(B, half, H, W, generator=g)
    w, w2 = torch.randn(cg, cl, 3, 3, generator=g) * 0.2, torch.randn(cg, half, 1, 1, generator=g) * 0.2
    scale, bias, resid = torch.rand(cg, generator=g) + 0.5, torch.randn(cg, generator=g), torch.randn(B, cg, H, W, generator=g)
    wf, w2f = w.double() * scale.double().view(-1, 1, 1, 1), w2.double() * scale.double().view(-1, 1, 1, 1)
    lin = lambda a, a2, u, u2: F.conv2d(F.pad(a, (1,) * 4, mode='reflect'), u) + F.conv2d(a2, u2)      # noqa: E731

    def ref_fn(xx, xx2):
        a, a2 = xx.double(), xx2.double()
        return (lin(a, a2, wf, w2f) + bias.double().view(1, -1, 1, 1)).relu() + resid.double(), (lin(a.abs(), a2.abs(), wf.abs(), w2f.abs()), lin(a.abs(), a2.abs(), sub_mask(wf), sub_mask(w2f)))
    return types.SimpleNamespace(x=x, x2=x2, w=w, w2=w2, scale=scale, bias=bias, resid=resid, ref_fn=ref_fn, clean=ref_fn(x, x2))


def check_fused_second_operand(lib, case, prec, dev):
    """relu(conv3x3(x) + conv1x1(x2) + b) + resid in one launch: 7e4 in x only and in x2 only, first and last position each."""
    o = _fused_operands(E.FUSED_CASES.index(case))
    what = f'fused {E.FUSED_ID(case)}'
    sc = o.scale.to(dev)
    wp, wp2 = lib.pack_conv_weight(o.w.to(dev), sc, precision=prec), lib.pack_conv_weight(o.w2.to(dev), sc, precision=prec)
    bias, resid = o.bias.to(dev), o.resid.to(dev)

    def launch(x, x2, preset=0):
        xbuf, x2buf = E.guarded_input(x, dev), E.guarded_input(x2, dev)
        ybuf = torch.full((x.shape[0], PRE + case['cg'] + POST, case['H'], case['W']), SENT, device=dev)
        flag = torch.full((1,), preset, dtype=torch.int32, device=dev)
        lib.conv2d(L.view(xbuf, PRE, case['cl']), wp, L.view(ybuf, PRE, case['cg']), x.shape[0], 3, 1, 1, L.PAD_REFLECT, False, bias, L.ACT_RELU,
                   L.view(resid), x2=L.view(x2buf, PRE, case['half']), w2_packed=wp2, precision=prec, stream=_st(dev), range_flag=flag)
        _sync(dev)
        h = ybuf.cpu()
        return h[:, PRE:PRE + case['cg']].double(), guards_intact(h, case['cg']), int(flag.cpu())

    judge(what, 'fused-x2', what, prec, '-', None, *_yfo(launch(o.x, o.x2)), lambda: o.clean, dev)
    for operand in ('x', 'x2'):
        src = getattr(o, operand)
        for pname, idx in positions(src.shape)[:2]:
            p = plant(src, idx, 7.0e4)
            xs = (p, o.x2) if operand == 'x' else (o.x, p)
            ref = o.ref_fn(*xs)
            assert not torch.equal(ref[0], o.clean[0])
            judge(what, 'fused-x2', what, prec, f'{operand}:{pname}', 7.0e4, *_yfo(launch(*xs)), lambda: ref, dev)
    if prec == L.PREC_F16X3:
        judge(what, 'fused-x2', what, prec, 'preset', None, *_yfo(launch(o.x, o.x2, 1)), lambda: o.clean, dev, preset=1)


def _yfo(r):
    """(y, guards, flag) of a launch in the argument order of ``judge``: (flag, y, guards)."""
    return r[2], r[0], r[1]


# ---- fuse1: the re-split of y for the fused conv1 ----------------------------------------------------------------------------------------------------
FUSE1_SPOTS = [('first', 0, (0, 0)), ('last', 383, (E.FUSE1_CASE['H'] - 1, E.FUSE1_CASE['W'] - 1))]     # (name, channel of y, pixel)


@functools.lru_cache(None)
def _fuse1_operands(spot):
    """Every input and every weight in range, ONE element of the intermediate y = relu(conv3x3(x) + conv1x1(x2) + b) + resid beyond it: the 1x1 weight
    of (y channel, x2 channel 5) is 300 and x2 is 300 at that channel and pixel: y = 9e4 + O(10) there (checked in float64), O(100) around it."""
    c = E.FUSE1_CASE
    _, ch, (py, px) = FUSE1_SPOTS[spot]
    g = torch.Generator().manual_seed(9200 + spot)
    B, cl, cg, half, H, W = c['B'], c['cl'], c['cg'], c['half'], c['H'], c['W']
    x, x2 = torch.randn(B, cl, H, W, generator=g), torch.randn(B, half, H, W, generator=g)
    w, w2 = torch.randn(cg, cl, 3, 3, generator=g) * 0.03, torch.randn(cg, half, 1, 1, generator=g) * 0.07
    bias, resid = torch.randn(cg, generator=g), torch.randn(B, cg, H, W, generator=g)
    w1, b1 = torch.randn(192, cg, 1, 1, generator=g) * 0.05, torch.randn(192, generator=g)
    x2[0, 5, py, px] = 300.0
    w2[ch, 5, 0, 0] = 300.0
    lin = lambda a, a2, u, u2: F.conv2d(F.pad(a, (1,) * 4, mode='reflect'), u) + F.conv2d(a2, u2)      # noqa: E731
    y = (lin(x.double(), x2.double(), w.double(), w2.double()) + bias.double().view(1, -1, 1, 1)).relu() + resid.double()
    absconv = (lin(x.double().abs(), x2.double().abs(), w.double().abs(), w2.double().abs()),
               lin(x.double().abs(), x2.double().abs(), sub_mask(w.double()), sub_mask(w2.double())))
    over = y.abs() >= 65504.0
    assert int(over.sum()) == 1 and float(y[0, ch, py, px]) > 7.0e4 and float(max(x.abs().max(), x2.abs().max(), w.abs().max(), w2.abs().max())) <= 300.0
    return types.SimpleNamespace(x=x, x2=x2, w=w, w2=w2, bias=bias, resid=resid, w1=w1, b1=b1, y=y, absconv=absconv)


def check_fuse1(lib, spot, prec, dev):
    """With fuse1_w the launch re-splits its own output y for the fused conv1 and must raise; the same launch without it watches x and x2 only:
    flag 0 and y within the bar."""
    c, o = E.FUSE1_CASE, _fuse1_operands(spot)
    B = c['B']
    what = f'fuse1 c128+192o384->192_9x37 y@{FUSE1_SPOTS[spot][0]}'
    wp, wp2 = lib.pack_conv_weight(o.w.to(dev), None, precision=prec), lib.pack_conv_weight(o.w2.to(dev), None, precision=prec)
    wpc = lib.pack_conv_weight(o.w1[:, lib.fuse1_channel_order()].contiguous().to(dev), None, precision=prec)
    bias, resid, b1 = o.bias.to(dev), o.resid.to(dev), o.b1.to(dev)
    for fused in (False, True):
        xbuf, x2buf = E.guarded_input(o.x, dev), E.guarded_input(o.x2, dev)
        ybuf = torch.full((B, PRE + c['cg'] + POST, c['H'], c['W']), SENT, device=dev)
        x1buf = torch.full((B, PRE + 192 + POST, c['H'], c['W']), SENT, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        kw = dict(fuse1=(wpc, b1, L.view(x1buf, PRE, 192))) if fused else {}
        lib.conv2d(L.view(xbuf, PRE, c['cl']), wp, L.view(ybuf, PRE, c['cg']), B, 3, 1, 1, L.PAD_REFLECT, False, bias, L.ACT_RELU, L.view(resid),
                   x2=L.view(x2buf, PRE, c['half']), w2_packed=wp2, precision=prec, stream=_st(dev), range_flag=flag, **kw)
        _sync(dev)
        h, h1, f = ybuf.cpu(), x1buf.cpu(), int(flag.cpu())
        assert guards_intact(h, c['cg']) and guards_intact(h1, 192), f'{what}: a channel outside an output view was written'
        ratio = float('nan')
        if fused and prec == L.PREC_F16X3:
            assert f == 1, f'{what} {PREC_NAME[prec]}: y = {float(o.y.abs().max()):.0f} was re-split for conv1 and the flag is {f}'
        else:
            assert f == 0, f'{what} {PREC_NAME[prec]} fuse1 {fused}: raised although every split operand is in range'
            y = h[:, PRE:PRE + c['cg']].double()
            ratio = float(((y - o.y).abs() / bar_of(o.y, o.absconv, prec)).max())
            assert ratio <= 1.0, f'{what} {PREC_NAME[prec]} fuse1 {fused}: y err / bar = {ratio:.3f}'
            Worst.add('fuse1', prec, ratio)
        if dev != 'cpu':
            print(f'[range-watch] fuse1 c128+192o384->192_9x37 {PREC_NAME[prec]} y@{FUSE1_SPOTS[spot][0]} v={float(o.y.abs().max()):.1f} '
                  f'fuse1_w={int(fused)} flag={f} err/bar={ratio:.4f}')


# ---- LAMA_DT_SPLIT16 outputs: the writer watches what it stores -----------------------------------------------------------------------------------------
SPLIT16_CASES = {'stem': dict(cin=4, cout=64, k=7, stride=1, pad=3, H=9, W=40), 'down': dict(cin=64, cout=128, k=3, stride=2, pad=1, H=11, W=37)}
SPLIT16_SPOTS = ['first', 'last']


@functools.lru_cache(None)
def _split16_operands(name, spot):
    """In-range input and weights; the centre tap of one filter is 300 and the pixel under it 300: y = 9e4 at ONE output (float64), the first
    channel and pixel or the last ones."""
    c = SPLIT16_CASES[name]
    g = torch.Generator().manual_seed(9300 + spot + len(name))
    B, k, s, p = 2, c['k'], c['stride'], c['pad']
    Ho, Wo = (c['H'] + 2 * p - k) // s + 1, (c['W'] + 2 * p - k) // s + 1
    x = torch.rand(B, c['cin'], c['H'], c['W'], generator=g) * 2 - 1
    w = torch.randn(c['cout'], c['cin'], k, k, generator=g) * 0.05
    bias = torch.randn(c['cout'], generator=g) * 0.5
    b, ch, oy, ox = (0, 0, 0, 0) if SPLIT16_SPOTS[spot] == 'first' else (B - 1, c['cout'] - 1, Ho - 1, Wo - 1)
    ci = 0 if spot == 0 else c['cin'] - 1
    x[b, ci, oy * s - p + k // 2, ox * s - p + k // 2] = 300.0
    w[ch, ci, k // 2, k // 2] = 300.0
    lin = lambda a, u: F.conv2d(F.pad(a, (p,) * 4, mode='reflect'), u, stride=s)      # noqa: E731
    y = (lin(x.double(), w.double()) + bias.double().view(1, -1, 1, 1)).relu()
    assert int((y >= 65504.0).sum()) == 1 and float(y[b, ch, oy, ox]) > 7.0e4
    return types.SimpleNamespace(x=x, w=w, bias=bias, y=y, absconv=(lin(x.double().abs(), w.double().abs()), lin(x.double().abs(), sub_mask(w.double()))))


def check_split16_writer(lib, name, spot, prec, dev):
    """The same launch with a LAMA_DT_SPLIT16 y (the writer stores an fp16 inf: it must raise) and with an fp32 y (nothing it splits is out of
    range: flag 0, y within the bar)."""
    from tests import presplit_outer_util as P
    c, o = SPLIT16_CASES[name], _split16_operands(name, spot)
    what = f'split16-y {name} {E.CONV_ID(dict(c))} y@{SPLIT16_SPOTS[spot]}'
    want = {'stem': L.CONV_FAM_STEM7, 'down': L.CONV_FAM_CONV_WR}[name]          # the two writers of a split output (forced build / emulator)
    xq, yq = o.x.to(dev), torch.empty(tuple(o.y.shape), device=dev)
    wq = lib.pack_conv_weight(o.w.to(dev), None, stride=c['stride'], precision=prec)
    for y_split in (False, True):
        rc, fam, _ = lib.conv2d(L.view(xq), wq, L.view_split(yq) if y_split else L.view(yq), xq.shape[0], c['k'], c['stride'], c['pad'], L.PAD_REFLECT, False,
                                o.bias.to(dev), L.ACT_RELU, None, precision=prec, route=True)
        assert (rc, fam) == (0, want), f'{what} split y {y_split}: route {(rc, fam)}, not the writer this case is about'
        y, f, flat = P.conv(lib, dev, o.x, o.w, o.bias, c['stride'], c['pad'], prec, y_split=y_split)
        P.assert_guards(flat, what)
        ratio = float('nan')
        if y_split and prec == L.PREC_F16X3:
            assert f == 1, f'{what}: a hi part beyond the fp16 range was stored and the flag is {f}'
        else:
            assert f == 0, f'{what} {PREC_NAME[prec]} split y {y_split}: raised'
            if not y_split:
                ratio = float(((y.double() - o.y).abs() / bar_of(o.y, o.absconv, prec)).max())
                assert ratio <= 1.0, f'{what} {PREC_NAME[prec]}: y err / bar = {ratio:.3f}'
                Worst.add('split16-y', prec, ratio)
        if dev != 'cpu':
            print(f'[range-watch] split16-y-{name} {E.CONV_ID(dict(c))} {PREC_NAME[prec]} y@{SPLIT16_SPOTS[spot]} v={float(o.y.max()):.1f} split_y={int(y_split)} '
                  f'flag={f} err/bar={ratio:.4f}')


# ---- lama_multidilated_conv3x3_fwd, lama_conv2d_rect_fwd ------------------------------------------------------------------------------------------------
def _simple_operands(seed, xshape, wshape, lin, w_std, scale=True, bias=True, resid=True, relu=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*xshape, generator=g)
    w = torch.randn(*wshape, generator=g) * w_std
    sc = torch.rand(wshape[0], generator=g) + 0.5 if scale else None
    b = torch.randn(wshape[0], generator=g) if bias else None
    wf = w.double() if sc is None else w.double() * sc.double().view(-1, 1, 1, 1)
    oshape = lin(x.double(), wf).shape
    r = torch.randn(*oshape, generator=g) if resid else None

    def ref_fn(xx):
        y = lin(xx.double(), wf)
        y = y if b is None else y + b.double().view(1, -1, 1, 1)
        y = y.relu() if relu else y
        return (y if r is None else y + r.double()), (lin(xx.double().abs(), wf.abs()), lin(xx.double().abs(), sub_mask(wf)))
    return types.SimpleNamespace(x=x, w=w, scale=sc, bias=b, resid=r, ref_fn=ref_fn, oshape=tuple(oshape), clean=ref_fn(x))


@functools.lru_cache(None)
def _md_operands(idx):
    c = E.MD_CASES[idx]
    cin = c['G'] * c['cpg']
    return _simple_operands(9400 + idx, (c['B'], cin, c['H'], c['W']), (c['cout'], cin, 3, 3), E._md_lin(c['G']), 0.1)


def check_multidilated(lib, case, prec, dev, thin=False):
    o = _md_operands(E.MD_CASES.index(case))
    cin, cout = case['G'] * case['cpg'], case['cout']
    wp = lib.pack_conv_weight(o.w.to(dev), o.scale.to(dev), precision=prec)
    bias, resid = o.bias.to(dev), o.resid.to(dev)

    def launch(x, preset):
        xbuf = E.guarded_input(x, dev)
        ybuf = torch.full((o.oshape[0], PRE + cout + POST, *o.oshape[2:]), SENT, device=dev)
        flag = torch.full((1,), preset, dtype=torch.int32, device=dev)
        lib.multidilated_conv3x3(L.view(xbuf, PRE, cin), wp, L.view(ybuf, PRE, cout), case['B'], case['G'], 1, bias, L.ACT_RELU, L.view(resid),
                                 precision=prec, stream=_st(dev), range_flag=flag)
        _sync(dev)
        h = ybuf.cpu()
        return h[:, PRE:PRE + cout].double(), guards_intact(h, cout), int(flag.cpu())
    run_plan(f'multidilated {E.MD_ID(case)}', 'multidilated', o, launch, prec, dev, thin)


@functools.lru_cache(None)
def _rect_operands(case):
    B, cin, cout, H, W, k, s, p = E.FE.RECT_CASES[case]
    o = _simple_operands(9500 + sum(map(ord, case)), (B, cin, H, W), (cout, cin, *k), lambda x, w: F.conv2d(x, w, stride=s, padding=p),
                         (cin * k[0] * k[1]) ** -0.5, resid=False)
    Ho, Wo = o.oshape[2:]
    # an even plane under stride 2 without padding: the last row / column is read by no output -- the positions are those of the part that is read
    o.read_shape = (B, cin, min(H, (Ho - 1) * s - p[0] + k[0]), min(W, (Wo - 1) * s - p[1] + k[1]))
    return o


def check_rect(lib, case, prec, dev, thin=False):
    B, cin, cout, H, W, k, s, p = E.FE.RECT_CASES[case]
    o = _rect_operands(case)
    wp = lib.pack_conv_rect_weight(o.w.to(dev), o.scale.to(dev), prec)
    bias = o.bias.to(dev)

    def launch(x, preset):
        xbuf = E.guarded_input(x, dev)
        ybuf = torch.full((B, PRE + cout + POST, *o.oshape[2:]), SENT, device=dev)
        flag = torch.full((1,), preset, dtype=torch.int32, device=dev)
        lib.conv2d_rect(L.view(xbuf, PRE, cin), wp, L.view(ybuf, PRE, cout), B, k[0], k[1], s, p[0], p[1], bias=bias, act=L.ACT_RELU, precision=prec,
                        stream=_st(dev), range_flag=flag)
        _sync(dev)
        h = ybuf.cpu()
        return h[:, PRE:PRE + cout].double(), guards_intact(h, cout), int(flag.cpu())
    run_plan(f'rect {case}', 'rect', o, launch, prec, dev, thin)


# ---- LAMA_PREC_F16: fp16 tensors that already hold inf / NaN (cb_range_watch) ---------------------------------------------------------------------------
F16_VALUES = [(None, 0), (65504.0, 0), (INF, 1), (-INF, 1), (NAN, 1)]


def check_f16_io(lib, case, dev):
    """fp16 I/O (tests/test_conv_zero_pad_emu.py ZP_F16_CASES): nothing is split, the watch is on the loaded fp16 values themselves -- +-inf and NaN
    at the first, the last and the centre position raise, 65504 (the largest fp16) and the clean input do not, and the output of an unraised launch
    is finite."""
    from tests import test_conv_zero_pad_emu as Z
    o = Z.operands(case, True)
    c = case
    Ho, Wo = Z.out_size(c)
    wp = lib.pack_conv_weight(o.w.to(dev), _d(o.scale, dev), stride=c['stride'], precision=L.PREC_F16)
    bias, resid = _d(o.bias, dev), _d(o.resid, dev)
    pos = positions(o.x.shape)
    for v, want in F16_VALUES:
        for pname, idx in ([('-', None)] if v is None else [pos[0], pos[1], pos[4]]):
            x = plant(o.x, idx, v)
            xbuf = Z._guarded_input(x, dev)
            ybuf = torch.full((o.B, PRE + c['cout'] + POST, Ho, Wo), SENT, dtype=torch.float16, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            lib.conv2d(L.view(xbuf, PRE, c['cin']), wp, L.view(ybuf, PRE, c['cout']), o.B, c['k'], c['stride'], c['pad'], L.PAD_ZERO, False, bias,
                       c['act'], None if resid is None else L.view(resid), precision=L.PREC_F16, stream=_st(dev), range_flag=flag)
            _sync(dev)
            h, f = ybuf.cpu().float(), int(flag.cpu())
            assert guards_intact(h, c['cout']), f'f16 {Z.ZP_ID(c)} {pname} v={v!r}: a channel outside the output view was written'
            assert f == want, f'f16 {Z.ZP_ID(c)} {pname} v={v!r}: flag {f}, want {want}'
            if want == 0:
                assert bool(torch.isfinite(h[:, PRE:PRE + c['cout']]).all()), f'f16 {Z.ZP_ID(c)} {pname} v={v!r}: a non-finite output without the flag'
            if dev != 'cpu':
                print(f'[range-watch] f16-io {Z.ZP_ID(c)} f16 {pname} v={v!r} flag={f} err/bar=nan')


# ---- lama_winograd_conv3x3_fwd ------------------------------------------------------------------------------------------------------------------------
# The header's contract, not the direct kernels': the watch is on the row sums r of the input transform and compares 2 |r| with 65504.  With
# Vmax = max |B^T d B| over every input tile (float64): it MUST raise for Vmax >= 65520 (a transformed operand rounds to inf), it MUST NOT for
# 4 max|x| < 65504 (|r| <= 2 max|x|), and in between it raises or the output is within WINO_TOL + c (|x| (*) |w scale|).  Blind to NaN by
# contract: the system property that covers it is ``check_ffc_layer_nan``.
WINO_VALUES = [-1.0e5, INF, 1.6e4, 3.0e4, 65504.0]          # at the last position; 7e4 at all five


def wino_vmax(x, pad_mode):
    """max |B^T d B| over the tiles of the padded plane (a tile past an odd edge takes one more padded row / column); inf where x holds one."""
    H, W = x.shape[2:]
    d = F.pad(x.double(), (1, 1 + W % 2, 1, 1 + H % 2), mode='reflect' if pad_mode == L.PAD_REFLECT else 'constant').unfold(2, 4, 2).unfold(3, 4, 2)
    return float(torch.nan_to_num((E._BT @ d @ E._BT.T).abs(), nan=INF).max())


def _wino_tiles(x, pad_mode):
    H, W = x.shape[2:]
    d = F.pad(x.double(), (1, 1 + W % 2, 1, 1 + H % 2), mode='reflect' if pad_mode == L.PAD_REFLECT else 'constant').unfold(2, 4, 2).unfold(3, 4, 2)
    return (E._BT @ d @ E._BT.T).abs()


def _wino_domain(U, V, H, W):
    """|A^T| (sum_c U V) |A| per output pixel for non-negative U [o, c, 4, 4] and V [b, c, ty, tx, 4, 4]."""
    yt = E._AT.abs() @ torch.einsum('ocpq,bctupq->botupq', U, V) @ E._AT.abs().T
    return yt.permute(0, 1, 2, 4, 3, 5).reshape(yt.shape[0], yt.shape[1], 2 * yt.shape[2], 2 * yt.shape[3])[:, :, :H, :W]


def _wino_ref(o, x, pad_mode):
    """(reference, (|x| (*) |w'|, the fp16 floor of THIS kernel), the transformed form of the c term).  The kernel splits U = G g G^T scale and
    V = B^T d B: a U entry below 2^-3 carries the absolute 2^-25 (module docstring) and meets |V|, so the floor is 2^-25 |A^T| (sum |V| [0 < |U| < 2^-3]) |A|;
    the transformed c term is |A^T| (sum |U| |V|) |A| (``check_winograd``)."""
    dbl = lambda t: None if t is None else t.double()          # noqa: E731
    refl = pad_mode == L.PAD_REFLECT
    ref = KE._conv_ref(x.double(), o.w.double(), 1, 1, refl, False, dbl(o.bias), o.act, dbl(o.resid), scale=dbl(o.scale))
    absconv = KE._conv_ref(x.double().abs(), o.w.double().abs(), 1, 1, refl, False, None, 0, None, scale=dbl(o.scale))
    wf = o.w.double() if o.scale is None else o.w.double() * o.scale.double().view(-1, 1, 1, 1)
    U, V = E._G @ wf @ E._G.T, _wino_tiles(x, pad_mode)
    H, W = x.shape[2:]
    return ref, (absconv, _wino_domain(sub_mask(U), V, H, W)), _wino_domain(U.abs(), V, H, W)


def _wino_launch(lib, o, x, pad_mode, preset=0):
    xbuf = torch.full_like(o.xbuf, NAN)
    xbuf[:, 1:1 + o.cin] = x.to(o.dev)
    ybuf = torch.full((o.B, o.cout + 3, o.H, o.W), SENT, device=o.dev)
    flag = torch.full((1,), preset, dtype=torch.int32, device=o.dev)
    keep, o.xbuf = o.xbuf, xbuf
    try:
        KE.wino_run(lib, o, ybuf, range_flag=flag, pad_mode=pad_mode)
    finally:
        o.xbuf = keep
    _sync(o.dev)
    h = ybuf.cpu()
    return h[:, 2:2 + o.cout].double(), float(h[:, :2].min()) == SENT == float(h[:, :2].max()) == float(h[:, -1].min()) == float(h[:, -1].max()), int(flag.cpu())


def _wino_judge(what, prec, pname, v, vmax, xmax, flag, y, ok, ref_fn, dev, preset=0):
    name = f'winograd {what} {PREC_NAME[prec]} {pname} v={v!r} (Vmax {vmax:.1f})'
    assert ok, f'{name}: a channel outside the output view was written'
    ratio = issue = tr = float('nan')
    if preset:
        assert flag == 1, f'{name}: the flag was cleared'
    elif prec == L.PREC_BF16X3:
        assert flag == 0, f'{name}: raised'
    elif vmax >= TIE:
        assert flag == 1, f'{name}: a transformed operand beyond the fp16 range and no flag'
    elif 4.0 * xmax < 65504.0:
        assert flag == 0, f'{name}: raised although 4 max|x| = {4 * xmax:.1f}'
    if math.isfinite(vmax) and not (flag == 1 and not preset):
        ref, absconv, domain = ref_fn()
        assert bool(torch.isfinite(y).all()), f'{name}: a non-finite output'
        err, tol = (y - ref).abs(), KE.WINO_TOL[prec]
        issue = float((err / bar_of(ref, absconv, prec, tol, floor=False)).max())              # WINO_TOL + c (|x| (*) |w'|): the issue's form
        ratio = float((err / bar_of(ref, absconv, prec, tol)).max())                           # ... + the fp16 floor (f16x3)
        tr = float((err / bar_of(ref, domain, prec, tol)).max())                               # WINO_TOL + c |A^T| (sum |U| |V|) |A|
        if v is not None:
            # the documented exception (include/lama_hip.h, lama_winograd_conv3x3_fwd): see check_winograd
            assert tr <= 1.0, f'{name}: flag {flag} and err / transformed bar = {tr:.3f} (direct form {ratio:.3f})'
        else:
            assert ratio <= 1.0, f'{name}: flag {flag} and err / bar = {ratio:.3f} (transformed form {tr:.3f})'
        Worst.add('winograd', prec, ratio)
        Worst.add('winograd issue-bar', prec, issue)
        Worst.add('winograd transformed-bar', prec, tr)
    if dev != 'cpu':
        print(f'[range-watch] winograd {what} {PREC_NAME[prec]} {pname} v={v!r} flag={flag} err/bar={ratio:.4f} issue-bar={issue:.4f} transformed-bar={tr:.4f}')


def check_winograd(lib, case, prec, dev, pad_mode=L.PAD_REFLECT, thin=False):
    """The header's contract as stated above.  The output of an unflagged launch on the CLEAN input is within WINO_TOL + c (|x| (*) |w scale|) (+ the
    fp16 floor under f16x3), the form the issue states.  With a planted element the documented exception of include/lama_hip.h
    (lama_winograd_conv3x3_fwd) holds in both precisions: the c term is taken on the operands this kernel splits, c |A^T| (sum |U| |V|) |A| -- the
    planted element reaches up to nine entries of V and meets U = G g G^T, which mixes all nine taps, so an output whose own tap is small carries
    the rounding of its neighbours' taps.  Against the direct form such launches measure (flag 0): f16x3 at most 1.02 with one element of 3e4 and
    1.05 / 1.23 with the +-1.6e4 pairs (c32o128 4 x 136 zero-padded, c128o128 16 x 32, MI355X); bf16x3 1.0 .. 2.1 at 3e4 and 1.5 .. 21 at 7e4;
    against the transformed form everything is below 0.25.  Every launch prints all three ('err/bar' direct + floor, 'issue-bar' direct,
    'transformed-bar'): profiles/range_watch.txt.
    Two elements of +-1.6e4 two columns (rows) apart in one tile pin the documented factor of the watch: |r| = 2 max|x| there, 2 |r| = 64000 stays
    below 65504 and the flag must stay down -- a watch on 4 |r| would raise."""
    o = KE.wino_operands(lib, case, prec, dev)
    what = KE.WINO_ID(case) + ('' if pad_mode == L.PAD_REFLECT else '-zero')
    pos = positions(o.x.shape)
    todo = [('-', None, None)]
    if prec == L.PREC_BF16X3:
        todo += [('last', pos[1][1], v) for v in (3.0e4, 7.0e4, INF)]
    else:
        todo += [(n, i, 7.0e4) for n, i in (pos[:2] if thin or pad_mode != L.PAD_REFLECT else pos)]
        todo += [('last', pos[1][1], v) for v in ((3.0e4,) if thin else WINO_VALUES)]
        todo += [('pairs', 'pairs', 1.6e4)]
    clean = _wino_ref(o, o.x, pad_mode)
    for pname, idx, v in todo:
        if idx == 'pairs':                     # channel 0: columns 1 and 3 of row 1; the last channel: rows 1 and 3 of column 1 (odd: d0 and d2 of a tile)
            x = o.x.clone()
            x[0, 0, 1, 1], x[0, 0, 1, 3] = v, -v
            x[o.B - 1, o.cin - 1, 1, 1], x[o.B - 1, o.cin - 1, 3, 1] = -v, v
            assert 3.1e4 < wino_vmax(x, pad_mode) < TIE and 4 * float(x.abs().max()) < 65504.0
        else:
            x = plant(o.x, idx, v)
        y, ok, flag = _wino_launch(lib, o, x, pad_mode)
        _wino_judge(what, prec, pname, v, wino_vmax(x, pad_mode), float(torch.nan_to_num(x.abs(), nan=INF).max()), flag, y, ok,
                    lambda: clean if idx is None else _wino_ref(o, x, pad_mode), dev)
    if prec == L.PREC_F16X3:
        y, ok, flag = _wino_launch(lib, o, o.x, pad_mode, preset=1)
        _wino_judge(what, prec, 'preset', None, wino_vmax(o.x, pad_mode), float(o.x.abs().max()), flag, y, ok, lambda: clean, dev, preset=1)


def check_winograd_transformed_overflow(lib, case, dev):
    """The case the direct kernels do not have: four IN-RANGE elements +-2e4 at rows y, y + 2 and columns x, x + 2 of one tile (y, x odd), signs
    + - / - +, so that V00 = d00 - d02 - d20 + d22 = 8e4: Winograd must raise; lama_conv2d_fwd on the same input must not, and is right."""
    prec = L.PREC_F16X3
    o = KE.wino_operands(lib, case, prec, dev)
    yy, xx = (o.H - 3) // 2 * 2 - 1 + 2 * ((o.H - 3) // 2 == 0), (o.W - 3) // 2 * 2 - 1
    assert yy % 2 == 1 and xx % 2 == 1 and yy + 2 < o.H and xx + 2 < o.W
    x = o.x.clone()
    for dy, dx, s in ((0, 0, 1), (0, 2, -1), (2, 0, -1), (2, 2, 1)):
        x[o.B - 1, o.cin - 1, yy + dy, xx + dx] = s * 2.0e4
    vmax = wino_vmax(x, L.PAD_REFLECT)
    assert vmax >= 7.9e4 and float(x.abs().max()) == 2.0e4
    y, ok, flag = _wino_launch(lib, o, x, L.PAD_REFLECT)
    assert ok and flag == 1, f'winograd {KE.WINO_ID(case)}: V00 = {vmax:.0f} from four in-range inputs and the flag is {flag}'
    ref, (absconv, _), _ = _wino_ref(o, x, L.PAD_REFLECT)
    wf = o.w.double() if o.scale is None else o.w.double() * o.scale.double().view(-1, 1, 1, 1)
    sub = F.conv2d(F.pad(x.double().abs(), (1,) * 4, mode='reflect'), sub_mask(wf))
    xbuf = E.guarded_input(x, dev)
    ybuf = torch.full((o.B, PRE + o.cout + POST, o.H, o.W), SENT, device=dev)
    f2 = torch.zeros(1, dtype=torch.int32, device=dev)
    wd = lib.pack_conv_weight(o.w.to(dev), _d(o.scale, dev), precision=prec)
    lib.conv2d(L.view(xbuf, PRE, o.cin), wd, L.view(ybuf, PRE, o.cout), o.B, 3, 1, 1, L.PAD_REFLECT, False, o.bias_d, o.act,
               None if o.resid_d is None else L.view(o.resid_d), precision=prec, stream=_st(dev), range_flag=f2)
    _sync(dev)
    h = ybuf.cpu()
    judge(f'direct conv of {KE.WINO_ID(case)} +-2e4 x 4', 'conv2d-vs-winograd', KE.WINO_ID(case), prec, 'tile', 2.0e4, int(f2.cpu()),
          h[:, PRE:PRE + o.cout].double(), guards_intact(h, o.cout), lambda: (ref, (absconv, sub)), dev)
    if dev != 'cpu':
        print(f'[range-watch] winograd {KE.WINO_ID(case)} f16x3 tile v=+-2e4x4 flag={flag} err/bar=nan')


def check_ffc_layer_nan(lib, dev, shape=(1, 512, 32, 32)):
    """The system property the header promises for the NaN the Winograd watch cannot see: a stand-alone FFC layer whose local 3x3 conv takes the
    Winograd route, with a NaN in x_l, ends with the exec's flag raised -- through the global-branch launch (lama_conv2d_fwd) that reads the same
    buffer.  (512 channels at 32 x 32 is the smallest layer ``lama_winograd_preferred`` sends there: GPU only.)"""
    import pytest
    import torch.nn as nn
    from lama_amd import ffc
    B, C, H, W = shape
    cl = C // 4
    assert lib.winograd_preferred(B, cl, C, H, W, L.PREC_F16X3)
    torch.manual_seed(11)
    layer = ffc.FFC_BN_ACT(C, C, 3, 0.75, 0.75, padding=1, activation_layer=nn.ReLU, enable_lfu=False).eval()
    if dev != 'cpu':
        layer.to(dev)
    ex = ffc._Exec(lib)
    layer.set_exec(ex)
    assert ex.winograd and layer.ffc.precision == L.PREC_F16X3
    assert 'wino' in layer.ffc.make_scratch((B, C, H, W), torch.device(dev)), 'the layer does not take the Winograd route'
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, C, H, W, generator=g)
    xl, xg = x[:, :cl].contiguous().to(dev), x[:, cl:].contiguous().to(dev)
    yl, yg = layer((xl, xg))                                     # in range: no raise
    assert bool(torch.isfinite(yl).all()) and bool(torch.isfinite(yg).all())
    for idx in ((0, 0, 0, 0), (B - 1, cl - 1, H - 1, W - 1)):
        bad = xl.clone()
        bad[idx] = NAN
        with pytest.raises(L.LamaRangeError):
            layer((bad, xg))
    layer((xl, xg))                                              # and the flag is clean again for the next forward


# ---- lama_fourier_unit_fwd --------------------------------------------------------------------------------------------------------------------------
FU_PLANES = [(16, 16), (10, 12)]                # a power-of-two plane (fused LDS kernels) and a mixed-radix one (fft_mr_dev.inc)
FU_BINS = ['dc', 'interior-cos', 'interior-sin', 'nyquist']


def fu_plane(h, w, bin_name, amp_bin):
    """The plane whose ortho-normalised spectrum has |bin| = amp_bin at one bin of the half spectrum (and nowhere else)."""
    yy, xx = torch.arange(h, dtype=torch.float64)[:, None], torch.arange(w, dtype=torch.float64)[None, :]
    root = math.sqrt(h * w)
    if bin_name == 'dc':
        return torch.full((h, w), amp_bin / root, dtype=torch.float64)
    if bin_name == 'nyquist':
        return (amp_bin / root) * torch.cos(math.pi * xx).expand(h, w)
    ph = 2 * math.pi * (1 * yy / h + 2 * xx / w)                 # bin (ky, kx) = (1, 2)
    return (2 * amp_bin / root) * (torch.cos(ph) if bin_name == 'interior-cos' else torch.sin(ph))


@functools.lru_cache(None)
def _fu_operands(h, w):
    g = torch.Generator().manual_seed(9600 + h * 31 + w)
    B, Cn = 2, 6
    x = torch.randn(B, Cn, h, w, generator=g)
    sd = {'fu.conv_layer.weight': torch.randn(2 * Cn, 2 * Cn, 1, 1, generator=g) * 0.3,
          'fu.bn.weight': torch.rand(2 * Cn, generator=g) + 0.5, 'fu.bn.bias': torch.randn(2 * Cn, generator=g) * 0.2,
          'fu.bn.running_mean': torch.randn(2 * Cn, generator=g) * 0.1, 'fu.bn.running_var': torch.rand(2 * Cn, generator=g) * 0.5 + 0.5}
    scale = sd['fu.bn.weight'] / torch.sqrt(sd['fu.bn.running_var'] + 1e-5)
    shift = sd['fu.bn.bias'] - sd['fu.bn.running_mean'] * scale
    return types.SimpleNamespace(B=B, Cn=Cn, x=x, sd=sd, scale=scale, shift=shift)


def fu_reference(o, x):
    """(x + fu(x), the bound of the spectral 1x1's split error behind the inverse transform) in float64.  With e[o, bin] <= c (|spec| (*) |W'|) on
    the pre-activation spectrum, ReLU 1-Lipschitz and the ortho-normalised inverse (every half-spectrum bin counts at most twice, real and
    imaginary part each), a pixel of output channel o is off by at most (2 / sqrt(hw)) sum_bins (e[2o] + e[2o + 1])."""
    from oracle import lama_oracle as O
    xd = x.double()
    with torch.no_grad():
        ref = xd + O.fourier_unit(xd, {k: v.double() for k, v in o.sd.items()}, 'fu')
    h, w = x.shape[2:]
    wf = o.sd['fu.conv_layer.weight'].double() * o.scale.double().view(-1, 1, 1, 1)
    spec = KE._spec_ref(xd).abs()

    def behind_the_inverse(kernel):
        ab = F.conv2d(spec, kernel)
        return ((ab[:, 0::2] + ab[:, 1::2]).sum((2, 3)) * (2.0 / math.sqrt(h * w)))[:, :, None, None].expand_as(ref)
    return ref, (behind_the_inverse(wf.abs()), behind_the_inverse(sub_mask(wf)))           # the c term and the fp16 floor (module docstring)


def check_fourier_unit(lib, hw, prec, dev):
    """x + fu(x) (add_input on) with one spectrum bin of the first image's first channel / the last image's last channel at 7e4 (f16x3 raises,
    bf16x3 does not and matches) and at 3.5e4 (neither raises, both match), while |x| stays below 1.8e4."""
    h, w = hw
    o = _fu_operands(h, w)
    B, Cn = o.B, o.Cn
    wp = lib.pack_conv_weight(o.sd['fu.conv_layer.weight'].to(dev), o.scale.to(dev), precision=prec)
    shift = o.shift.to(dev)
    ws = torch.zeros(lib.fourier_unit_workspace_bytes(B, Cn, h, w) // 4 + 1, device=dev)
    for bi, bin_name in enumerate(FU_BINS):
        b, c = ((0, 0), (B - 1, Cn - 1))[bi % 2]
        for amp in (7.0e4, 3.5e4):
            x = o.x.clone()
            x[b, c] += fu_plane(h, w, bin_name, amp).float()
            spec = KE._spec_ref(x.double()).abs()
            assert float(x.abs().max()) < 1.8e4 and abs(float(spec.max()) - amp) < 16 and int((spec > 0.5 * amp).sum()) == 1, (bin_name, float(spec.max()))
            xbuf = E.guarded_input(x, dev)
            ybuf = torch.full((B, PRE + Cn + POST, h, w), SENT, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            lib.fourier_unit(L.view(xbuf, PRE, Cn), wp, shift, L.view(ybuf, PRE, Cn), B, True, ws, precision=prec, stream=_st(dev), range_flag=flag)
            _sync(dev)
            hy, f = ybuf.cpu(), int(flag.cpu())
            name = f'fourier_unit {h}x{w} {PREC_NAME[prec]} {bin_name} bin {amp:.0f}'
            assert guards_intact(hy, Cn), f'{name}: a channel outside the output view was written'
            ratio = float('nan')
            if prec == L.PREC_F16X3 and amp > TIE:
                assert f == 1, f'{name}: not raised'
            else:
                assert f == 0, f'{name}: raised'
                ref, bound = fu_reference(o, x)
                ratio = float(((hy[:, PRE:PRE + Cn].double() - ref).abs() / bar_of(ref, bound, prec)).max())
                assert ratio <= 1.0, f'{name}: err / bar = {ratio:.3f}'
                Worst.add('fourier_unit', prec, ratio)
            if dev != 'cpu':
                print(f'[range-watch] fourier_unit {B}x{Cn}x{h}x{w} {PREC_NAME[prec]} {bin_name}@({b},{c}) v={amp!r} flag={f} err/bar={ratio:.4f}')


def check_fft_families_differ(lib):
    """The two FU_PLANES go through different FFT kernel families (lama_fft_route_query), forward and inverse."""
    fams = []
    for (h, w) in FU_PLANES:
        x, spec = torch.zeros(1, 2, h, w), torch.zeros(1, 4, h, w // 2 + 1)
        row = []
        for inverse in (False, True):
            rc, fam, _ = lib.fft_route_query(L.view(x), None, L.view(spec), 1, inverse)
            assert rc == 0
            row.append(fam)
        fams.append(row)
    assert fams[0][0] != fams[1][0] and fams[0][1] != fams[1][1], fams


# ---- model level: LPIPS.auto_fallback, InceptionV3.auto_fallback ---------------------------------------------------------------------------------------
def check_model_fallback(make, run, x_in, x_out, first_conv_input):
    """``make()`` -> a fresh model on f16x3, ``run(model, x)`` -> its result, ``x_out`` an input whose first convolution input leaves the fp16
    range (``first_conv_input(x)`` in float64), ``x_in`` one in range.  With auto_fallback: one warning, precision bf16x3, the value bit-identical
    to a fresh bf16x3 model's; without: LamaRangeError, precision unchanged; an in-range input afterwards: no raise, no warning, no fallback."""
    import warnings
    import pytest
    assert float(first_conv_input(x_out.double().cpu()).abs().max()) > TIE > 65504.0 > float(first_conv_input(x_in.double().cpu()).abs().max())
    m = make()
    assert m.precision == L.PREC_F16X3 and m.auto_fallback
    with pytest.warns(UserWarning, match='bf16'):
        got = run(m, x_out)
    assert m.precision == L.PREC_BF16X3
    fresh = make()
    fresh.set_precision(L.PREC_BF16X3)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        want = run(fresh, x_out)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want), 'the repeated forward is not the bf16x3 result'
    strict = make()
    strict.auto_fallback = False
    with pytest.raises(L.LamaRangeError):
        run(strict, x_out)
    assert strict.precision == L.PREC_F16X3
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        y = run(strict, x_in)
    assert strict.precision == L.PREC_F16X3 and bool(torch.isfinite(y).all())
    auto = make()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        y2 = run(auto, x_in)
    assert auto.precision == L.PREC_F16X3 and torch.equal(y2, y)


def check_lpips_fallback(dev, ex=None, hw=(32, 32)):
    import numpy as np_
    from lama_amd import evaluation as EV
    from tests import lpips_util as LU
    gold = np_.load(LU.GOLDEN)
    backbone, heads = LU.backbone_state_dict(), LU.heads_state_dict(gold)

    def make():
        m = EV.PerceptualLoss(model_path=heads, backbone=backbone)
        if dev != 'cpu':
            m.to(dev)
        if ex is not None:
            m.set_exec(ex())
        return m.model
    g = torch.Generator().manual_seed(9700)
    a, b = torch.rand(2, 3, *hw, generator=g).to(dev), torch.rand(2, 3, *hw, generator=g).to(dev)
    shift, scale = torch.tensor(LU.SHIFT, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(LU.SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    # (in0, in1) stacked on a new axis so that one tensor carries the pair
    check_model_fallback(make, lambda m, x: m(x[0], x[1], normalize=True).cpu(), torch.stack([a, b]), torch.stack([a * 1.0e5, b]),
                         lambda x: (2 * x - 1 - shift) / scale)


def check_inception_fallback(dev, ex=None):
    import numpy as np_
    from lama_amd import evaluation as EV
    from tests import inception_util as IU
    weights = IU.synthetic_state_dict(np_.load(IU.GOLDEN))

    def make():
        m = EV.InceptionV3([3], resize_input=False, weights=weights)
        if dev != 'cpu':
            m.to(dev)
        if ex is not None:
            m.set_exec(ex())
        return m
    g = torch.Generator().manual_seed(9701)
    a, b = torch.rand(1, 3, 75, 75, generator=g).to(dev), torch.rand(1, 3, 75, 75, generator=g).to(dev)
    check_model_fallback(make, lambda m, x: torch.cat(m.pair(x[0], x[1])).cpu(), torch.stack([a, b]), torch.stack([a, b * 1.0e5]), lambda x: 2 * x - 1)
