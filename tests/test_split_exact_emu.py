"""CPU tests of the 3-term split (hi*hi + hi*lo + lo*hi) of every conv kernel family through the host SIMT emulator, BIT FOR BIT: operands on which
every product and every partial sum in any order is exact in fp32 and the split reproduces every operand exactly, so that a kernel's output must
EQUAL the float64 reference.  A lo word that is dropped, narrowed, misplaced or paired with the wrong hi word in the staging or packing code of
one family -- in one channel octet, the K tail, one tap, the fused second operand -- changes outputs; no tolerance hides it.

The operands, the exactness conditions and the functions that assert each of them: tests/split_exact_util.py (``build``).  Forms: 'A' lo on the
activations, 'B' lo on the weights (one launch cannot carry lo on both sides: lo*lo is dropped by design), 'WA' / 'WB' the width forms, in
which lo carries 10 (f16x3) / 7 (bf16x3) significant bits.  PREC_F32 runs forms A and B as a control.

Every ``check_*(lib, case, prec, form, dev)`` runs ONE launch: the input is channels [2, 2 + cin) of a buffer whose other channels hold NaN, the
output channels [2, 2 + cout) of a buffer filled with 7.0; it asserts that the guards of the output keep 7.0, that ``range_flag`` stays 0 and
``torch.equal(y.double(), ref)``; a failure reports the number of differing outputs, the first index and got / want.
tests/test_split_exact_gpu.py reruns the checks on the MI355X.

Families:
  * ``lama_conv2d_fwd``: every geometry of CONV_CASES (tests/test_kernels_emu.py) with its environment forcing -- LDS-staged, weights in
    registers (stride 1 / 2, flat 1x1, full-M), the persistent GEMMs (w4 / wk variants), stem, head, the transposed launches.  A case that asks
    for a sigmoid runs without activation (not exact).
  * the fused second operand (3x3 over x + 1x1 over x2), shapes of the two fused_second_operand tests: the target term is the 3x3 (forms 'A',
    'B', ...) or the 1x1 ('A2', 'B2', ...), the other term is plain integers times {0, +-1}.
  * ``fuse1_*`` (the next layer's conv1 in the epilogue of the 384-row launch): stage 1 is all plain (integers, weights in {0, +-1}, integer
    bias and residual) so its output y is an integer below 2^8, exact in the hi word of both splits; stage 2 carries lo on the conv1 WEIGHTS
    (folded +-(1 + m 2^-14), 4 per row) and its own any-order bound (4 * max|y| * (1 + 7 * 2^-14) + 3 < 2^10) is asserted in
    ``fuse1_operands``.  Covered: the second stage's weight split and its reading of y.  NOT covered: activation lo in stage 2 -- y would need
    lo bits, which needs lo on one side of stage 1 and an exactly splittable 17-bit y; no grid was derived for it.
  * ``lama_multidilated_conv3x3_fwd``: groups 1, 2 and 4 at the planes of KERNEL (tests/test_multidilated_emu.py).
  * ``lama_conv2d_rect_fwd``: RECT_CASES (tests/test_fid_emu.py), which hold a K tail (K = 27) and an M tail (80 rows).
  * ``lama_winograd_conv3x3_fwd``: every entry of WINO_CASES (exact and any-size geometries, split-K, forced segment widths), forms A and B on
    a grid of its own, restated on the TRANSFORMED operands: the comment above ``_wino_operands``.  Its width form exists for bf16x3 only; the
    derivation of why f16x3 has none is in the same comment.
No family is excluded.

Sensitivity, measured on a scratch copy with the lo word of every second element masked off in ``cb_split2`` (conv_split3.inc): every CONV_CASES
geometry and every fused case fails (profiles/split_exact.txt); the unmodified tree passes."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lama_amd import _lib as L
from tests import split_exact_util as U
from tests import test_fid_emu as FE
from tests import test_kernels_emu as KE
from tests import test_multidilated_emu as ME
from tests.emu import emu_lib

assert (U.PREC_F32, U.PREC_BF16X3, U.PREC_F16X3) == (L.PREC_F32, L.PREC_BF16X3, L.PREC_F16X3)

SENT = 7.0
PRE, POST = 2, 1            # guard channels in front of / behind the view
PREC_NAME = {L.PREC_F32: 'f32', L.PREC_BF16X3: 'bf16x3', L.PREC_F16X3: 'f16x3'}
# (precision, form): both splits in every form, exact fp32 as a control in forms A and B
PREC_FORMS = [(p, f) for p in (L.PREC_BF16X3, L.PREC_F16X3) for f in U.FORMS] + [(L.PREC_F32, 'A'), (L.PREC_F32, 'B')]
PF_ID = lambda pf: f'{PREC_NAME[pf[0]]}-{pf[1]}'          # noqa: E731
CONV_ID = lambda c: (f"k{c['k']}s{c['stride']}c{c['cin']}o{c['cout']}_{c['H']}x{c['W']}{'T' if c.get('transposed') else ''}"      # noqa: E731
                     + ''.join(f'{n}{c[n]}' for n in ('geo', 'w4_slots', 'wk_slots', 'ct', 'ct_grid') if n in c))


def _st(dev):
    return 0 if dev == 'cpu' else torch.cuda.current_stream().cuda_stream


def _sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


def force_env(case, monkeypatch):
    """The environment forcing of KE.test_conv2d_emulated (read by the emulator and the profiling build)."""
    for key, var in (('ct', 'LAMA_CT'), ('ct_grid', 'LAMA_CT_GRID'), ('w4_slots', 'LAMA_GEMM_W4_SLOTS'), ('wk_slots', 'LAMA_GEMM_WK_SLOTS'),
                     ('geo', 'LAMA_CW_41'), ('qr', 'LAMA_WG_QR')):
        if case.get(key) is not None:
            monkeypatch.setenv(var, str(case[key]))
    if 'w4_slots' in case:
        monkeypatch.setenv('LAMA_GEMM_W4', '2')
    if 'wk_slots' in case:
        monkeypatch.setenv('LAMA_GEMM_WK', '2')


def guarded_input(x, dev):
    """``x`` as channels [PRE, PRE + C) of a buffer whose other channels hold NaN."""
    B, C, H, W = x.shape
    buf = torch.full((B, PRE + C + POST, H, W), float('nan'))
    buf[:, PRE:PRE + C] = x
    return buf.to(dev)


def guarded_output(ref, dev):
    B, C, H, W = ref.shape
    return torch.full((B, PRE + C + POST, H, W), SENT, device=dev)


def assert_exact(ybuf, flag, ref, what):
    """The three assertions of every check: guards, range_flag, equality."""
    cout = ref.shape[1]
    h = ybuf.cpu()
    guards = torch.cat([h[:, :PRE], h[:, PRE + cout:]], 1)
    assert float(guards.min()) == SENT == float(guards.max()), f'{what}: a channel outside the output view was written'
    assert int(flag) == 0, f'{what}: range_flag raised'
    y = h[:, PRE:PRE + cout].double()
    if not torch.equal(y, ref):
        bad = (y != ref).nonzero()           # NaN != anything: counted
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {y.numel()} outputs differ; first at {i}: got {float(y[i])!r}, want {float(ref[i])!r} '
                             f'(difference {float(y[i] - ref[i]):.3e})')
    return y.numel()


def report(dev, family, what, prec, form, n):
    if dev != 'cpu':
        print(f'[split-exact] {family} {what} {PREC_NAME[prec]} form {form}: {n} outputs compared, all equal')


def _d(v, dev):
    return None if v is None else v.to(dev)


# ---- lama_conv2d_fwd ---------------------------------------------------------------------------------------------------------------------------
def conv_term(c, B=2):
    cin, cout, k, tr = c['cin'], c['cout'], c['k'], c.get('transposed', False)
    lin = lambda x, w: KE._conv_ref(x, w, c['stride'], c['pad'], True, tr, None, 0, None)      # noqa: E731
    if k == 7 and c['H'] * c['W'] > 4096:                 # production-size planes (the GPU module): no dense float64 7x7
        lin = lambda x, w: U.tap_conv2d(x, w, c['stride'], c['pad'], True)                  # noqa: E731
    return U.Term((B, cin, c['H'], c['W']), (cin, cout, k, k) if tr else (cout, cin, k, k), lin, row_axis=1 if tr else 0)


@functools.lru_cache(None)
def _conv_operands(key, prec, form, x_scale):
    c = dict(key)
    seed = 7000 + sum(int(v) * (i + 1) for i, (_, v) in enumerate(key) if isinstance(v, (int, bool)))
    return U.build([conv_term(c, c.get('B', 2))], form, prec, seed, bias=c['bias'], resid=c['resid'], relu=c['act'] == L.ACT_RELU, scale=c['scale'],
                   x_scale=x_scale)


def conv_operands(case, prec, form, x_scale=1.0):
    """Computed once per (geometry, precision, form), shared by the emulator and GPU runs of one process, never written to."""
    return _conv_operands(tuple(sorted((k, v) for k, v in case.items() if k in ('cin', 'cout', 'k', 'stride', 'pad', 'H', 'W', 'B', 'act', 'bias',
                                                                                  'resid', 'scale', 'transposed'))), prec, form, x_scale)


def run_conv(lib, case, prec, o, dev):
    """One lama_conv2d_fwd launch of the operands ``o`` on guarded buffers: (output buffer, range flag)."""
    c, tr = case, case.get('transposed', False)
    xbuf, ybuf = guarded_input(o.xs[0], dev), guarded_output(o.ref, dev)
    wp = lib.pack_conv_weight(o.ws[0].to(dev), _d(o.scale, dev), stride=c['stride'], transposed=tr, precision=prec)
    bias, resid = _d(o.bias, dev), _d(o.resid, dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.conv2d(L.view(xbuf, PRE, c['cin']), wp, L.view(ybuf, PRE, c['cout']), o.xs[0].shape[0], c['k'], c['stride'], c['pad'],
               L.PAD_ZERO if tr else L.PAD_REFLECT, tr, bias, L.ACT_RELU if o.relu else L.ACT_NONE, None if resid is None else L.view(resid),
               precision=prec, stream=_st(dev), range_flag=flag, cooperative=c.get('geo') == 3)
    _sync(dev)
    return ybuf, flag.cpu()


def check_conv(lib, case, prec, form, dev, family='conv2d'):
    o = conv_operands(case, prec, form)
    ybuf, flag = run_conv(lib, case, prec, o, dev)
    n = assert_exact(ybuf, flag, o.ref, f'{CONV_ID(case)} {PREC_NAME[prec]} form {form} (nnz {o.nnz}, grid {o.q})')
    report(dev, family, CONV_ID(case), prec, form, n)


# ---- the fused second operand ----------------------------------------------------------------------------------------------------------------------
FUSED_CASES = [dict(cl=8, cg=24, half=12, H=10, W=12), dict(cl=32, cg=160, half=64, H=6, W=35), dict(cl=32, cg=384, half=64, H=6, W=35)]
FUSED_ID = lambda c: f"cg{c['cg']}"                      # noqa: E731
FUSED_FORMS = [(p, f + t) for (p, f) in PREC_FORMS for t in ('', '2')]      # '2': the target term is the 1x1 over x2


def fused_terms(c, B=2):
    cl, cg, half, H, W = c['cl'], c['cg'], c['half'], c['H'], c['W']
    return [U.Term((B, cl, H, W), (cg, cl, 3, 3), lambda x, w: F.conv2d(F.pad(x, (1,) * 4, mode='reflect'), w)),
            U.Term((B, half, H, W), (cg, half, 1, 1), lambda x, w: F.conv2d(x, w))]


@functools.lru_cache(None)
def _fused_operands(idx, prec, form):
    c = FUSED_CASES[idx]
    return U.build(fused_terms(c), form.rstrip('2'), prec, 7100 + idx, bias=True, resid=True, relu=True, scale=True, lo_term=int(form.endswith('2')))


def check_fused_second_operand(lib, case, prec, form, dev):
    """relu(conv3x3(x) + conv1x1(x2) + b) + resid in one launch, lo on x / w ('A', 'B', ...) and on x2 / w2 ('A2', 'B2', ...) in turn."""
    o = _fused_operands(FUSED_CASES.index(case), prec, form)
    xbuf, x2buf, ybuf = guarded_input(o.xs[0], dev), guarded_input(o.xs[1], dev), guarded_output(o.ref, dev)
    sc = o.scale.to(dev)
    wp, wp2 = lib.pack_conv_weight(o.ws[0].to(dev), sc, precision=prec), lib.pack_conv_weight(o.ws[1].to(dev), sc, precision=prec)
    bias, resid = o.bias.to(dev), o.resid.to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.conv2d(L.view(xbuf, PRE, case['cl']), wp, L.view(ybuf, PRE, case['cg']), o.xs[0].shape[0], 3, 1, 1, L.PAD_REFLECT, False, bias, L.ACT_RELU,
               L.view(resid), x2=L.view(x2buf, PRE, case['half']), w2_packed=wp2, precision=prec, stream=_st(dev), range_flag=flag)
    _sync(dev)
    n = assert_exact(ybuf, flag.cpu(), o.ref, f'fused {FUSED_ID(case)} {PREC_NAME[prec]} form {form} (nnz {o.nnz})')
    report(dev, 'fused-x2', FUSED_ID(case), prec, form, n)


# ---- fuse1: the next layer's conv1 in the epilogue of the 384-row launch -------------------------------------------------------------------------------
FUSE1_CASE = dict(cl=128, cg=384, half=192, H=9, W=37, B=1)       # the ragged plane of test_conv2d_fused_next_conv1 (tests/test_kernels_gpu.py), one image


@functools.lru_cache(None)
def fuse1_operands(prec):
    """Stage 1 plain (module docstring), stage 2 = Form B of a 1x1 over y = the float64 result of stage 1."""
    c = FUSE1_CASE
    g = torch.Generator().manual_seed(7200)
    terms = fused_terms(c, c['B'])
    xs = [U._ints(t.x_shape, 2, g) for t in terms]
    wfs = [t.w_from_rows(U._pattern(t, 4, g)) for t in terms]
    bias, resid = U._ints((c['cg'],), 2, g), U._ints((c['B'], c['cg'], c['H'], c['W']), 2, g)
    y = (sum(t.lin(x, w) for t, x, w in zip(terms, xs, wfs)) + bias.view(1, -1, 1, 1)).relu() + resid
    assert torch.equal(y, y.round()) and float(y.abs().max()) < 2 ** 8, 'stage 1: y is an integer that the hi word of both splits holds'
    U._check_split(y, prec, False, 'y')
    t2 = U.Term(tuple(y.shape), (192, c['cg'], 1, 1), lambda x, w: F.conv2d(x, w))
    vals, q = U._grid_values((192, c['cg']), 'B', prec, 14, g)
    w1f = t2.w_from_rows(U._pattern(t2, 4, g).abs() * vals)
    s1 = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (192,), generator=g)]
    w1 = w1f / s1.view(-1, 1, 1, 1)
    b1 = torch.randint(-2, 3, (192,), generator=g).double() + torch.randint(0, 8, (192,), generator=g).double() * q
    U._f32_exact(w1, 'conv1 w'), U._f32_exact(w1f, 'folded conv1 w'), U._check_split(w1f, prec, True, 'folded conv1 w')
    U._any_order_bound([t2], [y], [w1f], b1, None, q)
    U._coverage(t2, t2.rows_of(w1f), full=True)           # 192 * 4 >= 384
    x1 = (t2.lin(y, w1f) + b1.view(1, -1, 1, 1)).relu()
    U._f32_exact(x1, 'the float64 reference of stage 2')
    f = lambda v: v.float()                                # noqa: E731
    return types.SimpleNamespace(xs=[f(x) for x in xs], ws=[f(w) for w in wfs], bias=f(bias), resid=f(resid), y=y, w1=f(w1), s1=f(s1), b1=f(b1), x1=x1)


def check_fuse1(lib, prec, dev):
    """lo on W1 of the fused conv1; y (stage 1) and x1 (stage 2) both equal their float64 references."""
    c, o = FUSE1_CASE, fuse1_operands(prec)
    B = c['B']
    xbuf, x2buf = guarded_input(o.xs[0], dev), guarded_input(o.xs[1], dev)
    ybuf, x1buf = guarded_output(o.y, dev), guarded_output(o.x1, dev)
    wp, wp2 = lib.pack_conv_weight(o.ws[0].to(dev), None, precision=prec), lib.pack_conv_weight(o.ws[1].to(dev), None, precision=prec)
    order = lib.fuse1_channel_order()
    wpc = lib.pack_conv_weight(o.w1[:, order].contiguous().to(dev), o.s1.to(dev), precision=prec)
    bias, resid, b1 = o.bias.to(dev), o.resid.to(dev), o.b1.to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.conv2d(L.view(xbuf, PRE, c['cl']), wp, L.view(ybuf, PRE, c['cg']), B, 3, 1, 1, L.PAD_REFLECT, False, bias, L.ACT_RELU, L.view(resid),
               x2=L.view(x2buf, PRE, c['half']), w2_packed=wp2, precision=prec, stream=_st(dev), range_flag=flag,
               fuse1=(wpc, b1, L.view(x1buf, PRE, 192)))
    _sync(dev)
    n = assert_exact(ybuf, flag.cpu(), o.y, f'fuse1 stage 1 {PREC_NAME[prec]}')
    n += assert_exact(x1buf, flag.cpu(), o.x1, f'fuse1 stage 2 {PREC_NAME[prec]} form B')
    report(dev, 'fuse1', 'c128+192o384->192_9x37', prec, 'B', n)


# ---- lama_multidilated_conv3x3_fwd ------------------------------------------------------------------------------------------------------------------
MD_CASES = [next(c for c in ME.KERNEL if c['G'] == G) for G in (1, 2, 4)]          # the smallest plane of each group count
MD_ID = lambda c: f"g{c['G']}c{c['cpg']}o{c['cout']}_{c['B']}x{c['H']}x{c['W']}"   # noqa: E731


def _md_lin(G):
    def lin(x, w):
        y = 0
        for j, (xj, wj) in enumerate(zip(x.chunk(G, 1), w.chunk(G, 1))):
            d = 2 ** j
            y = y + F.conv2d(F.pad(xj, (d,) * 4, mode='reflect'), wj, dilation=d)
        return y
    return lin


@functools.lru_cache(None)
def _md_operands(idx, prec, form):
    c = MD_CASES[idx]
    cin = c['G'] * c['cpg']
    term = U.Term((c['B'], cin, c['H'], c['W']), (c['cout'], cin, 3, 3), _md_lin(c['G']))
    return U.build([term], form, prec, 7300 + idx, bias=True, resid=True, relu=True, scale=True)


def check_multidilated(lib, case, prec, form, dev):
    o = _md_operands(MD_CASES.index(case), prec, form)
    cin = case['G'] * case['cpg']
    xbuf, ybuf = guarded_input(o.xs[0], dev), guarded_output(o.ref, dev)
    wp = lib.pack_conv_weight(o.ws[0].to(dev), o.scale.to(dev), precision=prec)
    bias, resid = o.bias.to(dev), o.resid.to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.multidilated_conv3x3(L.view(xbuf, PRE, cin), wp, L.view(ybuf, PRE, case['cout']), case['B'], case['G'], 1, bias, L.ACT_RELU, L.view(resid),
                             precision=prec, stream=_st(dev), range_flag=flag)
    _sync(dev)
    n = assert_exact(ybuf, flag.cpu(), o.ref, f'multidilated {MD_ID(case)} {PREC_NAME[prec]} form {form} (nnz {o.nnz})')
    report(dev, 'multidilated', MD_ID(case), prec, form, n)


# ---- lama_conv2d_rect_fwd ------------------------------------------------------------------------------------------------------------------------------
RECT_FORMS = [pf for pf in PREC_FORMS if pf[0] != L.PREC_F32]            # the entry refuses PREC_F32


@functools.lru_cache(None)
def _rect_operands(case, prec, form):
    B, cin, cout, H, W, k, s, p = FE.RECT_CASES[case]
    term = U.Term((B, cin, H, W), (cout, cin, *k), lambda x, w: F.conv2d(x, w, stride=s, padding=p))
    return U.build([term], form, prec, 7400 + sum(map(ord, case)), bias=True, relu=True, scale=True)


def check_rect(lib, case, prec, form, dev):
    B, cin, cout, H, W, k, s, p = FE.RECT_CASES[case]
    o = _rect_operands(case, prec, form)
    xbuf, ybuf = guarded_input(o.xs[0], dev), guarded_output(o.ref, dev)
    wp = lib.pack_conv_rect_weight(o.ws[0].to(dev), o.scale.to(dev), prec)
    bias = o.bias.to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.conv2d_rect(L.view(xbuf, PRE, cin), wp, L.view(ybuf, PRE, cout), B, k[0], k[1], s, p[0], p[1], bias=bias, act=L.ACT_RELU, precision=prec,
                    stream=_st(dev), range_flag=flag)
    _sync(dev)
    n = assert_exact(ybuf, flag.cpu(), o.ref, f'rect {case} {PREC_NAME[prec]} form {form} (nnz {o.nnz})')
    report(dev, 'rect', case, prec, form, n)


# ---- lama_winograd_conv3x3_fwd ---------------------------------------------------------------------------------------------------------------------------
# F(2x2, 3x3): Y = A^T [(G g G^T) (.) (B^T d B)] A; the split is applied to the TRANSFORMED operands U = G g G^T * scale (at pack time) and
# V = B^T d B (as it is staged), so the conditions of tests/split_exact_util.py are restated on U and V here (``_wino_operands``):
#   * at most ONE non-zero tap per (output channel, input channel) filter, so that every entry of U is that tap times 1, 1/2 or 1/4 (times the fold
#     scale 1/2, 1 or 2): a power-of-two multiple, as splittable as the tap itself; U is on the grid 2^-3 times the grid of g;
#   * form 'A': d = +-(1 + m 2^-11), 1 <= m <= 7, g in {0, +-1}.  V is a signed sum of four d: a multiple of 2^-11 below 4.02, 14 bits -- inside the
#     16 of bf16x3; hi + lo == V is asserted on every element, lo != 0 on more than a quarter (the fractions of four d can cancel, or fit the hi word),
#     |lo| >= 2^-14; U is plain;
#   * form 'B': d integers 1 <= |d| <= 2 (V an integer up to 8: plain), g = +-(1 + m 2^-11) with m ODD (an even m fits the 11 bits of an fp16 hi word): the lo
#     word of U is at least 2^-11 / 8 = 2^-14;
#   * both: every product U V is a multiple of q = 2^-14, and so is every sum of the K loop, of the split-K slices and of the output transform;
#     max |A^T| (sum_c |U| |V|) |A| + |bias| + |resid| < 2^24 q = 2^10 is asserted with the numpy restatement below;
#   * every (c, ky, kx) is non-zero in some row: tap i = r * 16 + j of row r sits at channel i mod cin, tap (i / cin) mod 9.
#   * width form 'WA', bf16x3 only: d = +-(1 + m 2^-13), 1 <= m < 32: V is a multiple of 2^-13 below 4.02, the full 16 bits, its lo word up to 7
#     bits wide.  q = 2^-13 2^-3 = 2^-16 leaves 2^24 q = 256 for nine transform-domain sums of nnz products of up to 2 * 4.02: nnz = 2 (9 * 2 * 8.04 + 6 =
#     151 < 256; nnz = 4 would reach 295); every channel octet is hit, not every tap.
# For f16x3 no width form exists: a V with a 10-bit lo word spans 21 bits, V = n q_V with n up to 2^21; U has entries of magnitude 1 on a grid
# of 1/4, so products are multiples of q_V / 4 and ONE product already reaches 2^21 q_V = 2^23 (q_V / 4), the output transform adds up to nine of
# them: past 2^24 (q_V / 4).  There the width of lo in this family's staging is covered only as far as form A goes (lo of V up to 6 bits).  A width
# form on the weights (U) is not built.
WINO_CASES = KE.WINO_CASES
_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
_G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
_AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)
WINO_FORMS = [(p, f) for p in (L.PREC_BF16X3, L.PREC_F16X3) for f in ('A', 'B')] + [(L.PREC_BF16X3, 'WA')]


def wino_transforms(x, wf):
    """(U [o, c, 4, 4], V [b, c, ty, tx, 4, 4]) of the reflect-padded plane, tiles past an odd edge on the reflected row / column."""
    H, W = x.shape[2:]
    d = F.pad(x, (1, 1 + W % 2, 1, 1 + H % 2), mode='reflect').unfold(2, 4, 2).unfold(3, 4, 2)
    return _G @ wf @ _G.T, _BT @ d @ _BT.T


@functools.lru_cache(None)
def _wino_operands(idx, prec, form):
    c = WINO_CASES[idx]
    g = torch.Generator().manual_seed(7500 + idx)
    B, cin, cout, H, W = c['B'], c['cin'], c['cout'], c['H'], c['W']
    wide = form == 'WA'
    assert not wide or prec == L.PREC_BF16X3
    q, nnz, dbits, mmax = (2.0 ** -16, 2, 13, 32) if wide else (2.0 ** -14, 16, 11, 8)
    sign = lambda shape: (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()                           # noqa: E731
    lo_vals = lambda shape, odd: sign(shape) * (1.0 + (torch.randint(0, 4, shape, generator=g) * 2 + 1 if odd else torch.randint(1, mmax, shape, generator=g)).double() * 2.0 ** -dbits)   # noqa: E731
    i = torch.arange(cout)[:, None] * nnz + torch.arange(nnz)[None, :]
    rows = torch.zeros(cout, cin * 9, dtype=torch.float64)
    rows.scatter_(1, (i % cin) * 9 + (i // cin) % 9, lo_vals((cout, nnz), True) if form == 'B' else sign((cout, nnz)))
    w = rows.view(cout, cin, 3, 3)
    assert int((w != 0).flatten(2).sum(2).max()) == 1, 'one non-zero tap per filter'
    x = U._ints((B, cin, H, W), 2, g) if form == 'B' else lo_vals((B, cin, H, W), False)
    sc = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (cout,), generator=g)] if c['scale'] else None
    wf = w if sc is None else w * sc.view(-1, 1, 1, 1)
    epi = lambda shape: torch.randint(-2, 3, shape, generator=g).double() + torch.randint(0, 8, shape, generator=g).double() * q   # noqa: E731
    bias = epi((cout,)) if c['bias'] else None
    resid = epi((B, cout, H, W)) if c['resid'] else None
    term = conv_term(dict(cin=cin, cout=cout, k=3, stride=1, pad=1, H=H, W=W), B)
    U._coverage(term, rows, full=not wide)
    Ut, V = wino_transforms(x, wf)
    for t, what in ((x, 'x'), (w, 'w'), (Ut, 'U'), (V, 'V')):
        U._f32_exact(t, what)
    U._check_split(Ut, prec, form == 'B', 'U = G g G^T * scale')
    U._check_split(V, prec, False if form == 'B' else 'some', 'V = B^T d B')
    m_abs = torch.einsum('ocpq,bctupq->botupq', Ut.abs(), V.abs())
    worst = float((_AT.abs() @ m_abs @ _AT.abs().T).max()) + (float(bias.abs().max()) if c['bias'] else 0) + (float(resid.abs().max()) if c['resid'] else 0)
    g_u, g_v = (2.0 ** -14, 1.0) if form == 'B' else (2.0 ** -3, 2.0 ** -dbits)                 # the grids of U and V: their product is q
    assert g_u * g_v == q and torch.equal((Ut / g_u).round() * g_u, Ut) and torch.equal((V / g_v).round() * g_v, V), 'a product off the grid'
    assert worst / q < 2.0 ** 24, f'any-order bound: {worst} >= 2^24 * {q}'
    ref = term.lin(x, wf)
    if bias is not None:
        ref = ref + bias.view(1, -1, 1, 1)
    if c['act'] == L.ACT_RELU:
        ref = ref.relu()
    if resid is not None:
        ref = ref + resid
    U._f32_exact(ref, 'the float64 reference')
    f = lambda v: None if v is None else v.float()           # noqa: E731
    return types.SimpleNamespace(x=f(x), w=f(w), scale=f(sc), bias=f(bias), resid=f(resid), ref=ref, worst=worst)


def check_winograd(lib, case, prec, form, dev):
    o = _wino_operands(WINO_CASES.index(case), prec, form)
    B, cin, cout, H, W = case['B'], case['cin'], case['cout'], case['H'], case['W']
    assert lib.winograd_supported(cout, cin, H, W, prec)
    xbuf, ybuf = guarded_input(o.x, dev), guarded_output(o.ref, dev)
    wp = lib.pack_winograd_weight(o.w.to(dev), _d(o.scale, dev), prec)
    ws = torch.zeros(lib.winograd_workspace_bytes(B, cout, H, W) // 4, device=dev)
    bias, resid = _d(o.bias, dev), _d(o.resid, dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.winograd_conv3x3(L.view(xbuf, PRE, cin), wp, L.view(ybuf, PRE, cout), B, ws, bias, case['act'], None if resid is None else L.view(resid),
                         precision=prec, stream=_st(dev), range_flag=flag)
    _sync(dev)
    n = assert_exact(ybuf, flag.cpu(), o.ref, f'winograd {KE.WINO_ID(case)} {PREC_NAME[prec]} form {form}')
    report(dev, 'winograd', KE.WINO_ID(case), prec, form, n)


# ---- the builder itself ----------------------------------------------------------------------------------------------------------------------------------
def test_split_model_known_answers():
    """The numpy model of the two splits on values worked out by hand."""
    for prec in (L.PREC_F16X3, L.PREC_BF16X3):
        hi, lo = U.split_model(np.float32([1 + 3 * 2.0 ** -14, -(1 + 7 * 2.0 ** -14), 4.0, 0.0]), prec)
        assert hi.tolist() == [1.0, -1.0, 4.0, 0.0] and lo.tolist() == [3 * 2.0 ** -14, -7 * 2.0 ** -14, 0.0, 0.0]
    hi, lo = U.split_model(np.float32([1024 + 1023 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -24]), L.PREC_F16X3)
    assert hi.tolist() == [1024.0, 1.0] and lo.tolist() == [1023 * 2.0 ** -11, 2.0 ** -11]           # 22 bits; the 24th is lost
    hi, lo = U.split_model(np.float32([1 + 127 * 2.0 ** -15, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -17]), L.PREC_BF16X3)
    assert hi.tolist() == [1.0, 1 + 2.0 ** -6, 1.0] and lo.tolist() == [127 * 2.0 ** -15, -2.0 ** -8, 2.0 ** -17]   # ties to even
    assert U.to_bf16(np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8])).tolist() == [1.0, 1 + 2.0 ** -6]


def test_builder_operands_and_derived_nnz():
    """What ``build`` returns on one 3x3 geometry: the grids, the lo words, the fold, and the derived nnz of the width forms."""
    c = dict(cin=8, cout=16, k=3, stride=1, pad=1, H=6, W=7)
    for prec in (L.PREC_BF16X3, L.PREC_F16X3):
        a = U.build([conv_term(c)], 'A', prec, 1, bias=True, resid=True, relu=True, scale=True)
        m = (a.xs[0].double().abs() - 1) * 2 ** 14
        assert a.q == 2.0 ** -14 and torch.equal(m, m.round()) and 1 <= float(m.min()) and float(m.max()) <= 7
        assert set(a.wfs[0].unique().tolist()) == {-1.0, 0.0, 1.0} and set(a.scale.unique().tolist()) <= {0.5, 1.0, 2.0}
        assert torch.equal(a.ws[0] * a.scale.view(-1, 1, 1, 1), a.wfs[0]) and not torch.equal(a.ws[0], a.wfs[0])
        assert a.nnz == 16 and bool(((a.wfs[0] != 0).flatten(1).sum(1) == 16).all())
        b = U.build([conv_term(c)], 'B', prec, 1, scale=True)
        assert float(b.xs[0].abs().min()) >= 1 and float(b.xs[0].abs().max()) <= 4 and torch.equal(b.xs[0], b.xs[0].round())
        nz = b.wfs[0][b.wfs[0] != 0].double().abs()
        assert float(((nz - 1) * 2 ** 14).min()) >= 1 and float(((nz - 1) * 2 ** 14).max()) <= 7
        wa, wb = U.build([conv_term(c)], 'WA', prec, 1, bias=True, resid=True), U.build([conv_term(c)], 'WB', prec, 1, bias=True, resid=True)
        # f16x3: 2^24 * 2^-11 = 8192 over |x| < 1024.5 (times 2 for the integers of WB); bf16x3: 2^24 * 2^-15 = 512 over |x| < 1.004: the cap of 64
        assert (wa.nnz, wb.nnz) == ((7, 3) if prec == L.PREC_F16X3 else (64, 64))
        _, lo = U.split_model(wa.xs[0].numpy(), prec)
        bits = np.log2(np.abs(lo).max() / np.abs(lo).min())
        assert bits > (9 if prec == L.PREC_F16X3 else 6), 'the lo words of the width form span their full width'
    with pytest.raises(AssertionError):
        U.build([conv_term(c)], 'WA', L.PREC_F32, 1)


def test_builder_any_order_bound_fires():
    c = dict(cin=64, cout=3, k=7, stride=1, pad=3, H=8, W=8)                   # the head: K = 3136 over 3 rows
    with pytest.raises(AssertionError, match='any-order bound'):                # 1046 products of |x| < 1.0005 reach 2^10 = 2^24 * 2^-14
        U.build([conv_term(c)], 'A', L.PREC_F16X3, 1, nnz=1046, adapt=False)
    with pytest.raises(AssertionError, match='any-order bound'):
        U.build([conv_term(dict(c, cout=16, k=3, pad=1))], 'B', L.PREC_F16X3, 1, nnz=500, adapt=False)    # 500 products of |x| in 1 .. 4 (2.5 on average) pass 2^10
    o = U.build([conv_term(c)], 'A', L.PREC_F16X3, 1)                           # adapt: nnz raised to 1046 on the 2^-13 grid
    assert o.nnz == 1046 and o.q == 2.0 ** -13 and o.worst < 2.0 ** 11
    o = U.build([conv_term(c)], 'B', L.PREC_BF16X3, 1)
    assert o.nnz == 1046 and o.q == 2.0 ** -13 and float(o.xs[0].abs().max()) == 2.0 and o.worst < 2.0 ** 11    # integers shrunk from 4 to 2
    with pytest.raises(AssertionError, match='no non-zero fits'):
        U._width_nnz(2.0 ** -11, 1024.5, 8, 6.0, 0.0)


def test_builder_coverage_fires():
    c = dict(cin=64, cout=3, k=7, stride=1, pad=3, H=8, W=8)
    with pytest.raises(AssertionError, match='coverage'):
        U.build([conv_term(c)], 'A', L.PREC_F16X3, 1, nnz=64, adapt=False)      # 3 * 64 < 3136
    t = conv_term(dict(cin=64, cout=8, k=1, stride=1, pad=0, H=2, W=2))
    with pytest.raises(AssertionError, match='channel octets'):
        U._coverage(t, U._pattern(t, 2, torch.Generator().manual_seed(0), prime=1), full=False)    # 16 contiguous positions: octets 0 and 1 of 8
    with pytest.raises(AssertionError, match='lo word'):
        U._check_split(torch.tensor([1.0, 1 + 2.0 ** -14], dtype=torch.float64), L.PREC_F16X3, True, 'x')
    with pytest.raises(AssertionError, match='subnormal'):
        U._check_split(torch.tensor([1 + 2.0 ** -15], dtype=torch.float64), L.PREC_F16X3, True, 'x')
    with pytest.raises(AssertionError, match='hi \\+ lo'):
        U._check_split(torch.tensor([1 + 2.0 ** -9 + 2.0 ** -20], dtype=torch.float64), L.PREC_BF16X3, True, 'x')      # 21 bits


# ---- the emulator runs -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pf', PREC_FORMS, ids=PF_ID)
@pytest.mark.parametrize('case', KE.CONV_CASES, ids=CONV_ID)
def test_conv2d_split_exact_emulated(case, pf, monkeypatch):
    force_env(case, monkeypatch)
    check_conv(emu_lib(), case, pf[0], pf[1], 'cpu')


@pytest.mark.parametrize('pf', FUSED_FORMS, ids=PF_ID)
@pytest.mark.parametrize('case', FUSED_CASES, ids=FUSED_ID)
def test_fused_second_operand_split_exact_emulated(case, pf):
    check_fused_second_operand(emu_lib(), case, pf[0], pf[1], 'cpu')


@pytest.mark.parametrize('prec', [L.PREC_BF16X3, L.PREC_F16X3], ids=['bf16x3', 'f16x3'])
def test_fuse1_split_exact_emulated(prec):
    check_fuse1(emu_lib(), prec, 'cpu')


@pytest.mark.parametrize('pf', PREC_FORMS, ids=PF_ID)
@pytest.mark.parametrize('case', MD_CASES, ids=MD_ID)
def test_multidilated_split_exact_emulated(case, pf):
    check_multidilated(emu_lib(), case, pf[0], pf[1], 'cpu')


@pytest.mark.parametrize('pf', RECT_FORMS, ids=PF_ID)
@pytest.mark.parametrize('case', list(FE.RECT_CASES))
def test_rect_split_exact_emulated(case, pf):
    check_rect(emu_lib(), case, pf[0], pf[1], 'cpu')


@pytest.mark.parametrize('pf', WINO_FORMS, ids=PF_ID)
@pytest.mark.parametrize('case', WINO_CASES, ids=KE.WINO_ID)
def test_winograd_split_exact_emulated(case, pf, monkeypatch):
    force_env(case, monkeypatch)
    check_winograd(emu_lib(), case, pf[0], pf[1], 'cpu')


def test_tap_conv2d_matches_conv2d():
    """The float64 reference of the production-size 7x7 planes (tests/test_split_exact_gpu.py) against F.conv2d, both of its branches."""
    g = torch.Generator().manual_seed(3)
    for (B, cin, cout, H, W, stride) in [(2, 5, 3, 9, 11, 1), (1, 4, 6, 10, 9, 2), (3, 4, 64, 130, 130, 1)]:
        x, w = U._ints((B, cin, H, W), 4, g), U._ints((cout, cin, 7, 7), 4, g)
        want = F.conv2d(F.pad(x, (3,) * 4, mode='reflect'), w, stride=stride)
        assert torch.equal(U.tap_conv2d(x, w, stride, 3, True), want)          # integers: exact in any order
        assert torch.equal(U.tap_conv2d(x, w, stride, 3, False), F.conv2d(x, w, stride=stride, padding=3))


def test_gpu_only_shapes_keep_an_emulator_twin():
    """The production-route shapes of the GPU module are too large for the emulator: each has a CONV_CASES geometry with the same kernel size and
    input channel count (the same K, chunking and staging code) that runs here in every form."""
    from tests import test_split_exact_gpu as G
    for (B, cin, cout, k, H, W) in G.PROD_SHAPES:
        assert any(c['k'] == k and c['cin'] == cin and c['stride'] == 1 and not c.get('transposed') and (c['cout'] <= 4) == (cout <= 4)
                   for c in KE.CONV_CASES), (cin, cout, k)
