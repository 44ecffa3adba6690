"""Test helper: operands on which a 3-term split convolution (hi*hi + hi*lo + lo*hi, fp32 accumulation) is EXACT, so that a kernel can be
compared with a float64 reference by equality (tests/test_split_exact_emu.py, tests/test_split_exact_gpu.py).

A launch computes  y = act(sum_t lin_t(x_t, w_t * scale) + bias) + resid  over one or more terms t (the conv itself, the fused 1x1 second
operand).  ``build`` returns operands with these properties and asserts each of them (the name of the asserting function in brackets):

  1. every operand equals its float32 value [_f32_exact];
  2. one side of every term is "plain": weights in {0, +-1} or activations that are small integers.  A plain value has lo = 0 in both
     splits, so only ONE side of a product carries lo bits and the dropped lo*lo term is zero [_check_split with want_lo=False];
  3. the other side of the TARGET term is on a dyadic grid q = 2^-g and the numpy model of the split (round to fp16 / bf16, round the fp32
     residual again: ``split_model``) gives hi + lo == value with lo != 0 for every element, and for fp16 |lo| >= 2^-14: no test depends on
     fp16 subnormals [_check_split with want_lo=True];
  4. any-order exactness: every product is a multiple of q, so every partial sum in any order is a multiple of q too, and it is exactly
     representable in fp32 iff its magnitude stays below 2^24 q.  max_out (sum_k |w x| + |bias| + |resid|) < 2^24 q is computed with
     lin(|x|, |w|) [_any_order_bound];
  5. forms 'A' and 'B': every K position (c, ky, kx) of the target term is non-zero in at least one output row; width forms: every channel
     octet is [_coverage];
  6. the float64 reference round-trips through float32 [build].

Forms (``form``), the target term being ``lo_term``:
  'A'   activation lo:  x = +-(1 + m q), 1 <= m <= 7, q = 2^-14 (2^-13 where the bound needs it); w in {0, +-1}: hi = +-1, lo = +-m q;
  'B'   weight lo:      x integers 1 <= |x| <= 4 (fewer where the bound needs it); folded w = +-(1 + m q) on the sparse pattern;
  'WA'  width, activations: f16x3  x = +-(2^10 + m 2^-11), m odd < 2^10 (lo = m 2^-11: 10 significant bits, normal);
                            bf16x3 x = +-(1 + m 2^-15), 1 <= m < 128 (lo = m 2^-15: 7 significant bits);   w in {0, +-1};
  'WB'  width, weights: the same values as folded weights, x integers 1 <= |x| <= 2.
The other terms of a launch are plain on both sides (integers times {0, +-1}).

Row r of the target weight has ``nnz`` non-zeros at K positions ((r nnz + j) P mod K), j < nnz, P a prime that does not divide K: a bijection of
Z_K, so the rows cover K iff cout nnz >= K.  nnz starts at 16 and is raised to ceil(K / cout) where that is needed for coverage (the 7x7 head); for
the width forms it is the largest value the bound allows, derived in ``_width_nnz`` (f16x3: 2^24 2^-11 = 8192, |x| < 1024.5: 7 products of
+-1 weights, 3 of |x| <= 2 integers -- coverage of K is not asked of them).

Epilogue: bias and resid are multiples of q with |v| < 3, the activation is ReLU or none (sigmoid / tanh are not exact; a case that asks for
one runs without).  The BatchNorm fold scale is drawn from {0.5, 1, 2} per output row; the RAW weight handed to the packer is folded / scale (an
exact fp32 quotient), so the packer's multiplication runs and its product is the value described above."""
import math
import types

import numpy as np
import torch

PREC_F32, PREC_BF16X3, PREC_F16X3 = 0, 1, 2            # lama_amd._lib.PREC_*: asserted by tests/test_split_exact_emu.py
FORMS = ('A', 'B', 'WA', 'WB')
F16_MIN_NORMAL = 2.0 ** -14
_PRIMES = (7919, 104729, 1299709, 15485863, 32452843)


class Term:
    """One linear term of a launch: ``lin(x, w)`` is bilinear, float64 in and out; ``w_shape`` is the reference layout, its output-channel axis
    ``row_axis`` (1 for ConvTranspose2d)."""

    def __init__(self, x_shape, w_shape, lin, row_axis=0):
        self.x_shape, self.w_shape, self.lin, self.row_axis = tuple(x_shape), tuple(w_shape), lin, row_axis
        self.cout = self.w_shape[row_axis]
        self.K = int(np.prod(self.w_shape)) // self.cout
        rest = [s for i, s in enumerate(self.w_shape) if i != row_axis]
        self.taps = int(np.prod(rest[1:]))                 # K = cin * taps, c = position // taps

    def w_from_rows(self, rows):
        """[cout, K] -> the reference layout."""
        rest = [s for i, s in enumerate(self.w_shape) if i != self.row_axis]
        w = rows.reshape(self.cout, *rest)
        return w.transpose(0, 1).contiguous() if self.row_axis == 1 else w

    def rows_of(self, w):
        return (w.transpose(0, 1) if self.row_axis == 1 else w).reshape(self.cout, self.K)


def tap_conv2d(x, w, stride, pad, reflect):
    """F.conv2d(F.pad(x, pad), w, stride=stride) in float64 as matrix products over the channels and shifted adds over the taps.  For the
    7x7 layers on production-size planes, where the dense float64 conv builds a column buffer of gigabytes."""
    xp = torch.nn.functional.pad(x, (pad,) * 4, mode='reflect') if (pad and reflect) else torch.nn.functional.pad(x, (pad,) * 4)
    (B, cin, Hp, Wp), (cout, _, kh, kw) = xp.shape, w.shape
    Ho, Wo = (Hp - kh) // stride + 1, (Wp - kw) // stride + 1
    win = lambda t, ky, kx: t[..., ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]       # noqa: E731
    y = torch.zeros(B, cout, Ho, Wo, dtype=torch.float64)
    if B * cout * kh * kw * Hp * Wp <= 2 ** 26:           # few output channels (the head): z[o, ky, kx] = w[o, :, ky, kx] . x over the whole plane first
        z = (w.permute(0, 2, 3, 1).reshape(cout * kh * kw, cin) @ xp.reshape(B, cin, Hp * Wp)).view(B, cout, kh, kw, Hp, Wp)
        for ky in range(kh):
            for kx in range(kw):
                y += win(z[:, :, ky, kx], ky, kx)
    else:
        for ky in range(kh):
            for kx in range(kw):
                y += torch.einsum('oc,bchw->bohw', w[:, :, ky, kx], win(xp, ky, kx))
    return y


def to_bf16(a):
    """float32 array rounded to bf16 (nearest even), as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def split_model(a, prec):
    """(hi, lo) of the 3-term split as float64 arrays: hi = rnd(a), lo = rnd(fl32(a - hi)), rnd = fp16 / bf16 round-to-nearest-even."""
    a = np.ascontiguousarray(a, np.float32)
    rnd = (lambda v: v.astype(np.float16).astype(np.float32)) if prec == PREC_F16X3 else to_bf16
    hi = rnd(a)
    lo = rnd((a - hi).astype(np.float32))
    return hi.astype(np.float64), lo.astype(np.float64)


def _f32_exact(t, what):
    assert torch.equal(t.float().double(), t), f'{what}: not a float32 value'


def _check_split(t, prec, want_lo, what):
    """Condition 2 / 3 of the module docstring on the NON-ZERO elements of ``t`` (float64)."""
    if prec == PREC_F32:
        return
    v = t[t != 0].numpy()
    hi, lo = split_model(v, prec)
    assert np.array_equal(hi + lo, v), f'{what}: hi + lo != value for {int((hi + lo != v).sum())} elements'
    if prec == PREC_F16X3:
        assert float(np.abs(v).max(initial=0.0)) <= 65504.0, f'{what}: beyond the fp16 range'
    if want_lo:
        if want_lo == 'some':             # sums of lo-carrying values (the Winograd input transform): the fractions can cancel, or fit the hi word
            assert v.size and int((lo != 0).sum()) * 4 > lo.size, f'{what}: only {int((lo != 0).sum())} of {lo.size} elements have a lo word'
            lo = lo[lo != 0]
        assert v.size and bool((lo != 0).all()), f'{what}: {int((lo == 0).sum())} elements without a lo word'
        if prec == PREC_F16X3:
            assert float(np.abs(lo).min()) >= F16_MIN_NORMAL, f'{what}: a subnormal fp16 lo word ({float(np.abs(lo).min())})'
    else:
        assert not bool(lo.any()), f'{what}: a plain operand with a lo word'


def _any_order_bound(terms, xs, wfs, bias, resid, q):
    """Condition 4: max over the outputs of sum |w x| + |bias| + |resid|, asserted < 2^24 q.  Returns the maximum."""
    tot = sum(t.lin(x.abs(), w.abs()) for t, x, w in zip(terms, xs, wfs))
    if bias is not None:
        tot = tot + bias.abs().view(1, -1, 1, 1)
    if resid is not None:
        tot = tot + resid.abs()
    worst = float(tot.max())
    assert worst / q < 2.0 ** 24, f'any-order bound: max sum |w x| = {worst} >= 2^24 * {q} = {2.0 ** 24 * q}'
    return worst


def _coverage(term, rows, full):
    """Condition 5 on the [cout, K] pattern of the target term."""
    hit = (rows != 0).any(0)
    if full:
        assert bool(hit.all()), f'coverage: {int((~hit).sum())} of {term.K} K positions are zero in every output row'
    else:
        cin = term.K // term.taps
        octet = torch.arange(term.K) // term.taps // 8
        got = set(octet[hit].tolist())
        assert got == set(range((cin + 7) // 8)), f'coverage: channel octets {sorted(set(range((cin + 7) // 8)) - got)} are hit by no row'


def _pattern(term, nnz, g, prime=None, spread=False):
    """[cout, K] of {0, +-1}: ``nnz`` non-zeros per row at ((r nnz + j) P mod K); ``spread``: see below."""
    K, cout = term.K, term.cout
    nnz = min(nnz, K)
    P = prime or next(p for p in _PRIMES if math.gcd(p, K) == 1)
    idx = torch.arange(cout)[:, None] * nnz + torch.arange(nnz)[None, :]
    # fewer non-zeros than K positions and no prime asked for (the width forms): evenly spaced, so that cout nnz >= cin / 8 of them meet every octet
    idx = idx * K // (cout * nnz) if (spread and cout * nnz < K) else idx * P % K
    rows = torch.zeros(cout, K, dtype=torch.float64)
    sign = torch.randint(0, 2, (cout, nnz), generator=g).double() * 2 - 1
    rows.scatter_(1, idx, sign)
    return rows


def _ints(shape, amax, g):
    """Integers with 1 <= |v| <= amax."""
    return (torch.randint(1, amax + 1, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).double()


def _grid_values(shape, form, prec, gbits, g):
    """The lo-carrying values of the module docstring, and their grid q."""
    sign = (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()
    if form in ('A', 'B'):
        q = 2.0 ** -gbits
        return sign * (1.0 + torch.randint(1, 8, shape, generator=g).double() * q), q
    if prec == PREC_F16X3:
        q = 2.0 ** -11
        return sign * (1024.0 + (torch.randint(0, 512, shape, generator=g) * 2 + 1).double() * q), q
    q = 2.0 ** -15
    return sign * (1.0 + torch.randint(1, 128, shape, generator=g).double() * q), q


def _width_nnz(q, vmax, xmax, epi_max, other, want=64):
    """The width forms' non-zeros per row: the largest n <= ``want`` with n * vmax * xmax + epi_max + other < 2^24 q (condition 4 with every
    product at its largest).  f16x3: (8192 - 6 - other) / 1024.5 -> 7 for +-1 weights, / 2049 -> 3 for |x| <= 2."""
    budget = 2.0 ** 24 * q - epi_max - other
    n = int(np.ceil(budget / (vmax * xmax))) - 1          # strict inequality
    assert n >= 1, f'width form: no non-zero fits the any-order bound (budget {budget}, product {vmax * xmax})'
    return min(n, want)


def build(terms, form, prec, seed, bias=False, resid=False, relu=False, scale=False, lo_term=0, nnz=16, gbits=14, xmax=4, x_scale=1.0,
          adapt=True):
    """Operands of one launch (module docstring).  ``terms``: list of Term with the same cout and output shape.  ``adapt``: let the builder
    raise nnz for coverage and coarsen the grid / shrink the integers for the bound (the tests of the builder switch it off to see the
    assertions fire).  ``x_scale``: a power of two applied to the target activations of form 'A' AFTER the checks -- only for the recorded
    subnormal measurement, which leaves condition 3 on purpose.
    Returns a namespace: xs, ws (raw weights, reference layout), wfs (folded), scale, bias, resid (float32 tensors or None), ref (float64),
    q, nnz, worst (the any-order maximum), relu."""
    assert form in FORMS and prec in (PREC_F32, PREC_BF16X3, PREC_F16X3) and not (form in ('WA', 'WB') and prec == PREC_F32)
    T = terms[lo_term]
    cout = T.cout
    assert all(t.cout == cout for t in terms)
    width = form in ('WA', 'WB')
    tries = [(nnz, gbits, xmax)]
    if adapt and not width:
        need = -(-T.K // cout)
        tries = [(max(nnz, need), gb, xm) for gb, xm in ((gbits, xmax), (gbits - 1, xmax), (gbits - 1, 2), (gbits - 1, 1), (gbits - 2, 1))]
    err = None
    for (n_try, gb, xm) in tries:
        g = torch.Generator().manual_seed(seed)
        try:
            return _build_once(terms, form, prec, g, bias, resid, relu, scale, lo_term, n_try, gb, xm, x_scale, width)
        except AssertionError as e:
            if not str(e).startswith('any-order bound'):
                raise
            err = e
    raise err


def _build_once(terms, form, prec, g, bias, resid, relu, scale, lo_term, nnz, gbits, xmax, x_scale, width):
    T = terms[lo_term]
    cout = T.cout
    if form == 'WB':
        xmax = min(xmax, 2)
    # the target term's lo-carrying side first: it fixes the grid
    act_side = form in ('A', 'WA')
    vals, q = _grid_values(T.x_shape if act_side else (cout, T.K), form, prec, gbits, g)
    epi = lambda shape: (torch.randint(-2, 3, shape, generator=g).double() + torch.randint(0, 8, shape, generator=g).double() * q)   # noqa: E731
    out_shape = tuple(T.lin(torch.zeros(T.x_shape, dtype=torch.float64), torch.zeros(T.w_shape, dtype=torch.float64)).shape)
    b = epi((cout,)) if bias else None
    r = epi(out_shape) if resid else None
    epi_max = (float(b.abs().max()) if bias else 0.0) + (float(r.abs().max()) if resid else 0.0)
    xs, wfs = [None] * len(terms), [None] * len(terms)
    other = 0.0
    for i, t in enumerate(terms):                       # the plain terms: integers times {0, +-1}
        if i != lo_term:
            xs[i] = _ints(t.x_shape, xmax, g)
            wfs[i] = t.w_from_rows(_pattern(t, 16, g))
            other += min(16, t.K) * xmax
    if width:
        vmax = float(vals.abs().max())
        nnz = _width_nnz(q, vmax, 1 if act_side else xmax, epi_max, other)
    rows = _pattern(T, nnz, g, spread=width)
    if act_side:
        xs[lo_term], wfs[lo_term] = vals, T.w_from_rows(rows)
    else:
        xs[lo_term], wfs[lo_term] = _ints(T.x_shape, xmax, g), T.w_from_rows(rows.abs() * vals)      # vals carries the sign
    _coverage(T, T.rows_of(wfs[lo_term]), full=not width)
    sc = None
    if scale:
        sc = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (cout,), generator=g)]
    ws = []
    for t, wf in zip(terms, wfs):
        if sc is None:
            ws.append(wf.clone())
        else:
            shape = [1] * wf.dim()
            shape[t.row_axis] = cout
            raw = wf / sc.view(shape)
            assert torch.equal(raw.float().double() * sc.view(shape), wf), 'the fold scale is not exact'
            ws.append(raw)
    for i, (x, w, wf) in enumerate(zip(xs, ws, wfs)):
        _f32_exact(x, f'x[{i}]'), _f32_exact(w, f'w[{i}]'), _f32_exact(wf, f'folded w[{i}]')
        _check_split(x, prec, i == lo_term and act_side, f'x[{i}]')
        _check_split(wf, prec, i == lo_term and not act_side, f'folded w[{i}]')
    for v, what in ((b, 'bias'), (r, 'resid')):
        if v is not None:
            _f32_exact(v, what)
            assert torch.equal(torch.round(v / q) * q, v), f'{what}: off the grid'
    worst = _any_order_bound(terms, xs, wfs, b, r, q)
    if x_scale != 1.0:
        assert form == 'A' and np.log2(x_scale) == int(np.log2(x_scale))
        xs[lo_term] = xs[lo_term] * x_scale
        b = None if b is None else b * x_scale
        r = None if r is None else r * x_scale
        for i in range(len(terms)):
            if i != lo_term:
                xs[i] = xs[i] * x_scale
        q *= x_scale
    ref = sum(t.lin(x, wf) for t, x, wf in zip(terms, xs, wfs))
    if b is not None:
        ref = ref + b.view(1, -1, 1, 1)
    if relu:
        ref = ref.relu()
    if r is not None:
        ref = ref + r
    _f32_exact(ref, 'the float64 reference')
    assert torch.equal(torch.round(ref / q) * q, ref), 'the reference is off the grid'
    f = lambda v: None if v is None else v.float()       # noqa: E731
    return types.SimpleNamespace(xs=[f(x) for x in xs], ws=[f(w) for w in ws], wfs=[f(w) for w in wfs], scale=f(sc), bias=f(b), resid=f(r),
                                 ref=ref, q=q, nnz=nnz, worst=worst, relu=relu, form=form, prec=prec)
