"""Test helper of tests/test_fft_routes_emu.py and tests/test_fft_routes_gpu.py: hand-placed views, the float64 reference, the bars and the
report line of the FFT route tests.

Views.  ``L.view()`` on a fresh torch tensor always gives a 16-byte aligned pointer and a dense batch stride, so the alignment predicates of
``fft_route()`` (lama_amd/csrc/fft.hip) never see anything else.  ``View`` places a ``L.Tensor4`` by hand inside ONE flat buffer filled with a
sentinel: ``PRE`` guard elements, an element offset ``off``, ``B`` batches ``C*H*W + pad`` elements apart, ``POST`` guard elements.  The
buffer's own start is 16-byte aligned (asserted) and ``PRE`` elements are a multiple of 16 bytes in both dtypes, so ``off`` and ``pad`` alone
decide the alignment the router sees.  ``guards_intact()`` compares every element outside the view -- before it, after it, between the
batches -- with the sentinel BIT PATTERN.  ``Workspace`` does the same for the float2 scratch, ``shift`` floats (4 bytes each) off alignment.

Reference.  float64 ``numpy.fft`` on the dtype-rounded inputs: forward ``rfft2(norm='ortho')`` with the Re / Im channel interleave of the
library; inverse on the NON-Hermitian spectrum ``irfft(ifft(z, axis=-2), n=w, axis=-1)``, both ortho (the c2r step ignores Im of bins 0 and
w / 2, like torch.fft.irfftn and the kernels).  Computed once per (plane, batch, dtype) and shared by every view variant (``operands``).

Bars.  fp32: the project's own, from ``test_rfft2_irfft2``: |out - ref| <= atol + rtol |ref| with atol = 3e-5 where max(h, w) <= 128 and 2e-4
above, rtol = 1e-4.  fp16: the kernels compute in fp32 and round ONCE on the store, so the bar is the fp32 bar plus half an fp16 ulp of the
reference: the same atol, rtol = 1e-4 + 2^-11.  Derived, not measured; a case over the bar is a finding."""
import functools
import types

import numpy as np
import torch

from lama_amd import _lib as L

PRE, POST = 8, 8                  # guard elements: 32 / 16 bytes of fp32 / fp16 in front (keeps the alignment of the buffer), 8 elements behind
SENTINEL = -777.25                # exact in fp16 and fp32; no transform of these inputs produces it
WS_LEAD = 4                       # guard floats in front of the workspace (16 bytes)

# view variants: element offsets of the real-side views (x, y, resid) and of the spectrum views, batch-stride padding of both, workspace shift in floats
VARIANTS = {
    'aligned': dict(real_off=0, spec_off=0, pad=0, ws_shift=0),
    'real+1': dict(real_off=1, spec_off=0, pad=0, ws_shift=0),
    'real+2': dict(real_off=2, spec_off=0, pad=0, ws_shift=0),
    'spec+1': dict(real_off=0, spec_off=1, pad=0, ws_shift=0),
    'stride+2': dict(real_off=0, spec_off=0, pad=2, ws_shift=0),
    'ws+4': dict(real_off=0, spec_off=0, pad=0, ws_shift=1),
}
DT_NAME = {torch.float32: 'fp32', torch.float16: 'fp16'}


def bars(h, w, dtype):
    """(atol, rtol) of the module docstring."""
    atol = 3e-5 if max(h, w) <= 128 else 2e-4
    return atol, 1e-4 + (2.0 ** -11 if dtype == torch.float16 else 0.0)


def spec_ref(x):
    """x [B,C,h,w] float64 numpy -> [B,2C,h,w/2+1]: channel 2c = Re, 2c+1 = Im of rfft2(norm='ortho')."""
    z = np.fft.rfft2(x, norm='ortho')
    B, C, h, wf = z.shape
    return np.stack([z.real, z.imag], axis=2).reshape(B, 2 * C, h, wf)


def inv_ref(spec, w):
    """spec [B,2C,h,wf] float64 numpy (not Hermitian) -> [B,C,h,w]."""
    z = spec[:, 0::2] + 1j * spec[:, 1::2]
    return np.fft.irfft(np.fft.ifft(z, axis=-2, norm='ortho'), n=w, axis=-1, norm='ortho')


@functools.lru_cache(None)
def operands(h, w, B, C, dtype):
    """Inputs (torch, ``dtype``) and float64 references of one plane size, shared by every variant and both devices; never modified."""
    g = torch.Generator().manual_seed(h * 2053 + w * 7 + B * 3 + C + (1 if dtype == torch.float16 else 0))
    wf = w // 2 + 1
    x = torch.randn(B, C, h, w, generator=g).to(dtype)
    spec2 = torch.relu(torch.randn(B, 2 * C, h, wf, generator=g)).to(dtype)        # as after conv + BN + ReLU: not Hermitian
    resid = torch.randn(B, C, h, w, generator=g).to(dtype)
    inv = inv_ref(spec2.double().numpy(), w)
    return types.SimpleNamespace(x=x, spec2=spec2, resid=resid, fwd=torch.from_numpy(spec_ref(x.double().numpy())), inv=torch.from_numpy(inv),
                                 inv_resid=torch.from_numpy(inv + resid.double().numpy()))


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class View:
    """A [B,C,H,W] view placed by hand in a sentinel-filled flat buffer (module docstring).  ``data``: the contents (None: an output, left at the
    sentinel)."""

    def __init__(self, shape, dtype, dev, off=0, pad=0, data=None):
        self.shape = B, C, H, W = tuple(shape)
        self.n = C * H * W
        self.stride = self.n + pad
        self.start = PRE + off
        self.buf = torch.full((self.start + B * self.stride + POST,), SENTINEL, dtype=dtype, device=dev)
        assert self.buf.data_ptr() % 16 == 0, 'the allocator no longer returns 16-byte aligned buffers: the variants would not mean what they say'
        if data is not None:
            assert tuple(data.shape) == self.shape and data.dtype == dtype
            self._window()[:] = data.reshape(B, self.n).to(dev)
        self.t4 = L.Tensor4(self.buf.data_ptr() + self.buf.element_size() * self.start, self.stride, C, H, W,
                            L.DT_F16 if dtype == torch.float16 else L.DT_F32)

    def _window(self):
        B = self.shape[0]
        return self.buf[self.start:self.start + B * self.stride].view(B, self.stride)[:, :self.n]

    def read(self):
        """The view's contents as float64 on the host."""
        return self._window().cpu().double().view(self.shape)

    def guards_intact(self):
        B = self.shape[0]
        outside = torch.ones(self.buf.numel(), dtype=torch.bool)
        outside[self.start:self.start + B * self.stride].view(B, self.stride)[:, :self.n] = False
        want = _bits(torch.tensor([SENTINEL], dtype=self.buf.dtype))[0]
        return bool((_bits(self.buf.cpu())[outside] == want).all())

    def untouched(self):
        want = _bits(torch.tensor([SENTINEL], dtype=self.buf.dtype))[0]
        return bool((_bits(self.buf.cpu()) == want).all())


class Workspace:
    """``nbytes`` of float scratch ``shift`` floats behind a 16-byte aligned address, sentinel-filled guards on both sides.  ``nbytes`` == 0: no
    workspace at all (``t`` is None)."""

    def __init__(self, nbytes, dev, shift=0):
        self.t, self.buf = None, None
        if nbytes:
            n = (nbytes + 3) // 4
            self.buf = torch.full((WS_LEAD + shift + n + POST,), SENTINEL, dtype=torch.float32, device=dev)
            assert self.buf.data_ptr() % 16 == 0
            self.lo, self.hi = WS_LEAD + shift, WS_LEAD + shift + n
            self.t = self.buf[self.lo:self.hi]

    @property
    def addr(self):
        return None if self.t is None else self.t.data_ptr()

    @property
    def nbytes(self):
        return 0 if self.t is None else self.t.numel() * 4

    def guards_intact(self):
        if self.buf is None:
            return True
        b = _bits(self.buf.cpu())
        want = _bits(torch.tensor([SENTINEL]))[0]
        return bool((b[:self.lo] == want).all() and (b[self.hi:] == want).all())


def sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


def stream(dev):
    return 0 if dev == 'cpu' else torch.cuda.current_stream().cuda_stream


def max_err(out, ref, h, w, dtype, what):
    """Asserts the bar element by element; returns the largest absolute error."""
    atol, rtol = bars(h, w, dtype)
    err = (out - ref).abs()
    over = err > atol + rtol * ref.abs()
    worst = float(err.max())
    assert not bool(over.any()), (f'{what}: {int(over.sum())} of {over.numel()} elements over atol {atol} + rtol {rtol:.3e} |ref|; worst error {worst:.3e} '
                                  f'(|ref| max {float(ref.abs().max()):.3e})')
    assert bool(torch.isfinite(out).all()), what
    return worst


def report(dev, route, h, w, B, C, dtype, variant, e_fwd, e_inv_resid, e_inv, tag=''):
    print(f"[fft-routes] {'emu' if dev == 'cpu' else 'gpu'} route {route[0]}/{route[1]} {h}x{w} B{B} C{C} {DT_NAME[dtype]} {variant}{tag}: "
          f'max error fwd {e_fwd:.3e}, inv+resid {e_inv_resid:.3e}, inv {e_inv:.3e}')


def check_case(lib, dev, h, w, B, C, dtype, variant, route, tag=''):
    """One plane size through one view variant: asserts the route (``route`` = (family, kind), pinned by the caller) by the query for the views
    actually built, both directions; then rfft2, irfft2 with a residual and irfft2 without one against the reference at the bars, with the
    guards of every output and of the workspace checked after each launch."""
    v = VARIANTS[variant]
    o = operands(h, w, B, C, dtype)
    wf = w // 2 + 1
    rshape, sshape = (B, C, h, w), (B, 2 * C, h, wf)
    x = View(rshape, dtype, dev, v['real_off'], v['pad'], o.x)
    resid = View(rshape, dtype, dev, v['real_off'], v['pad'], o.resid)
    spec_in = View(sshape, dtype, dev, v['spec_off'], v['pad'], o.spec2)
    spec_out = View(sshape, dtype, dev, v['spec_off'], v['pad'])
    y_r, y_n = View(rshape, dtype, dev, v['real_off'], v['pad']), View(rshape, dtype, dev, v['real_off'], v['pad'])
    ws = Workspace(lib.fft_workspace_bytes(B, C, h, w), dev, v['ws_shift'])
    assert ws.t is not None or not v['ws_shift'], 'the workspace variant needs a plane with a workspace'
    what = f'{h}x{w} B{B} C{C} {DT_NAME[dtype]} {variant}{tag}'
    for (real, r, spec, inverse) in ((x, None, spec_out, False), (y_r, resid, spec_in, True), (y_n, None, spec_in, True)):
        got = lib.fft_route_query(real.t4, None if r is None else r.t4, spec.t4, B, inverse, ws.addr, ws.nbytes)
        assert got == (0,) + tuple(route), f'{what} inverse={inverse}: route query says {got}, expected {(0,) + tuple(route)}'
    st = stream(dev)
    lib.rfft2(x.t4, spec_out.t4, B, ws.t, stream=st)
    sync(dev)
    e_fwd = max_err(spec_out.read(), o.fwd, h, w, dtype, what + ' forward')
    assert spec_out.guards_intact() and ws.guards_intact(), what + ' forward: wrote outside its views'
    lib.irfft2(spec_in.t4, resid.t4, y_r.t4, B, ws.t, stream=st)
    sync(dev)
    e_ir = max_err(y_r.read(), o.inv_resid, h, w, dtype, what + ' inverse + resid')
    assert y_r.guards_intact() and ws.guards_intact(), what + ' inverse + resid: wrote outside its views'
    lib.irfft2(spec_in.t4, None, y_n.t4, B, ws.t, stream=st)
    sync(dev)
    e_in = max_err(y_n.read(), o.inv, h, w, dtype, what + ' inverse')
    assert y_n.guards_intact() and ws.guards_intact(), what + ' inverse: wrote outside its views'
    for inp, src in ((x, o.x), (resid, o.resid), (spec_in, o.spec2)):            # the inputs are read only
        assert torch.equal(inp.read(), src.double()) and inp.guards_intact(), what + ': an input changed'
    report(dev, route, h, w, B, C, dtype, variant, e_fwd, e_ir, e_in, tag)


def check_refused(lib, dev, h, w, dtype=torch.float32, B=1, C=2):
    """A plane that no kernel serves in one direction is refused in BOTH, with nothing launched: LAMA_ERR_UNSUPPORTED from the query and from the
    entries, every output buffer still at its sentinel."""
    o = operands(h, w, B, C, dtype)
    wf = w // 2 + 1
    x, resid = View((B, C, h, w), dtype, dev, data=o.x), View((B, C, h, w), dtype, dev, data=o.resid)
    spec_in, spec_out, y = View((B, 2 * C, h, wf), dtype, dev, data=o.spec2), View((B, 2 * C, h, wf), dtype, dev), View((B, C, h, w), dtype, dev)
    ws = Workspace(lib.fft_workspace_bytes(B, C, h, w), dev)
    assert ws.nbytes > 0
    codes = []
    for (real, r, spec, inverse) in ((x, None, spec_out, False), (y, resid, spec_in, True), (y, None, spec_in, True)):
        codes.append(lib.fft_route_query(real.t4, None if r is None else r.t4, spec.t4, B, inverse, ws.addr, ws.nbytes)[0])
        try:
            if inverse:
                lib.irfft2(spec.t4, None if r is None else r.t4, real.t4, B, ws.t, stream=stream(dev))
            else:
                lib.rfft2(real.t4, spec.t4, B, ws.t, stream=stream(dev))
            codes.append(0)
        except L.LamaError as e:
            codes.append(e.code)
        sync(dev)
    assert codes == [L.ERR_UNSUPPORTED] * 6, (h, w, codes)
    assert spec_out.untouched() and y.untouched() and ws.guards_intact() and bool((ws.t == SENTINEL).all()), f'{h}x{w}: a refused call wrote something'
    print(f"[fft-routes] {'emu' if dev == 'cpu' else 'gpu'} refused {h}x{w} {DT_NAME[dtype]}: LAMA_ERR_UNSUPPORTED in both directions, outputs untouched")


def check_fourier_unit_refused(lib, dev, h=2, w=1204, C=2):
    """lama_fourier_unit_fwd on a plane the transforms refuse: LAMA_ERR_UNSUPPORTED before the first launch -- y keeps its sentinel and the
    NaN-filled workspace stays NaN (the rfft2 would have written the spectrum there)."""
    g = torch.Generator().manual_seed(h * 5 + w)
    x = View((1, C, h, w), torch.float32, dev, data=torch.randn(1, C, h, w, generator=g))
    y = View((1, C, h, w), torch.float32, dev)
    wp = lib.pack_conv_weight((torch.randn(2 * C, 2 * C, 1, 1, generator=g) * 0.3).to(dev), None)
    bias = torch.zeros(2 * C, device=dev)
    ws = torch.full((lib.fourier_unit_workspace_bytes(1, C, h, w) // 4 + 1,), float('nan'), device=dev)
    code = 0
    try:
        lib.fourier_unit(x.t4, wp, bias, y.t4, 1, True, ws, stream=stream(dev))
    except L.LamaError as e:
        code = e.code
    sync(dev)
    assert code == L.ERR_UNSUPPORTED, code
    assert y.untouched(), 'the refused FourierUnit wrote y'
    assert bool(torch.isnan(ws).all()), 'the refused FourierUnit launched something: its workspace was written'
    print(f"[fft-routes] {'emu' if dev == 'cpu' else 'gpu'} refused fourier_unit {h}x{w} C{C}: LAMA_ERR_UNSUPPORTED, y and workspace untouched")
