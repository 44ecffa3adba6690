"""Per-layer activation ranges of a generator: WHICH tensor leaves the range of the fp16 split, in which channel, by how much.

The range watch (``ffc._Exec``) is one OR-flag per device: when it rises the whole generator moves to the bf16 split and nothing says where.
``probe_ranges`` runs ONE forward layer by layer and launches ``lama_range_stats_fwd`` on every tensor a split kernel reads or a layer hands
on; one D2H copy at the end brings every statistic back.

The probe's forward is the UN-FUSED, ONE-STREAM order: eager launches through the stand-alone module path (``FFC_BN_ACT.run`` /
``FFCResnetBlock``'s two layers / ``Conv2dBN.run`` ...) with scratch buffers of the probe's own -- no graph, no split batch, no conv1 riding in
another launch, no deferred Winograd output transform, no sparse tail -- so every intermediate exists when it is measured.  Its tensors agree
with the serving plan's to the rounding the layer-by-layer tests accept (fp32 summation order); they are not bit-equal.

Row names are the reference's module paths (``model.5.conv1.ffc.convg2g.conv1``), so they match state-dict keys.  A launch that folds several
reference modules (ConvTranspose2d + BatchNorm2d + ReLU, pad + 7x7 conv + activation) is named after the LAST of them -- the module whose
output the tensor is; ``row.module`` names the one that holds the launch's weights.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib as L
from ._lib import LamaError, LamaRangeError
from . import ffc as F
from . import pix2pixhd as P


@dataclasses.dataclass
class RangeRow:
    """One measured tensor.  ``abs_max`` is over its finite elements, ``channel`` the channel that attains it; the counters are sums over the
    channels (``per_channel``: the arrays abs_max float32 [C], n_nan, n_inf, n_over uint32 [C] as the kernel wrote them).  ``bound`` (tensors
    read by a Winograd F(2x2, 3x3) launch only) = 4 * abs_max: every element of the transformed operand B^T d B is a signed sum of four inputs.
    It is a BOUND on what that launch splits, not a measurement.  ``refused`` / ``note``: the row stands for a
    weight packing the library refused (see probe_ranges): nothing was measured, the counters stay 0 and ``abs_max`` is NaN; ``bad`` counts it."""
    name: str
    module: str
    shape: tuple
    dtype: str
    abs_max: float = 0.0
    channel: int = 0
    n_nan: int = 0
    n_inf: int = 0
    n_over: int = 0
    bound: Optional[float] = None
    winograd: bool = False
    note: str = ''
    refused: bool = False
    per_channel: Optional[tuple] = dataclasses.field(default=None, repr=False)

    @property
    def bad(self) -> int:
        return self.n_over + self.n_nan + self.n_inf + int(self.refused)

    @property
    def bad_channel(self) -> Optional[int]:
        """The first channel with an element out of range (None: the row is clean or stands for weights)."""
        if self.per_channel is None or not self.bad:
            return None
        _, nn, ni, no = self.per_channel
        return int(np.flatnonzero((nn.astype(np.uint64) + ni + no) > 0)[0])

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k in ('name', 'module', 'dtype', 'abs_max', 'channel', 'n_nan', 'n_inf', 'n_over', 'bound', 'note', 'refused')}
        d['shape'] = list(self.shape)
        if d['abs_max'] != d['abs_max']:
            d['abs_max'] = None                      # (a refused weight packing: nothing was measured; NaN is not JSON)
        return d


class RangeReport:
    """``rows`` in launch order, ``output`` = the generator's output of the probe's forward, ``tensors`` (``keep=True``) = clones of the
    measured tensors by row name."""

    def __init__(self, rows: List[RangeRow], output: torch.Tensor, limit: float, precision: int, tensors: Optional[Dict[str, torch.Tensor]]):
        self.rows, self.output, self.limit, self.precision, self.tensors = rows, output, limit, precision, tensors

    def __getitem__(self, name: str) -> RangeRow:
        for r in self.rows:
            if r.name == name:
                return r
        raise KeyError(name)

    def names(self) -> List[str]:
        return [r.name for r in self.rows]

    def first_over(self) -> Optional[RangeRow]:
        """The first row in launch order with an element beyond the limit, a NaN or an inf."""
        return next((r for r in self.rows if r.bad), None)

    def worst(self, k: int = 5) -> List[RangeRow]:
        """The k rows closest to (or furthest beyond) the limit: rows with NaN / inf first, then by the largest finite magnitude -- the Winograd
        bound where a row has one."""
        def key(r):
            m = r.bound if r.bound is not None else r.abs_max
            return (r.n_nan + r.n_inf > 0 or bool(r.note), m if m == m else float('inf'))
        return sorted(self.rows, key=key, reverse=True)[:k]

    def format(self, rows: Optional[List[RangeRow]] = None) -> str:
        rows = self.rows if rows is None else rows
        w = max([4] + [len(r.name) for r in rows])
        out = [f'{"name":<{w}}  {"shape":<20} {"dtype":<7} {"abs_max":>11} {"ch":>4} {"nan":>8} {"inf":>8} {"over":>8}  bound(4x, Winograd)']
        for r in rows:
            shp = 'x'.join(str(v) for v in r.shape)
            bound = '' if r.bound is None else f'<= {r.bound:.4g}'
            out.append(f'{r.name:<{w}}  {shp:<20} {r.dtype:<7} {r.abs_max:>11.5g} {r.channel:>4} {r.n_nan:>8} {r.n_inf:>8} {r.n_over:>8}  {bound}{r.note}')
        return '\n'.join(out)


class _Meter:
    """Launches lama_range_stats_fwd per tensor on one stream; every record stays on the device until ``finish``."""

    def __init__(self, ex: 'F._Exec', x: torch.Tensor, limit: float, keep: bool):
        self.ex, self.lib, self.limit, self.keep = ex, ex.lib, float(limit), keep
        self.device, self.stream = x.device, ex.stream(x)
        self.rows: List[RangeRow] = []
        self.outs: List[Optional[torch.Tensor]] = []
        self.tensors: Optional[Dict[str, torch.Tensor]] = {} if keep else None
        self.ws = None

    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self.ws is None or self.ws.numel() * 4 < nbytes:          # one stream: the launch before has read it when the next one writes
            self.ws = torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.int32, device=self.device)
        return self.ws

    def view(self, name: str, module: str, v: L.Tensor4, batch: int, tensor: Optional[torch.Tensor]) -> RangeRow:
        out = torch.empty(v.C, 4, dtype=torch.int32, device=self.device)
        ws = self._workspace(self.lib.range_stats_workspace_bytes(batch, v.C, v.H, v.W))
        self.lib.range_stats(v, batch, self.limit, stream=self.stream, out=out, ws=ws)
        row = RangeRow(name, module, (batch, v.C, v.H, v.W), 'float16' if v.dtype == L.DT_F16 else 'float32')
        self.rows.append(row)
        self.outs.append(out)
        if self.keep and tensor is not None:
            self.tensors[name] = tensor.clone()
        return row

    def tensor(self, name: str, module: str, t: torch.Tensor, c0: int = 0, c: Optional[int] = None) -> RangeRow:
        v = L.view(t, c0, c)
        return self.view(name, module, v, t.shape[0], t[:, c0:c0 + v.C] if self.keep else None)

    def pair(self, name: str, module: str, t: torch.Tensor, cl: int, cg: int) -> List[RangeRow]:
        """The (x_l | x_g) state of the FFC layers as two channel slices of one buffer; one row where the layer has no global output."""
        if not cg or not cl:
            return [self.tensor(name, module, t)]
        return [self.tensor(name + ':x_l', module, t, 0, cl), self.tensor(name + ':x_g', module, t, cl, cg)]

    def weights(self, name: str, module: str, err: Exception) -> RangeRow:
        """A packing the library refused (a folded weight beyond the fp16 split's range): there is no tensor to measure."""
        row = RangeRow(name, module, (), 'float32', abs_max=float('nan'), refused=True, note=f'  {err}')
        self.rows.append(row)
        self.outs.append(None)
        return row

    def finish(self):
        """ONE device-to-host copy of every record, then the host-side summary of each row."""
        got = [o for o in self.outs if o is not None]
        if not got:
            return
        amax, nn, ni, no = L.unpack_range_stats(torch.cat(got, 0))
        at = 0
        for row, o in zip(self.rows, self.outs):
            if o is None:
                continue
            C = o.shape[0]
            pc = tuple(a[at:at + C].copy() for a in (amax, nn, ni, no))
            at += C
            row.per_channel = pc
            row.channel = int(np.argmax(pc[0]))
            row.abs_max = float(pc[0][row.channel])
            row.n_nan, row.n_inf, row.n_over = (int(a.astype(np.uint64).sum()) for a in pc[1:])
            if row.winograd:
                row.bound = 4.0 * row.abs_max


def _with_fallback(m: _Meter, lay, name: str, module: str, run):
    """Run one layer; a weight the fp16 split cannot hold (LamaRangeError at pack time -- what makes ``generator(x)`` fall back before its first
    launch) becomes a row of the report, and THIS layer runs on the bf16 split so that the layers behind it are still measured."""
    try:
        return run()
    except LamaRangeError as e:
        m.weights(name + ':weights', module, e)
        prec = lay.precision
        lay.set_precision(L.PREC_BF16X3)
        try:
            return run()
        finally:
            lay.set_precision(prec)


def _mark(rows: List[RangeRow]):
    for r in rows:
        r.winograd = True


def _spectral_rows(m: _Meter, lay: 'F.FFC_BN_ACT', name: str, scratch: dict):
    """The tensors inside the global branch of an FFC layer (SpectralTransform, ffc.py:142-163), as its launches left them in the scratch set."""
    x1, t = scratch['x1'], scratch['t']
    B, C1, H, W = x1.shape
    p = name + '.ffc.convg2g'
    m.tensor(p + '.conv1', p + '.conv1.0', x1)
    ws = scratch['ws']
    dt = L.DT_F16 if x1.dtype == torch.float16 else L.DT_F32
    si, so = m.lib.fourier_unit_views(ws, B, C1, H, W, dt)
    for nm, v in ((p + '.fu:spectrum', si), (p + '.fu:spectrum_out', so)):
        kept = None
        if m.keep:                                       # the same bytes as a torch tensor
            flat = ws.view(torch.uint8)[v.ptr - ws.data_ptr():][:B * v.batch_stride * x1.element_size()]
            kept = flat.view(x1.dtype).view(B, v.C, v.H, v.W)
        m.view(nm, p + '.fu.conv_layer', v, B, kept)
    if 'lfu' in scratch:
        # the local Fourier unit (SpectralTransformLFU): its input (the gathered quadrants of x1), and the operand and the output of its spectral
        # 1x1 in the workspace of its own that _ffc_layer asked for; ':t' below then includes the tiled LFU output
        xs_in, _, ws_l = scratch['lfu']
        s = xs_in.shape[2]
        m.tensor(p + '.lfu:in', p + '.lfu', xs_in)
        si, so = m.lib.fourier_unit_views(ws_l, B, C1, s, s, dt)
        for nm, v in ((p + '.lfu:spectrum', si), (p + '.lfu:spectrum_out', so)):
            kept = None
            if m.keep:
                flat = ws_l.view(torch.uint8)[v.ptr - ws_l.data_ptr():][:B * v.batch_stride * x1.element_size()]
                kept = flat.view(x1.dtype).view(B, v.C, v.H, v.W)
            m.view(nm, p + '.lfu.conv_layer', v, B, kept)
    m.tensor(p + ':t', p + '.conv2', t)


def _ffc_layer(m: _Meter, lay: 'F.FFC_BN_ACT', name: str, src: torch.Tensor, dst: torch.Tensor, src_rows, resid=None, pad: int = 0):
    """One FFC_BN_ACT through its stand-alone path with a scratch set of the probe's own; returns nothing, measures the inner tensors."""
    f = lay.ffc
    scratch = lay.make_scratch(src.shape, src.device, own_lfu_ws=True)      # (both units' spectra are read below)
    _with_fallback(m, lay, name, name, lambda: lay.run(src, dst, scratch, resid, pad))
    if f.in_cg:
        _spectral_rows(m, lay, name, scratch)
    # the local conv took the Winograd kernel (FFC.launch's own predicate -- only layers with a global input have that launch; a refused
    # launch clears scratch['wino']): it read the whole state
    if (f.in_cg and m.ex.winograd and f.padding + pad == 1 and scratch is not None and scratch.get('wino') is not None
            and 'w_lout_wino' in (lay._packed or {}) and src.dtype == torch.float32 and dst.dtype == torch.float32):
        _mark(src_rows)


def _tail_layer(m: _Meter, layers, i: int, cur: torch.Tensor, pad: int):
    """ConvTranspose2dUp (+ BatchNorm + activation) or Conv2dOut (+ pending pad + activation) at ``layers[i]``: (output, layers taken)."""
    lay, n = layers[i], len(layers)
    B, _, H, W = cur.shape
    if isinstance(lay, F.ConvTranspose2dUp):
        bn = layers[i + 1] if i + 1 < n and isinstance(layers[i + 1], F.BatchNorm2dEval) else None
        act = layers[i + 2] if bn is not None and i + 2 < n and isinstance(layers[i + 2], F.Activation) else None
        took = 1 + (bn is not None) + (act is not None)
        dst = torch.empty(B, lay.out_channels, 2 * H, 2 * W, device=cur.device, dtype=F._act_dtype(lay.precision))
        _with_fallback(m, lay, f'model.{i}', f'model.{i}', lambda: lay.run(cur, dst, bn, F._ACT[act.kind] if act else L.ACT_NONE))
    else:
        act = layers[i + 1] if i + 1 < n and isinstance(layers[i + 1], F.Activation) else None
        took = 2 if act else 1
        k, p = lay.kernel_size[0], lay.padding[0] + pad
        dst = torch.empty(B, lay.out_channels, H + 2 * p - k + 1, W + 2 * p - k + 1, device=cur.device, dtype=torch.float32)
        _with_fallback(m, lay, f'model.{i}', f'model.{i}', lambda: lay.run(cur, dst, pad, F._ACT[act.kind] if act else L.ACT_NONE))
    return dst, took, [m.tensor(f'model.{i + took - 1}', f'model.{i}', dst)]


def _probe_ffc(gen: 'F.FFCResNetGenerator', x: torch.Tensor, m: _Meter) -> torch.Tensor:
    layers = list(gen.model)
    cur, rows, pad, i, n = x, [m.tensor('in', 'in', x)], 0, 0, len(layers)
    while i < n:
        lay, name = layers[i], f'model.{i}'
        if isinstance(lay, F.ReflectionPad2d):
            pad, i = lay.padding, i + 1
        elif isinstance(lay, F.FFC_BN_ACT):
            f = lay.ffc
            dst = torch.empty(lay.out_shape(cur.shape, pad), device=cur.device, dtype=torch.float32 if f.out_cg else F._act_dtype(lay.precision))
            _ffc_layer(m, lay, name, cur, dst, rows, None, pad)
            rows = m.pair(name, name, dst, f.out_cl, f.out_cg)
            cur, pad, i = dst, 0, i + 1
        elif isinstance(lay, F.FFCResnetBlock):
            f = lay.conv1.ffc
            tmp, dst = torch.empty_like(cur, dtype=F._act_dtype(lay.precision)), torch.empty_like(cur)      # as FFCResnetBlock.forward
            _ffc_layer(m, lay.conv1, name + '.conv1', cur, tmp, rows)
            mid = m.pair(name + '.conv1', name + '.conv1', tmp, f.out_cl, f.out_cg)
            _ffc_layer(m, lay.conv2, name + '.conv2', tmp, dst, mid, resid=cur)
            rows = m.pair(name, name + '.conv2', dst, lay.conv2.ffc.out_cl, lay.conv2.ffc.out_cg)
            cur, i = dst, i + 1
        elif isinstance(lay, F.ConcatTupleLayer):
            i += 1                                                   # free: x_l | x_g already share one buffer
        elif isinstance(lay, (F.ConvTranspose2dUp, F.Conv2dOut)):
            cur, took, rows = _tail_layer(m, layers, i, cur, pad)
            pad, i = 0, i + took
        elif isinstance(lay, (F.BatchNorm2dEval, F.Activation)):     # a bare affine layer (not behind a ConvTranspose2d): its own launch
            cur = lay(cur)
            rows = [m.tensor(name, name, cur)]
            i += 1
        else:
            raise LamaError(f'probe_ranges: no stand-alone path for layer {type(lay).__name__} of generator.model')
    return cur


def _probe_pix2pixhd(gen: 'P.GlobalGenerator', x: torch.Tensor, m: _Meter) -> torch.Tensor:
    layers = list(gen.model)
    ex, lib = gen._exec, gen._exec.lib
    cur, rows, pad, i, n = x, [m.tensor('in', 'in', x)], 0, 0, len(layers)
    while i < n:
        lay, name = layers[i], f'model.{i}'
        if isinstance(lay, F.ReflectionPad2d):
            pad, i = lay.padding, i + 1
        elif isinstance(lay, P.Conv2dBN):
            bn = layers[i + 1] if i + 1 < n and isinstance(layers[i + 1], F.BatchNorm2dEval) else None
            act = layers[i + 2] if bn is not None and i + 2 < n and isinstance(layers[i + 2], F.Activation) else None
            took = 1 + (bn is not None) + (act is not None)
            p_, mode = (pad, L.PAD_REFLECT) if pad else (lay.padding[0], L.PAD_ZERO)
            dst = torch.empty(lay.out_shape(cur.shape, p_), device=cur.device, dtype=torch.float32)
            src = cur
            _with_fallback(m, lay, name, name, lambda: lay.run(src, dst, bn, F._ACT[act.kind] if act else L.ACT_NONE, p_, mode))
            rows = [m.tensor(f'model.{i + took - 1}', name, dst)]
            cur, pad, i = dst, 0, i + took
        elif isinstance(lay, (P.ResnetBlock, P.MultidilatedResnetBlock)):
            (ca, bna), (cb, bnb) = lay.convs()
            cbk = list(lay.conv_block)
            ia, ib = cbk.index(ca), cbk.index(cb)
            t, dst = torch.empty_like(cur), torch.empty_like(cur)
            src = cur
            if isinstance(lay, P.ResnetBlock):
                B, C, H, W = cur.shape
                ws = None
                if ex.winograd and lay.precision in (L.PREC_F16X3, L.PREC_BF16X3) and lib.winograd_preferred(B, C, C, H, W, lay.precision):
                    try:
                        ok = ca.wino_ok(bna) and cb.wino_ok(bnb)
                    except LamaRangeError:                           # (the plain packing was refused: the launches below report it)
                        ok = False
                    if ok:
                        ws = torch.empty(lib.winograd_workspace_bytes(B, C, H, W) // 4, device=cur.device, dtype=torch.float32)
                if _with_fallback(m, ca, f'{name}.conv_block.{ia}', f'{name}.conv_block.{ia}',
                                  lambda: ca.run(src, t, bna, L.ACT_RELU, 1, L.PAD_REFLECT, wino_ws=ws)):
                    _mark(rows)
                mid = [m.tensor(f'{name}.conv_block.{ia + 2}', f'{name}.conv_block.{ia}', t)]
                if _with_fallback(m, cb, f'{name}.conv_block.{ib}', f'{name}.conv_block.{ib}',
                                  lambda: cb.run(t, dst, bnb, L.ACT_NONE, 1, L.PAD_REFLECT, resid=src, wino_ws=ws)):
                    _mark(mid)
            else:
                _with_fallback(m, ca, f'{name}.conv_block.{ia}', f'{name}.conv_block.{ia}', lambda: ca.run(src, t, bna, L.ACT_RELU))
                m.tensor(f'{name}.conv_block.{ia + 2}', f'{name}.conv_block.{ia}', t)
                _with_fallback(m, cb, f'{name}.conv_block.{ib}', f'{name}.conv_block.{ib}', lambda: cb.run(t, dst, bnb, L.ACT_NONE, resid=src))
            rows = [m.tensor(name, f'{name}.conv_block.{ib}', dst)]
            cur, i = dst, i + 1
        elif isinstance(lay, (F.ConvTranspose2dUp, F.Conv2dOut)):
            cur, took, rows = _tail_layer(m, layers, i, cur, pad)
            pad, i = 0, i + took
        elif isinstance(lay, (F.BatchNorm2dEval, F.Activation)):
            cur = lay(cur)
            rows = [m.tensor(name, name, cur)]
            i += 1
        else:
            raise LamaError(f'probe_ranges: no stand-alone path for layer {type(lay).__name__} of generator.model')
    return cur


def probe_ranges(generator, x: torch.Tensor, limit: float = L.F16_MAX, keep: bool = False) -> RangeReport:
    """One forward of ``generator`` (FFCResNetGenerator, GlobalGenerator or MultiDilatedGlobalGenerator) on ``x`` at its current precision and
    on its current exec, layer by layer, with the range statistics of every tensor a split kernel reads or a layer hands on (module
    docstring).  ``limit``: what counts as out of range (the fp16 split's 65504).  ``keep``: ``report.tensors[name]`` holds a clone of each
    measured tensor.

    Never raises LamaRangeError: activations beyond the range are what the report is for, and a WEIGHT the fp16 split cannot hold (the library
    refuses to pack it) becomes a row ``<layer>:weights`` while that one layer runs on the bf16 split.  The generator is left as it was found --
    precision, cached plans, ``use_graph`` -- and so is the exec's range watch, a report that deferred forwards left pending included
    (``_Exec.scratch_range_scope``).  Host-synchronising (one D2H copy at the end); a diagnostic, not a serving path."""
    if not isinstance(generator, (F.FFCResNetGenerator, P.GlobalGenerator)):
        raise LamaError(f'probe_ranges: {type(generator).__name__} is not a lama_amd generator')
    generator._check_input(x)
    x = x.contiguous()
    ex = generator._exec
    m = _Meter(ex, x, limit, keep)
    walk = _probe_ffc if isinstance(generator, F.FFCResNetGenerator) else _probe_pix2pixhd
    with torch.no_grad(), ex.scratch_range_scope(x, generator.precision):
        out = walk(generator, x, m)
        m.finish()
    return RangeReport(m.rows, out, float(limit), generator.precision, m.tensors)
