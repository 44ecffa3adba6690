"""Host-side mirror of ``GlobalGenerator`` / ``ResnetBlock`` of ``saicinpainting/training/modules/pix2pixhd.py`` (the
``pix2pixhd_global`` generator kind of the big-lama-regular and lama-regular checkpoints) and of ``MultiDilatedGlobalGenerator`` /
``MultidilatedResnetBlock`` / ``MultidilatedConv`` (the ``pix2pixhd_multidilated`` kind of the lama-dilated checkpoint) whose forward runs on
the gfx950 kernels of liblama_hip.so.

Same class names, constructor signatures, sub-module names and therefore ``state_dict`` keys as the reference
(``generator.model.13.conv_block.1.weight`` ...).  As in ``lama_amd.ffc``, the ``nn.Conv2d`` / ``nn.BatchNorm2d`` /
``nn.ConvTranspose2d`` objects are parameter containers only: every conv carries its bias (``nn.Conv2d``'s default), which folds
with the eval-mode BatchNorm behind it into one epilogue shift ``shift + scale * b``.  There is no eager / CPU fallback.

Inference only.  Options no shipped config uses (dilated blocks, FFC positions, depthwise blocks, other conv kinds / norms /
paddings, ``affine``, dilation) raise ``NotImplementedError`` at construction.
"""
from __future__ import annotations

import functools
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import LamaError, LamaRangeError
from .ffc import (_ACT, _DEFAULT_EXEC, Activation, BatchNorm2dEval, Conv2dOut, ConvTranspose2dUp, LayerSequence, ReflectionPad2d,
                  _bn_fold, _HipModule, _plan_out, _plan_up, _PlanGenerator, _run_step)


def _is_bn(norm_layer) -> bool:
    return norm_layer == 'bn' or norm_layer is nn.BatchNorm2d


def _is_relu(act) -> bool:
    return isinstance(act, nn.ReLU) or act is nn.ReLU


class Conv2dBN(nn.Conv2d, _HipModule):
    """``nn.Conv2d`` parameter container (bias included) whose forward is ``lama_conv2d_fwd``.  ``run`` folds the eval-mode
    BatchNorm that follows it in ``generator.model`` into the packed weights and the epilogue shift, and takes the activation and
    the residual add into the same launch.  A 3x3 stride-1 conv runs as Winograd F(2x2, 3x3) (``lama_winograd_conv3x3_fwd``)
    when the caller hands it a workspace."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
        nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding)
        self._packed = None
        self._exec = _DEFAULT_EXEC

    def pack(self, bn: Optional[nn.BatchNorm2d], wino: bool = False) -> dict:
        key = (id(bn), self.precision)
        if self._packed is None or self._packed['key'] != key:
            lib, w = self._exec.lib, self.weight.detach()
            b = self.bias.detach().float()
            if bn is not None:
                scale, shift = _bn_fold(bn)
                bias = shift + scale * b
            else:
                scale, bias = None, b
            self._packed = dict(key=key, scale=scale, b=bias.contiguous(),
                                w=lib.pack_conv_weight(w, scale, stride=self.stride[0], precision=self.precision))
        pk = self._packed
        if wino and 'wino' not in pk:
            # a transformed weight beyond the fp16 split's range keeps the direct kernel (as FFC.pack does)
            try:
                pk['wino'] = self._exec.lib.pack_winograd_weight(self.weight.detach(), pk['scale'], self.precision)
            except LamaRangeError:
                pk['wino'] = None
        return pk

    def wino_ok(self, bn) -> bool:
        """The Winograd form exists for this conv at the current precision (3x3, stride 1, cout % 128, cin % 32, weight in range)."""
        if (self.kernel_size != (3, 3) or self.stride != (1, 1) or self.precision not in (L.PREC_F16X3, L.PREC_BF16X3)
                or self.out_channels % 128 or self.in_channels % 32):
            return False
        return self.pack(bn, True)['wino'] is not None

    def run(self, src: torch.Tensor, dst: torch.Tensor, bn: Optional[nn.BatchNorm2d] = None, act: int = L.ACT_NONE, pad: int = 0,
            pad_mode: int = L.PAD_ZERO, resid: Optional[torch.Tensor] = None, wino_ws: Optional[torch.Tensor] = None) -> bool:
        """src -> dst = act(bn(conv(pad(src)))) [+ resid]; ``resid`` may be ``dst`` itself (every element is read before it is written, by
        the thread that writes it).  Returns True when the Winograd launch ran."""
        ex = self._exec
        pk = self.pack(bn, wino_ws is not None)
        st = ex.stream(src)
        rv = None if resid is None else L.view(resid)
        if wino_ws is not None and pk.get('wino') is not None and pad == 1:
            try:
                ex.winograd_conv3x3(L.view(src), pk['wino'], L.view(dst), src.shape[0], wino_ws, pk['b'], act, rv, precision=self.precision,
                                    stream=st, pad_mode=pad_mode)
                return True
            except LamaError as e:      # a view the Winograd entry does not take (alignment): the direct kernel
                if e.code != L.ERR_UNSUPPORTED:
                    raise
        ex.conv2d(L.view(src), pk['w'], L.view(dst), src.shape[0], self.kernel_size[0], self.stride[0], pad, pad_mode, False, pk['b'], act, rv,
                  precision=self.precision, stream=st)
        return False

    def out_shape(self, shape, pad: int):
        B, _, H, W = shape
        k, s = self.kernel_size[0], self.stride[0]
        return (B, self.out_channels, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1)

    def forward(self, x):
        self._exec.check(x)
        x = x.contiguous()
        y = torch.empty(self.out_shape(x.shape, self.padding[0]), device=x.device, dtype=torch.float32)
        with self._exec.range_scope(x, self.precision):
            self.run(x, y, None, L.ACT_NONE, self.padding[0], L.PAD_ZERO)
        return y


class ResnetBlock(_HipModule):
    """pix2pixhd.py:30-90 with reflect padding: x + BN(conv3x3(pad(ReLU(BN(conv3x3(pad(x))))))), two launches (the second one's epilogue
    adds the residual)."""

    def __init__(self, dim, padding_type, norm_layer, activation=nn.ReLU(True), use_dropout=False, conv_kind='default', dilation=1,
                 in_dim=None, groups=1, second_dilation=None):
        super().__init__()
        if padding_type != 'reflect':
            raise NotImplementedError(f'ResnetBlock: padding {padding_type!r} (only reflect, the shipped configs\' padding, is implemented)')
        if not _is_bn(norm_layer):
            raise NotImplementedError('ResnetBlock: only BatchNorm2d (eval) is folded into the kernels')
        if conv_kind not in ('default', nn.Conv2d):
            raise NotImplementedError(f'ResnetBlock: conv_kind {conv_kind!r} (only default)')
        if dilation != 1 or second_dilation not in (None, 1):
            raise NotImplementedError('ResnetBlock: dilation != 1 is not used by the shipped configs')
        if use_dropout or in_dim is not None or groups != 1:
            raise NotImplementedError('ResnetBlock: dropout / in_dim / groups are not used by the shipped configs')
        if not _is_relu(activation):
            raise NotImplementedError('ResnetBlock: the activation must be ReLU')
        self.in_dim = in_dim
        self.dim = dim
        self.conv_block = LayerSequence(ReflectionPad2d(1), Conv2dBN(dim, dim, 3), BatchNorm2dEval(dim), Activation('relu'),
                                        ReflectionPad2d(1), Conv2dBN(dim, dim, 3), BatchNorm2dEval(dim))
        self.out_channnels = dim           # (sic: the reference's attribute name)

    def convs(self):
        cb = self.conv_block
        return (cb[1], cb[2]), (cb[5], cb[6])

    def run(self, src: torch.Tensor, t: torch.Tensor, dst: torch.Tensor, wino_ws: Optional[torch.Tensor] = None) -> tuple:
        """conv A (bias + BN + ReLU) into the scratch ``t``, conv B (bias + BN + residual ``src``) into ``dst`` -- which may be ``src``: the
        state then walks in one buffer.  Returns which launches took the Winograd form."""
        (ca, bna), (cb, bnb) = self.convs()
        wa = ca.run(src, t, bna, L.ACT_RELU, 1, L.PAD_REFLECT, wino_ws=wino_ws)
        wb = cb.run(t, dst, bnb, L.ACT_NONE, 1, L.PAD_REFLECT, resid=src, wino_ws=wino_ws)
        return wa, wb

    def forward(self, x):
        self._exec.check(x)
        x = x.contiguous()
        t, dst = torch.empty_like(x, dtype=torch.float32), torch.empty_like(x, dtype=torch.float32)
        with self._exec.range_scope(x, self.precision):
            self.run(x, t, dst)
        return dst


class MultidilatedConv(_HipModule):
    """multidilated_conv.py:7-98 with ``comb_mode='cat_in'``: the input channels are cut into ``dilation_num`` equal chunks, chunk j goes through
    its own 3x3 conv to ALL output channels with dilation ``2^j`` and reflect padding ``2^j``, and the results are summed.  ``convs`` holds the
    reference's ``nn.Conv2d`` objects as parameter containers (keys ``convs.{j}.weight|bias``); the forward is ONE launch of
    ``lama_multidilated_conv3x3_fwd`` over the weights concatenated along Cin, with the BatchNorm behind it, the activation and the residual
    in its epilogue.  Every other option of the reference raises ``NotImplementedError``."""

    def __init__(self, in_dim, out_dim, kernel_size, dilation_num=3, comb_mode='sum', equal_dim=True, shared_weights=False, padding=1,
                 min_dilation=1, shuffle_in_channels=False, use_depthwise=False, **kwargs):
        super().__init__()
        if comb_mode not in ('cat_out', 'sum', 'cat_in', 'cat_both'):
            raise ValueError(f'MultidilatedConv: unknown comb_mode {comb_mode!r}')
        if comb_mode != 'cat_in':
            raise NotImplementedError(f'MultidilatedConv: comb_mode {comb_mode!r} (only cat_in, the published lama-dilated config, is implemented)')
        if not equal_dim or shared_weights or shuffle_in_channels or use_depthwise:
            raise NotImplementedError('MultidilatedConv: equal_dim=False / shared_weights / shuffle_in_channels / use_depthwise are not implemented')
        if min_dilation != 1 or padding != 1:
            raise NotImplementedError('MultidilatedConv: only min_dilation = 1 and padding = 1 (the defaults) are implemented')
        if kernel_size not in (3, (3, 3)):
            raise NotImplementedError('MultidilatedConv: only 3x3 kernels')
        if kwargs.pop('padding_mode', 'reflect') != 'reflect':
            raise NotImplementedError('MultidilatedConv: only reflect padding')
        if kwargs:
            raise NotImplementedError(f'MultidilatedConv: conv options {sorted(kwargs)} are not implemented')
        if dilation_num not in (1, 2, 4) or in_dim % (16 * dilation_num) or out_dim % 32:
            raise NotImplementedError('MultidilatedConv: dilation_num in {1, 2, 4}, (in_dim / dilation_num) % 16 == 0 and out_dim % 32 == 0 '
                                      f'are what lama_multidilated_conv3x3_fwd takes (got {dilation_num}, {in_dim}, {out_dim})')
        self.equal_dim, self.cat_in, self.cat_out = True, True, False
        self.in_dims, self.out_dims = [in_dim // dilation_num] * dilation_num, [out_dim] * dilation_num
        self.in_channels, self.out_channels, self.min_dilation = in_dim, out_dim, min_dilation
        self.convs = nn.ModuleList([nn.Conv2d(in_dim // dilation_num, out_dim, 3, padding=min_dilation * 2 ** j, dilation=min_dilation * 2 ** j,
                                              padding_mode='reflect') for j in range(dilation_num)])
        self.shuffle_in_channels = False

    @property
    def max_dilation(self) -> int:
        return self.min_dilation * 2 ** (len(self.convs) - 1)

    def pack(self, bn: Optional[nn.BatchNorm2d]) -> dict:
        key = (id(bn), self.precision)
        if self._packed is None or self._packed['key'] != key:
            w = torch.cat([c.weight.detach().float() for c in self.convs], dim=1)       # [Cout, Cin, 3, 3]: chunk j of Cin is group j
            b = torch.stack([c.bias.detach().float() for c in self.convs]).sum(0)
            if bn is not None:
                scale, shift = _bn_fold(bn)
                bias = shift + scale * b
            else:
                scale, bias = None, b
            self._packed = dict(key=key, b=bias.contiguous(), w=self._exec.lib.pack_conv_weight(w, scale, stride=1, precision=self.precision))
        return self._packed

    def run(self, src: torch.Tensor, dst: torch.Tensor, bn: Optional[nn.BatchNorm2d] = None, act: int = L.ACT_NONE,
            resid: Optional[torch.Tensor] = None):
        """src -> dst = act(bn(sum_j conv_j(pad(src_j)))) [+ resid]; ``resid`` may be ``dst`` itself (as Conv2dBN.run)."""
        if min(src.shape[2], src.shape[3]) <= self.max_dilation:
            raise LamaError(f'MultidilatedConv: a {src.shape[2]} x {src.shape[3]} plane has no reflect padding of {self.max_dilation} '
                            f'(each side must exceed the largest dilation)', code=L.ERR_UNSUPPORTED)
        ex = self._exec
        pk = self.pack(bn)
        ex.multidilated_conv3x3(L.view(src), pk['w'], L.view(dst), src.shape[0], len(self.convs), self.min_dilation, bias=pk['b'], act=act,
                                resid=None if resid is None else L.view(resid), precision=self.precision, stream=ex.stream(src))

    def forward(self, x):
        self._exec.check(x)
        x = x.contiguous()
        y = torch.empty((x.shape[0], self.out_channels) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
        with self._exec.range_scope(x, self.precision):
            self.run(x, y)
        return y


class MultidilatedResnetBlock(_HipModule):
    """pix2pixhd.py:155-175: x + BN(mdconv(ReLU(BN(mdconv(x))))) -- ``conv_block`` = [conv, BN, ReLU, conv, BN] (the padding lives in the convs),
    two launches like ``ResnetBlock``; there is no Winograd form of a dilated conv, so both always take the multi-dilated kernel."""

    def __init__(self, dim, padding_type, conv_layer, norm_layer, activation=nn.ReLU(True), use_dropout=False):
        super().__init__()
        if padding_type != 'reflect':
            raise NotImplementedError(f'MultidilatedResnetBlock: padding {padding_type!r} (only reflect)')
        if not _is_bn(norm_layer):
            raise NotImplementedError('MultidilatedResnetBlock: only BatchNorm2d (eval) is folded into the kernels')
        if use_dropout or not _is_relu(activation):
            raise NotImplementedError('MultidilatedResnetBlock: dropout / activations other than ReLU are not implemented')
        self.dim = dim
        self.conv_block = LayerSequence(conv_layer(dim, dim, kernel_size=3, padding_mode=padding_type), BatchNorm2dEval(dim), Activation('relu'),
                                        conv_layer(dim, dim, kernel_size=3, padding_mode=padding_type), BatchNorm2dEval(dim))

    def convs(self):
        cb = self.conv_block
        return (cb[0], cb[1]), (cb[3], cb[4])

    def run(self, src: torch.Tensor, t: torch.Tensor, dst: torch.Tensor, wino_ws: Optional[torch.Tensor] = None) -> tuple:
        """As ``ResnetBlock.run`` (``dst`` may be ``src``); ``wino_ws`` is ignored.  Returns the path of the two launches."""
        (ca, bna), (cb, bnb) = self.convs()
        ca.run(src, t, bna, L.ACT_RELU)
        cb.run(t, dst, bnb, L.ACT_NONE, resid=src)
        return 'multidilated', 'multidilated'

    def forward(self, x):
        self._exec.check(x)
        x = x.contiguous()
        t, dst = torch.empty_like(x, dtype=torch.float32), torch.empty_like(x, dtype=torch.float32)
        with self._exec.range_scope(x, self.precision):
            self.run(x, t, dst)
        return dst


class GlobalGenerator(_PlanGenerator):
    """pix2pixhd.py:341-436.  ``forward(x[B,input_nc,H,W]) -> [B,output_nc,H,W]``; ``.model`` has the reference's layout
    (stem 0-3, downsampling 4-12, ``n_blocks`` ResnetBlocks, 3 x (ConvTranspose2d, BN, ReLU), pad + 7x7 conv, output activation).

    The fused forward is a plan of HIP launches per input shape: stem (reflect pad + 7x7 conv + BN + ReLU), three stride-2 convs + BN +
    ReLU, the blocks on ONE state buffer (conv A into a scratch, conv B in place over the block input), three ConvTranspose2d + BN + ReLU
    and the 7x7 head with its activation.  The 512 -> 512 convs of the blocks run as Winograd F(2x2, 3x3) where
    ``lama_winograd_preferred`` says so (split precisions), otherwise as the direct kernel.  The plan cache, ``use_graph`` (replay from a
    captured hipGraph), ``input_buffer`` / ``clone_output`` and the fp16 split's range fallback (``auto_fallback``, ``defer_range_check`` /
    ``check_range``) are ``ffc._PlanGenerator``'s.  ``split_batch`` is fixed at one part (``tune_split`` decides nothing for this generator)."""

    def __init__(self, input_nc, output_nc, ngf=64, n_downsampling=3, n_blocks=9, norm_layer=nn.BatchNorm2d, padding_type='reflect',
                 conv_kind='default', activation=nn.ReLU(True), up_norm_layer=nn.BatchNorm2d, affine=None, up_activation=nn.ReLU(True),
                 dilated_blocks_n=0, dilated_blocks_n_start=0, dilated_blocks_n_middle=0, add_out_act=True, max_features=1024,
                 is_resblock_depthwise=False, ffc_positions=None, ffc_kwargs={}, dilation=1, second_dilation=None,
                 dilation_block_kind='simple', multidilation_kwargs={}):
        assert (n_blocks >= 0)
        super().__init__()
        if dilated_blocks_n or dilated_blocks_n_start or dilated_blocks_n_middle:
            raise NotImplementedError('GlobalGenerator: dilated blocks are not used by the published pix2pixhd_global checkpoints')
        if ffc_positions is not None:
            raise NotImplementedError('GlobalGenerator: ffc_positions is not implemented')
        if is_resblock_depthwise:
            raise NotImplementedError('GlobalGenerator: depthwise resnet blocks are not implemented')
        if conv_kind not in ('default', nn.Conv2d):
            raise NotImplementedError(f'GlobalGenerator: conv_kind {conv_kind!r} (only default)')
        if affine is not None:
            raise NotImplementedError('GlobalGenerator: affine is not used by the shipped configs')
        if padding_type != 'reflect':
            raise NotImplementedError(f'GlobalGenerator: padding {padding_type!r} (only reflect)')
        if not _is_bn(norm_layer) or not _is_bn(up_norm_layer):
            raise NotImplementedError('GlobalGenerator: only BatchNorm2d (eval) is folded into the kernels')
        if dilation != 1 or second_dilation not in (None, 1):
            raise NotImplementedError('GlobalGenerator: dilation != 1 is not used by the shipped configs')
        if not _is_relu(activation) or not _is_relu(up_activation):
            raise NotImplementedError('GlobalGenerator: activation / up_activation must be ReLU')

        model: List[nn.Module] = [ReflectionPad2d(3), Conv2dBN(input_nc, ngf, kernel_size=7, padding=0), BatchNorm2dEval(ngf),
                                  Activation('relu')]
        for i in range(n_downsampling):
            mult = 2 ** i
            cin, cout = min(max_features, ngf * mult), min(max_features, ngf * mult * 2)
            model += [Conv2dBN(cin, cout, kernel_size=3, stride=2, padding=1), BatchNorm2dEval(cout), Activation('relu')]
        mult = 2 ** n_downsampling
        feats_num_bottleneck = min(max_features, ngf * mult)
        for i in range(n_blocks):
            model += [ResnetBlock(feats_num_bottleneck, padding_type=padding_type, activation=activation, norm_layer=norm_layer)]
        for i in range(n_downsampling):
            mult = 2 ** (n_downsampling - i)
            cin, cout = min(max_features, ngf * mult), min(max_features, int(ngf * mult / 2))
            model += [ConvTranspose2dUp(cin, cout), BatchNorm2dEval(cout), Activation('relu')]
        model += [ReflectionPad2d(3), Conv2dOut(ngf, output_nc, kernel_size=7, padding=0)]
        if add_out_act:                                                       # base.get_activation
            kind = 'tanh' if add_out_act is True else add_out_act
            if kind not in ('tanh', 'sigmoid'):
                raise ValueError(f'Unknown activation kind {kind}')
            model.append(Activation(kind))
        self.model = LayerSequence(*model)
        self.n_downsampling = n_downsampling
        self.split_batch = 1              # one part: no split-batch plans for this generator
        super().train(False)

    # ------------------------------------------------------------------------------------------------
    def set_precision(self, precision: int):
        if precision == L.PREC_F16:
            raise NotImplementedError('GlobalGenerator: fp16 activations (LAMA_PREC_F16) are not implemented; use f16x3, bf16x3 or f32')
        return super().set_precision(precision)

    def tune_split(self, shape, device) -> int:
        """Split-batch plans are not built for this generator: always one part."""
        return 1

    def _build_plan(self, shape, device) -> dict:
        """Pre-allocate every activation buffer of an input shape and record the launch list."""
        layers = list(self.model)
        steps, bufs = [], {}
        cur, cur_shape, pad_pending = 'in', tuple(int(v) for v in shape), 0
        i, n, k = 0, len(layers), 0

        def new(shp):
            nonlocal k
            name = f'a{k}'
            k += 1
            bufs[name] = torch.empty(shp, device=device, dtype=torch.float32)
            return name

        def bn_act(j):
            bn = layers[j] if j < n and isinstance(layers[j], BatchNorm2dEval) else None
            act = layers[j + 1] if bn is not None and j + 1 < n and isinstance(layers[j + 1], Activation) else None
            return bn, act

        while i < n:
            lay = layers[i]
            if isinstance(lay, ReflectionPad2d):
                pad_pending = lay.padding
                i += 1
            elif isinstance(lay, Conv2dBN):
                bn, act = bn_act(i + 1)
                pad, mode = (pad_pending, L.PAD_REFLECT) if pad_pending else (lay.padding[0], L.PAD_ZERO)
                shp = lay.out_shape(cur_shape, pad)
                dst = new(shp)
                steps.append(('conv', lay, cur, dst, bn, _ACT[act.kind] if act else L.ACT_NONE, pad, mode))
                cur, cur_shape, pad_pending = dst, shp, 0
                i += 1 + (bn is not None) + (act is not None)
            elif isinstance(lay, (ResnetBlock, MultidilatedResnetBlock)):
                if 'st' not in bufs:
                    if cur == 'in':                   # (a generator without a stem / downsampling: the input is not overwritten)
                        bufs['st'] = torch.empty(cur_shape, device=device, dtype=torch.float32)
                        steps.append(('copy', cur, 'st'))
                    else:
                        bufs['st'] = bufs.pop(cur)
                        for j, s in enumerate(steps):
                            if s[3] == cur:
                                steps[j] = s[:3] + ('st',) + s[4:]
                    bufs['t'] = torch.empty(cur_shape, device=device, dtype=torch.float32)
                    cur = 'st'
                steps.append(('res', lay))
                i += 1
            elif isinstance(lay, ConvTranspose2dUp):
                dst = f'a{k}'; k += 1
                cur_shape, took = _plan_up(layers, i, cur, dst, cur_shape, bufs, steps, device)
                cur, i = dst, i + took
            elif isinstance(lay, Conv2dOut):
                dst = f'a{k}'; k += 1
                cur_shape, took = _plan_out(layers, i, cur, dst, cur_shape, pad_pending, bufs, steps, device)
                cur, pad_pending, i = dst, 0, i + took
            else:
                raise LamaError(f'no fused plan for layer {type(lay).__name__}; run generator.model layer by layer')
        # the 512 -> 512 convs of the blocks: Winograd where the library expects it to beat the direct kernel at this shape and every block
        # conv has its transformed weights (one workspace serves every launch: they run one after the other on one stream)
        ws = None
        blocks = [s[1] for s in steps if s[0] == 'res' and isinstance(s[1], ResnetBlock)]
        if blocks and self._exec.winograd and self.precision in (L.PREC_F16X3, L.PREC_BF16X3):
            B, C, H, W = bufs['st'].shape
            lib = self._exec.lib
            if lib.winograd_preferred(B, C, C, H, W, self.precision) and all(c.wino_ok(bn) for b in blocks for c, bn in b.convs()):
                ws = torch.empty(lib.winograd_workspace_bytes(B, C, H, W) // 4, device=device, dtype=torch.float32)
        return dict(steps=steps, bufs=bufs, out=cur, wino_ws=ws, graph=None, static_in=None, paths=None)

    def _run_plan(self, plan, x):
        bufs = plan['bufs']

        def B(name):
            return x if name == 'in' else bufs[name]

        paths = []
        for st in plan['steps']:
            kind = st[0]
            if kind == 'res':
                paths.extend(st[1].run(bufs['st'], bufs['t'], bufs['st'], plan['wino_ws']))
            elif kind == 'copy':
                B(st[2]).copy_(B(st[1]))
            else:                                   # 'conv', 'up', 'out'
                _run_step(st, B)
        plan['paths'] = [w if isinstance(w, str) else ('winograd' if w else 'direct') for w in paths]   # per bottleneck launch, in launch order
        return bufs[plan['out']]

    def conv_paths(self, shape, device) -> Optional[List[str]]:
        """'winograd' / 'direct' ('multidilated' in MultiDilatedGlobalGenerator) for each bottleneck launch of this shape's plan, in launch order (None before its first forward)."""
        plan = self._plans.get(self._plan_key(shape, device))
        return None if plan is None else plan['paths']

    def _check_input(self, x: torch.Tensor):
        super()._check_input(x)
        if x.dtype != torch.float32:
            raise LamaError(f'GlobalGenerator: fp32 input expected, got {x.dtype}')


class MultiDilatedGlobalGenerator(GlobalGenerator):
    """pix2pixhd.py:178-237 (the ``pix2pixhd_multidilated`` generator kind of the lama-dilated checkpoint): ``GlobalGenerator``'s stem, downsampling,
    ``ConvTranspose2d`` upsampling and head around ``n_blocks`` ``MultidilatedResnetBlock``s.  The plan builder and runner, the plan cache, graph
    replay and the range fallback are ``GlobalGenerator``'s; every bottleneck launch reports the path 'multidilated'.  An input must be larger
    than ``2^n_downsampling`` times the largest dilation on each side (72 pixels for the shipped config): the reference's reflect padding
    raises below that, and so does this class (``LamaError``)."""

    def __init__(self, input_nc, output_nc, ngf=64, n_downsampling=3, n_blocks=3, norm_layer=nn.BatchNorm2d, padding_type='reflect',
                 conv_kind='default', deconv_kind='convtranspose', activation=nn.ReLU(True), up_norm_layer=nn.BatchNorm2d, affine=None,
                 up_activation=nn.ReLU(True), add_out_act=True, max_features=1024, multidilation_kwargs={}, ffc_positions=None, ffc_kwargs={}):
        if deconv_kind != 'convtranspose':
            raise NotImplementedError(f'MultiDilatedGlobalGenerator: deconv_kind {deconv_kind!r} (only convtranspose)')
        # everything but the blocks is GlobalGenerator's (which refuses ffc_positions, affine, other norms / paddings / activations)
        super().__init__(input_nc, output_nc, ngf=ngf, n_downsampling=n_downsampling, n_blocks=0, norm_layer=norm_layer, padding_type=padding_type,
                         conv_kind=conv_kind, activation=activation, up_norm_layer=up_norm_layer, affine=affine, up_activation=up_activation,
                         add_out_act=add_out_act, max_features=max_features, ffc_positions=ffc_positions)
        dim = min(max_features, ngf * 2 ** n_downsampling)
        conv_layer = functools.partial(MultidilatedConv, **dict(multidilation_kwargs))
        blocks = [MultidilatedResnetBlock(dim, padding_type=padding_type, conv_layer=conv_layer, activation=activation, norm_layer=norm_layer)
                  for _ in range(n_blocks)]
        layers = list(self.model)
        at = 4 + 3 * n_downsampling
        self.model = LayerSequence(*(layers[:at] + blocks + layers[at:]))
        self.max_dilation = max([1] + [c.max_dilation for b in blocks for c, _ in b.convs()])
        super().train(False)

    @property
    def min_input_side(self) -> int:
        """The smallest input side whose bottleneck plane still has the reflect padding of the largest dilation."""
        return (self.max_dilation + 1) << self.n_downsampling

    def _check_input(self, x: torch.Tensor):
        super()._check_input(x)
        if min(x.shape[2], x.shape[3]) < self.min_input_side:
            raise LamaError(f'MultiDilatedGlobalGenerator: input {x.shape[2]} x {x.shape[3]} is too small: the bottleneck plane must exceed the '
                            f'largest dilation ({self.max_dilation}) for its reflect padding; the minimum input side is {self.min_input_side}',
                            code=L.ERR_UNSUPPORTED)
