"""Test helper for the pix2pixhd_multidilated generator (lama_amd.pix2pixhd.MultiDilatedGlobalGenerator, the lama-dilated checkpoint): the
shipped config, seeded BN-calibrated synthetic weights and an fp32 torch restatement of the reference's forward (pix2pixhd.py:155-237,
multidilated_conv.py:36-98) written from the state dict alone."""
import torch
import torch.nn.functional as F

from tests.regular_util import block_input, calib_input, sample  # noqa: F401  (shared with the regular generator's helper)

# configs/training/generator/pix2pixhd_multidilated_catin_4dil_9b.yaml
LAMA_DILATED = dict(input_nc=4, output_nc=3, ngf=64, n_downsampling=3, n_blocks=9, conv_kind='default', add_out_act='sigmoid',
                    multidilation_kwargs=dict(comb_mode='cat_in', dilation_num=4))
CALIB_HW = 96            # the bottleneck plane must exceed the largest dilation (8): 96 / 8 = 12


def small_config(ngf=16, n_blocks=2, add_out_act='sigmoid', dilation_num=4):
    """A small generator of the same layout: bottleneck ngf * 8 channels, ngf * 8 / dilation_num per dilation group."""
    return dict(input_nc=4, output_nc=3, ngf=ngf, n_downsampling=3, n_blocks=n_blocks, conv_kind='default', add_out_act=add_out_act,
                multidilation_kwargs=dict(comb_mode='cat_in', dilation_num=dilation_num))


def _groups(cfg):
    return cfg['multidilation_kwargs']['dilation_num']


def layout(cfg):
    """(key prefix, kind, shape) of every parametrised layer of generator.model, in order; kind conv / convT / bn."""
    ngf, nd, nb, mf = cfg.get('ngf', 64), cfg.get('n_downsampling', 3), cfg.get('n_blocks', 3), cfg.get('max_features', 1024)
    G = _groups(cfg)
    out = [('model.1', 'conv', (ngf, cfg['input_nc'], 7, 7)), ('model.2', 'bn', (ngf,))]
    i = 4
    for d in range(nd):
        cin, cout = min(mf, ngf * 2 ** d), min(mf, ngf * 2 ** (d + 1))
        out += [(f'model.{i}', 'conv', (cout, cin, 3, 3)), (f'model.{i + 1}', 'bn', (cout,))]
        i += 3
    dim = min(mf, ngf * 2 ** nd)
    for b in range(nb):
        p = f'model.{i}.conv_block'
        for c, n in ((0, 1), (3, 4)):
            out += [(f'{p}.{c}.convs.{j}', 'conv', (dim, dim // G, 3, 3)) for j in range(G)]
            out += [(f'{p}.{n}', 'bn', (dim,))]
        i += 1
    for u in range(nd):
        mult = 2 ** (nd - u)
        cin, cout = min(mf, ngf * mult), min(mf, int(ngf * mult / 2))
        out += [(f'model.{i}', 'convT', (cin, cout, 3, 3)), (f'model.{i + 1}', 'bn', (cout,))]
        i += 3
    out += [(f'model.{i + 1}', 'conv', (cfg['output_nc'], ngf, 7, 7))]
    return out


def state_dict_keys(cfg):
    keys = {}
    for k, kind, shp in layout(cfg):
        if kind == 'bn':
            for s in ('weight', 'bias', 'running_mean', 'running_var'):
                keys[f'{k}.{s}'] = shp
            keys[f'{k}.num_batches_tracked'] = ()
        else:
            keys[f'{k}.weight'] = shp
            keys[f'{k}.bias'] = (shp[1] if kind == 'convT' else shp[0],)
    return keys


def make_state_dict(cfg, seed=0, calib_hw=CALIB_HW):
    """Seeded weights (conv biases included) with every BatchNorm's running statistics set to the batch statistics of its input on a seeded
    calibration batch (as tests/regular_util.make_state_dict); a group conv is scaled by its share of the summed fan-in."""
    g = torch.Generator().manual_seed(seed)
    G = _groups(cfg)
    sd = {}
    for k, kind, shp in layout(cfg):
        if kind == 'bn':
            sd[k + '.weight'] = 0.6 + 0.6 * torch.rand(shp, generator=g)
            sd[k + '.bias'] = 0.1 * torch.randn(shp, generator=g)
            sd[k + '.running_mean'] = torch.zeros(shp)
            sd[k + '.running_var'] = torch.ones(shp)
            sd[k + '.num_batches_tracked'] = torch.tensor(0)
        else:
            fan_in = shp[1] * shp[2] * shp[3] if kind == 'conv' else shp[0] * shp[2] * shp[3] / 4
            if '.convs.' in k:
                fan_in *= G
            sd[k + '.weight'] = torch.randn(shp, generator=g) * (1.0 / fan_in) ** 0.5
            sd[k + '.bias'] = 0.05 * torch.randn((shp[1] if kind == 'convT' else shp[0],), generator=g)
    forward(sd, cfg, calib_input(2, calib_hw, calib_hw, seed + 1), calibrate=True)
    for b in range(cfg.get('n_blocks', 3)):            # the second BN of a block: a smaller residual step
        k = f"model.{4 + 3 * cfg.get('n_downsampling', 3) + b}.conv_block.4.weight"
        sd[k] = sd[k] * 0.4
    return sd


def mdconv(sd, prefix, x, G):
    """MultidilatedConv(comb_mode='cat_in').forward: chunk j of the channels through conv j (dilation = reflect padding = 2^j), summed in the
    reference's order (Python's sum: 0 + out_0 + out_1 + ...)."""
    outs = []
    for j, xj in enumerate(x.chunk(G, dim=1)):
        d = 2 ** j
        outs.append(F.conv2d(F.pad(xj, (d,) * 4, mode='reflect'), sd[f'{prefix}.convs.{j}.weight'], sd[f'{prefix}.convs.{j}.bias'], dilation=d))
    return sum(outs)


@torch.no_grad()
def forward(sd, cfg, x, calibrate=False, taps=None):
    """fp32 torch restatement of MultiDilatedGlobalGenerator.forward from the state dict (keys without the 'generator.' prefix)."""
    nd, nb, G = cfg.get('n_downsampling', 3), cfg.get('n_blocks', 3), _groups(cfg)

    def bn(y, k):
        if calibrate:
            sd[k + '.running_mean'] = y.mean((0, 2, 3))
            sd[k + '.running_var'] = y.var((0, 2, 3), unbiased=False)
        return F.batch_norm(y, sd[k + '.running_mean'], sd[k + '.running_var'], sd[k + '.weight'], sd[k + '.bias'], False, 0.0, 1e-5)

    def conv(y, k, stride=1, pad=0, reflect=False):
        if reflect:
            y = F.pad(y, (pad,) * 4, mode='reflect')
            pad = 0
        return F.conv2d(y, sd[k + '.weight'], sd[k + '.bias'], stride, pad)

    x = F.relu(bn(conv(x, 'model.1', pad=3, reflect=True), 'model.2'))
    i = 4
    for _ in range(nd):
        x = F.relu(bn(conv(x, f'model.{i}', 2, 1), f'model.{i + 1}'))
        i += 3
    if taps is not None:
        taps['down'] = x.clone()
    for b in range(nb):
        p = f'model.{i}.conv_block'
        t = F.relu(bn(mdconv(sd, p + '.0', x, G), p + '.1'))
        x = x + bn(mdconv(sd, p + '.3', t, G), p + '.4')
        if taps is not None:
            taps[f'block{b}'] = x.clone()
        i += 1
    for _ in range(nd):
        x = F.conv_transpose2d(x, sd[f'model.{i}.weight'], sd[f'model.{i}.bias'], 2, 1, 1)
        x = F.relu(bn(x, f'model.{i + 1}'))
        i += 3
    x = conv(x, f'model.{i + 1}', pad=3, reflect=True)
    act = cfg.get('add_out_act', True)
    if act:
        x = torch.tanh(x) if act in (True, 'tanh') else torch.sigmoid(x)
    return x


def _bn(t, sd, k):
    return F.batch_norm(t, sd[k + '.running_mean'], sd[k + '.running_var'], sd[k + '.weight'], sd[k + '.bias'], False, 0.0, 1e-5)


def block_forward(sd_block, x, G=4):
    """One MultidilatedResnetBlock (keys conv_block.*) in fp32 torch."""
    with torch.no_grad():
        t = F.relu(_bn(mdconv(sd_block, 'conv_block.0', x, G), sd_block, 'conv_block.1'))
        return x + _bn(mdconv(sd_block, 'conv_block.3', t, G), sd_block, 'conv_block.4')


def block_state_dict(dim=512, seed=3, G=4):
    """Seeded weights of one MultidilatedResnetBlock(dim) (keys conv_block.*), BN statistics calibrated on ``block_input``."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k in ('conv_block.0', 'conv_block.3'):
        for j in range(G):
            sd[f'{k}.convs.{j}.weight'] = torch.randn(dim, dim // G, 3, 3, generator=g) * (1.0 / (9 * dim)) ** 0.5
            sd[f'{k}.convs.{j}.bias'] = 0.05 * torch.randn(dim, generator=g)
    for k in ('conv_block.1', 'conv_block.4'):
        sd[k + '.weight'] = 0.6 + 0.6 * torch.rand(dim, generator=g)
        sd[k + '.bias'] = 0.1 * torch.randn(dim, generator=g)
        sd[k + '.running_mean'] = torch.zeros(dim)
        sd[k + '.running_var'] = torch.ones(dim)
        sd[k + '.num_batches_tracked'] = torch.tensor(0)
    x = block_input(1, dim, 32, seed + 1)
    with torch.no_grad():
        t = mdconv(sd, 'conv_block.0', x, G)
        sd['conv_block.1.running_mean'], sd['conv_block.1.running_var'] = t.mean((0, 2, 3)), t.var((0, 2, 3), unbiased=False)
        t = mdconv(sd, 'conv_block.3', F.relu(_bn(t, sd, 'conv_block.1')), G)
        sd['conv_block.4.running_mean'], sd['conv_block.4.running_var'] = t.mean((0, 2, 3)), t.var((0, 2, 3), unbiased=False)
    return sd


def mdconv_ref(x, ws, bias, resid=None, relu=False, min_dilation=1):
    """The kernel's function in fp32 torch from a list of group weights: per group F.pad(reflect, d) + F.conv2d(dilation=d), summed."""
    y = 0
    for j, xj in enumerate(x.chunk(len(ws), dim=1)):
        d = min_dilation * 2 ** j
        y = y + F.conv2d(F.pad(xj, (d,) * 4, mode='reflect'), ws[j], dilation=d)
    y = y + bias.view(1, -1, 1, 1)
    if relu:
        y = y.relu()
    return y if resid is None else y + resid
