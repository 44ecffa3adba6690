"""The table of the predict step's options, shared by tests/test_step_matrix_emu.py, tests/test_step_matrix_gpu.py and
tests/test_step_matrix_gloo.py: every pairing of input / output FORM, device ENCODER, HostFedStep MODE and GENERATOR family is one cell of
``TABLE``, either served or refused, and a new option of lama_amd.predict gets its row (a form) or its column (an encoder) HERE.

A served cell is checked by composing the helpers the options' own suites use -- nothing is restated and no tolerance is added:

    form                       the expected u8 result (the form's existing definition)                       compared as
    plain, predicted_image     the module's forward on ``load_item``'s fp32 tensors + lama_quantize_u8_hwc    array_equal
                               (what the step with every option off is held to: tests/test_host_emu.py)
    scale_factor               the same on the host-scaled tensors (tests/test_scale_device_*.py)            array_equal
    scale_factor+paste_back    paste_back_util.pasted_want                                                    array_equal
    crop                       crop_util.cropped_want (the u8 step on the host-cropped arrays, pasted)        array_equal
    crop+shrink                crop_shrink_util.definition_want (the numpy restatement)                       array_equal

With ``png`` every stream, wrapped by ``png_from_zlib``, decodes to exactly that result cropped by ``crop_sizes``; with ``jpeg`` every scan is
byte for byte ``jpeg_ref.scan_ref`` of it; an empty slot yields an empty stream and (0, 0); ``result()`` raises.  In mode 'graph' the same step
object runs a second time with other images in the same slots (the second launch replays the captured graph).

A refused cell names its rule.  ``HostFedStep`` must raise for it, and the same combination spelled as CLI keys must stop
``parse_overrides`` / ``main`` before anything is loaded or written: the layers agree, the step being the authority."""
import io
import os

import numpy as np
import torch

from lama_amd import _lib as L
from lama_amd import predict as P
from tests import crop_shrink_util as CS
from tests import crop_util as CU
from tests import jpeg_ref
from tests import paste_back_util as PB

# ---- the axes -------------------------------------------------------------------------------------------------------------------------------
SERVED_FORMS = ('plain', 'predicted_image', 'scale_factor', 'scale_factor+paste_back', 'crop', 'crop+shrink')
# forms no layer serves (each word is one option; 'fp32' = HostFedStep(u8_input=False), which has no CLI key; 'refine' = the CLI's refine=true,
# which never reaches the step: a refiner run is served by predict_refine, so its cell without an encoder is 'refiner', not 'served')
OTHER_FORMS = ('fp32', 'paste_back', 'scale_factor+paste_back+predicted_image', 'crop+scale_factor', 'crop+predicted_image',
               'crop+shrink+scale_factor', 'crop+shrink+predicted_image', 'shrink',
               'refine', 'refine+scale_factor+paste_back', 'refine+crop', 'refine+crop+shrink')
FORMS = SERVED_FORMS + OTHER_FORMS
ENCODERS = ('none', 'png', 'jpeg', 'png+jpeg')
MODES = ('host', 'replay', 'streams', 'graph')
GENERATORS = ('ffc_resnet', 'pix2pixhd_global', 'pix2pixhd_multidilated')

SERVED, REFUSED, REFINER = 'served', 'refused', 'refiner'
FACTOR = PB.FACTOR
CROP_KEYS = ['crop_to_mask=true', f'crop_margin={CU.MARGIN}', f'crop_step={CU.STEP}', f'dataset.pad_out_to_modulo={CU.PAD_MOD}']


def rule_of(form: str, encoder: str):
    """The rule of lama_amd/predict.py that refuses (form, encoder), or None where the pair is served.  No rule depends on the mode or on the
    generator: every mode serves every form, and the three generator families share the step (ffc._PlanGenerator)."""
    opts = set(form.split('+'))
    if encoder == 'png+jpeg':
        return 'a step ends with ONE encoder: encode_jpeg and encode_png exclude each other (CLI: device_jpeg=true with device_png=true)'
    if 'shrink' in opts and 'crop' not in opts:
        return 'crop_shrink is a variant of the crop form: crop=True is needed (CLI: crop_max_side needs crop_to_mask=true)'
    if 'crop' in opts and 'refine' in opts:
        return 'crop_to_mask=true with refine=true is not served: refinement works on the whole image (a CLI rule: the step has no refine)'
    if 'crop' in opts and 'scale_factor' in opts:
        return 'crop with scale_factor is not served: the window is inpainted at the source resolution'
    if 'crop' in opts and 'predicted_image' in opts:
        return "crop with out_key 'predicted_image': the pasted result is made from 'inpainted'"
    if 'paste_back' in opts and 'scale_factor' not in opts:
        return 'paste_back needs scale_factor: without one the result has the source size already'
    if 'paste_back' in opts and 'refine' in opts:
        return 'paste_back=true with refine=true is not served: refinement writes its own result at the scaled size (a CLI rule)'
    if 'paste_back' in opts and 'predicted_image' in opts:
        return "paste_back with out_key 'predicted_image': the pasted result is made from 'inpainted'"
    if 'fp32' in opts and encoder != 'none':
        return "an encoder needs a u8 input form (its crops are the step's device sizes array): not with u8_input=False"
    if 'refine' in opts and encoder != 'none':
        return 'device_png / device_jpeg with refine=true is not served: refinement writes from host tensors (a CLI rule)'
    return None


def _status(form, encoder):
    rule = rule_of(form, encoder)
    if rule is not None:
        return REFUSED, rule
    return (REFINER if 'refine' in form.split('+') else SERVED), None


# THE TABLE: (form, encoder, mode, generator) -> (status, the refusing rule or None)
TABLE = {(f, e, m, g): _status(f, e) for f in FORMS for e in ENCODERS for m in MODES for g in GENERATORS}


def pairs_of(status):
    """The (form, encoder) pairs of the table with that status (no rule depends on mode or generator: asserted by the suites)."""
    return sorted({(f, e) for (f, e, _, _), (s, _) in TABLE.items() if s == status}, key=lambda fe: (FORMS.index(fe[0]), ENCODERS.index(fe[1])))


def jpeg_params(form):
    """One jpeg row runs 4:4:4 at quality 50 (as the encoder's own suite has it: 'predicted_image'); the others the defaults."""
    return (50, '444') if form == 'predicted_image' else (95, '420')


# ---- the spellings of a cell at each layer -----------------------------------------------------------------------------------------------------
def step_kwargs(form, encoder, src_hw=(40, 56)):
    """HostFedStep's keywords of (form, encoder), or None where the form has no spelling there ('refine')."""
    opts = form.split('+')
    if 'refine' in opts:
        return None
    kw = {}
    if 'predicted_image' in opts:
        kw['out_key'] = 'predicted_image'
    if 'scale_factor' in opts:
        kw.update(scale_factor=FACTOR, src_hw=src_hw)
    if 'paste_back' in opts:
        kw['paste_back'] = True
    if 'crop' in opts:
        kw.update(crop=True, src_hw=src_hw)
    if 'shrink' in opts:
        kw['crop_shrink'] = True
    if 'fp32' in opts:
        kw['u8_input'] = False
    q, ss = jpeg_params(form)
    if 'png' in encoder:
        kw['encode_png'] = True
    if 'jpeg' in encoder:
        kw.update(encode_jpeg=True, jpeg_quality=q, jpeg_subsampling=ss)
    return kw


def cli_keys(form, encoder, max_side=CS.MAX_SIDE):
    """The same cell as CLI keys, or None where it has no spelling there ('fp32')."""
    opts = form.split('+')
    if 'fp32' in opts:
        return None
    keys = []
    if 'refine' in opts:
        keys.append('refine=true')
    if 'predicted_image' in opts:
        keys.append('out_key=predicted_image')
    if 'scale_factor' in opts:
        keys.append(f'dataset.scale_factor={FACTOR}')
    if 'paste_back' in opts:
        keys.append('paste_back=true')
    if 'crop' in opts:
        keys += CROP_KEYS
    if 'shrink' in opts:
        keys.append(f'crop_max_side={max_side}')
    q, ss = jpeg_params(form)
    if 'png' in encoder:
        keys.append('device_png=true')
    if 'jpeg' in encoder:
        keys += ['device_jpeg=true', f'jpeg_quality={q}', f'jpeg_subsampling={ss}']
    if encoder == 'jpeg':
        keys.append('out_ext=.jpg')
    return keys


def predict_kwargs(form, encoder, max_side=CS.MAX_SIDE):
    """... and as keywords of ``predict()``, or None ('fp32', 'refine': not options of the loop)."""
    opts = form.split('+')
    if 'fp32' in opts or 'refine' in opts:
        return None
    kw = dict(pad_mod=CU.PAD_MOD)
    if 'predicted_image' in opts:
        kw['out_key'] = 'predicted_image'
    if 'scale_factor' in opts:
        kw['scale_factor'] = FACTOR
    if 'paste_back' in opts:
        kw['paste_back'] = True
    if 'crop' in opts:
        kw.update(crop_to_mask=True, crop_margin=CU.MARGIN, crop_step=CU.STEP)
    if 'shrink' in opts:
        kw['crop_max_side'] = max_side
    q, ss = jpeg_params(form)
    if 'png' in encoder:
        kw['device_png'] = True
    if 'jpeg' in encoder:
        kw.update(device_jpeg=True, jpeg_quality=q, jpeg_subsampling=ss)
    if encoder == 'jpeg':
        kw['out_ext'] = '.jpg'
    return kw


# ---- the refused cells ------------------------------------------------------------------------------------------------------------------------
def check_step_refuses(model, form, encoder, device, modes=MODES):
    """Constructing the step raises LamaError, in every mode, whatever the bucket."""
    kw = step_kwargs(form, encoder)
    for mode in modes:
        try:
            P.HostFedStep(model, 2, 16, 16, device, mode=mode, **kw)
        except (L.LamaError, NotImplementedError):
            continue
        raise AssertionError(f'HostFedStep served the refused cell {form} x {encoder} in mode {mode}')


def check_cli_refuses(monkeypatch, tmp_path, form, encoder):
    """``main`` stops before anything is loaded or written: no checkpoint is opened and the output directory does not exist afterwards."""
    def no_launch(*a, **k):
        raise AssertionError('the refusal came after the model was loaded')
    monkeypatch.setattr(P.trainers, 'load_checkpoint', no_launch)
    monkeypatch.setattr(P.lcfg, 'load_train_config', no_launch)
    out = str(tmp_path / 'out')
    argv = [f'model.path={tmp_path / "model"}', f'indir={tmp_path / "in"}', f'outdir={out}'] + cli_keys(form, encoder)
    for run in (P.parse_overrides, P.main):
        try:
            run(argv)
        except (SystemExit, L.LamaError, NotImplementedError) as e:
            assert not isinstance(e, SystemExit) or e.code not in (0, None), (form, encoder)
        else:
            raise AssertionError(f'{run.__name__} accepted the refused cell {form} x {encoder}')
        assert not os.path.exists(out)


def check_cli_accepts(form, encoder):
    """``parse_overrides`` takes the served cell's keys and reports them back."""
    cfg = P.parse_overrides(['model.path=/m', 'indir=i', 'outdir=o'] + cli_keys(form, encoder))
    opts = form.split('+')
    assert cfg['crop_to_mask'] == ('crop' in opts) and cfg['paste_back'] == ('paste_back' in opts) and bool(cfg['crop_max_side']) == ('shrink' in opts)
    assert (cfg.get('dataset.scale_factor') is not None) == ('scale_factor' in opts) and (cfg['out_key'] == 'predicted_image') == ('predicted_image' in opts)
    assert cfg['device_png'] == (encoder == 'png') and cfg['device_jpeg'] == (encoder == 'jpeg') and bool(cfg.get('refine', False)) == ('refine' in opts)
    if encoder == 'jpeg':
        assert (cfg['jpeg_quality'], cfg['jpeg_subsampling']) == jpeg_params(form)


def check_predict_refuses(model, items, indir, tmp_path, form, encoder, device='cpu'):
    """The loop raises LamaError before it writes anything: the output directory does not exist afterwards."""
    out = str(tmp_path / 'out')
    try:
        P.predict(model, items, indir, out, batch_size=2, device=device, io_threads=2, **predict_kwargs(form, encoder))
    except L.LamaError:
        pass
    else:
        raise AssertionError(f'predict() served the refused cell {form} x {encoder}')
    assert not os.path.exists(out)


# ---- models and inputs ------------------------------------------------------------------------------------------------------------------------
def build_model(generator, device):
    """The small synthetic model of a generator family, as the existing helpers build it -> (model, state dict, train config).  'cpu': the host
    SIMT emulator behind the same C ABI (the smallest sizes); 'cuda': the production library, as the CLI sets the model up."""
    from lama_amd import ffc as F
    from lama_amd import trainers
    on_gpu = torch.device(device).type == 'cuda'
    if generator == 'ffc_resnet':
        if not on_gpu:
            from tests.test_dist_gloo import _build_model
            model, sd, cfg = _build_model()
            return model, sd, dict(generator=dict(kind='ffc_resnet', **cfg))
        from tests.test_paste_back_gpu import _small_model
        return _small_model()
    if generator == 'pix2pixhd_global':
        from tests import regular_util as G
    else:
        from tests import multidilated_util as G
    cfg = G.small_config(ngf=16, n_blocks=2) if on_gpu else G.small_config(ngf=8, n_blocks=1)
    sd = {'generator.' + k: v for k, v in G.make_state_dict(cfg, seed=3).items()}
    train_config = dict(generator=dict(kind=generator, **cfg))
    model = trainers.DefaultInpaintingTrainingModule(train_config)
    model.load_state_dict(sd, strict=True)
    model.freeze()
    if on_gpu:
        model.cuda()
        model.generator.use_graph = True
    else:
        from tests.emu import emu_lib
        model.generator.set_exec(F._Exec(emu_lib()))
    return model, sd, train_config


# The dilated generator needs a bottleneck plane larger than its largest dilation (8): a padded input, or padded crop window, of at least 72 a
# side.  Its own pairs, in the manner of crop_util.PAIRS: (h, w), the mask's box (y, x, height, width) -> an 80 x 80 window each (box + 8 is
# 68 x 72, rounded up to the step 16), centred / clamped to the bottom and right edges / clamped to the top-left corner
DILATED_PAIRS = [((96, 104), (20, 24, 60, 64)), ((90, 100), (28, 34, 60, 64)), ((88, 101), (0, 0, 58, 66))]
DILATED_WINDOWS = [(10, 16, 80, 80, 80, 80), (10, 20, 80, 80, 80, 80), (0, 0, 80, 80, 80, 80)]
DILATED_MAX_SIDE = 80       # crop+shrink: the windows fit at k = 1 and run through the shrink kernels (a k >= 2 window of 72 generator pixels
#                             would need a source image of 144 pixels a side: above what a cell of this table runs)
PLAIN_SHAPES = {'cpu': [(13, 16), (16, 11), (16, 16)], 'cuda': [(95, 119), (96, 120), (94, 120)]}       # one bucket: 16 x 16 / 96 x 120
SCALED_SHAPES = {'cpu': PB.SHAPES, 'cuda': PB.SHAPES_GPU}
DILATED_PLAIN_CPU = [(70, 72)]                                                                          # the 72 x 72 bucket


class Inputs:
    """The PNG pairs of one generator family on one device class, written once under ``root``."""

    def __init__(self, root, generator, device):
        kind = torch.device(device).type
        dilated = generator == 'pix2pixhd_multidilated'
        few = dilated and kind == 'cpu'                          # the emulator runs the dilated model on one image and one empty slot
        d = lambda name: os.path.join(str(root), name) + os.sep
        plain = DILATED_PLAIN_CPU if few else PLAIN_SHAPES[kind]
        self.plain = PB.write_pairs(d('plain'), plain, seed=9)
        self.plain_bucket = (max(P.ceil_modulo(h, 8) for h, _ in plain), max(P.ceil_modulo(w, 8) for _, w in plain))
        assert all((P.ceil_modulo(h, 8), P.ceil_modulo(w, 8)) == self.plain_bucket for h, w in plain)
        self.scaled_shapes = SCALED_SHAPES['cuda' if dilated else kind]
        self.scaled = PB.write_pairs(d('scaled'), self.scaled_shapes)
        self.scaled_bucket, self.scaled_src = PB.geometry(self.scaled_shapes)
        self.crop_dir, self.shrink_dir = d('crop'), d('shrink')
        if dilated:
            self.crop_pairs = self.shrink_pairs = DILATED_PAIRS[:1] if few else DILATED_PAIRS
            windows = DILATED_WINDOWS[:len(self.crop_pairs)]
            self.max_side = DILATED_MAX_SIDE
            self.crop = CU.write_pairs(self.crop_dir, pairs=self.crop_pairs)
            self.shrink = CU.write_pairs(self.shrink_dir, pairs=self.crop_pairs)
            self.rects = CU.item_rects(self.crop, windows)                      # asserts that the windows are the ones intended
            self.wins = CS.item_windows(self.shrink, [(y0, x0, ch, cw, 1, ch, cw, Hp, Wp) for y0, x0, ch, cw, Hp, Wp in windows], self.max_side)
        else:
            self.crop_pairs, self.shrink_pairs, self.max_side = CU.PAIRS, CS.PAIRS, CS.MAX_SIDE
            self.crop, self.shrink = CU.write_pairs(self.crop_dir), CS.write_pairs(self.shrink_dir)
            self.rects, self.wins = CU.item_rects(self.crop), CS.item_windows(self.shrink)
        self.crop_n = len(self.crop_pairs) if not dilated else len(self.crop_pairs) + 1           # one empty slot per batch in every bucket


class Context:
    """What a module's cells share: one model per generator, one set of inputs per family, and every definition computed once."""

    def __init__(self, root, device):
        self.root, self.device = root, device
        self.ref_mode = 'host' if torch.device(device).type == 'cuda' else 'replay'       # the mode the definitions' own steps run in
        self._models, self._inputs, self._wants = {}, {}, {}

    def built(self, generator):
        if generator not in self._models:
            self._models[generator] = build_model(generator, self.device)
        return self._models[generator]

    def model(self, generator):
        return self.built(generator)[0]

    def inputs(self, generator):
        family = 'dilated' if generator == 'pix2pixhd_multidilated' else 'small'
        if family not in self._inputs:
            self._inputs[family] = Inputs(os.path.join(str(self.root), family), generator, self.device)
        return self._inputs[family]

    def want(self, key, make):
        if key not in self._wants:
            self._wants[key] = make()
        return self._wants[key]


# ---- the definitions of the forms without a crop ----------------------------------------------------------------------------------------------
def forward_want(model, items, n, device, out_key='inpainted', factor=None):
    """The u8 results [len(items)] of the module's forward on ``load_item``'s (host-scaled,) padded fp32 tensors, the rest of the batch of ``n``
    all-zero slots, quantised by lama_quantize_u8_hwc and cropped to each image's (scaled) size: bin/predict.py:82-92 as the fp32 form of the
    step runs it, what ``forward_u8`` and the ``scale_factor`` step are defined as bit for bit."""
    host = [P.load_item(m, i, 8, factor) for m, i in items]
    image = np.zeros((n,) + host[0][0].shape, np.float32)
    mask = np.zeros((n,) + host[0][1].shape, np.float32)
    for j, it in enumerate(host):
        image[j], mask[j] = it[0], it[1]
    Hp, Wp = image.shape[2:]
    lib = model.generator._exec.lib
    keep = model.keep_predicted_image
    model.keep_predicted_image = False
    try:
        with torch.no_grad():
            mk = torch.from_numpy(mask).to(device)
            out = model(dict(image=torch.from_numpy(image).to(device), mask=(mk > 0) * 1))[out_key]
            u8 = torch.zeros(n, Hp, Wp, 3, dtype=torch.uint8, device=device)
            lib.quantize_u8_hwc(L.view(out), u8, n, Hp, Wp, CU._stream(device))
            CU._sync(device)
    finally:
        model.keep_predicted_image = keep
    u8 = u8.cpu().numpy()
    return [u8[j, :it[2][0], :it[2][1]].copy() for j, it in enumerate(host)]


def check_results(hs, encoder, wants, quality, ss, what):
    """Result set 0 of ``hs`` against the definition ``wants`` (one [h,w,3] u8 image per filled slot; the other slots are empty)."""
    sizes = hs.crop_sizes(0)
    assert np.array_equal(sizes[:len(wants)], [w.shape[:2] for w in wants]) and not sizes[len(wants):].any(), what
    source_slots = tuple(hs.out_hw) != (hs.Hp, hs.Wp) or hs.paste_back
    if encoder == 'none':
        res = hs.result(0)
        assert tuple(res.shape) == (hs.n, *hs.out_hw, 3)
        for j, w in enumerate(wants):
            h, wd = w.shape[:2]
            assert np.array_equal(res[j, :h, :wd], w), (what, j, np.argwhere(res[j, :h, :wd] != w)[:4].tolist())
            if source_slots:                                  # zeros around each image and in the empty slots
                assert not res[j, h:].any() and not res[j, :, wd:].any(), (what, j)
        if source_slots:
            assert not res[len(wants):].any(), what
        return
    assert CU.result_raises(hs) and hs.h_u8 is None, what
    code = jpeg_ref.J444 if str(ss) == '444' else jpeg_ref.J420
    for j in range(hs.n):
        data = bytes(hs.result_png(0, j) if encoder == 'png' else hs.result_jpeg(0, j))
        if j >= len(wants):
            assert data == b'' and tuple(sizes[j]) == (0, 0), (what, j)
            continue
        h, wd = wants[j].shape[:2]
        if encoder == 'png':
            from PIL import Image
            assert np.array_equal(np.array(Image.open(io.BytesIO(P.png_from_zlib(h, wd, 3, data)))), wants[j]), (what, j)
        else:
            assert data == jpeg_ref.scan_ref(wants[j], h, wd, quality, code), (what, j, len(data))


# ---- a served cell ----------------------------------------------------------------------------------------------------------------------------
def check_cell(ctx, form, encoder, mode, generator):
    """One served cell: the step of (form, encoder) in ``mode`` on the generator's small model against the form's definition.  In 'graph' the
    same step object runs again with other images in the same slots: the replay of the captured graph gives their bytes."""
    assert TABLE[(form, encoder, mode, generator)] == (SERVED, None)
    model, inp, dev = ctx.model(generator), ctx.inputs(generator), ctx.device
    q, ss = jpeg_params(form)
    again = mode == 'graph'
    enc = dict(encode_png=encoder == 'png', encode_jpeg=encoder == 'jpeg', jpeg_quality=q, jpeg_subsampling=ss)
    if form == 'crop':
        # a crop form with an encoder has source-sized result slots: check_step asserts out_hw == src_hw for every bucket
        for n in (inp.crop_n, 1) if again else (inp.crop_n,):                  # (batches of one: a bucket's images through slot 0, one by one)
            want = ctx.want((generator, form, n), lambda: CU.cropped_want(model, inp.crop, inp.rects, n, dev, ctx.ref_mode, inp.crop_pairs))
            CU.check_step(model, inp.crop, inp.rects, dev, mode, want, n, pairs=inp.crop_pairs, **enc)
        return
    if form == 'crop+shrink':
        for n in (inp.crop_n, 1) if again else (inp.crop_n,):
            want = ctx.want((generator, form, n), lambda: CS.definition_want(model, inp.shrink, inp.wins, dev, n, shrink_k1=True, pairs=inp.shrink_pairs))
            CS.check_step(model, inp.shrink, inp.wins, dev, mode, want, n, pairs=inp.shrink_pairs, **enc)
        return
    scaled = form.startswith('scale_factor')
    items, bucket, src_hw = (inp.scaled, inp.scaled_bucket, inp.scaled_src) if scaled else (inp.plain, inp.plain_bucket, None)
    n = len(items) + 1                                                         # one empty slot
    hs = P.HostFedStep(model, n, *bucket, dev, drain=True, mode=mode, **step_kwargs(form, encoder, src_hw))
    assert hs.mode == mode and hs.encode_png == (encoder == 'png') and hs.encode_jpeg == (encoder == 'jpeg')
    assert tuple(hs.out_hw) == (tuple(src_hw) if form.endswith('paste_back') else tuple(bucket))
    u8 = [P.load_item_u8(*it) for it in items]
    orders = [list(range(len(items)))]
    if again and len(items) > 1:
        orders.append(orders[0][1:] + orders[0][:1])                           # the same slots, other images (of other sizes)
    if form == 'fp32':      # the caller's own padded fp32 tensors (``load_item``'s): no sizes array, full slots down
        host = [P.load_item(m, i, 8) for m, i in items]
        for order in orders:
            wants = ctx.want((generator, 'plain', tuple(order)), lambda: forward_want(model, [items[i] for i in order], n, dev))
            CU.run_step(hs, [(host[i][0], host[i][1]) for i in order])
            res = hs.result(0)
            for j, w in enumerate(wants):
                assert np.array_equal(res[j, :w.shape[0], :w.shape[1]], w), (form, mode, generator, tuple(order), j)
        return
    for order in orders:
        rows = [items[i] for i in order]
        if form == 'scale_factor+paste_back':
            make = lambda: PB.pasted_want(model, rows, n, dev)
        else:
            make = lambda: forward_want(model, rows, n, dev, out_key='predicted_image' if form == 'predicted_image' else 'inpainted',
                                        factor=FACTOR if scaled else None)
        wants = ctx.want((generator, form, tuple(order)), make)
        CU.run_step(hs, [(u8[i][0], u8[i][1]) for i in order])
        check_results(hs, encoder, wants, q, ss, (form, encoder, mode, generator, tuple(order)))
    if mode == 'graph' and torch.device(dev).type == 'cuda':
        assert hs.graphs[0] is not None
    assert model.generator.check_range(dev) is True


def model_dir(built, root):
    """A synthetic checkpoint directory for ``predict.main`` (config.yaml + models/best.ckpt), as tests/test_jpeg_gpu.py builds one."""
    import yaml
    _, sd, train_config = built
    mdir = os.path.join(str(root), 'model')
    os.makedirs(os.path.join(mdir, 'models'))
    with open(os.path.join(mdir, 'config.yaml'), 'w') as f:
        yaml.safe_dump(train_config, f)
    torch.save(dict(state_dict=sd), os.path.join(mdir, 'models', 'best.ckpt'))
    return mdir


# ---- the loop: crop_to_mask [+ crop_max_side] with device_jpeg, and its overflow fallback --------------------------------------------------------
def files_of(d):
    return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)


def check_crop_jpeg_files(out, names, want, sizes_of=None, quality=95, ss='420'):
    """The files of a crop_to_mask + device_jpeg run: the PNG run's names; every device-encoded file byte for byte
    jpeg_from_scan(scan_ref(the definition)); every other one (the host fallback's) decodes to the source size with a PSNR against the definition
    within 1 dB of the device file's.  -> {name: made on the device?}"""
    from tests import jpeg_util as JU
    code = jpeg_ref.J444 if str(ss) == '444' else jpeg_ref.J420
    got = files_of(out)
    assert [os.path.splitext(nm)[0] for nm in got] == [os.path.splitext(nm)[0] for nm in names], (got, names)
    made = {}
    for nm, w in zip(got, want):
        h, wd = w.shape[:2]
        with open(os.path.join(out, nm), 'rb') as f:
            data = f.read()
        dev_file = P.jpeg_from_scan(h, wd, quality, code, jpeg_ref.scan_ref(w, h, wd, quality, code))
        made[nm] = data == dev_file
        if not made[nm]:
            dec = JU.decode_jpeg(data)
            assert dec.shape == w.shape, nm
            assert JU.psnr(dec, w) >= JU.psnr(JU.decode_jpeg(dev_file), w) - 1.0, nm
    return made


def overflow_stride(want, quality=95, ss='420'):
    """A scan slot size that some but not all of the images' scans exceed: the shortest scan's length, as tests/test_jpeg_gpu.py chooses it."""
    code = jpeg_ref.J444 if str(ss) == '444' else jpeg_ref.J420
    lens = [len(jpeg_ref.scan_ref(w, *w.shape[:2], quality, code)) for w in want]
    assert len(set(lens)) >= 2, lens
    return min(lens), lens
