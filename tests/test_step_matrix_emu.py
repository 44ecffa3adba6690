"""The table of the predict step's options (tests/step_matrix_util.py) on the host SIMT emulator: that the table is complete, every refused cell
at every layer, the agreement of the CLI with the step, the served cells no other emulator test runs (mode 'replay': the emulator's device
offers one), and ``crop_to_mask`` [+ ``crop_max_side``] with ``device_jpeg`` through the loop, its overflow fallback included.  Every check is
equality against a definition the repository already has; the cells the other emulator suites run (and every mode) are on the GPU's list
(tests/test_step_matrix_gpu.py)."""
import itertools
import os

import pytest

from lama_amd import predict as P
from tests import crop_shrink_util as CS
from tests import crop_util as CU
from tests import step_matrix_util as M


# ---- the table itself -------------------------------------------------------------------------------------------------------------------------
def test_table_covers_the_full_cross_product():
    cells = set(itertools.product(M.FORMS, M.ENCODERS, M.MODES, M.GENERATORS))
    assert set(M.TABLE) == cells and len(M.TABLE) == len(M.FORMS) * len(M.ENCODERS) * len(M.MODES) * len(M.GENERATORS)
    assert set(M.SERVED_FORMS) == {'plain', 'predicted_image', 'scale_factor', 'scale_factor+paste_back', 'crop', 'crop+shrink'}
    assert set(M.MODES) == {'host', 'replay', 'streams', 'graph'} and set(M.ENCODERS) >= {'none', 'png', 'jpeg'}
    assert set(M.GENERATORS) == {'ffc_resnet', 'pix2pixhd_global', 'pix2pixhd_multidilated'}
    for (form, enc, mode, gen), (status, rule) in M.TABLE.items():
        assert status in (M.SERVED, M.REFUSED, M.REFINER)
        assert (rule is not None and len(rule) > 20) == (status == M.REFUSED), (form, enc)        # every refused cell names its rule
        assert (status == M.SERVED) == (form in M.SERVED_FORMS + ('fp32',) and enc in ('none', 'png', 'jpeg') and (form != 'fp32' or enc == 'none'))
    # the issue's examples are refused cells
    for form, enc in (('crop+scale_factor', 'none'), ('crop+predicted_image', 'none'), ('scale_factor+paste_back+predicted_image', 'none'),
                      ('plain', 'png+jpeg'), ('fp32', 'png'), ('fp32', 'jpeg'), ('refine+crop', 'none'), ('refine', 'jpeg')):
        assert all(M.TABLE[(form, enc, m, g)][0] == M.REFUSED for m in M.MODES for g in M.GENERATORS)
    # one jpeg row is 4:4:4 at quality 50, the others the defaults
    assert [f for f in M.SERVED_FORMS if M.jpeg_params(f) == (50, '444')] == ['predicted_image']
    assert all(M.jpeg_params(f) == (P.DEFAULTS['jpeg_quality'], P.DEFAULTS['jpeg_subsampling']) for f in M.SERVED_FORMS if f != 'predicted_image')


# ---- refusals and the agreement of the layers -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ctx(tmp_path_factory):
    return M.Context(tmp_path_factory.mktemp('step_matrix'), 'cpu')


REFUSED = M.pairs_of(M.REFUSED)
ACCEPTED = M.pairs_of(M.SERVED) + M.pairs_of(M.REFINER)
_id = lambda fe: f'{fe[0]}-{fe[1]}'


@pytest.mark.parametrize('cell', [c for c in REFUSED if M.step_kwargs(*c) is not None], ids=_id)
def test_the_step_refuses_the_cell_for_every_generator_and_mode(ctx, cell):
    for gen in M.GENERATORS:
        M.check_step_refuses(ctx.model(gen), *cell, 'cpu')


@pytest.mark.parametrize('cell', [c for c in REFUSED if M.cli_keys(*c) is not None], ids=_id)
def test_the_cli_refuses_the_cell_before_anything_is_loaded_or_written(cell, monkeypatch, tmp_path):
    M.check_cli_refuses(monkeypatch, tmp_path, *cell)


@pytest.mark.parametrize('cell', [c for c in REFUSED if M.predict_kwargs(*c) is not None], ids=_id)
def test_the_loop_refuses_the_cell_before_anything_is_written(ctx, cell, tmp_path):
    inp = ctx.inputs('ffc_resnet')
    M.check_predict_refuses(ctx.model('ffc_resnet'), inp.crop, inp.crop_dir, tmp_path, *cell)


@pytest.mark.parametrize('cell', [c for c in ACCEPTED if M.cli_keys(*c) is not None], ids=_id)
def test_the_cli_accepts_what_the_step_serves(cell):
    M.check_cli_accepts(*cell)


def test_every_cell_has_a_spelling_at_some_layer_and_the_layers_cover_the_same_pairs():
    """The step is the authority: every (form, encoder) the step can spell is refused by the CLI exactly where the table says so (the two
    parametrised tests above run both directions); what only one layer can spell ('fp32': the step; 'refine': the CLI) is named here."""
    for form, enc in itertools.product(M.FORMS, M.ENCODERS):
        step, cli = M.step_kwargs(form, enc), M.cli_keys(form, enc)
        assert step is not None or cli is not None
        assert (step is None) == ('refine' in form.split('+')) and (cli is None) == ('fp32' in form.split('+'))
    assert set(REFUSED) | set(ACCEPTED) == set(itertools.product(M.FORMS, M.ENCODERS)) and not set(REFUSED) & set(ACCEPTED)


# ---- the served cells no other emulator test runs ---------------------------------------------------------------------------------------------
EMU_CELLS = ([('crop', 'jpeg', 'ffc_resnet'), ('crop+shrink', 'jpeg', 'ffc_resnet')] +
             [(form, enc, 'pix2pixhd_global') for form in ('plain', 'predicted_image', 'scale_factor+paste_back', 'crop') for enc in ('none', 'jpeg')] +
             [('plain', 'none', 'pix2pixhd_multidilated'), ('crop', 'none', 'pix2pixhd_multidilated')])


@pytest.mark.parametrize('form,encoder,generator', EMU_CELLS, ids=lambda v: v)
def test_served_cell(ctx, form, encoder, generator):
    M.check_cell(ctx, form, encoder, 'replay', generator)


# ---- the loop: crop_to_mask [+ crop_max_side] with device_jpeg ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def loop(ctx):
    """Per crop form: the items, the loop's keywords and the definition in the loop's batches -- of three, as the cells above run them, so that
    the definitions are computed once -- and the names the loop gives its files (bin/predict.py:69-72: the mask's path relative to indir; that
    the PNG run writes exactly these is held by tests/test_crop_emu.py and tests/test_crop_shrink_emu.py)."""
    gen = 'ffc_resnet'
    model, inp = ctx.model(gen), ctx.inputs(gen)
    base = dict(pad_mod=CU.PAD_MOD, batch_size=3, device='cpu', io_threads=2, crop_to_mask=True, crop_margin=CU.MARGIN, crop_step=CU.STEP)
    names = lambda items, indir: sorted(os.path.splitext(m[len(indir):])[0] + '.png' for m, _ in items)
    return {'crop': dict(model=model, items=inp.crop, indir=inp.crop_dir, kw=base, names=names(inp.crop, inp.crop_dir),
                         want=ctx.want((gen, 'crop', 3), lambda: CU.cropped_want(model, inp.crop, inp.rects, 3, 'cpu', 'replay'))),
            'crop+shrink': dict(model=model, items=inp.shrink, indir=inp.shrink_dir, kw=dict(base, crop_max_side=CS.MAX_SIDE),
                                names=names(inp.shrink, inp.shrink_dir),
                                want=ctx.want((gen, 'crop+shrink', 3), lambda: CS.definition_want(model, inp.shrink, inp.wins, 'cpu', 3, shrink_k1=True)))}


@pytest.mark.parametrize('form', ['crop', 'crop+shrink'])
def test_predict_loop_crop_with_device_jpeg_and_its_overflow_fallback(loop, form, tmp_path, monkeypatch):
    """predict(crop_to_mask=True[, crop_max_side=32], device_jpeg=True): the PNG run's names, every file byte for byte
    jpeg_from_scan(scan_ref(the definition)).  Then with scan slots as long as the shortest scan: that image keeps the device's bytes, the
    others overflow and go through the fallback's second step -- built with the bucket's ``crop=`` / ``crop_shrink=`` and fed the windows --
    and are written by the host at the source size, as close to the definition as the device's file."""
    c = loop[form]
    on, small = str(tmp_path / 'on'), str(tmp_path / 'small')
    kw = dict(c['kw'], out_ext='.jpg', device_jpeg=True)
    assert P.predict(c['model'], c['items'], c['indir'], on, **kw) == len(c['items'])
    made = M.check_crop_jpeg_files(on, c['names'], c['want'])
    assert all(made.values()), made
    stride, lens = M.overflow_stride(c['want'])
    monkeypatch.setattr(P, 'JPEG_OUT_STRIDE', stride)
    assert P.predict(c['model'], c['items'], c['indir'], small, **kw) == len(c['items'])
    made = M.check_crop_jpeg_files(small, c['names'], c['want'])
    assert list(made.values()) == [n <= stride for n in lens], (made, lens, stride)
    assert any(made.values()) and not all(made.values())                         # at least one file of each kind
