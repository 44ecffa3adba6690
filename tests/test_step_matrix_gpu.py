"""The table of the predict step's options (tests/step_matrix_util.py) on the MI355X, on the production library: every served cell for the FFC
model in all four modes; for the two pix2pixhd models the modes 'host' and 'graph' with no encoder and with ``jpeg``; every refused cell at the
step; and the two CLI runs of ``crop_to_mask`` [+ ``crop_max_side``] with ``device_jpeg`` through ``predict.main``, the overflow fallback
included.  The cells other GPU suites run already are run again: the point is that the table is complete.  One model per generator per
module, one or two steps per cell on images under 128 pixels a side, and every comparison is equality."""
import pytest

from tests import crop_shrink_util as CS
from tests import crop_util as CU
from tests import step_matrix_util as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx(tmp_path_factory):
    from lama_amd import _lib as L
    L.get_lib()                 # raises if liblama_hip.so was not built: no fallback
    return M.Context(tmp_path_factory.mktemp('step_matrix'), 'cuda')


def _runs_here(form, encoder, mode, generator):
    return generator == 'ffc_resnet' or (mode in ('host', 'graph') and encoder in ('none', 'jpeg'))


GPU_CELLS = [cell for cell, (status, _) in M.TABLE.items() if status == M.SERVED and _runs_here(*cell)]


def test_the_list_is_every_served_cell_of_the_table():
    """(six forms with three encoders and the fp32 input form, which takes none)"""
    assert len(GPU_CELLS) == (6 * 3 + 1) * 4 + 2 * (6 * 2 + 1) * 2
    left = [c for c, (s, _) in M.TABLE.items() if s == M.SERVED and c not in GPU_CELLS]
    assert all(c[3] != 'ffc_resnet' and (c[2] in ('replay', 'streams') or c[1] == 'png') for c in left)      # what is left out, as decided


@pytest.mark.parametrize('form,encoder,mode,generator', GPU_CELLS, ids=lambda v: v)
def test_served_cell(ctx, form, encoder, mode, generator):
    M.check_cell(ctx, form, encoder, mode, generator)


@pytest.mark.parametrize('cell', [c for c in M.pairs_of(M.REFUSED) if M.step_kwargs(*c) is not None], ids=lambda fe: f'{fe[0]}-{fe[1]}')
def test_the_step_refuses_the_cell_for_every_generator_and_mode(ctx, cell):
    for gen in M.GENERATORS:
        M.check_step_refuses(ctx.model(gen), *cell, 'cuda')


@pytest.mark.parametrize('form', ['crop', 'crop+shrink'])
def test_cli_crop_with_device_jpeg_and_its_overflow_fallback(ctx, form, tmp_path, monkeypatch):
    """lama_amd.predict's main on a synthetic checkpoint directory: the PNG run, then out_ext=.jpg device_jpeg=true -- the same names, every file
    byte for byte jpeg_from_scan(scan_ref(the definition)) -- then with scan slots as long as the shortest scan: the other images take the
    fallback's second crop step and the host's encoder, and decode to the source size as close to the definition as the device's file."""
    from lama_amd import predict as P
    gen = 'ffc_resnet'
    model, inp = ctx.model(gen), ctx.inputs(gen)
    mdir = M.model_dir(ctx.built(gen), tmp_path)
    if form == 'crop':
        items, indir = inp.crop, inp.crop_dir
        want = ctx.want((gen, 'cli', form), lambda: CU.cropped_want(model, items, inp.rects, 2, 'cuda', 'host'))
    else:
        items, indir = inp.shrink, inp.shrink_dir
        want = ctx.want((gen, 'cli', form), lambda: CS.definition_want(model, items, inp.wins, 'cuda', 2))
    outs = {tag: str(tmp_path / tag) for tag in ('png', 'on', 'small')}
    base = [f'model.path={mdir}', f'indir={indir}', 'batch_size=2'] + M.cli_keys(form, 'none')
    assert P.main(base + [f"outdir={outs['png']}"]) == 0
    CU.check_written_pngs(outs['png'], indir, items, want)
    names = M.files_of(outs['png'])
    jpeg = ['out_ext=.jpg', 'device_jpeg=true']
    assert P.main(base + jpeg + [f"outdir={outs['on']}"]) == 0
    made = M.check_crop_jpeg_files(outs['on'], names, want)
    assert all(made.values()), made
    stride, lens = M.overflow_stride(want)
    monkeypatch.setattr(P, 'JPEG_OUT_STRIDE', stride)
    assert P.main(base + jpeg + [f"outdir={outs['small']}"]) == 0
    made = M.check_crop_jpeg_files(outs['small'], names, want)
    assert list(made.values()) == [n <= stride for n in lens], (made, lens, stride)
    assert any(made.values()) and not all(made.values())                         # at least one file of each kind
