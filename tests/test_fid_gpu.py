"""GPU: FID.  The kernels of csrc/inception.hip through the product library (the check functions of tests/test_fid_emu.py), the whole
InceptionV3 of lama_amd.evaluation on the seeded synthetic network against the reference's fp64 activations (tests/golden/fid.npz), graph
replay, and the CLI with fid_weights=.

Bar of the network tests: 8 x `unit` on max |a - a64| / max |a64|, `unit` = the reference's own fp32-vs-fp64 distance over the recorded cases
(4.5e-4: eager fp32 through 94 BatchNorm-normalised layers on noise images).  Measured on MI355X: see the docstring of
test_network_against_fp64."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import inception_util as U  # noqa: E402
import test_fid_emu as E  # noqa: E402
from lama_amd import _lib as L  # noqa: E402
from lama_amd import evaluation as EV  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = E.GOLD
UNIT = E.UNIT
PREC_NAMES = {L.PREC_F16X3: 'f16x3', L.PREC_BF16X3: 'bf16x3'}


@pytest.fixture(scope='module')
def lib():
    return L.get_lib()


@pytest.fixture(scope='module')
def weights():
    return U.synthetic_state_dict(GOLD)


@pytest.fixture(scope='module')
def models(weights):
    """(resize_input, precision) -> InceptionV3 on the device; built once."""
    return {(r, p): EV.InceptionV3([3], resize_input=r, weights=weights).cuda().set_precision(p) for r in (True, False) for p in E.PRECS}


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('prec', E.PRECS)
@pytest.mark.parametrize('case', list(E.RECT_CASES))
def test_rect_conv(lib, case, prec):
    E.check_rect_conv(lib, case, prec)


@pytest.mark.parametrize('prec', E.PRECS)
@pytest.mark.parametrize('case', list(E.RECT_CASES))
def test_rect_conv_tap_count(lib, case, prec):
    E.check_rect_tap_count(lib, case, prec)


@pytest.mark.parametrize('prec', E.PRECS)
def test_rect_conv_channel_slice(lib, prec):
    E.check_rect_slice(lib, prec)


def test_rect_conv_refusals(lib):
    E.check_rect_refusals(lib)
    torch.cuda.synchronize()


def test_rect_conv_fills_the_chip_at_8x8_batch_16_and_is_reproducible(lib):
    """2048 -> 448 1x1 at 8 x 8, B = 16 (Mixed_7c's branch3x3dbl_1: 1024 pixels, the small-tile geometry) against fp64, twice: bit-identical."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(16, 2048, 8, 8, generator=g).cuda()
    w = (torch.randn(448, 2048, 1, 1, generator=g) / 2048 ** 0.5).cuda()
    wp = lib.pack_conv_rect_weight(w, None, L.PREC_F16X3)
    ys = []
    for _ in range(2):
        y = torch.full((16, 448, 8, 8), float('nan'), device='cuda')
        lib.conv2d_rect(L.view(x), wp, L.view(y), 16, 1, 1, stream=L.LamaLib.stream_of(x))
        ys.append(y)
    ref = torch.nn.functional.conv2d(x.double(), w.double())
    tol = E.CONV_TOL[L.PREC_F16X3]
    assert bool(((ys[0].double() - ref).abs() <= tol['atol'] + tol['rtol'] * ref.abs()).all())
    assert torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32))


@pytest.mark.parametrize('H,W,s,p', E.POOL_CASES)
def test_pool3x3(lib, H, W, s, p):
    E.check_pool(lib, H, W, s, p)
    E.check_pool(lib, H, W, s, p, sliced=True)


@pytest.mark.parametrize('h,w', [(8, 8), (3, 5), (1, 1)])
def test_global_avgpool(lib, h, w):
    E.check_global_avgpool(lib, h, w)


@pytest.mark.parametrize('H,W', [(64, 48), (320, 299), (299, 299)])
def test_fid_input(lib, H, W):
    E.check_fid_input(lib, H, W)


# ---- the network ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('prec', E.PRECS)
@pytest.mark.parametrize('tag', ['a', 'b', 'd'])
def test_network_against_fp64(models, tag, prec):
    """Golden cases a, b (resized to 299 x 299) and d (75 x 75 as it is) in f16x3 and bf16x3 against the reference's fp64 activations: 8 x unit.
    Measured on MI355X (units of 4.5e-4): f16x3 a 0.198, b 1.007, d 0.010; bf16x3 a 1.041, b 1.116, d 0.113 (profiles/fid.txt).  Case b is the
    resized 320 x 299 image: the fp64 reference takes its bilinear weights in fp64, the launch in fp32."""
    model = models[(bool(GOLD[f'{tag}_resize']), prec)]
    units, _ = E.network_distance(model, tag)
    print(f'\n[fid] case {tag} {PREC_NAMES[prec]}: {units:.4f} units of {UNIT:.3e}')
    assert units <= 8.0
    assert model.precision == prec                      # no range fallback happened


def test_identical_pair(models):
    """Case c: pred equal to target -> the two activation rows are bit-identical and |FID| <= 1e-6 (tr S1 + tr S2)."""
    model = models[(True, L.PREC_F16X3)]
    pred, target = U.case_inputs(GOLD, 'c')
    ap, at = model.pair(pred.cuda(), target.cuda())
    ap, at = ap.flatten(1).cpu(), at.flatten(1).cpu()
    assert torch.equal(ap.view(torch.int32), at.view(torch.int32))
    fid = EV.calculate_frechet_distance(ap.numpy(), at.numpy())
    _, s1 = EV.fid_calculate_activation_statistics(ap.numpy())
    assert abs(fid) <= 1e-6 * 2 * np.trace(s1)


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    """What tests/fid_child.py saw, in ONE process of its own: the captured launch sequence beside the eager one, and the CLI with and without
    fid_weights=.  (This process keeps no graph, side stream or pinned buffer of that run.)"""
    root = tmp_path_factory.mktemp('fid')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'fid_child.py'), str(root)], cwd=os.path.dirname(HERE), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(root / 'child.pkl', 'rb') as f:
        return pickle.load(f)


def test_graph_replay_is_bit_identical(run):
    """use_graph=True: the capture, a replay, and other inputs through the same graph, bit-identical to the eager launch sequence."""
    g = run['graph']
    assert g['captured'] and g['eager'].shape == (4, 2048, 1, 1) and float(np.abs(g['eager']).max()) > 0
    assert g['capture'].tobytes() == g['eager'].tobytes() and g['replay'].tobytes() == g['eager'].tobytes()
    assert g['swapped'].tobytes() == np.concatenate([g['eager'][2:], g['eager'][:2]]).tobytes()


def test_forward_has_the_references_interface(models):
    model = models[(True, L.PREC_F16X3)]
    pred, target = (t.cuda() for t in U.case_inputs(GOLD, 'a'))
    out = model(torch.cat([pred, target]))
    assert isinstance(out, list) and len(out) == 1 and tuple(out[0].shape) == (4, 2048, 1, 1)
    assert torch.equal(out[0][:2], model.pair(pred, target)[0])
    assert len(model.conv_paths(pred.shape, 'cuda')) == 94


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------------

def test_cli_with_fid_weights(run):
    """python -m lama_amd.evaluate on the recorded dataset of tests/golden/evaluate.npz with LPIPS and fid_weights= (in the child process): the
    report has the fid and lpips_fid100_f1 columns, and its fid total is calculate_frechet_distance of the activations InceptionV3 gives on the
    same tensors."""
    assert run['rc'] == 0 and run['rc_plain'] == 0
    lines = [ln.split('\t') for ln in run['report'].splitlines()]
    assert lines[0] == ['', 'ssim', 'ssim', 'lpips', 'lpips', 'fid', 'lpips_fid100_f1'] and lines[1][5:] == ['mean', 'mean']
    total = [ln for ln in lines if ln[0] == 'total'][0]
    results = dict(run['results'])
    want = EV.calculate_frechet_distance(run['direct_pred'], run['direct_target'])
    assert results[('fid', 'total')]['mean'] == want
    assert total[5] == '%.4f' % want
    assert ('lpips_fid100_f1', 'total') not in results          # the tapped run had no LPIPS: no integral row
    assert float(total[6]) >= 0
    # without fid_weights= the run says so and has no fid column
    assert 'no fid_weights=' in run['plain_stdout']
    assert run['plain_report'].splitlines()[0].split('\t') == ['', 'ssim', 'ssim']
