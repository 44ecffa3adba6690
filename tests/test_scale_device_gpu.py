"""``dataset.scale_factor`` on the device, on hardware: lama_resize_u8_fwd through the C ABI against lama_amd.predict's host restatement of
cv2.resize + pad_img_to_modulo + ``mask > 0``, and HostFedStep(scale_factor=...) against the step fed with the host-scaled fp32 tensors.  Every
bar is bit-equality (the kernel performs the same IEEE operations in the same order; no contraction), as in tests/test_scale_device_emu.py."""
import numpy as np
import pytest
import torch

from lama_amd import _lib as L
from lama_amd import predict as P
from lama_amd import trainers
from oracle import lama_oracle as O
from tests import scale_device_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return L.get_lib()          # raises if liblama_hip.so was not built: no fallback


@pytest.mark.parametrize('case', U.REGIME_CASES, ids=U.case_id)
def test_regime_table_is_bit_equal_to_the_host_chain(lib, case):
    factor, (h, w) = case
    pair = U.random_pair(h, w, seed=h * 100 + w)
    Hp, Wp = U.padded_scaled(h, w, factor)
    for binarize in (True, False):
        want_i, want_m = U.host_chain(*pair, factor, binarize=binarize)
        got_i, got_m = U.device_resize(lib, [pair], factor, h, w, Hp, Wp, device='cuda', binarize=binarize)
        assert np.array_equal(got_i[0], want_i), binarize
        assert np.array_equal(got_m[0], want_m), binarize


def test_batch_of_different_source_sizes_and_an_empty_slot(lib):
    factor, a, b = 0.75, (37, 50), (40, 51)
    Hp, Wp = U.padded_scaled(*a, factor)
    pa, pb = U.random_pair(*a, seed=1), U.random_pair(*b, seed=2)
    got_i, got_m = U.device_resize(lib, [pa, None, pb], factor, 45, 54, Hp, Wp, device='cuda')
    for j, pr in ((0, pa), (2, pb)):
        want_i, want_m = U.host_chain(*pr, factor)
        assert np.array_equal(got_i[j], want_i) and np.array_equal(got_m[j], want_m), j
    assert not got_i[1].any() and not got_m[1].any()


def test_past_the_grid_cap_of_the_grid_stride_loop(lib):
    """2 x 1080 x 1920 at 0.5: 2 x 544 x 960 output pixels, twice what the capped grid (2048 blocks of 256 threads) covers in one pass, with the
    padded rows 540 ... 543."""
    factor, h, w = 0.5, 1080, 1920
    assert U.padded_scaled(h, w, factor) == (544, 960) and 2 * 544 * 960 > 2048 * 256
    pairs = [U.random_pair(h, w, seed=11), U.random_pair(h, w, seed=12)]
    got_i, got_m = U.device_resize(lib, pairs, factor, h, w, 544, 960, device='cuda')
    for j, pr in enumerate(pairs):
        want_i, want_m = U.host_chain(*pr, factor)
        assert np.array_equal(got_i[j], want_i) and np.array_equal(got_m[j], want_m), j


# ---- the step ---------------------------------------------------------------------------------------------------------------------------------

FACTOR, N, HP, WP, SLOT = 0.75, 2, 96, 120, (128, 160)
# per step the source sizes of its two images: 125 x 157 first, then -- in the same slots, through the same captured graphs -- other sizes that
# scale into the same 96 x 120 bucket
STEP_SIZES = [((125, 157), (125, 157)), ((125, 157), (125, 157)), ((124, 155), (126, 158)), ((126, 158), (124, 155))]


@pytest.fixture(scope='module')
def step_case():
    """The model, per step the decoded u8 pairs and, computed once, the u8 results of the module's forward on the host-scaled fp32 tensors."""
    cfg = O.small_config(ngf=16, n_blocks=2)
    sd = {'generator.' + k: v for k, v in O.make_synthetic_state_dict(cfg, seed=3, calib_hw=32).items()}
    model = trainers.DefaultInpaintingTrainingModule(dict(generator=dict(kind='ffc_resnet', **cfg)))
    model.load_state_dict(sd, strict=True)
    model.freeze().cuda()
    model.generator.use_graph = True
    lib = model.generator._exec.lib
    raw, want, host = [], [], []
    for k, sizes in enumerate(STEP_SIZES):
        pairs = []
        for j, (h, w) in enumerate(sizes):
            assert U.padded_scaled(h, w, FACTOR) == (HP, WP)
            image, mask = U.random_pair(h, w, seed=50 + 2 * k + j)
            mask[h // 4: h // 2, w // 3: 2 * w // 3] = 255
            pairs.append((image, mask))
        raw.append(pairs)
        chains = [U.host_chain(*pr, FACTOR, binarize=False) for pr in pairs]             # what load_item returns: the mask as mask / 255
        im, mk = np.stack([c[0] for c in chains]), np.stack([c[1] for c in chains])
        host.append((im, mk))
        out = model(dict(image=torch.from_numpy(im).cuda(), mask=(torch.from_numpy(mk).cuda() > 0) * 1))['inpainted']
        u8 = torch.empty(N, HP, WP, 3, dtype=torch.uint8, device='cuda')
        lib.quantize_u8_hwc(L.view(out), u8, N, HP, WP, torch.cuda.current_stream().cuda_stream)
        want.append(u8.cpu())
    assert not torch.equal(want[0], want[1])
    return dict(model=model, raw=raw, want=want, host=host)


def _run(hs, fill, steps):
    got = {}
    fill(0, 0)
    hs.prime(0)
    for k in range(steps):
        p = k & 1
        if k + 1 < steps:
            fill(1 - p, k + 1)
        hs.launch(p)
        hs.wait(p)
        if k >= 1:
            got[k - 1] = torch.from_numpy(hs.result(1 - p).copy())
    hs.flush((steps - 1) & 1)
    got[steps - 1] = torch.from_numpy(hs.result((steps - 1) & 1).copy())
    return got


@pytest.mark.parametrize('mode', ['host', 'replay', 'graph'])
def test_host_fed_step_with_scale_factor_equals_the_fp32_form(step_case, mode):
    """HostFedStep(scale_factor=0.75) fed with decoded u8 originals against HostFedStep(u8_input=False) fed with the host-scaled fp32 tensors of
    the same images (and against the module's plain forward on them): the same u8 results, bitwise, in every step -- the second use of each
    parity's slots (and, in 'graph', the second replay of each captured step) has other images of other source sizes."""
    model, raw, want, host = (step_case[k] for k in ('model', 'raw', 'want', 'host'))
    steps = len(STEP_SIZES)
    ref = P.HostFedStep(model, N, HP, WP, 'cuda', drain=True, mode=mode, u8_input=False)

    def fill_ref(p, k):
        for j in range(N):
            ref.put(p, j, host[k][0][j], host[k][1][j])
    want_step = _run(ref, fill_ref, steps)
    hs = P.HostFedStep(model, N, HP, WP, 'cuda', drain=True, mode=mode, scale_factor=FACTOR, src_hw=SLOT)
    assert hs.mode == mode and not hs.u8_input and tuple(hs.d_img[0].shape) == (N,) + SLOT + (3,)

    def fill(p, k):
        for j in range(N):
            hs.put(p, j, *raw[k][j])
    got = _run(hs, fill, steps)
    for k in range(steps):
        assert torch.equal(want_step[k], want[k]), (mode, k)
        assert torch.equal(got[k], want[k]), (mode, k)
    assert (hs.graphs[0] is not None and hs.graphs[1] is not None) == (mode == 'graph')
    assert model.generator.check_range('cuda') is True
