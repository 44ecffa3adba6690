"""GPU tests of the sparse tail: the work lists against the torch restatement of the closure rule, the list variants of the
ConvTranspose2d and head kernels against their dense launches (torch.equal), and big-lama's u8 predict step on sparse-tail plans against the
dense plans: with every tail buffer poisoned with NaN before each forward (no listed unit reads an unlisted one), under graph replay with
changing masks, as parts of a split plan, and beside the paths that stay dense.

big-lama runs at 2 x 256^2 as the issue states -- where the head's dedicated kernel does not take the plane (2 x 10 columns x 256 rows < 8192), so the
whole tail runs dense there and only the plumbing is exercised -- and at 4 x 256^2, where all four launches walk their lists (asserted)."""
import pytest
import torch

from lama_amd import _lib as L
from lama_amd import trainers
from oracle import lama_oracle as O
from tests import sparse_tail_util as U

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def lib():
    return L.get_lib()


@pytest.mark.parametrize('plane', U.PLANES, ids=['1x64x96', '2x40x72'])
@pytest.mark.parametrize('kind', U.MASKS)
def test_lists_match_the_closure_rule(lib, kind, plane):
    U.check_lists(lib, kind, plane, DEV)


CONVT_CASES = [
    (2, 32, 64, 12, 40, 0.6),        # ragged, one tile per workgroup
    (8, 32, 64, 64, 320, 0.7),       # 1280 tiles, ~896 listed on 512 workgroups: they walk several
    (2, 32, 128, 8, 64, 0.5),        # MG = 2
    (2, 32, 64, 12, 40, 0.0),        # an empty list
]


@pytest.mark.parametrize('prec', [L.PREC_F16X3, L.PREC_BF16X3], ids=['f16x3', 'bf16x3'])
@pytest.mark.parametrize('case', CONVT_CASES, ids=['ragged', 'several_per_wg', 'mg2', 'empty'])
def test_convt_list_variant(lib, case, prec):
    B, cin, cout, H, W, frac = case
    listed, n = U.check_convt_list(lib, DEV, B, cin, cout, H, W, frac, prec)
    assert (listed == 0) == (frac == 0.0)
    if case[0] == 8:
        assert listed > 512


@pytest.mark.parametrize('prec', [L.PREC_F16X3, L.PREC_BF16X3], ids=['f16x3', 'bf16x3'])
@pytest.mark.parametrize('case', [(4, 128, 416, 0.5), (4, 128, 420, 0.7), (4, 128, 416, 0.0)], ids=['4x128x416', 'ragged_last_segment', 'empty'])
def test_head_list_variant(lib, case, prec):
    B, H, W, frac = case                       # the smallest planes the dedicated kernel takes: batch * ceil(W / 26) * H >= 8192
    listed, n = U.check_head_list(lib, DEV, B, H, W, frac, prec)
    assert (listed == 0) == (frac == 0.0)


@pytest.mark.parametrize('prec', [L.PREC_F16X3, L.PREC_BF16X3], ids=['f16x3', 'bf16x3'])
@pytest.mark.parametrize('plane', [(4, 136, 420), (4, 200, 272)], ids=['4x136x420', '4x200x272'])
def test_head_list_variant_reads_inside_the_closure_on_ragged_planes(lib, plane, prec):
    B, H, W = plane                            # W % 26 = 4 and 12 (272: the photo width whose last segment reads columns 254..256); ragged last parts
    U.check_head_list_reads_inside_closure(lib, DEV, B, H, W, prec)


# ---- big-lama -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    torch.manual_seed(0)
    m = trainers.DefaultInpaintingTrainingModule(dict(generator=dict(kind='ffc_resnet', **O.BIG_LAMA)))
    g = torch.Generator().manual_seed(1)
    for mod in m.modules():                    # non-trivial BatchNorm statistics: nothing folds to identity
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data = torch.rand(mod.weight.shape, generator=g) + 0.5
            mod.bias.data = torch.randn(mod.bias.shape, generator=g) * 0.2
            mod.running_mean.data = torch.randn(mod.bias.shape, generator=g) * 0.1
            mod.running_var.data = torch.rand(mod.bias.shape, generator=g) + 0.5
    m.freeze().to(DEV)
    m.generator.auto_fallback = False          # a raised range flag is an error here, not a change of precision
    return m


def _u8_batch(B, r, masks, seed=3):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, r, r, 3), generator=g, dtype=torch.uint8).to(DEV)
    return img, [(m[:, 0] * 255).to(torch.uint8).contiguous().to(DEV) for m in masks]


def _rect(B, r, y0, y1, x0, x1):
    m = torch.zeros(B, 1, r, r)
    m[:, :, y0:y1, x0:x1] = 1.0
    return m


def _dense_u8(model, img, mask):
    """The u8 step on the dense plans: the generator's own switch (``has_sparse_tail``: what the regular generators set) turned off on this instance."""
    gen = model.generator
    gen.has_sparse_tail = False
    try:
        return model.forward_u8(img, mask, None, torch.empty_like(img)).clone()
    finally:
        del gen.has_sparse_tail


def _sparse_plan(gen, B, r):
    return gen._plans[gen._plan_key((B, 4, r, r), DEV) + ('sparse_tail',)]


@pytest.mark.parametrize('B', [2, 4])
def test_poisoned_tail_buffers_do_not_reach_the_output(model, B):
    gen, r = model.generator, 256
    gen.use_graph = False
    masks = [U.bench_mask(B, r, 1234), _rect(B, r, 3, 40, 200, 256)]
    img, mk = _u8_batch(B, r, masks)
    for m in mk:
        want = _dense_u8(model, img, m)
        out = torch.empty_like(img)
        model.forward_u8(img, m, None, out)                      # builds the sparse plan of this shape
        plan = _sparse_plan(gen, B, r)
        tail = plan['tail']
        assert len(tail['ups']) == 3
        if B == 4:
            assert len(tail['taken']) == 4                       # the head and the three upsamplings walk their lists
        for j in tail['ups'] + [tail['out']]:
            plan['bufs'][plan['steps'][j][3]].fill_(float('nan'))
        model.forward_u8(img, m, None, out)                      # (raises LamaRangeError if a NaN is split)
        assert torch.equal(out, want)
        assert gen.check_range(DEV) is True and gen.precision == L.PREC_F16X3


@pytest.mark.parametrize('B,split', [(2, None), (4, None), (8, 2)], ids=['2x256', '4x256', '8x256_two_parts'])
def test_graph_replay_with_changing_masks(model, B, split):
    gen, r = model.generator, 256
    seq = [_rect(B, r, 64, 192, 64, 192), torch.zeros(B, 1, r, r), torch.ones(B, 1, r, r), _rect(B, r, 10, 57, 130, 250)]
    for m in seq:
        m[1] = 0.0                                               # one image of the batch has nothing to inpaint, throughout
    img, mk = _u8_batch(B, r, seq, seed=4)
    gen.use_graph, keep = False, (gen.split_batch, gen.verify_split)
    want = [_dense_u8(model, img, m) for m in mk]
    gen.use_graph, gen.split_batch, gen.verify_split = True, split, False
    try:
        gen._plans.clear()
        out = torch.empty_like(img)
        for k, m in enumerate(mk):
            model.forward_u8(img, m, None, out)
            assert torch.equal(out, want[k]), k
            assert torch.equal(out[1], img[1])
        plan = _sparse_plan(gen, B, r)
        assert plan['graph'] is not None and ('parts' in plan) == (split is not None)
        if B >= 4:
            assert all(len(p['tail']['taken']) == 4 for p in plan.get('parts', [plan]))
        assert gen.check_range(DEV) is True
    finally:
        gen.use_graph, (gen.split_batch, gen.verify_split) = False, keep
        gen._plans.clear()


def test_dense_paths_stay_dense(model):
    """A proxy for "the dense paths return what they returned before the sparse tail existed": a test cannot run another commit, so it checks that
    predicted_image, forward(batch) and generator(x) never build or touch a sparse-tail plan, and return the same bits before and after the
    sparse plan of their shape has been built and run."""
    gen, B, r = model.generator, 4, 256
    gen.use_graph = False
    gen._plans.clear()
    img, (mk,) = _u8_batch(B, r, [U.bench_mask(B, r, 1235)], seed=5)
    fimg = (img.cpu().permute(0, 3, 1, 2).float() / 255.0).contiguous().to(DEV)      # the IEEE division of the loader, on the host
    fmask = (mk > 0).float()[:, None].contiguous()
    x = torch.cat([fimg * (1 - fmask), fmask], 1)
    pred0 = gen(x).clone()
    fwd0 = model(dict(image=fimg, mask=fmask))
    pi0 = model.forward_u8(img, mk, None, torch.empty_like(img), out_key='predicted_image').clone()
    assert gen._plan_key(x.shape, DEV) + ('sparse_tail',) not in gen._plans           # none of them asked for a sparse plan
    model.forward_u8(img, mk, None, torch.empty_like(img))                            # ... this one does
    assert _sparse_plan(gen, B, r)['tail']['taken']
    dense = gen._plans[gen._plan_key(x.shape, DEV)]
    assert dense['tail'] is None
    assert torch.equal(gen(x), pred0)
    fwd1 = model(dict(image=fimg, mask=fmask))
    assert torch.equal(fwd1['inpainted'], fwd0['inpainted']) and torch.equal(fwd1['predicted_image'], fwd0['predicted_image'])
    assert torch.equal(fwd0['predicted_image'], pred0)
    assert torch.equal(model.forward_u8(img, mk, None, torch.empty_like(img), out_key='predicted_image'), pi0)
    want = torch.empty_like(img)
    gen._exec.lib.quantize_u8_hwc(L.view(pred0), want, B, r, r, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(pi0, want)
