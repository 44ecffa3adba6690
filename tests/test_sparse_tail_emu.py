"""CPU tests of the sparse tail through the host SIMT emulator: the work lists of lama_tail_lists_build against a plain torch restatement of the
closure rule (tests/sparse_tail_util.py), small cases of the list variants of the ConvTranspose2d and head kernels beside their dense launches,
and the u8 blend that must not read the prediction where the mask is 0.  tests/test_sparse_tail_gpu.py reruns the same checks on the MI355X."""
import pytest
import torch

from lama_amd import _lib as L
from tests import sparse_tail_util as U
from tests.emu import emu_lib


@pytest.mark.parametrize('plane', U.PLANES, ids=['1x64x96', '2x40x72'])
@pytest.mark.parametrize('kind', U.MASKS)
def test_lists_match_the_closure_rule(kind, plane):
    U.check_lists(emu_lib(), kind, plane, 'cpu')


@pytest.mark.parametrize('prec', [L.PREC_F16X3, L.PREC_BF16X3], ids=['f16x3', 'bf16x3'])
def test_convt_list_variant_small(prec):
    listed, n = U.check_convt_list(emu_lib(), 'cpu', 1, 32, 64, 6, 40, 0.6, prec)      # ragged in both directions: 2 x 2 tiles
    assert 0 < listed < n
    assert U.check_convt_list(emu_lib(), 'cpu', 1, 32, 64, 6, 40, 0.0, prec)[0] == 0   # an empty list: nothing is written


def test_head_list_variant_small():
    listed, n = U.check_head_list(emu_lib(), 'cpu', 1, 20, 30, 0.5, L.PREC_F16X3, rs=8)  # 3 parts (the last ragged) x 2 columns (the last ragged)
    assert 0 < listed < n


def test_head_list_variant_reads_inside_the_closure_on_ragged_planes():
    U.check_head_list_reads_inside_closure(emu_lib(), 'cpu', 1, 20, 30, L.PREC_F16X3, rs=8)   # last segment 4 columns wide, last part 4 rows


def test_list_entry_refuses_what_the_tail_kernels_do_not_take():
    lib = emu_lib()
    x, y = torch.zeros(1, 32, 8, 32), torch.zeros(1, 64, 8, 32)
    wp = lib.pack_conv_weight(torch.zeros(64, 32, 3, 3), None, precision=L.PREC_F16X3)
    tl = (torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 16)
    assert lib.conv2d(L.view(x), wp, L.view(y), 1, 3, 1, 1, precision=L.PREC_F16X3, tile_list=tl, query=True) is False      # a 3x3 stride-1 conv
    with pytest.raises(L.LamaError):
        lib.conv2d(L.view(x), wp, L.view(y), 1, 3, 1, 1, precision=L.PREC_F16X3, tile_list=tl)
    assert bool((y == 0).all())


def test_blend_u8_does_not_read_pred_where_the_mask_is_zero():
    lib = emu_lib()
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 9, 14
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    mask = (torch.rand(B, H, W, generator=g) < 0.4).to(torch.uint8) * 255
    mask[0, 0, :4] = torch.tensor([1, 77, 128, 254], dtype=torch.uint8)                   # fractional masks with binarize off
    pred = torch.rand(B, 3, H, W, generator=g)
    for binarize in (True, False):
        want = torch.empty(B, H, W, 3, dtype=torch.uint8)
        lib.blend_quantize_u8(img, mask, None, L.view(pred), want, B, binarize)
        poisoned = pred.clone()
        poisoned[(mask == 0)[:, None].expand(-1, 3, -1, -1)] = float('nan')
        got = torch.empty_like(want)
        lib.blend_quantize_u8(img, mask, None, L.view(poisoned), got, B, binarize)
        assert torch.equal(got, want)
        assert torch.equal(got[mask == 0], img[mask == 0])                                # the image byte itself
