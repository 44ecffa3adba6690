"""Shared by tests/test_scale_device_emu.py and tests/test_scale_device_gpu.py: the regime table of ``dataset.scale_factor`` on the device, the
host chain it is held to (lama_amd.predict's restatement of cv2.resize + pad_img_to_modulo + ``mask > 0``) and the call through the C ABI."""
import numpy as np
import torch

from lama_amd import _lib as L
from lama_amd import predict as P

# (factor, (h, w)): every regime of _resize_area.  Integer shrink: the border loop (5 x 7, 9 x 11, 10 x 13, 9 x 10) and both roundings of x.5
# (5 -> 2.5 -> 2, 7 -> 3.5 -> 4); box areas 4, 9 (two groups of four + one) and 16 (four groups).
REGIME_CASES = [
    (0.5, (4, 4)), (0.5, (5, 7)), (0.5, (9, 11)),
    (1 / 3, (9, 9)), (1 / 3, (10, 13)),
    (0.25, (16, 24)), (0.25, (9, 10)),
    (1.0, (7, 9)),
    (0.75, (37, 50)), (0.37, (40, 56)), (0.9, (11, 13)),
    (1.5, (9, 11)), (2.0, (5, 6)), (1.25, (13, 8)),
]


def case_id(case):
    f, (h, w) = case
    return f'{f:.4g}-{h}x{w}'


def random_pair(h, w, seed):
    """A u8 HWC image and a u8 mask with the values 0 / 100 / 200 (so that binarize=False differs from binarize=True)."""
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (h, w, 3)).astype('uint8'), (rng.randint(0, 3, (h, w)) * 100).astype('uint8')


def host_chain(image_u8, mask_u8, factor, pad_mod=8, binarize=True):
    """What ``load_item`` + bin/predict.py:84 build on the host: (image [3,Hp,Wp], mask [1,Hp,Wp]) float32."""
    image = P.pad_img_to_modulo(P.scale_image(np.transpose(image_u8, (2, 0, 1)).astype('float32') / 255, factor), pad_mod)
    mask = P.pad_img_to_modulo(P.scale_image(mask_u8[None].astype('float32') / 255, factor, interpolation='nearest'), pad_mod)
    if binarize:
        mask = ((mask > 0) * 1).astype('float32')
    return image, mask


def padded_scaled(h, w, factor, pad_mod=8):
    dh, dw = P.scaled_size(h, w, factor)
    return P.ceil_modulo(dh, pad_mod), P.ceil_modulo(dw, pad_mod)


def device_resize(lib, pairs, factor, Hs, Ws, Hp, Wp, device='cpu', binarize=True):
    """``pairs``: (image_u8, mask_u8) or None (an empty slot) per image of the batch -> (image [B,3,Hp,Wp], mask [B,1,Hp,Wp]) numpy float32 as
    lama_resize_u8_fwd wrote them.  The outputs start as NaN: every element must be written."""
    B = len(pairs)
    img = np.full((B, Hs, Ws, 3), 77, np.uint8)                  # the slots outside an image hold garbage: nothing may read it
    msk = np.full((B, Hs, Ws), 77, np.uint8)
    ssz, dsz = np.zeros((B, 2), np.int32), np.zeros((B, 2), np.int32)
    for j, pr in enumerate(pairs):
        if pr is None:
            continue
        h, w = pr[1].shape
        img[j, :h, :w], msk[j, :h, :w] = pr
        ssz[j], dsz[j] = (h, w), P.scaled_size(h, w, factor)
    t = [torch.from_numpy(a).to(device) for a in (img, msk, ssz, dsz)]
    out_i = torch.full((B, 3, Hp, Wp), float('nan'), device=device)
    out_m = torch.full((B, 1, Hp, Wp), float('nan'), device=device)
    stream = torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == 'cuda' else 0
    lib.resize_u8(t[0], t[1], t[2], t[3], factor, L.view(out_i), L.view(out_m), B, binarize=binarize, stream=stream)
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize(device)
    return out_i.cpu().numpy(), out_m.cpu().numpy()
