"""Host references of the glue kernels (lama_amd/csrc/elementwise.hip) for tests/test_glue_kernels_emu.py / _gpu.py: plain numpy / torch.

The u8 predict-step ends restate the loader's own chain -- ``astype('float32') / 255``, ``np.pad(mode='symmetric')`` up to the slot,
``mask > 0`` or ``mask / 255``, ``cat(img * (1 - m), m)`` / ``m * pred + (1 - m) * img``, ``np.clip(x * 255, 0, 255).astype('uint8')`` in HWC
order -- in fp32, one IEEE operation per step.  Where a compiler may contract a product into the sum that follows it (``a * b + c * d``,
``x * s + t``) the references come as the set of legal evaluations: unfused, the first product fused, the second product fused; a wider
type (fp64, or longdouble as a cross-check) stands in for the fused step."""
import numpy as np
import torch

MASK_VALUES = np.array([0, 1, 128, 255], dtype=np.uint8)


def u8_operands(B, Hp, Wp, seed):
    """u8 HWC image slots [B,Hp,Wp,3] and mask slots [B,Hp,Wp]; each image's h x w pixels in the top-left corner of its slot, the rest of the
    slot filled with other random bytes (the kernels must never read them: the padding mirrors the valid part).  The mask holds 0, 1, 128
    and 255."""
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, size=(B, Hp, Wp, 3)).astype(np.uint8)
    mask = MASK_VALUES[rng.randint(0, 4, size=(B, Hp, Wp))]
    return img, mask


def pad_symmetric(a, Hp, Wp):
    """pad_img_to_modulo's padding of a CHW array: np.pad(mode='symmetric') at the bottom / right (periodic for any amount)."""
    return np.pad(a, ((0, 0), (0, Hp - a.shape[1]), (0, Wp - a.shape[2])), mode='symmetric')


def host_image_mask(img_u8, mask_u8, sizes, binarize):
    """The loader's fp32 operands of one batch: image [B,3,Hp,Wp] and mask [B,1,Hp,Wp]; an empty slot (h = 0 or w = 0) is zeros."""
    B, Hp, Wp = mask_u8.shape
    img = np.zeros((B, 3, Hp, Wp), np.float32)
    m = np.zeros((B, 1, Hp, Wp), np.float32)
    for b in range(B):
        h, w = (Hp, Wp) if sizes is None else sizes[b]
        if h <= 0 or w <= 0:
            continue
        img[b] = pad_symmetric(np.transpose(img_u8[b, :h, :w].astype('float32') / 255, (2, 0, 1)), Hp, Wp)
        mb = pad_symmetric(mask_u8[b, :h, :w].astype('float32')[None] / 255, Hp, Wp)
        m[b] = (mb > 0).astype('float32') if binarize else mb
    return img, m


def compose(img, m):
    """cat(img * (1 - m), m) in fp32: one subtraction, one product -- nothing to contract."""
    return np.concatenate([img * (np.float32(1) - m), m], axis=1)


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def sum_of_products_variants(a, b, c, d, wide=np.float64):
    """The legal fp32 evaluations of a * b + c * d (all fp32 arrays): {name: fp32 array}."""
    a, b, c, d = _f32(a), _f32(b), _f32(c), _f32(d)
    p1, p2 = a * b, c * d
    return {'unfused': p1 + p2,
            'first product fused': _f32(a.astype(wide) * b.astype(wide) + p2.astype(wide)),
            'second product fused': _f32(p1.astype(wide) + c.astype(wide) * d.astype(wide))}


def blend_variants(img, m, pred, wide=np.float64):
    """m * pred + (1 - m) * img; k = 1 - m is rounded to fp32 in every variant (it is a value of its own in the source)."""
    return sum_of_products_variants(m, pred, np.float32(1) - m, img, wide)


def affine_variants(x, scale, shift, wide=np.float64):
    """x * scale[c] + shift[c] over NCHW."""
    x, s, t = _f32(x), _f32(scale).reshape(1, -1, 1, 1), _f32(shift).reshape(1, -1, 1, 1)
    return {'unfused': x * s + t, 'product fused': _f32(x.astype(wide) * s.astype(wide) + t.astype(wide))}


def quantize_hwc(x, ch=None, cw=None):
    """np.clip(x * 255, 0, 255).astype('uint8') of x.permute(0, 2, 3, 1)[:, :ch, :cw] (truncation)."""
    x = np.transpose(_f32(x), (0, 2, 3, 1))[:, :ch, :cw]
    return np.clip(x * np.float32(255), 0, 255).astype('uint8')


def match_variant(got, variants):
    """The names of the variants ``got`` equals everywhere (bits of fp32, bytes of u8), joined with ' = ' where the data cannot tell them
    apart, or None if it equals none."""
    got = np.ascontiguousarray(got)
    names = []
    for name, ref in variants.items():
        ref = np.ascontiguousarray(ref)
        if got.dtype == np.float32:
            same = np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        else:
            same = np.array_equal(got, ref)
        if same:
            names.append(name)
    return ' = '.join(names) if names else None


def act_unit(v32, fn):
    """(fp64 reference, unit): fn of the fp32 values v32 evaluated in fp64, and the largest absolute distance of torch's own CPU fp32 fn from it."""
    t = torch.from_numpy(np.ascontiguousarray(v32))
    ref = fn(t.double())
    return ref, float((fn(t).double() - ref).abs().max())
