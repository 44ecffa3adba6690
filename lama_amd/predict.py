#!/usr/bin/env python3
"""Batched, data-parallel mirror of ``bin/predict.py`` (reference lines 38-100) on the HIP path.

    python -m lama_amd.predict model.path=<dir> indir=<dir> outdir=<dir> \
        [model.checkpoint=best.ckpt] [dataset.img_suffix=.png] [dataset.pad_out_to_modulo=8] [out_ext=.png] \
        [batch_size=8] [precision=f16x3|bf16x3|f32] [io_threads=8] [dataset.scale_factor=F [paste_back=true]] [device_png=true] \
        [crop_to_mask=true [crop_margin=128] [crop_step=128] [crop_max_side=512]] \
        [device_jpeg=true [jpeg_quality=95] [jpeg_subsampling=420|444]]
    python -m torch.distributed.run --nproc-per-node N -m lama_amd.predict ...        # one process per GPU

Same on-disk contract as the reference: masks are ``**/*mask*.png`` (sorted, recursive), the image of a mask
is ``<mask path up to '_mask'><img_suffix>`` (``evaluation/data.py:59-62``), the result of a mask is written to
``<outdir>/<mask path relative to indir, extension replaced by out_ext>`` (``bin/predict.py:69-72``) as
``clip(inpainted*255, 0, 255).astype(uint8)`` cropped to the unpadded size (``bin/predict.py:86-94``).
``paste_back=true`` (with ``dataset.scale_factor`` only; an output of this driver's own, the reference has none like it) writes the SOURCE image
with the pixels under the mask taken from the scaled prediction, resampled bilinearly on the device (lama_paste_back_u8_fwd).
``crop_to_mask=true`` (another output of this driver's own) runs the generator on a window around each mask (``crop_rect``) at the source resolution
and writes the SOURCE image with the window's inpainted pixels pasted in on the device (lama_crop_compose_u8_fwd / lama_crop_paste_u8_fwd).
``crop_max_side=N`` (with ``crop_to_mask``; 0 = off; this driver's own too) shrinks a window whose padded size would exceed N pixels a side by the
smallest integer k that makes it fit (``crop_rect_limited``: box means of the image, the MAX of each box's mask bytes) and pastes the k-fold
bilinear upsampling of the prediction under the mask (lama_crop_shrink_compose_u8_fwd / lama_crop_shrink_paste_u8_fwd); windows that fit are served as without it.

What differs from the reference's batch-1 Python loop: images are padded to ``pad_out_to_modulo`` and *bucketed by
padded shape*, each bucket is cut into batches, batches are dealt round-robin to the ranks (one process per GPU,
weights replicated, no communication during compute), the u8 HWC results are produced on the device and the only
collective is one gather of those output images to rank 0 per round (RCCL over xGMI on GPUs, gloo in the CPU tests); rank 0
writes the PNGs on a thread pool so file IO overlaps the next round's compute.
"""
from __future__ import annotations

import contextlib
import glob
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import config as lcfg
from . import jpeg as ljpeg
from . import trainers

DEFAULTS = {'model.checkpoint': 'best.ckpt', 'dataset.img_suffix': '.png', 'dataset.pad_out_to_modulo': 8,
            'out_ext': '.png', 'out_key': 'inpainted', 'batch_size': 8, 'precision': 'f16x3',
            'io_threads': 8,   # configs/prediction/default.yaml (+ batch_size / precision / io_threads: this driver's own)
            'paste_back': False,   # extension, with dataset.scale_factor only: write the SOURCE image with the hole taken from the scaled prediction
            'device_png': False,   # extension: the PNGs' zlib streams are made on the device (lama_png_deflate_u8_fwd), the host wraps and writes
            # extension (out_ext .jpg / .jpeg): the JPEGs' entropy-coded scans are made on the device (lama_jpeg_scan_u8_fwd) at cv2.imwrite's
            # quality 95 and libjpeg's 4:2:0, the host adds the headers and writes.  Off: PIL.Image.save at PIL's own defaults (quality 75)
            'device_jpeg': False, 'jpeg_quality': 95, 'jpeg_subsampling': '420',
            # extension: the generator runs on a window around each mask's bounding box (crop_rect: the box + crop_margin a side, rounded up to
            # crop_step) at native resolution, and the result is pasted into the source image on the device (lama_crop_paste_u8_fwd)
            'crop_to_mask': False, 'crop_margin': 128, 'crop_step': 128,
            # extension (with crop_to_mask): a window whose padded size exceeds crop_max_side is shrunk by the smallest integer k that fits
            # (crop_rect_limited) for the generator and the prediction is upsampled under the mask (lama_crop_shrink_*_u8_fwd); 0: no limit
            'crop_max_side': 0}
jpeg_from_scan = ljpeg.jpeg_from_scan
JPEG_OUT_STRIDE = None      # test hook: bytes per scan slot of the device_jpeg steps (None: the slot's raw byte count)


# ----------------------------------------------------------------------------------------------------------------
# dataset glue (saicinpainting/evaluation/data.py:12-33,58-83)
# ----------------------------------------------------------------------------------------------------------------

# keys of configs/prediction/default.yaml this driver honours; anything else is rejected instead of silently ignored
KNOWN_KEYS = set(DEFAULTS) | {'model.path', 'indir', 'outdir', 'device', 'dataset.kind', 'dataset.scale_factor', 'refine', 'profile',
                              'refiner.gpu_ids', 'refiner.modulo', 'refiner.n_iters', 'refiner.lr', 'refiner.min_side',
                              'refiner.max_scales', 'refiner.px_budget', 'refiner.batch_size'}
REFINER_DEFAULTS = {'refiner.gpu_ids': '0,', 'refiner.modulo': 8, 'refiner.n_iters': 15, 'refiner.lr': 0.002, 'refiner.min_side': 512,
                    'refiner.max_scales': 3, 'refiner.px_budget': 1800000,     # configs/prediction/default.yaml:16-24
                    'refiner.batch_size': 1}     # extension: images of one size refined as one batched optimisation (refine_predict_batch)


# option types: paths, suffixes and names stay strings whatever they look like (indir=2024, model.checkpoint=100 are a directory and
# a file name); everything else is a bool / int / float as in the YAML defaults
STRING_KEYS = {'model.path', 'model.checkpoint', 'indir', 'outdir', 'device', 'dataset.kind', 'dataset.img_suffix', 'out_ext', 'out_key',
               'precision', 'refiner.gpu_ids', 'jpeg_subsampling'}
BOOL_KEYS = {'refine', 'profile', 'paste_back', 'device_png', 'device_jpeg', 'crop_to_mask'}
INT_KEYS = {'dataset.pad_out_to_modulo', 'batch_size', 'io_threads', 'jpeg_quality', 'crop_margin', 'crop_step', 'crop_max_side', 'refiner.modulo', 'refiner.n_iters', 'refiner.min_side', 'refiner.max_scales',
            'refiner.px_budget', 'refiner.batch_size'}
FLOAT_KEYS = {'refiner.lr', 'dataset.scale_factor'}


def _parse_value(k: str, v: str):
    if k in STRING_KEYS:
        return v
    try:
        if k in BOOL_KEYS:
            if v.lower() not in ('true', 'false'):
                raise ValueError(v)
            return v.lower() == 'true'
        if k in INT_KEYS:
            return int(v)
        if k in FLOAT_KEYS:
            return float(v)
    except ValueError:
        raise SystemExit(f'{k}={v!r}: expected a {"bool" if k in BOOL_KEYS else "number"}')
    raise AssertionError(f'option {k!r} has no declared type')


def parse_overrides(argv: Sequence[str]) -> Dict[str, object]:
    """Hydra-style ``a.b=c`` overrides on top of configs/prediction/default.yaml's defaults.  Unknown keys and options of the
    reference this driver does not implement are errors (the reference would act on them; ignoring them silently would not be
    a drop-in)."""
    cfg = dict(DEFAULTS)
    cfg.update(REFINER_DEFAULTS)
    given = set()
    for a in argv:
        if '=' not in a:
            raise SystemExit(f'expected key=value, got {a!r}')
        k, v = a.split('=', 1)
        if k not in KNOWN_KEYS:
            raise SystemExit(f'unknown option {k!r}; known: {sorted(KNOWN_KEYS)}')
        cfg[k] = _parse_value(k, v)
        given.add(k)
    for need in ('model.path', 'indir', 'outdir'):
        if need not in cfg:
            raise SystemExit(f'missing {need}=...')
    if str(cfg.get('device', 'cuda')).split(':')[0] != 'cuda':
        raise L.LamaError(f"device={cfg['device']}: lama_amd runs on an MI355X only (there is no CPU path)")
    if cfg.get('dataset.kind', 'default') != 'default':
        raise NotImplementedError(f"dataset.kind={cfg['dataset.kind']} (only the default InpaintingDataset of bin/predict.py)")
    if cfg.get('out_key', 'inpainted') not in ('inpainted', 'predicted_image'):
        raise SystemExit(f"out_key={cfg['out_key']!r}: the predict_only forward (trainers/default.py:56-71) produces 'inpainted' and 'predicted_image'")
    if cfg.get('dataset.scale_factor') is not None and not cfg['dataset.scale_factor'] > 0:
        raise SystemExit(f"dataset.scale_factor={cfg['dataset.scale_factor']!r}: a positive factor (evaluation/data.py:74-77)")
    if cfg['refiner.batch_size'] < 1:
        raise SystemExit(f"refiner.batch_size={cfg['refiner.batch_size']!r}: at least 1 image per refinement")
    if cfg['paste_back']:
        # the scaled prediction resampled (bilinear) to the source grid and pasted into the source image where the mask is not 0
        # (lama_paste_back_u8_fwd): this driver's own output, the reference writes the scaled image
        if cfg.get('dataset.scale_factor') is None:
            raise SystemExit('paste_back=true needs dataset.scale_factor: without one the result has the source size already')
        if cfg.get('refine', False):
            raise SystemExit('paste_back=true with refine=true is not served: refinement writes its own result at the scaled size')
        if cfg['out_key'] != 'inpainted':
            raise SystemExit(f"paste_back=true with out_key={cfg['out_key']!r} is not served: the pasted result is made from 'inpainted' "
                             f"('predicted_image' is undefined where the mask is 0)")
    if cfg['crop_to_mask']:
        # the u8 step on a window around the mask, pasted into the source image (lama_crop_compose_u8_fwd / lama_crop_paste_u8_fwd): this driver's own
        # output, the reference runs the generator on the whole image
        if cfg.get('dataset.scale_factor') is not None:
            raise SystemExit('crop_to_mask=true with dataset.scale_factor is not served: the window is inpainted at the source resolution')
        if cfg.get('refine', False):
            raise SystemExit('crop_to_mask=true with refine=true is not served: refinement works on the whole image')
        if cfg['out_key'] != 'inpainted':
            raise SystemExit(f"crop_to_mask=true with out_key={cfg['out_key']!r} is not served: the pasted result is made from 'inpainted' "
                             f"(a rectangle of raw prediction inside the source image is not a result)")
        try:
            check_crop_options(cfg['crop_margin'], cfg['crop_step'], cfg['dataset.pad_out_to_modulo'])
            check_crop_max_side(cfg['crop_max_side'], cfg['crop_margin'], cfg['crop_step'], cfg['dataset.pad_out_to_modulo'])
        except L.LamaError as e:
            raise SystemExit(f'crop_to_mask=true: {e}')
    elif cfg['crop_max_side']:
        raise SystemExit(f"crop_max_side={cfg['crop_max_side']!r} needs crop_to_mask=true: it limits the window that option inpaints")
    if cfg['device_png'] and cfg['device_jpeg']:
        raise SystemExit('device_jpeg=true with device_png=true: a step ends with one encoder, and out_ext names one format')
    if cfg['device_png']:
        if not str(cfg['out_ext']).lower().endswith('.png'):
            raise SystemExit(f"device_png=true writes PNG files only: out_ext={cfg['out_ext']!r}")
        if cfg.get('refine', False):
            raise SystemExit('device_png=true with refine=true is not served: refinement writes from host tensors')
    if not 1 <= cfg['jpeg_quality'] <= 100:
        raise SystemExit(f"jpeg_quality={cfg['jpeg_quality']!r}: 1 .. 100")
    if cfg['jpeg_subsampling'] not in ljpeg.SUBSAMPLING:
        raise SystemExit(f"jpeg_subsampling={cfg['jpeg_subsampling']!r}: 420 or 444")
    if cfg['device_jpeg']:
        if not str(cfg['out_ext']).lower().endswith(('.jpg', '.jpeg')):
            raise SystemExit(f"device_jpeg=true writes JPEG files only (out_ext=.jpg or .jpeg): out_ext={cfg['out_ext']!r}")
        if cfg.get('refine', False):
            raise SystemExit('device_jpeg=true with refine=true is not served: refinement writes from host tensors')
    else:
        for k in ('jpeg_quality', 'jpeg_subsampling'):
            if k in given:
                raise SystemExit(f'{k}= is an option of device_jpeg=true: without it a .jpg is written by PIL at PIL\'s defaults')
    return cfg


def list_dataset(indir: str, img_suffix: str = '.png') -> List[Tuple[str, str]]:
    """(mask path, image path) pairs: InpaintingDataset.__init__, evaluation/data.py:59-62."""
    masks = sorted(glob.glob(os.path.join(indir, '**', '*mask*.png'), recursive=True))
    return [(m, m.rsplit('_mask', 1)[0] + img_suffix) for m in masks]


def load_image(fname: str, mode: str = 'RGB') -> np.ndarray:
    """evaluation/data.py:12-20 (PIL instead of cv2: same decoded values)."""
    from PIL import Image
    img = np.array(Image.open(fname).convert(mode))
    if img.ndim == 3:
        img = np.transpose(img, (2, 0, 1))
    return img.astype('float32') / 255


def ceil_modulo(x: int, mod: int) -> int:
    return x if x % mod == 0 else (x // mod + 1) * mod


def pad_img_to_modulo(img: np.ndarray, mod: int) -> np.ndarray:
    """evaluation/data.py:29-33: symmetric padding at the bottom / right."""
    c, h, w = img.shape
    return np.pad(img, ((0, 0), (0, ceil_modulo(h, mod) - h), (0, ceil_modulo(w, mod) - w)), mode='symmetric')


# ---- dataset.scale_factor (evaluation/data.py:42-55,74-77): cv2.resize(img, dsize=None, fx=f, fy=f) with INTER_AREA on the float image and
# INTER_NEAREST on the float mask.  cv2 is not in this image, so this is a restatement of OpenCV 4's imgproc/resize.cpp from its published
# algorithm -- PARITY UNPINNED (no cv2 here to generate vectors from): the index / weight tables and the float32 accumulation order follow
# resize.cpp (computeResizeAreaTab + ResizeArea_Invoker; resizeAreaFast_Invoker's four-at-a-time sums; the INTER_AREA-upscaling coefficients of
# the linear path; resizeNN's floor(x / f) taps), known-answer tests in tests/test_scale_factor.py.  These host functions are the loader of
# ``refine=True`` (load_item) and the statement the device kernel is held to, bit for bit: the predict loop runs the same arithmetic inside its
# u8 step (lama_resize_u8_fwd, csrc/elementwise.hip) and the host only decodes and computes ``scaled_size``.

def scaled_size(h: int, w: int, factor: float) -> Tuple[int, int]:
    """dsize of cv::resize(dsize=None, fx, fy): saturate_cast<int>(size * f) = round half to even."""
    return int(round(h * factor)), int(round(w * factor))


def _area_taps(ssize: int, dsize: int, scale: float):
    """computeResizeAreaTab: per destination index the source taps and their float32 weights, padded to a common tap count with weight 0."""
    import math
    taps = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = math.ceil(f1), math.floor(f2)
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        t = []
        if s1 - f1 > 1e-3:
            t.append((s1 - 1, np.float32((s1 - f1) / cell)))
        for sx in range(s1, s2):
            t.append((sx, np.float32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            t.append((s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
        taps.append(t)
    T = max(len(t) for t in taps)
    idx = np.zeros((dsize, T), np.int64)
    wt = np.zeros((dsize, T), np.float32)
    for d, t in enumerate(taps):
        for k, (sx, a) in enumerate(t):
            idx[d, k], wt[d, k] = sx, a
    return idx, wt


def _resize_area(img: np.ndarray, factor: float) -> np.ndarray:
    """INTER_AREA of a float32 [H, W] or [H, W, C] image by ``factor`` in both directions."""
    import math
    a = np.ascontiguousarray(img, dtype=np.float32)
    H, W = a.shape[:2]
    dh, dw = scaled_size(H, W, factor)
    if dh <= 0 or dw <= 0:
        raise L.LamaError(f'scale_factor {factor}: a {W}x{H} image scales to nothing')
    scale = 1.0 / factor
    if scale >= 1.0:                                            # shrinking: true area averaging
        isc = int(round(scale))
        if abs(scale - isc) < np.finfo(np.float64).eps:         # integer factor: resizeAreaFast -- box sums in groups of four, * 1 / area
            # destination pixels whose box would leave the image are cut off by dsize = round(size * f) (<= size / isc only when it divides)
            dh2, dw2 = min(dh, H // isc), min(dw, W // isc)
            box = [a[sy:sy + dh2 * isc:isc, sx:sx + dw2 * isc:isc] for sy in range(isc) for sx in range(isc)]
            acc = np.zeros_like(box[0])
            k, area = 0, isc * isc
            while k <= area - 4:
                acc = acc + (((box[k] + box[k + 1]) + box[k + 2]) + box[k + 3])
                k += 4
            while k < area:
                acc = acc + box[k]
                k += 1
            out = acc * np.float32(1.0 / area)
            if (dh2, dw2) != (dh, dw):                          # (x.5 rounded up: the partial last boxes average the pixels inside the image)
                full = np.zeros((dh, dw) + a.shape[2:], np.float32)
                full[:dh2, :dw2] = out
                for yy in range(dh):
                    for xx in range(dw):
                        if yy >= dh2 or xx >= dw2:
                            blk = a[yy * isc:min((yy + 1) * isc, H), xx * isc:min((xx + 1) * isc, W)]
                            px = blk.reshape(-1, *a.shape[2:])                   # resizeAreaFast's border loop: sum / count of the pixels inside
                            acc1 = np.zeros(a.shape[2:], np.float32)
                            for v in px:
                                acc1 = acc1 + v
                            full[yy, xx] = acc1 / np.float32(len(px))
                out = full
            return out
        xi, xw = _area_taps(W, dw, scale)
        yi, yw = _area_taps(H, dh, scale)
        ex = (slice(None),) * 2 + (None,) * (a.ndim - 2)
        buf = np.zeros((H, dw) + a.shape[2:], np.float32)      # the x pass of every source row: buf[dx] += S[sx] * alpha, taps in table order
        for t in range(xi.shape[1]):
            buf = buf + a[:, xi[:, t]] * xw[None, :, t][ex] if t else a[:, xi[:, t]] * xw[None, :, t][ex]
        out = np.zeros((dh, dw) + a.shape[2:], np.float32)     # the y pass: sum[dx] = beta * buf, then += for the following rows
        for t in range(yi.shape[1]):
            term = buf[yi[:, t]] * yw[:, t][(slice(None), None) + (None,) * (a.ndim - 2)]
            out = out + term if t else term
        return out
    # enlarging with INTER_AREA = the linear path with area coefficients: sx = floor(dx * scale), fx = (dx + 1) - (sx + 1) * f, kept in [0, 1)
    def coef(ssize, dsize):
        sx = np.floor(np.arange(dsize) * scale).astype(np.int64)
        fx = ((np.arange(dsize) + 1) - (sx + 1) * factor).astype(np.float32)
        fx = np.where(fx <= 0, np.float32(0), fx - np.floor(fx)).astype(np.float32)
        lo = sx < 0
        fx[lo], sx[lo] = 0, 0
        hi = sx >= ssize - 1
        fx[hi], sx[hi] = 0, ssize - 1
        return sx, np.minimum(sx + 1, ssize - 1), (np.float32(1) - fx).astype(np.float32), fx
    x0, x1, ax0, ax1 = coef(W, dw)
    y0, y1, ay0, ay1 = coef(H, dh)
    ex = (None, slice(None)) + (None,) * (a.ndim - 2)
    rows = a[:, x0] * ax0[ex] + a[:, x1] * ax1[ex]
    ey = (slice(None), None) + (None,) * (a.ndim - 2)
    return (rows[y0] * ay0[ey] + rows[y1] * ay1[ey]).astype(np.float32)


def _resize_nearest(img: np.ndarray, factor: float) -> np.ndarray:
    """INTER_NEAREST: tap min(floor(d / f), size - 1) in each direction (resizeNN)."""
    H, W = img.shape[:2]
    dh, dw = scaled_size(H, W, factor)
    if dh <= 0 or dw <= 0:
        raise L.LamaError(f'scale_factor {factor}: a {W}x{H} image scales to nothing')
    inv = 1.0 / factor
    ys = np.minimum(np.floor(np.arange(dh) * inv).astype(np.int64), H - 1)
    xs = np.minimum(np.floor(np.arange(dw) * inv).astype(np.int64), W - 1)
    return np.ascontiguousarray(img[ys][:, xs])


def scale_image(img: np.ndarray, factor: float, interpolation: str = 'area') -> np.ndarray:
    """evaluation/data.py:42-55: a float32 [C,H,W] image through cv2.resize(fx=fy=factor) and back to [C,H',W'] ('area' = cv2.INTER_AREA, the
    default; 'nearest' = cv2.INTER_NEAREST, what InpaintingDataset uses for the mask)."""
    hwc = img[0] if img.shape[0] == 1 else np.transpose(img, (1, 2, 0))
    out = _resize_nearest(hwc, factor) if interpolation == 'nearest' else _resize_area(hwc, factor)
    return out[None, ...] if out.ndim == 2 else np.transpose(out, (2, 0, 1))


def load_item_u8(mask_path: str, img_path: str, mask: Optional[np.ndarray] = None):
    """The same pair as it is on disk: (u8 image [H,W,3], u8 mask [H,W], (H, W)).  ``load_image``'s / 255, ``pad_img_to_modulo`` and
    bin/predict.py:84's ``mask > 0`` happen on the device (lama_mask_compose_u8_fwd, ABI v110): the host only decodes.  ``mask``: the mask as
    decoded already (the crop_to_mask pre-pass keeps what fits its budget), not decoded again."""
    from PIL import Image
    image = np.asarray(Image.open(img_path).convert('RGB'))
    if mask is None:
        mask = np.asarray(Image.open(mask_path).convert('L'))
    if tuple(mask.shape) != tuple(image.shape[:2]):
        raise L.LamaError(f'{mask_path}: mask is {mask.shape[1]}x{mask.shape[0]} but {img_path} is {image.shape[1]}x{image.shape[0]}')
    return image, mask, tuple(image.shape[:2])


def load_item(mask_path: str, img_path: str, pad_mod: int, scale_factor: Optional[float] = None):
    """InpaintingDataset.__getitem__, evaluation/data.py:69-83 -> (image [3,H',W'], mask [1,H',W'], (H, W)): ``scale_factor`` rescales the image
    (INTER_AREA) and the mask (INTER_NEAREST) before the padding, and (H, W) = ``unpad_to_size`` is the rescaled size (data.py:74-79)."""
    image = load_image(img_path, 'RGB')
    mask = load_image(mask_path, 'L')[None, ...]
    if tuple(mask.shape[1:]) != tuple(image.shape[1:]):
        raise L.LamaError(f'{mask_path}: mask is {mask.shape[2]}x{mask.shape[1]} but {img_path} is {image.shape[2]}x{image.shape[1]}')
    if scale_factor is not None:
        image = scale_image(image, scale_factor)
        mask = scale_image(mask, scale_factor, interpolation='nearest')
    hw = image.shape[1:]
    if pad_mod and pad_mod > 1:
        image, mask = pad_img_to_modulo(image, pad_mod), pad_img_to_modulo(mask, pad_mod)
    return image, mask, hw


# ---- crop_to_mask: the window of an image the generator sees (an option of this driver's own: the reference has none like it) ----------------------

def check_crop_options(margin: int, step: int, pad_mod: int):
    """``crop_margin`` >= 0 and ``crop_step`` a positive multiple of ``pad_out_to_modulo``: every window that does not span its axis is then a
    padded size already."""
    mod = int(pad_mod) if pad_mod and int(pad_mod) > 1 else 1
    if int(margin) < 0:
        raise L.LamaError(f'crop_margin={margin!r}: 0 or more pixels around the mask')
    if int(step) < 1 or int(step) % mod:
        raise L.LamaError(f'crop_step={step!r}: a positive multiple of dataset.pad_out_to_modulo={pad_mod!r}')


def crop_rect(mask_u8: np.ndarray, margin: int, step: int, pad_mod: int) -> Tuple[int, int, int, int, int, int]:
    """The window of an h x w image that ``crop_to_mask`` inpaints -> (y0, x0, ch, cw, Hp, Wp), integers only (every rank computes the same
    window from the same file).  The box is the rows / columns where ``mask > 0`` (the raw bytes, whatever ``binarize`` says; an empty mask: the empty
    box at the origin).  Per axis: want = extent + 2 margin; c = min(side, want rounded up to ``step``) (at least one pixel: an empty box with
    margin 0 takes one step); the window is centred on the box and clamped into the image, o = clamp(lo - (c - extent) // 2, 0, side - c).
    A window that spans its axis (c = side, o = 0) is padded as the whole image would be, ceil_modulo(side, pad_mod); any other is ``c``, a
    multiple of ``step`` and so of ``pad_mod``."""
    check_crop_options(margin, step, pad_mod)
    if mask_u8.ndim != 2 or mask_u8.shape[0] < 1 or mask_u8.shape[1] < 1:
        raise L.LamaError(f'crop_rect: a [h, w] mask of at least one pixel, got {tuple(mask_u8.shape)}')
    margin, step = int(margin), int(step)
    hole = mask_u8 > 0
    out = []
    for axis in (0, 1):
        side = int(mask_u8.shape[axis])
        hit = np.flatnonzero(hole.any(axis=1 - axis))
        lo, extent = (int(hit[0]), int(hit[-1]) - int(hit[0]) + 1) if hit.size else (0, 0)
        want = max(1, extent + 2 * margin)
        c = min(side, (want + step - 1) // step * step)
        o = min(max(lo - (c - extent) // 2, 0), side - c)
        assert 0 <= o <= lo and lo + extent <= o + c <= side, (axis, side, lo, extent, o, c)           # inside the image, around the box
        out.append((o, c, ceil_modulo(side, pad_mod) if c == side and pad_mod and pad_mod > 1 else c))
    (y0, ch, Hp), (x0, cw, Wp) = out
    return y0, x0, ch, cw, Hp, Wp


def rect_fits(rect, h: int, w: int, Hs: int, Ws: int, Hp: int, Wp: int) -> bool:
    """The conditions lama_crop_compose_u8_fwd / lama_crop_paste_u8_fwd put on a window (y0, x0, ch, cw) of an h x w image in an Hs x Ws slot."""
    y0, x0, ch, cw = (int(v) for v in rect[:4])
    return (ch >= 1 and cw >= 1 and y0 >= 0 and x0 >= 0 and y0 + ch <= h and x0 + cw <= w and ch <= Hp and cw <= Wp and 0 < h <= Hs and 0 < w <= Ws)


# ---- crop_max_side: a window too large for the generator is shrunk by an integer k (this driver's own too) ------------------------------------------
CROP_SHRINK_MAX = 16     # the kernels' largest k (1.0 / (1.0 / k) == k holds in fp64 up to 48: the pin against the host's resize relies on it)


def check_crop_max_side(max_side: int, margin: int, step: int, pad_mod: int):
    """``crop_max_side`` is 0 (no limit) or a multiple of ``pad_out_to_modulo`` of at least 2 ``crop_margin`` + ``crop_step`` rounded up to
    ``crop_step``: below that no shrink k can ever make a window fit (margin and step are measured in generator pixels)."""
    mod = int(pad_mod) if pad_mod and int(pad_mod) > 1 else 1
    max_side, margin, step = int(max_side), int(margin), int(step)
    if max_side == 0:
        return
    least = (2 * margin + step + step - 1) // step * step
    if max_side < 0 or max_side % mod or max_side < least:
        raise L.LamaError(f'crop_max_side={max_side!r}: 0 (off) or a multiple of dataset.pad_out_to_modulo={pad_mod!r} of at least {least} '
                          f'(2 crop_margin + crop_step, rounded up to crop_step)')


def crop_rect_limited(mask_u8: np.ndarray, margin: int, step: int, pad_mod: int, max_side: int,
                      kmax: int = CROP_SHRINK_MAX) -> Tuple[int, int, int, int, int, int, int, int, int]:
    """The window of ``crop_to_mask`` under ``crop_max_side`` -> (y0, x0, ch, cw, k, dh, dw, Hp, Wp), integers only: for k = 1, 2, ... ``kmax`` the
    window is ``crop_rect(mask, margin k, step k, pad_mod)`` (margin and step in generator pixels), the generator sees dh x dw = ceil(ch / k) x
    ceil(cw / k) pixels padded to (Hp, Wp), and the first k with Hp, Wp <= ``max_side`` is taken -- k = 1: ``crop_rect``'s own window."""
    check_crop_options(margin, step, pad_mod)
    check_crop_max_side(max_side, margin, step, pad_mod)
    margin, step, max_side, kmax = int(margin), int(step), int(max_side), int(kmax)
    if max_side < 1 or not 1 <= kmax <= CROP_SHRINK_MAX:
        raise L.LamaError(f'crop_rect_limited: crop_max_side={max_side!r} (a positive limit) and kmax={kmax!r} (1 .. {CROP_SHRINK_MAX})')
    padded = (lambda n: ceil_modulo(n, pad_mod)) if pad_mod and pad_mod > 1 else (lambda n: n)
    for k in range(1, kmax + 1):
        y0, x0, ch, cw, _, _ = crop_rect(mask_u8, margin * k, step * k, pad_mod)
        dh, dw = (ch + k - 1) // k, (cw + k - 1) // k
        Hp, Wp = padded(dh), padded(dw)                   # (k = 1: crop_rect's own padded size)
        if Hp <= max_side and Wp <= max_side:
            return y0, x0, ch, cw, k, dh, dw, Hp, Wp
    raise L.LamaError(f'crop_rect_limited: the {cw}x{ch} window of a {mask_u8.shape[1]}x{mask_u8.shape[0]} image is still {Wp}x{Hp} at the largest '
                      f'shrink k={kmax}: larger than crop_max_side={max_side}')


def shrink_rect_fits(rect, h: int, w: int, Hs: int, Ws: int, Hp: int, Wp: int) -> bool:
    """The conditions lama_crop_shrink_compose_u8_fwd / lama_crop_shrink_paste_u8_fwd put on (y0, x0, ch, cw, k) of an h x w image in an Hs x Ws
    slot with an (Hp, Wp) low-resolution view."""
    y0, x0, ch, cw, k = (int(v) for v in rect[:5])
    return (1 <= k <= CROP_SHRINK_MAX and ch >= 1 and cw >= 1 and y0 >= 0 and x0 >= 0 and y0 + ch <= h and x0 + cw <= w and
            (ch + k - 1) // k <= Hp and (cw + k - 1) // k <= Wp and 0 < h <= Hs and 0 < w <= Ws)


# ----------------------------------------------------------------------------------------------------------------
# work distribution
# ----------------------------------------------------------------------------------------------------------------

def plan_rounds(shapes: Sequence[Tuple[int, int]], batch_size: int, world: int) -> List[dict]:
    """Bucket item indices by padded shape, cut buckets into batches, deal the batches of a bucket round-robin to ranks.
    Returns rounds: dict(shape=(H', W'), batches=[item-index list per rank (possibly empty)])."""
    buckets: Dict[Tuple[int, int], List[int]] = {}
    for i, s in enumerate(shapes):
        buckets.setdefault(tuple(s), []).append(i)
    rounds = []
    # largest padded shape first: the activation / pinned buffers of every later bucket then fit blocks the caching allocators already hold
    # (ascending order paid a round of hipMalloc / hipHostMalloc calls per new shape: ~30 ms each in a directory of differently sized photos)
    for shape in sorted(buckets, key=lambda hw: (-hw[0] * hw[1], hw)):
        idx = buckets[shape]
        batches = [idx[i:i + batch_size] for i in range(0, len(idx), batch_size)]
        for r0 in range(0, len(batches), world):
            chunk = batches[r0:r0 + world]
            rounds.append(dict(shape=shape, batches=chunk + [[] for _ in range(world - len(chunk))]))
    return rounds


def gather_to_root(dist, gathered: Optional[torch.Tensor], part: torch.Tensor, rank: int, world: int, root: int = 0):
    """The data path's only collective: the u8 result images of every rank to the WRITER rank.  ``dist.gather`` (RCCL: one
    send per non-root rank, ``world - 1`` receives on the root, point-to-point over xGMI) -- the other ranks allocate and receive nothing,
    unlike an all-gather, which moves ``world`` times the bytes to deliver copies nobody reads.  ``gathered`` = [world * n, ...] on the root,
    None elsewhere.  Returns the asynchronous work handle."""
    parts = list(gathered.chunk(world, dim=0)) if rank == root else None          # contiguous slices of the root's buffer: no staging copy
    return dist.gather(part, gather_list=parts, dst=root, async_op=True)


PROFILE_SPANS = False                    # profile=true: HostFedStep records timing events around every step's compute
LOOP_TIMES: Dict[str, float] = {}      # wall seconds of the main thread per phase of the round loop (python -m lama_amd.predict ... profile=true prints them)
TUNE_MIN_ROUNDS = 1024    # buckets with fewer rounds skip the split-plan timing check: ~0.35 s for at most 5 % of the bucket's time (HostFedStep(tune=False))
CROP_MASK_CACHE_BYTES = 512 << 20   # crop_to_mask: the decoded masks the pre-pass keeps for the loads of the round loop (the rest are decoded again)
CAPTURE_MIN_ROUNDS = 32   # ... and with fewer than this also the graph capture: ~30 ms for ~8 % of a round's 10 ms (HostFedStep(capture=False): plain launches)


class _RangeRestart(Exception):
    """A forward of this run left the fp16 split's range: the generator is on the bf16 split now, the run starts over."""


def encode_png(rgb: np.ndarray) -> bytes:
    """An 8-bit RGB (or gray) image as PNG bytes with the parameters cv2.imwrite uses by default (bin/predict.py:94: IMWRITE_PNG_COMPRESSION
    unset -> libpng filter SUB, zlib level 1, strategy Z_RLE): the Sub filter as one numpy subtraction, one zlib stream, one IDAT chunk.
    Same decoded pixels as any PNG writer; 7.4 ms per 512 x 512 image where PIL's encoder (adaptive filter choice per row, default strategy)
    takes 56 ms at the same level -- the CLI was encode-bound on the host at 0.47 of the GPU rate (bench.py predict_cli_leg, round 6)."""
    import struct
    import zlib
    a = np.ascontiguousarray(rgb)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)):
        raise L.LamaError(f'encode_png: uint8 [H,W] / [H,W,3] image, got {a.dtype} {a.shape}')
    h, w = a.shape[:2]
    c = 1 if a.ndim == 2 else a.shape[2]
    flat = a.reshape(h, w * c)
    raw = np.empty((h, 1 + w * c), np.uint8)
    raw[:, 0] = 1                                              # filter type Sub: byte - byte of the pixel to the left (mod 256)
    raw[:, 1:1 + c] = flat[:, :c]
    raw[:, 1 + c:] = flat[:, c:] - flat[:, :-c]
    co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    data = co.compress(raw.tobytes()) + co.flush()

    def chunk(tag: bytes, body: bytes) -> bytes:
        return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body) & 0xffffffff)

    ihdr = struct.pack('>IIBBBBB', w, h, 8, 2 if c == 3 else 0, 0, 0, 0)
    return b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', ihdr) + chunk(b'IDAT', data) + chunk(b'IEND', b'')


def png_from_zlib(h: int, w: int, channels: int, stream) -> bytes:
    """The PNG file around a finished zlib stream of the h x w image's filtered rows (lama_png_deflate_u8_fwd made it on the device): signature,
    IHDR (8 bits; RGB for 3 channels, gray for 1), ONE IDAT whose CRC is zlib.crc32 over the compressed bytes, IEND.  The host's share of a
    device-encoded PNG: one CRC pass and two copies."""
    import struct
    import zlib
    if channels not in (1, 3) or h < 1 or w < 1:
        raise L.LamaError(f'png_from_zlib: an 8-bit gray / RGB image of at least one pixel, got {h}x{w}x{channels}')
    ihdr = b'IHDR' + struct.pack('>IIBBBBB', w, h, 8, 2 if channels == 3 else 0, 0, 0, 0)
    n = len(stream)
    return b''.join((b'\x89PNG\r\n\x1a\n', struct.pack('>I', 13), ihdr, struct.pack('>I', zlib.crc32(ihdr) & 0xffffffff),
                     struct.pack('>I', n), b'IDAT', stream, struct.pack('>I', zlib.crc32(stream, zlib.crc32(b'IDAT')) & 0xffffffff),
                     b'\x00\x00\x00\x00IEND\xaeB`\x82'))


class _Latch:
    """Count-down latch: the round loop waits on it before a pinned result set is overwritten while pool workers still snapshot it."""

    def __init__(self):
        import threading
        self._c, self._n = threading.Condition(), 0

    def add(self, n: int = 1):
        with self._c:
            self._n += n

    def done(self):
        with self._c:
            self._n -= 1
            if self._n <= 0:
                self._c.notify_all()

    def wait(self):
        with self._c:
            while self._n > 0:
                self._c.wait()


def _snap_and_write(path: str, view: np.ndarray, latch: _Latch, pool):
    """``fast`` pool job: copy the image out of the pinned result set (then release the latch: the set may be overwritten) and queue its encode +
    write on ``pool``; returns that future."""
    try:
        rgb = view.copy()
    finally:
        latch.done()
    return pool.submit(_write_png, path, rgb)


def _snap_and_wrap(path: str, view: np.ndarray, h: int, w: int, latch: _Latch, pool):
    """``fast`` pool job of ``device_png``: copy the image's zlib stream out of the pinned result set (then release the latch) and queue its wrap
    (CRC + container) + write on ``pool``; returns that future."""
    try:
        data = view.tobytes()
    finally:
        latch.done()
    return pool.submit(_write_png_stream, path, h, w, data)


def _write_png_stream(path: str, h: int, w: int, data: bytes):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'wb') as f:
        f.write(png_from_zlib(h, w, 3, data))


class JpegOverflow(L.LamaError):
    """A device-encoded scan did not fit its slot (out_bytes = -(bytes needed)): nothing was written for that image."""

    def __init__(self, what: str, needed: int, slot: int):
        super().__init__(f'{what}: the JPEG scan needs {needed} bytes, its slot holds {slot}')
        self.needed, self.slot = needed, slot


def jpeg_stream_view(flat: np.ndarray, slot: int, len_at: int, j: int, what: str) -> np.ndarray:
    """Scan j of one flat ``encode_jpeg`` result set (the scan slots of ``slot`` bytes, the int32 lengths from byte ``len_at`` on): a view, empty
    for an empty slot; JpegOverflow (naming ``what``) for a negative length."""
    n = int(flat[len_at:].view(np.int32)[j])
    if n < 0:
        raise JpegOverflow(what, -n, slot)
    return flat[j * slot:j * slot + n]


def _snap_and_wrap_jpeg(path: str, view: np.ndarray, h: int, w: int, quality: int, subsampling: int, latch: _Latch, pool):
    """``fast`` pool job of ``device_jpeg``: copy the image's scan out of the pinned result set (then release the latch) and queue its headers +
    write on ``pool``; returns that future."""
    try:
        data = view.tobytes()
    finally:
        latch.done()
    return pool.submit(_write_jpeg_scan, path, h, w, quality, subsampling, data)


def _write_jpeg_scan(path: str, h: int, w: int, quality: int, subsampling: int, data: bytes):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'wb') as f:
        f.write(jpeg_from_scan(h, w, quality, subsampling, data))


def _write_jpeg_host(path: str, rgb: np.ndarray, quality: int, subsampling: int):
    """The fallback of ``device_jpeg`` for an image whose scan overflowed its slot: libjpeg on the host at the same quality and subsampling."""
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(rgb).save(path, 'JPEG', quality=int(quality), subsampling=2 if subsampling else 0)


def _write_png(path: str, rgb: np.ndarray):
    """bin/predict.py:93-94 (the reference converts RGB -> BGR only because cv2.imwrite expects BGR).  ``.png``: encode_png; any other
    extension goes through PIL, which picks the format from it as cv2.imwrite does."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if path.lower().endswith('.png'):
        with open(path, 'wb') as f:
            f.write(encode_png(rgb))
        return
    from PIL import Image
    Image.fromarray(rgb).save(path)


# ----------------------------------------------------------------------------------------------------------------
# one step fed from host memory
# ----------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _settings(gen, **attrs):
    """Set attributes of the generator for the duration of the block; they have their former values afterwards, a raise included."""
    keep = {k: getattr(gen, k) for k in attrs}
    for k, v in attrs.items():
        setattr(gen, k, v)
    try:
        yield
    finally:
        for k, v in keep.items():
            setattr(gen, k, v)


class HostFedStep:
    """One predict step -- mask binarisation (bin/predict.py:84), mask-compose + generator + blend (trainers/default.py:56-71), u8 HWC
    quantisation (bin/predict.py:92) -- fed from / drained to pinned HOST buffers, double-buffered:

        launch(p):   H2D  host input set 1-p -> device set 1-p        (the NEXT batch; copy stream)
                  || compute on device set p -> u8[p]                 (THIS batch)
                  || D2H  u8[1-p] -> host result set 1-p              (the PREVIOUS batch; copy stream; ``drain``)

    ``mode='replay'``: the copies run on streams of their own, forked and joined by events, beside the replay of the generator's own
    hipGraph (+ four plain launches: mask compose, blend, u8).  ``'streams'``: the same around ~270 plain launches.  ``'graph'``: the three as
    parallel branches INSIDE one captured hipGraph per parity (built in round 5).  Measured (bench.py value_host_fed, images/s; the boxes of
    the pool differ in GPU AND host speed; profiles/r05_host_fed.txt):

        box (resident)      serial (copies on the compute stream)   replay    streams    graph
        r4 driver (825)     761                                     788       819        --
        r05a      (800)     740                                     --        765        736
        r05b      (817)     754                                     --        740        756
        r05h      (852)     760                                     790       531        788     (the batch in four parallel parts)
        r05i      (837)     708                                     757       530        777     (the batch in four parallel parts)

    A replay of a graph overlaps copies of OTHER streams only partly (the r4 result); copy nodes INSIDE a graph run in line with its kernel
    nodes when the graph is one kernel chain (r05a / r05b: = the serial form) but overlap when it has parallel kernel branches already
    (r05h / r05i: the split plans of generator.split_batch -- the executor then runs the graph on several queues); plain launches overlap
    fully but make the step launch-bound on a slow host (r05b) and with the batch in four parts.  ``mode='auto'`` (the default): 'graph'
    where the generator splits this shape, else 'replay' -- neither ever lost to the serial form.

    The caller alternates p = 0, 1, 0, ...: it fills host set 1-p before ``launch(p)`` (after ``wait`` has told it that the launch that last
    read that set is complete), calls ``prime(p0)`` once before the first launch and ``flush(p_last)`` after the last.  ``drain=False``
    (multi-rank: the results go through the gather instead) leaves the D2H branch out.  On a CPU device (the emulator tests) the same body
    runs synchronously, unpinned.

    Three input forms: u8 HWC images as decoded, in padded slots (the default; ``put``); the same in SOURCE slots of ``src_hw`` pixels with
    ``scale_factor`` set -- the step's first launch, lama_resize_u8_fwd, then builds the loader's rescaled, padded fp32 image and 0 / 1 mask on
    the device and the fp32 chain (mask compose, generator, blend, u8 quantisation) runs on them; fp32 NCHW tensors the caller made
    (``u8_input=False``).  Every mode serves every form; in 'graph' the resize is one more kernel node of the captured step.

    ``paste_back`` (with ``scale_factor`` only; no counterpart in the reference, which writes the scaled image): the step ends with
    lama_paste_back_u8_fwd instead of the u8 quantisation -- the fp32 ``inpainted`` of the scaled step resampled bilinearly to each image's
    source grid and pasted into the decoded original (still on the device, in the source slots) wherever its mask is not 0.  The result sets are
    then source slots [n, Hs, Ws, 3], and every source pixel outside the mask comes back byte for byte.

    ``encode_png`` (off by default; the u8 input forms): the step ends with lama_png_deflate_u8_fwd over its u8 results -- the zlib stream of every
    image's PNG (Sub filter, literal-only dynamic Huffman chunks: tests/png_ref.py), cropped by the sizes array of the form (the scaled sizes with
    ``scale_factor``, the source sizes with ``paste_back``).  The result sets are then ONE flat u8 buffer per parity, ``n`` stream slots of
    ``png_slot`` bytes followed by the ``n`` int32 lengths (``d_out`` on the device, ``h_out`` pinned): one D2H, or one gather, carries both, the u8
    images are not downloaded (``h_u8`` is None) and ``result_png(p, j)`` is the j-th stream.  ``predict.png_from_zlib`` wraps it into the file.

    ``encode_jpeg`` (off by default; the u8 input forms; not together with ``encode_png``): the step ends with lama_jpeg_scan_u8_fwd instead -- the
    entropy-coded scan of every image's baseline JPEG at ``jpeg_quality`` and ``jpeg_subsampling`` ('420' / '444'; tests/jpeg_ref.py), cropped by the
    same sizes array.  The result sets are laid out as the PNG ones: ``n`` scan slots of ``jpeg_slot`` = ``jpeg_out_stride`` bytes (default: the
    slot's raw byte count Hs Ws 3), then, from byte ``jpeg_len_at`` on, the ``n`` int32 lengths.  ``result_jpeg(p, j)`` is the j-th scan;
    a scan that did not fit its slot (a negative length: noise at quality 100) raises JpegOverflow.  ``predict.jpeg_from_scan`` adds the headers.

    ``crop`` (crop_to_mask; not with ``scale_factor`` or out_key 'predicted_image'; no counterpart in the reference): source slots of ``src_hw``
    pixels up and down as in the ``scale_factor`` + ``paste_back`` form, and ``put`` takes a window (y0, x0, ch, cw) per image beside them (a
    pinned and a device ``rects`` array next to the sizes).  (Hp, Wp) is the padded size of the WINDOWS: the step is lama_crop_compose_u8_fwd, the
    generator call of the u8 form at that shape, lama_crop_paste_u8_fwd (model.forward_u8_crop) -- the u8 step on the cropped arrays, pasted into
    the source by slicing, byte for byte.  ``crop_sizes`` are the source sizes, so both encoders work on the pasted result unchanged.

    ``crop_shrink`` (crop_max_side; with ``crop``; no counterpart in the reference): ``put`` takes (y0, x0, ch, cw, k), and (Hp, Wp) is the padded size
    of the windows SHRUNK by their k (ceil(ch / k) x ceil(cw / k)): the step is lama_crop_shrink_compose_u8_fwd (k x k box means, the max of each
    box's mask bytes), the generator at that shape with its dense tail, lama_crop_shrink_paste_u8_fwd (model.forward_u8_crop_shrink): under the
    mask the results hold the k-fold bilinear upsampling of the prediction.  Everything else is as with ``crop``."""

    def __init__(self, model, batch_size: int, Hp: int, Wp: int, device, *, drain: bool = True, binarize: bool = True, mode: str = 'auto',
                 u8_input: bool = True, tune: bool = True, out_key: str = 'inpainted', capture: bool = True, scale_factor: Optional[float] = None,
                 src_hw: Optional[Tuple[int, int]] = None, paste_back: bool = False, encode_png: bool = False,
                 encode_jpeg: bool = False, jpeg_quality: int = 95, jpeg_subsampling='420', jpeg_out_stride: Optional[int] = None,
                 crop: bool = False, crop_shrink: bool = False):
        self.model, self.n, self.Hp, self.Wp = model, int(batch_size), int(Hp), int(Wp)
        # ``crop`` (crop_to_mask): the fourth input form -- the DECODED u8 originals in source slots of ``src_hw`` pixels plus a window per image;
        # (Hp, Wp) is the padded size of the WINDOWS, and the results are source slots
        self.crop = bool(crop)
        # ``crop_shrink`` (crop_max_side): the crop form with a shrink k per window -- (Hp, Wp) is the padded LOW-RESOLUTION size of the windows
        self.crop_shrink = bool(crop_shrink)
        if self.crop_shrink and not self.crop:
            raise L.LamaError('crop_shrink is a variant of the crop form: crop=True is needed')
        if self.crop_shrink and not hasattr(model, 'forward_u8_crop_shrink'):
            raise L.LamaError('crop_shrink needs model.forward_u8_crop_shrink')
        if self.crop:
            if scale_factor is not None:
                raise L.LamaError('crop with scale_factor is not served: the window is inpainted at the source resolution')
            if out_key != 'inpainted':
                raise L.LamaError(f"crop with out_key {out_key!r}: the pasted result is made from 'inpainted'")
            if not u8_input or not hasattr(model, 'forward_u8_crop'):
                raise L.LamaError('crop is a u8 input form (model.forward_u8_crop): not with u8_input=False')
            if src_hw is None or int(src_hw[0]) < 1 or int(src_hw[1]) < 1:
                raise L.LamaError(f'crop: src_hw = (Hs, Ws), the source slot size, is needed (got {src_hw!r})')
            self.Hs, self.Ws = int(src_hw[0]), int(src_hw[1])
        # ``scale_factor`` (dataset.scale_factor, evaluation/data.py:74-77): the third input form -- the step is fed with the DECODED u8 originals in
        # source slots of ``src_hw`` = (Hs, Ws) pixels, and its first launch (lama_resize_u8_fwd) does / 255, the INTER_AREA / INTER_NEAREST
        # rescale, the symmetric padding and mask > 0 on the device; (Hp, Wp) is the padded SCALED size
        self.scale = None if scale_factor is None else float(scale_factor)
        if self.scale is not None:
            if not self.scale > 0:
                raise L.LamaError(f'scale_factor {scale_factor!r}: a positive factor')
            if src_hw is None or int(src_hw[0]) < 1 or int(src_hw[1]) < 1:
                raise L.LamaError(f'scale_factor={scale_factor}: src_hw = (Hs, Ws), the source slot size, is needed (got {src_hw!r})')
            self.Hs, self.Ws = int(src_hw[0]), int(src_hw[1])
        if out_key not in ('inpainted', 'predicted_image'):                        # bin/predict.py:86: batch[predict_config.out_key]
            raise L.LamaError(f"out_key {out_key!r}: 'inpainted' or 'predicted_image'")
        self.out_key = out_key
        self.paste_back = bool(paste_back)
        if self.paste_back and self.scale is None:
            raise L.LamaError('paste_back needs scale_factor: without one the result has the source size already')
        if self.paste_back and out_key != 'inpainted':
            raise L.LamaError(f"paste_back with out_key {out_key!r}: the pasted result is made from 'inpainted' ('predicted_image' is undefined "
                              f"where the mask is 0)")
        self.device = torch.device(device)
        self.on_gpu = self.device.type == 'cuda'
        self.drain, self.binarize = drain, binarize
        if mode not in ('auto', 'replay', 'streams', 'graph', 'host'):
            raise L.LamaError(f'HostFedStep mode {mode!r}: auto, replay, streams, graph or host')
        self.one_part = False
        if mode == 'auto' and not capture:
            # a bucket of a few rounds (round 6, third session): not even ONE graph capture -- the one-part plan as plain launches beside
            # the copy streams (a warm-up + capture + instantiate is 10-40 ms per new shape, tools/newshape_probe.py; the ~270 launches of a step
            # cost the host 3 ms, less than the step takes on the GPU at any size)
            mode, self.one_part = 'streams', True
        elif mode == 'auto' and not tune:
            # a bucket of tens to hundreds of rounds: the one-part plan, captured once, in the host-synchronised form -- tune_split's two plans, two
            # captures and 18 replays (~0.35 s) buy at most 5 % of the bucket's time
            mode, self.one_part = ('host' if self.on_gpu else 'replay'), True
        if mode == 'auto':      # by measurement (table above): copy nodes overlap only in a graph that has parallel kernel branches already
            if self.on_gpu:
                # (the generator verifies once per shape that this runtime runs the parts side by side: FFCResNetGenerator.verify_split)
                with _settings(model.generator, _assume_graph=True):
                    model.generator.tune_split((self.n, 4, Hp, Wp), self.device)
            mode = 'host' if self.on_gpu else 'replay'       # round 6 (u8 copies): the host-synchronised copy streams beside whichever plan won, 0.999 of the resident rate (profiles/r06_host_fed.txt)
        self.mode = mode
        pin = dict(pin_memory=True) if self.on_gpu else {}
        # round 6: the step is fed with what is on disk -- u8 HWC image, u8 mask, (h, w) per image: 4 bytes per pixel over PCIe instead of 16, no
        # float conversion / padding on the host (forward_u8).  ``u8_input=False`` keeps the fp32 NCHW form of round 5 (A/B runs, callers with float data).
        self.u8_input = bool(u8_input) and hasattr(model, 'forward_u8') and self.scale is None and not self.crop
        self.h_dsizes = self.d_dsizes = None
        self.h_rects = self.d_rects = None
        self.h_shrinks = self.d_shrinks = None
        if self.crop:
            self.h_img = [torch.zeros(self.n, self.Hs, self.Ws, 3, dtype=torch.uint8, **pin) for _ in range(2)]
            self.h_mask = [torch.zeros(self.n, self.Hs, self.Ws, dtype=torch.uint8, **pin) for _ in range(2)]
            self.h_sizes = [torch.zeros(self.n, 2, dtype=torch.int32, **pin) for _ in range(2)]           # (h, w) of each source image
            self.h_rects = [torch.zeros(self.n, 4, dtype=torch.int32, **pin) for _ in range(2)]           # (y0, x0, ch, cw): its window
            self.d_img = [torch.zeros(self.n, self.Hs, self.Ws, 3, dtype=torch.uint8, device=self.device) for _ in range(2)]
            self.d_mask = [torch.zeros(self.n, self.Hs, self.Ws, dtype=torch.uint8, device=self.device) for _ in range(2)]
            self.d_sizes = [torch.zeros(self.n, 2, dtype=torch.int32, device=self.device) for _ in range(2)]
            self.d_rects = [torch.zeros(self.n, 4, dtype=torch.int32, device=self.device) for _ in range(2)]
            if self.crop_shrink:
                self.h_shrinks = [torch.zeros(self.n, dtype=torch.int32, **pin) for _ in range(2)]        # k: its window's shrink
                self.d_shrinks = [torch.zeros(self.n, dtype=torch.int32, device=self.device) for _ in range(2)]
        elif self.scale is not None:
            self.h_img = [torch.zeros(self.n, self.Hs, self.Ws, 3, dtype=torch.uint8, **pin) for _ in range(2)]
            self.h_mask = [torch.zeros(self.n, self.Hs, self.Ws, dtype=torch.uint8, **pin) for _ in range(2)]
            self.h_sizes = [torch.zeros(self.n, 2, dtype=torch.int32, **pin) for _ in range(2)]           # (h, w) of each source image
            self.h_dsizes = [torch.zeros(self.n, 2, dtype=torch.int32, **pin) for _ in range(2)]          # scaled_size of it
            self.d_img = [torch.zeros(self.n, self.Hs, self.Ws, 3, dtype=torch.uint8, device=self.device) for _ in range(2)]
            self.d_mask = [torch.zeros(self.n, self.Hs, self.Ws, dtype=torch.uint8, device=self.device) for _ in range(2)]
            self.d_sizes = [torch.zeros(self.n, 2, dtype=torch.int32, device=self.device) for _ in range(2)]
            self.d_dsizes = [torch.zeros(self.n, 2, dtype=torch.int32, device=self.device) for _ in range(2)]
            # the loader's fp32 tensors exist on the device only (one set: the steps of both parities run in order on one stream)
            self.f_img = torch.zeros(self.n, 3, Hp, Wp, dtype=torch.float32, device=self.device)
            self.f_mask = torch.zeros(self.n, 1, Hp, Wp, dtype=torch.float32, device=self.device)
        elif self.u8_input:
            self.h_img = [torch.zeros(self.n, Hp, Wp, 3, dtype=torch.uint8, **pin) for _ in range(2)]
            self.h_mask = [torch.zeros(self.n, Hp, Wp, dtype=torch.uint8, **pin) for _ in range(2)]
            self.h_sizes = [torch.zeros(self.n, 2, dtype=torch.int32, **pin) for _ in range(2)]
            self.d_img = [torch.zeros(self.n, Hp, Wp, 3, dtype=torch.uint8, device=self.device) for _ in range(2)]
            self.d_mask = [torch.zeros(self.n, Hp, Wp, dtype=torch.uint8, device=self.device) for _ in range(2)]
            self.d_sizes = [torch.zeros(self.n, 2, dtype=torch.int32, device=self.device) for _ in range(2)]
        else:
            self.h_img = [torch.zeros(self.n, 3, Hp, Wp, dtype=torch.float32, **pin) for _ in range(2)]
            self.h_mask = [torch.zeros(self.n, 1, Hp, Wp, dtype=torch.float32, **pin) for _ in range(2)]
            self.d_img = [torch.zeros(self.n, 3, Hp, Wp, dtype=torch.float32, device=self.device) for _ in range(2)]
            self.d_mask = [torch.zeros(self.n, 1, Hp, Wp, dtype=torch.float32, device=self.device) for _ in range(2)]
            self.h_sizes = self.d_sizes = None
        self.out_hw = (self.Hs, self.Ws) if self.paste_back or self.crop else (self.Hp, self.Wp)       # paste_back / crop: the results are source slots
        self.encode_png = bool(encode_png)
        self.u8 = [torch.zeros(self.n, *self.out_hw, 3, dtype=torch.uint8, device=self.device) for _ in range(2)]
        if self.encode_png:
            # the step ends with lama_png_deflate_u8_fwd over u8[p]: ONE flat u8 buffer per parity -- n stream slots, then the n int32 lengths -- is
            # what the D2H (or the gather) carries; the u8 images stay on the device
            if self.d_sizes is None:
                raise L.LamaError('encode_png needs a u8 input form (its crops are the step\'s device sizes array): not with u8_input=False')
            lib = model.generator._exec.lib
            ws_bytes = lib.png_deflate_workspace_bytes(self.n, *self.out_hw, 3, 0)       # (raises for result slots whose row is beyond 65535 bytes)
            self.png_slot = (lib.png_deflate_bound(*self.out_hw, 3, 0) + 15) & ~15
            self.png_bytes = self.n * self.png_slot + 4 * self.n
            self.png = [torch.zeros(self.png_bytes, dtype=torch.uint8, device=self.device) for _ in range(2)]
            self.h_png = [torch.zeros(self.png_bytes, dtype=torch.uint8, **pin) for _ in range(2)] if drain else None
            self.png_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)       # one: the steps of both parities run in order on one stream
            self.h_u8 = None
            self.d_out, self.h_out = self.png, self.h_png
        elif not encode_jpeg:
            self.h_u8 = [torch.zeros(self.n, *self.out_hw, 3, dtype=torch.uint8, **pin) for _ in range(2)] if drain else None
            self.d_out, self.h_out = self.u8, self.h_u8      # what the D2H branch (or the caller's gather) carries
        self.encode_jpeg = bool(encode_jpeg)
        if self.encode_jpeg:
            # the step ends with lama_jpeg_scan_u8_fwd over u8[p]; the result set is laid out as the PNG one: n scan slots, then the n int32 lengths
            if self.encode_png:
                raise L.LamaError('encode_jpeg and encode_png exclude each other: a step ends with one encoder')
            if self.d_sizes is None:
                raise L.LamaError('encode_jpeg needs a u8 input form (its crops are the step\'s device sizes array): not with u8_input=False')
            self.jpeg_quality, self.jpeg_subsampling = int(jpeg_quality), ljpeg.subsampling_code(jpeg_subsampling)
            if not 1 <= self.jpeg_quality <= 100:
                raise L.LamaError(f'jpeg_quality {jpeg_quality!r}: 1 .. 100')
            lib = model.generator._exec.lib
            ws_bytes = lib.jpeg_scan_workspace_bytes(self.n, *self.out_hw, self.jpeg_subsampling)      # (raises for slots beyond 65535 pixels a side)
            self.jpeg_slot = int(jpeg_out_stride) if jpeg_out_stride is not None else self.out_hw[0] * self.out_hw[1] * 3
            if self.jpeg_slot < 1:
                raise L.LamaError(f'jpeg_out_stride {jpeg_out_stride!r}: at least one byte')
            self.jpeg_len_at = (self.n * self.jpeg_slot + 15) & ~15
            self.jpeg_bytes = self.jpeg_len_at + 4 * self.n
            self.jpeg = [torch.zeros(self.jpeg_bytes, dtype=torch.uint8, device=self.device) for _ in range(2)]
            self.h_jpeg = [torch.zeros(self.jpeg_bytes, dtype=torch.uint8, **pin) for _ in range(2)] if drain else None
            self.jpeg_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)      # one: the steps of both parities run in order on one stream
            self.h_u8 = None
            self.d_out, self.h_out = self.jpeg, self.h_jpeg
        self.graphs = [None, None]
        self.span_events = None       # a list: launch() (mode 'host') appends (start, end) timing events around each step's compute
        self.done = [torch.cuda.Event() for _ in range(2)] if self.on_gpu else None
        self._launched = [False, False]
        self._h2d_issued = [False, False]
        if self.on_gpu:
            self.h2d = [torch.cuda.Event() for _ in range(2)]
            self.d2h = [torch.cuda.Event() for _ in range(2)]
            self.s_in, self.s_out = torch.cuda.Stream(device=self.device), torch.cuda.Stream(device=self.device)

    # -- host views -----------------------------------------------------------------------------------------------
    def host(self, p: int):
        """The pinned host set p as numpy views: (image, mask) -- u8 [n,Hp,Wp,3] / [n,Hp,Wp] (``u8_input``; ``put`` fills them), u8 source slots
        [n,Hs,Ws,3] / [n,Hs,Ws] (``scale_factor``) or fp32 NCHW."""
        return self.h_img[p].numpy(), self.h_mask[p].numpy()

    def put(self, p: int, j: int, image: Optional[np.ndarray], mask: Optional[np.ndarray], rect=None):
        """``u8_input``: image j of host set p = a decoded u8 HWC image [h,w,3] + u8 mask [h,w] (top-left corner of the slot), or None: an empty
        slot of a partial batch.  ``scale_factor``: the same pair, the decoded ORIGINAL, into its source slot.  ``crop``: the same, with ``rect`` =
        (y0, x0, ch, cw), the window the generator sees (``crop_rect``); a window that does not fit is refused here."""
        if self.crop:
            sz, rc = self.h_sizes[p].numpy(), self.h_rects[p].numpy()
            if image is None:
                sz[j], rc[j] = (0, 0), (0, 0, 0, 0)
                if self.crop_shrink:
                    self.h_shrinks[p].numpy()[j] = 0
                return
            h, w = image.shape[:2]
            if self.crop_shrink:                                                                    # ``crop_shrink``: rect = (y0, x0, ch, cw, k)
                if rect is None or len(rect) < 5 or not shrink_rect_fits(rect, h, w, self.Hs, self.Ws, self.Hp, self.Wp):
                    raise L.LamaError(f'window and shrink {None if rect is None else tuple(int(v) for v in rect[:5])} of a {h}x{w} image do not fit it, '
                                      f'the source slot {self.Hs}x{self.Ws} or the low-resolution bucket {self.Hp}x{self.Wp}')
                self.h_shrinks[p].numpy()[j] = int(rect[4])
            elif rect is None or len(rect) < 4 or not rect_fits(rect, h, w, self.Hs, self.Ws, self.Hp, self.Wp):     # (the kernels cannot report it)
                raise L.LamaError(f'window {None if rect is None else tuple(int(v) for v in rect[:4])} of a {h}x{w} image does not fit it, the source '
                                  f'slot {self.Hs}x{self.Ws} or the bucket {self.Hp}x{self.Wp}')
            self.h_img[p].numpy()[j, :h, :w] = image
            self.h_mask[p].numpy()[j, :h, :w] = mask
            sz[j], rc[j] = (h, w), tuple(int(v) for v in rect[:4])
            return
        if rect is not None:
            raise L.LamaError('put: a window is an operand of the crop form only')
        if self.scale is not None:
            sz, dz = self.h_sizes[p].numpy(), self.h_dsizes[p].numpy()
            if image is None:
                sz[j] = dz[j] = (0, 0)
                return
            h, w = image.shape[:2]
            dh, dw = scaled_size(h, w, self.scale)
            if dh <= 0 or dw <= 0:
                raise L.LamaError(f'scale_factor {self.scale}: a {w}x{h} image scales to nothing')
            if h > self.Hs or w > self.Ws or dh > self.Hp or dw > self.Wp:       # (the kernel cannot report it: the sizes are device data there)
                raise L.LamaError(f'image {h}x{w} (scaled {dh}x{dw}) does not fit the source slot {self.Hs}x{self.Ws} / the bucket {self.Hp}x{self.Wp}')
            self.h_img[p].numpy()[j, :h, :w] = image
            self.h_mask[p].numpy()[j, :h, :w] = mask
            sz[j], dz[j] = (h, w), (dh, dw)
            return
        if not self.u8_input:
            # fp32 NCHW form (callers with float data): image [3,Hp,Wp] / mask [1,Hp,Wp] float32 as ``load_item`` returns them, already padded;
            # an empty slot is zeros
            hi, hm = self.h_img[p].numpy(), self.h_mask[p].numpy()
            if image is None:
                hi[j] = 0
                hm[j] = 0
                return
            if tuple(image.shape) != (3, self.Hp, self.Wp) or tuple(mask.shape) != (1, self.Hp, self.Wp):
                raise L.LamaError(f'image {tuple(image.shape)} / mask {tuple(mask.shape)}: padded [3,{self.Hp},{self.Wp}] / [1,{self.Hp},{self.Wp}] float32')
            hi[j] = image
            hm[j] = mask
            return
        sz = self.h_sizes[p].numpy()
        if image is None:
            sz[j] = (0, 0)
            return
        h, w = image.shape[:2]
        if h > self.Hp or w > self.Wp:
            raise L.LamaError(f'image {h}x{w} does not fit the bucket {self.Hp}x{self.Wp}')
        self.h_img[p].numpy()[j, :h, :w] = image
        self.h_mask[p].numpy()[j, :h, :w] = mask
        sz[j] = (h, w)

    def result(self, p: int) -> np.ndarray:
        if self.encode_png:
            raise L.LamaError('encode_png: the u8 results are not downloaded; result_png(p, j) is the j-th stream')
        if self.encode_jpeg:
            raise L.LamaError('encode_jpeg: the u8 results are not downloaded; result_jpeg(p, j) is the j-th scan')
        return self.h_u8[p].numpy()

    def result_jpeg(self, p: int, j: int) -> memoryview:
        """``encode_jpeg``: the scan of image j of host result set p (empty for an empty slot), a view of the pinned set; JpegOverflow, naming the
        image, where the scan did not fit its slot."""
        return memoryview(jpeg_stream_view(self.h_jpeg[p].numpy(), self.jpeg_slot, self.jpeg_len_at, j, f'image {j} of result set {p}'))

    def result_png(self, p: int, j: int) -> memoryview:
        """``encode_png``: the zlib stream of image j of host result set p (empty for an empty slot), a view of the pinned set."""
        flat = self.h_png[p].numpy()
        n = int(flat[self.n * self.png_slot:].view(np.int32)[j])
        return memoryview(flat[j * self.png_slot:j * self.png_slot + n])

    def crop_sizes(self, p: int) -> np.ndarray:
        """(h, w) per image of the results computed from host input set p, as ``put`` recorded them: the scaled sizes with ``scale_factor``, the
        source sizes with ``paste_back`` or without a factor.  Valid until that host set is filled again."""
        return (self.h_dsizes if self.scale is not None and not self.paste_back else self.h_sizes)[p].numpy()

    def _encode(self, p: int):
        """``encode_png`` / ``encode_jpeg``: the encoder's launches over u8[p], cropped by the device sizes array of the form."""
        sizes = self.d_dsizes[p] if self.scale is not None and not self.paste_back else self.d_sizes[p]
        stream = torch.cuda.current_stream(self.device).cuda_stream if self.on_gpu else 0
        if self.encode_jpeg:
            flat = self.jpeg[p]
            self.model.generator._exec.lib.jpeg_scan_u8(self.u8[p], sizes, flat[:self.n * self.jpeg_slot], self.jpeg_slot,
                                                        flat[self.jpeg_len_at:].view(torch.int32), self.jpeg_ws, self.n, quality=self.jpeg_quality,
                                                        subsampling=self.jpeg_subsampling, stream=stream)
            return
        flat = self.png[p]
        self.model.generator._exec.lib.png_deflate_u8(self.u8[p], sizes, flat[:self.n * self.png_slot], self.png_slot,
                                                      flat[self.n * self.png_slot:].view(torch.int32), self.png_ws, self.n, stream=stream)

    # -- pieces ---------------------------------------------------------------------------------------------------
    def _compute(self, p: int):
        self._compute_u8(p)
        if self.encode_png or self.encode_jpeg:
            self._encode(p)

    def _compute_u8(self, p: int):
        lib = self.model.generator._exec.lib
        if self.crop:                                                                              # the same step on each image's window, pasted into the source slots
            with torch.no_grad():
                if self.crop_shrink:                                                               # ... shrunk by k for the generator, upsampled under the mask
                    self.model.forward_u8_crop_shrink(self.d_img[p], self.d_mask[p], self.d_sizes[p], self.d_rects[p], self.d_shrinks[p], self.u8[p],
                                                      self.Hp, self.Wp, binarize=self.binarize)
                    return
                self.model.forward_u8_crop(self.d_img[p], self.d_mask[p], self.d_sizes[p], self.d_rects[p], self.u8[p], self.Hp, self.Wp, binarize=self.binarize)
            return
        if self.u8_input:                                                                          # bin/predict.py:82-92 in two elementwise launches + the generator
            with torch.no_grad():
                self.model.forward_u8(self.d_img[p], self.d_mask[p], self.d_sizes[p], self.u8[p], binarize=self.binarize, out_key=self.out_key)
            return
        if self.scale is not None:                                                                 # data.py:69-83 + bin/predict.py:84 in one launch: fp32 image / mask
            stream = torch.cuda.current_stream(self.device).cuda_stream if self.on_gpu else 0
            lib.resize_u8(self.d_img[p], self.d_mask[p], self.d_sizes[p], self.d_dsizes[p], self.scale, L.view(self.f_img), L.view(self.f_mask), self.n,
                          binarize=self.binarize, stream=stream)
            batch = dict(image=self.f_img, mask=self.f_mask)
        else:
            mask = self.d_mask[p]
            batch = dict(image=self.d_img[p], mask=(mask > 0) * 1 if self.binarize else mask)      # bin/predict.py:84
        keep = self.model.keep_predicted_image
        self.model.keep_predicted_image = False
        try:
            with torch.no_grad():
                out = self.model(batch)[self.out_key]                                            # bin/predict.py:85-86
        finally:
            self.model.keep_predicted_image = keep
        stream = torch.cuda.current_stream(self.device).cuda_stream if self.on_gpu else 0
        if self.paste_back:     # the scaled result back on the source grid, inside the source image (the originals are still in their slots)
            lib.paste_back_u8(self.d_img[p], self.d_mask[p], self.d_sizes[p], self.d_dsizes[p], L.view(out), self.u8[p], self.n,
                              binarize=self.binarize, stream=stream)
            return
        lib.quantize_u8_hwc(L.view(out), self.u8[p], self.n, self.Hp, self.Wp, stream)             # bin/predict.py:92 on the device

    def _upload(self, q: int, non_blocking: bool):
        """H2D of input set q on the current stream: image, mask and -- the u8 forms -- the per-image sizes."""
        self.d_img[q].copy_(self.h_img[q], non_blocking=non_blocking)
        self.d_mask[q].copy_(self.h_mask[q], non_blocking=non_blocking)
        if self.d_sizes is not None:
            self.d_sizes[q].copy_(self.h_sizes[q], non_blocking=non_blocking)
        if self.d_dsizes is not None:
            self.d_dsizes[q].copy_(self.h_dsizes[q], non_blocking=non_blocking)
        if self.d_rects is not None:
            self.d_rects[q].copy_(self.h_rects[q], non_blocking=non_blocking)
        if self.d_shrinks is not None:
            self.d_shrinks[q].copy_(self.h_shrinks[q], non_blocking=non_blocking)

    def _body(self, p: int):
        q = 1 - p
        if not self.on_gpu:
            self._upload(q, False)
            if self.drain:
                self.h_out[q].copy_(self.d_out[q])
            self._compute(p)
            return
        main = torch.cuda.current_stream(self.device)
        self.s_in.wait_stream(main)
        with torch.cuda.stream(self.s_in):
            self._upload(q, True)
        if self.drain:
            self.s_out.wait_stream(main)
            with torch.cuda.stream(self.s_out):
                self.h_out[q].copy_(self.d_out[q], non_blocking=True)
        self._compute(p)
        main.wait_stream(self.s_in)
        if self.drain:
            main.wait_stream(self.s_out)

    def _generator(self, use_graph: bool):
        """The generator's settings while a step is issued: no flag read-back per forward (``predict`` asks ``check_range`` per bucket), the
        one-part plan where this step decided so."""
        one_part = dict(split_batch=1) if self.one_part else {}
        return _settings(self.model.generator, use_graph=use_graph, defer_range_check=True, **one_part)

    def _capture(self, p: int):
        # the plan's launches go into THIS graph, with no flag read-back (a host sync) inside it; _assume_graph: so the plan may be the split
        # one although generator.use_graph is off
        with _settings(self.model.generator, use_graph=False, defer_range_check=True, _assume_graph=True):
            if self.graphs[1 - p] is None:                       # first capture: pack the weights / build the plan outside it
                side = torch.cuda.Stream(device=self.device)
                side.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(side):
                    self._compute(p)
                torch.cuda.current_stream(self.device).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            # thread_local: RCCL's watchdog thread polls events of the gather that may still be in flight on the side stream
            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                self._body(p)
            self.graphs[p] = g

    # -- the caller's four verbs ----------------------------------------------------------------------------------
    def prime(self, p: int):
        """H2D of host set p on the current stream (before the first launch of a run) and a host wait for it: the caller refills that host
        set for the batch after next before any ``wait`` has covered this copy."""
        self._upload(p, self.on_gpu)
        if self.on_gpu:
            torch.cuda.current_stream(self.device).synchronize()

    def launch(self, p: int):
        if not self.on_gpu:
            with _settings(self.model.generator, defer_range_check=True):
                self._body(p)
            return
        if self.mode == 'host':
            # round 6: NO device-side fork / join between the queues.  The compute of this batch is queued first (behind nothing but the event of
            # its own upload, issued a step ago and long complete); then the HOST waits for the previous step -- the last reader of device set
            # 1 - p and the producer of u8[1 - p] -- and only then queues the next upload and the previous download on the copy streams, which
            # therefore need no barrier against the compute queue.  With 4 bytes per pixel up and 3 down the copies are ~0.3 ms of a 9.7 ms step:
            # the cross-queue dependencies of the other forms cost more than that (profiles/r06_host_fed.txt).
            q = 1 - p
            main = torch.cuda.current_stream(self.device)
            with self._generator(use_graph=True):
                if self._h2d_issued[p]:
                    main.wait_event(self.h2d[p])
                if self.span_events is not None:       # profile=true: the step's span on the GPU clock
                    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    ev[0].record(main)
                self._compute(p)
                if self.span_events is not None:
                    ev[1].record(main)
                    self.span_events.append(ev)
            self.done[p].record(main)
            if self._launched[q]:
                self.done[q].synchronize()               # host: step k - 1 is complete (step k is queued behind it: the GPU does not idle)
            with torch.cuda.stream(self.s_in):
                self._upload(q, True)
                self.h2d[q].record(self.s_in)
            self._h2d_issued[q] = True
            if self.drain:
                with torch.cuda.stream(self.s_out):
                    self.h_out[q].copy_(self.d_out[q], non_blocking=True)
                    self.d2h[q].record(self.s_out)
            self._launched[p] = True
            return
        if self.mode == 'graph':
            if self.graphs[p] is None:
                self._capture(p)
            self.graphs[p].replay()
        else:       # the two copies on streams of their own (fork / join by events) beside this batch's compute: the generator's own hipGraph
            with self._generator(use_graph=self.mode == 'replay'):          # replay ('replay') or its ~270 plain launches ('streams')
                self._body(p)
        self.done[p].record(torch.cuda.current_stream(self.device))
        self._launched[p] = True

    def wait(self, p: int):
        """Host: until the most recent launch(p) is complete (its H2D has read host set 1-p, its D2H has filled result(1-p))."""
        if self.on_gpu and self._launched[p]:
            self.done[p].synchronize()
            if self.mode == 'host':                      # ... and the copies that launch queued on the copy streams
                self.h2d[1 - p].synchronize()
                if self.drain:
                    self.d2h[1 - p].synchronize()

    def flush(self, p: int):
        """D2H of u8[p] (the last launch's own result: nothing follows to carry it) and a host wait for it."""
        if self.drain:
            self.h_out[p].copy_(self.d_out[p], non_blocking=self.on_gpu)
        if self.on_gpu:
            torch.cuda.current_stream(self.device).synchronize()
            if self.mode == 'host':
                self.s_in.synchronize()
                self.s_out.synchronize()


# ----------------------------------------------------------------------------------------------------------------
# the predict loop
# ----------------------------------------------------------------------------------------------------------------

def predict(model: trainers.DefaultInpaintingTrainingModule, items: List[Tuple[str, str]], indir: str, outdir: str, *,
            pad_mod: int = 8, batch_size: int = 8, out_ext: str = '.png', device='cuda', rank: int = 0, world: int = 1,
            dist=None, io_threads: int = 8, out_key: str = 'inpainted', scale_factor: Optional[float] = None, paste_back: bool = False,
            device_png: bool = False, device_jpeg: bool = False, jpeg_quality: int = 95, jpeg_subsampling='420',
            crop_to_mask: bool = False, crop_margin: int = 128, crop_step: int = 128, crop_max_side: int = 0) -> int:
    """Run every (mask, image) pair through ``model`` and write the results (rank 0).  Returns the number of images written.
    ``scale_factor`` = ``dataset.scale_factor`` (evaluation/data.py:74-77): every image / mask is rescaled before the padding -- on the device, by
    the first launch of the step, which is fed with the decoded u8 originals (lama_resize_u8_fwd) -- and the results have the rescaled size.
    ``paste_back`` (with ``scale_factor``): the results have the SOURCE size instead -- the source image, with the pixels under the mask taken from
    the scaled prediction resampled bilinearly (lama_paste_back_u8_fwd; the reference has no such output).
    ``device_png`` (``.png`` only, off by default): every step ends with the PNG's zlib stream made on the device (lama_png_deflate_u8_fwd); the D2H
    and, with several ranks, the gather carry the compressed bytes, and the host only wraps them (png_from_zlib: one CRC) and writes.  The files
    decode to the same pixels; their bytes differ from encode_png's.
    ``device_jpeg`` (``.jpg`` / ``.jpeg`` only, off by default, not with ``device_png``): every step ends with the JPEG's entropy-coded scan made on
    the device (lama_jpeg_scan_u8_fwd) at ``jpeg_quality`` / ``jpeg_subsampling``; the copies carry the flat set of scan slots (as large as the u8 set at the default slot size: what is saved is the host's encode) and the host adds the headers
    (jpeg_from_scan).  An image whose scan overflowed its slot is computed once more at the end of its bucket and encoded on the host.  With the
    option off a ``.jpg`` is PIL's, at PIL's defaults (quality 75).
    ``crop_to_mask`` (off by default; not with ``scale_factor`` or out_key 'predicted_image'; the reference has no such output): the generator runs
    on a window around each mask's bounding box (``crop_rect``: the box + ``crop_margin`` a side, rounded up to ``crop_step``) at the source
    resolution, and the results are the source images with the window's inpainted pixels pasted in on the device (lama_crop_paste_u8_fwd) -- the u8
    step on the cropped arrays, pasted by slicing.  The windows need the masks' pixels, so a pre-pass decodes every mask on the I/O pool before the
    buckets -- keyed by the windows' padded size -- are formed; every rank runs the whole pre-pass and so arrives at the same buckets.
    ``crop_max_side`` (with ``crop_to_mask``; 0 = off; no such output in the reference either): the pre-pass computes ``crop_rect_limited``; a window
    whose padded size exceeds the limit is shrunk by the smallest integer k that fits (box means of the image, the MAX of each box's mask bytes),
    the pixels under the mask are the k-fold bilinear upsampling of the prediction (lama_crop_shrink_compose_u8_fwd / lama_crop_shrink_paste_u8_fwd),
    and such windows form buckets of their own, keyed by their padded low-resolution size.  A window that fits (k = 1) is served as without the key.

    Host pipeline: the PNGs of round r + 1 are decoded / padded on the thread pool while round r computes, results are
    written on the same pool; a partial last batch of a bucket is zero-padded to ``batch_size`` so that it replays the bucket's
    captured plan instead of building (and capturing) a second one, and a bucket's plan is dropped when the bucket is done."""
    if crop_max_side and not crop_to_mask:     # as the CLI and the step (crop_shrink without crop) refuse it: the limit is not dropped silently
        raise L.LamaError(f'crop_max_side={crop_max_side!r} needs crop_to_mask: it limits the window that option inpaints')
    # no host synchronisation per forward: the fp16 split's range flag is read once per bucket, where every rank synchronises anyway
    with _settings(model.generator, defer_range_check=True):
        for _attempt in range(2):
            try:
                return _predict_once(model, items, indir, outdir, pad_mod=pad_mod, batch_size=batch_size, out_ext=out_ext, device=device,
                                     rank=rank, world=world, dist=dist, io_threads=io_threads, out_key=out_key, scale_factor=scale_factor,
                                     paste_back=paste_back, device_png=device_png,
                                     device_jpeg=(int(jpeg_quality), ljpeg.subsampling_code(jpeg_subsampling)) if device_jpeg else None,
                                     crop=(int(crop_margin), int(crop_step), int(crop_max_side)) if crop_to_mask else None)
            except _RangeRestart:
                continue                     # the generator switched to the 3-term bf16 split (every rank alike): all images again
        raise L.LamaError('range restart did not converge')


def _predict_once(model, items, indir, outdir, *, pad_mod, batch_size, out_ext, device, rank, world, dist, io_threads, out_key='inpainted', scale_factor=None,
                  paste_back=False, device_png=False, device_jpeg=None, crop=None) -> int:
    from PIL import Image

    def header_size(item):                   # padded shape from the IMAGE's PNG header only: every rank builds the same plan
        with Image.open(item[1]) as im:
            w, h = im.size
        return (h, w)

    masks: Dict[int, np.ndarray] = {}        # crop_to_mask: item -> its mask as the pre-pass decoded it, up to CROP_MASK_CACHE_BYTES in all
    room = [CROP_MASK_CACHE_BYTES]
    room_lock = threading.Lock()

    def mask_rect(i):                        # crop_to_mask: the window from the MASK's pixels (integers only: every rank computes the same one)
        mask = np.asarray(Image.open(items[i][0]).convert('L'))
        with room_lock:
            keep = room[0] >= mask.nbytes
            if keep:
                room[0] -= mask.nbytes
        if keep:
            masks[i] = mask
        if not crop[2]:
            return tuple(mask.shape), crop_rect(mask, crop[0], crop[1], pad_mod)
        try:                                 # crop_max_side: (y0, x0, ch, cw[, k]) and the bucket key (Hp, Wp[, 1]) -- k = 1: as without the limit
            y0, x0, ch, cw, k, _, _, Hp, Wp = crop_rect_limited(mask, crop[0], crop[1], pad_mod, crop[2])
        except L.LamaError as e:
            raise L.LamaError(f'{items[i][0]}: {e}; raise crop_max_side or use dataset.scale_factor with paste_back=true for this directory')
        return tuple(mask.shape), ((y0, x0, ch, cw, Hp, Wp) if k == 1 else (y0, x0, ch, cw, k, Hp, Wp, 1))

    if paste_back and scale_factor is None:
        raise L.LamaError('paste_back needs scale_factor: without one the result has the source size already')
    if crop is not None:
        if scale_factor is not None or out_key != 'inpainted':
            raise L.LamaError("crop_to_mask is not served with scale_factor or out_key 'predicted_image': the window is inpainted at the source "
                              "resolution and pasted from 'inpainted'")
        check_crop_options(crop[0], crop[1], pad_mod)
        check_crop_max_side(crop[2], crop[0], crop[1], pad_mod)
    if device_png and not out_ext.lower().endswith('.png'):
        raise L.LamaError(f'device_png writes PNG files only, not {out_ext!r}')
    if device_jpeg and (device_png or not out_ext.lower().endswith(('.jpg', '.jpeg'))):
        raise L.LamaError(f'device_jpeg writes JPEG files only (not {out_ext!r}) and excludes device_png')
    lib = model.generator._exec.lib
    pool = ThreadPoolExecutor(io_threads)
    # the copies into / out of the pinned sets are on the round loop's critical path (the next launch waits for them) and take 0.1-0.3 ms each: they
    # get workers of their own instead of queueing behind milliseconds of PNG work in ``pool``
    fast = ThreadPoolExecutor(min(4, max(1, io_threads)))
    try:
        src_sizes = list(pool.map(header_size, items, chunksize=64))   # (0.15 ms per file on the main thread was a tenth of a long directory's wall time)
        # dataset.scale_factor: results, buckets and crops have the SCALED size (data.py:74-79); the source sizes size each bucket's upload slots
        sizes = src_sizes if scale_factor is None else [scaled_size(h, w, scale_factor) for h, w in src_sizes]
        for (h, w), (sh, sw) in zip(sizes, src_sizes):
            if h <= 0 or w <= 0:
                raise L.LamaError(f'scale_factor {scale_factor}: a {sw}x{sh} image scales to nothing')
        shapes = [(ceil_modulo(h, pad_mod), ceil_modulo(w, pad_mod)) if pad_mod and pad_mod > 1 else (h, w) for h, w in sizes]
        rects = None
        if crop is not None:
            # the pre-pass: the windows need the masks' pixels, so every mask is decoded once here (on the I/O pool; every rank decodes them all and
            # arrives at the same buckets without a collective) and the buckets are keyed by the windows' padded size.  The decoded masks are kept
            # for the loads of the round loop as far as CROP_MASK_CACHE_BYTES goes; the others are decoded a second time there
            t_ = time.perf_counter()
            found = list(pool.map(mask_rect, range(len(items))))
            for item, hw, (mhw, _) in zip(items, src_sizes, found):
                if tuple(mhw) != tuple(hw):
                    raise L.LamaError(f'{item[0]}: mask is {mhw[1]}x{mhw[0]} but {item[1]} is {hw[1]}x{hw[0]}')
            rects = [r[:4] if len(r) == 6 else r[:5] for _, r in found]         # (a fifth value: the shrink k > 1 of crop_max_side)
            shapes = [r[4:] if len(r) == 6 else r[5:] for _, r in found]         # (a third value: the bucket of the shrunk windows of that size)
            LOOP_TIMES['crop_prepass'] = LOOP_TIMES.get('crop_prepass', 0.0) + time.perf_counter() - t_
        rounds = plan_rounds(shapes, batch_size, world)
        return _predict_rounds(model, items, indir, outdir, rounds, sizes, pool, lib, pad_mod=pad_mod, batch_size=batch_size, out_ext=out_ext,
                               device=device, rank=rank, world=world, dist=dist, out_key=out_key, fast=fast, scale_factor=scale_factor,
                               src_sizes=src_sizes, paste_back=paste_back, device_png=device_png, device_jpeg=device_jpeg, rects=rects, masks=masks)
    finally:
        fast.shutdown()
        pool.shutdown()                      # on every exit path (a raise out of a bucket included): no worker thread outlives the call


def _predict_rounds(model, items, indir, outdir, rounds, sizes, pool, lib, *, pad_mod, batch_size, out_ext, device, rank, world, dist, out_key='inpainted', fast=None,
                    scale_factor=None, src_sizes=None, paste_back=False, device_png=False, device_jpeg=None, rects=None, masks=None) -> int:
    """The rounds of one attempt.  Per bucket (padded shape) a ``HostFedStep``: round k computes from device input set k & 1 while the SAME graph
    launch uploads round k + 1's decoded images into the other set and (one rank) downloads round k - 1's u8 results; the host fills the
    pinned set of round k + 1 and queues round k - 2's PNG writes while round k runs.  Several ranks: the results go through the one
    collective -- ``gather_to_root`` of the u8 batch, on a side stream behind the step -- and rank 0 downloads the gathered rounds.
    ``paste_back``: the buckets stay keyed by the padded scaled size, but the u8 results (and the gathered rounds) are the bucket's source slots
    and each PNG is the h x w crop of its SOURCE size.
    ``rects`` (crop_to_mask: the window of every item): the buckets are keyed by the windows' padded size, the steps are ``HostFedStep(crop=True)`` over
    source slots that hold the bucket's largest source image, and results, gathered rounds and crops are as with ``paste_back``.  A round whose
    shape carries a third value (crop_max_side) belongs to a bucket of SHRUNK windows: its rects carry their k, its step has ``crop_shrink=True``.
    ``device_png``: a result set is the step's flat buffer (``batch_size`` stream slots, then their int32 lengths) per rank instead of the u8 images:
    the snapshot job copies the stream's bytes out of the pinned set and releases the latch, the pool job wraps and writes.
    ``device_jpeg`` = (quality, subsampling): the same with scans; an image whose scan did not fit its slot (JpegOverflow) is put aside, and at the
    end of its bucket rank 0 computes it once more in a plain u8 step, downloads it and encodes it on the host."""
    futures, written = [], 0                 # futures of the snapshot jobs; each returns the future of its encode + write
    fast = fast if fast is not None else pool
    bucket_paths: List[str] = []             # the PNGs queued for the bucket whose range flag has not been read yet

    def drain():
        for f in futures:
            f.result().result()

    on_gpu = torch.device(device).type == 'cuda'
    side = torch.cuda.Stream(device=device) if on_gpu else None     # gather + D2H of the gathered rounds, beside the next round's compute

    loads: Dict[int, list] = {}

    def submit_loads(r):
        if r < len(rounds) and r not in loads:
            # decode only: / 255, dataset.scale_factor's rescale, the padding and mask > 0 run on the device
            loads[r] = [pool.submit(load_item_u8, *items[i], masks.pop(i, None) if masks else None) for i in rounds[r]['batches'][rank]]

    snapped = [_Latch(), _Latch()]           # per pinned result set: the workers that still copy their image out of it
    png_slot = png_set = png_len_at = 0      # device_png / device_jpeg: bytes per stream slot / per rank's result buffer / in front of its lengths (current bucket)
    flat_sets = bool(device_png or device_jpeg)
    overflowed: List[Tuple[int, str]] = []   # device_jpeg: (item, path) of the scans that did not fit their slot in the current bucket
    crops = src_sizes if paste_back or rects is not None else sizes

    def write_round(rd, host, pset):
        """Rank 0: queue the PNG writes of one round from its u8 results on the host (``host`` = [ranks * batch_size, Hp, Wp, 3] = pinned result
        set ``pset``; ``paste_back``: [ranks * batch_size, Hs, Ws, 3]).  The workers snapshot their image themselves (the main thread only queues); ``snapped[pset].wait()`` before that set is
        downloaded into again."""
        nonlocal written
        host = host.reshape(-1) if flat_sets else host
        for r, idxs in enumerate(rd['batches']):
            for j, i in enumerate(idxs):
                mask_path = items[i][0]
                h, w = crops[i]
                rel = os.path.splitext(mask_path[len(indir):].lstrip(os.sep))[0] + out_ext      # bin/predict.py:69-72
                bucket_paths.append(os.path.join(outdir, rel))
                snapped[pset].add()
                if device_jpeg:
                    try:
                        view = jpeg_stream_view(host[r * png_set:(r + 1) * png_set], png_slot, png_len_at, j, mask_path)
                    except JpegOverflow:
                        snapped[pset].done()
                        overflowed.append((i, bucket_paths[-1]))
                        written += 1
                        continue
                    if view.size == 0:
                        snapped[pset].done()
                        raise L.LamaError(f'{mask_path}: the device encoder returned no scan for a {h}x{w} image')
                    futures.append(fast.submit(_snap_and_wrap_jpeg, bucket_paths[-1], view, h, w, *device_jpeg, snapped[pset], pool))
                elif device_png:
                    base = r * png_set + j * png_slot
                    n = int(host[r * png_set + png_len_at:(r + 1) * png_set].view(np.int32)[j])
                    if n <= 0:
                        snapped[pset].done()
                        raise L.LamaError(f'{mask_path}: the device encoder returned no stream for a {h}x{w} image')
                    futures.append(fast.submit(_snap_and_wrap, bucket_paths[-1], host[base:base + n], h, w, snapped[pset], pool))
                else:
                    futures.append(fast.submit(_snap_and_write, bucket_paths[-1], host[r * batch_size + j, :h, :w], snapped[pset], pool))
                written += 1

    submit_loads(0)
    submit_loads(1)
    r0 = 0
    while r0 < len(rounds):
        shape = rounds[r0]['shape']
        Hp, Wp = shape[:2]
        shrink = len(shape) > 2              # crop_max_side: the bucket of the windows shrunk to (Hp, Wp)
        r1 = r0
        while r1 < len(rounds) and rounds[r1]['shape'] == shape:
            r1 += 1
        K = r1 - r0
        t_ = time.perf_counter()
        src_hw = None
        if scale_factor is not None or rects is not None:             # the bucket's source slots hold its largest source image (every rank: the same plan, the same slots)
            members = [src_sizes[i] for rd in rounds[r0:r1] for b in rd['batches'] for i in b]
            src_hw = (max(h for h, _ in members), max(w for _, w in members))
        hs = HostFedStep(model, batch_size, Hp, Wp, device, drain=(world == 1), tune=(K >= TUNE_MIN_ROUNDS), capture=(K >= CAPTURE_MIN_ROUNDS), out_key=out_key,
                         scale_factor=scale_factor, src_hw=src_hw, paste_back=paste_back, encode_png=device_png, crop=rects is not None, crop_shrink=shrink,
                         **(dict(encode_jpeg=True, jpeg_quality=device_jpeg[0], jpeg_subsampling=device_jpeg[1], jpeg_out_stride=JPEG_OUT_STRIDE) if device_jpeg else {}))
        if device_png:
            png_slot, png_set, png_len_at = hs.png_slot, hs.png_bytes, batch_size * hs.png_slot
        if device_jpeg:
            png_slot, png_set, png_len_at = hs.jpeg_slot, hs.jpeg_bytes, hs.jpeg_len_at
        LOOP_TIMES['bucket_setup'] = LOOP_TIMES.get('bucket_setup', 0.0) + time.perf_counter() - t_
        if PROFILE_SPANS:
            hs.span_events = []
        gathered = h_out = None
        if world > 1 and rank == 0:
            set_shape = (world * png_set,) if flat_sets else (world * batch_size, *hs.out_hw, 3)      # device_png / device_jpeg: every rank's flat result buffer
            gathered = [torch.empty(*set_shape, dtype=torch.uint8, device=device) for _ in range(2)]
            h_out = [torch.zeros(*set_shape, dtype=torch.uint8, **(dict(pin_memory=True) if on_gpu else {})) for _ in range(2)]
        works = [None, None]
        collected = [torch.cuda.Event() for _ in range(2)] if (on_gpu and world > 1) else None

        def fill(pp, r):
            t_ = time.perf_counter()
            loaded = [f.result() for f in loads.pop(r)]
            mine = rounds[r]['batches'][rank]
            LOOP_TIMES['wait_decode'] = LOOP_TIMES.get('wait_decode', 0.0) + time.perf_counter() - t_
            t_ = time.perf_counter()

            def put(j):                                                               # partial (or, for a rank without a batch, empty) round: empty slots
                if j < len(loaded):
                    hs.put(pp, j, loaded[j][0], loaded[j][1], *(() if rects is None else (rects[mine[j]],)))
                else:
                    hs.put(pp, j, None, None)
            list(fast.map(put, range(batch_size)))                                    # the copies into the pinned set, side by side (distinct slots)
            LOOP_TIMES['fill_pinned'] = LOOP_TIMES.get('fill_pinned', 0.0) + time.perf_counter() - t_

        def collect(pp):
            """Several ranks: the round that launch(pp) just computed goes through the gather (side stream, behind the step); rank 0 downloads it."""
            snapped[pp].wait()                    # h_out[pp] is downloaded into again: round k - 2's images have been copied out of it
            if on_gpu:
                with torch.cuda.stream(side):
                    side.wait_event(hs.done[pp])
                    works[pp] = gather_to_root(dist, gathered[pp] if rank == 0 else None, hs.d_out[pp], rank, world)
                    works[pp].wait()                                                  # the side stream waits for RCCL's stream
                    if rank == 0:
                        h_out[pp].copy_(gathered[pp], non_blocking=True)
                    collected[pp].record(side)
            else:
                works[pp] = gather_to_root(dist, gathered[pp] if rank == 0 else None, hs.d_out[pp], rank, world)
                works[pp].wait()
                if rank == 0:
                    h_out[pp].copy_(gathered[pp])

        fill(0, r0)
        submit_loads(r0 + 2)
        t_ = time.perf_counter()
        hs.prime(0)
        LOOP_TIMES['bucket_setup'] += time.perf_counter() - t_
        for k in range(K):
            pp = k & 1
            if k + 1 < K:
                fill(1 - pp, r0 + k + 1)          # (the launch that last read this host set -- step k - 2 -- is complete: waited for below, at k - 1)
            submit_loads(r0 + k + 2)
            submit_loads(r0 + k + 3)
            if on_gpu and works[pp] is not None:
                torch.cuda.current_stream(hs.device).wait_event(collected[pp])        # step k - 2's gather has read u8[pp]
            t_ = time.perf_counter()
            snapped[1 - pp].wait()                # (one rank) this launch downloads into result set 1 - pp: round k - 3's images have been copied out of it
            hs.launch(pp)
            LOOP_TIMES['launch'] = LOOP_TIMES.get('launch', 0.0) + time.perf_counter() - t_
            if world > 1:
                collect(pp)
                if k >= 1:                        # round k - 1: gathered and downloaded while step k runs
                    if on_gpu:
                        collected[1 - pp].synchronize()
                    if rank == 0:
                        write_round(rounds[r0 + k - 1], h_out[1 - pp].numpy(), 1 - pp)
            elif k >= 1:
                t_ = time.perf_counter()
                hs.wait(1 - pp)                   # step k - 1 is complete: it downloaded round k - 2 and read the host set filled above
                LOOP_TIMES['wait_step'] = LOOP_TIMES.get('wait_step', 0.0) + time.perf_counter() - t_
                if k >= 2:
                    t_ = time.perf_counter()
                    write_round(rounds[r0 + k - 2], hs.h_out[pp].numpy(), pp)
                    LOOP_TIMES['queue_writes'] = LOOP_TIMES.get('queue_writes', 0.0) + time.perf_counter() - t_
        pl = (K - 1) & 1
        if world > 1:
            if on_gpu:
                collected[pl].synchronize()
            if rank == 0:
                write_round(rounds[r1 - 1], h_out[pl].numpy(), pl)
        else:
            hs.wait(pl)
            if K >= 2:
                write_round(rounds[r1 - 2], hs.h_out[1 - pl].numpy(), 1 - pl)
            snapped[pl].wait()
            hs.flush(pl)
            write_round(rounds[r1 - 1], hs.h_out[pl].numpy(), pl)
        if on_gpu:
            torch.cuda.current_stream(hs.device).synchronize()                      # every rank: the graphs / buffers below are idle now
            if hs.span_events:
                ev = hs.span_events
                LOOP_TIMES['gpu_step_spans'] = LOOP_TIMES.get('gpu_step_spans', 0.0) + sum(a.elapsed_time(b) for a, b in ev) * 1e-3
                LOOP_TIMES['gpu_first_start_to_last_end'] = LOOP_TIMES.get('gpu_first_start_to_last_end', 0.0) + ev[0][0].elapsed_time(ev[-1][1]) * 1e-3
                LOOP_TIMES['steps'] = LOOP_TIMES.get('steps', 0.0) + len(ev)

        if overflowed:                       # device_jpeg, rank 0: the images whose scan did not fit -- a plain u8 step, a download of their own, libjpeg
            fb = HostFedStep(model, batch_size, Hp, Wp, device, drain=True, tune=False, capture=False, out_key=out_key, scale_factor=scale_factor,
                             src_hw=src_hw, paste_back=paste_back, crop=rects is not None, crop_shrink=shrink)
            for c0 in range(0, len(overflowed), batch_size):
                part = overflowed[c0:c0 + batch_size]
                for j in range(batch_size):
                    fb.put(0, j, *(load_item_u8(*items[part[j][0]])[:2] if j < len(part) else (None, None)),
                           *((rects[part[j][0]],) if rects is not None and j < len(part) else ()))
                fb.prime(0)
                fb.launch(0)
                fb.wait(0)
                fb.flush(0)
                for j, (i, pth) in enumerate(part):
                    h, w = crops[i]
                    futures.append(fast.submit(pool.submit, _write_jpeg_host, pth, fb.result(0)[j, :h, :w].copy(), *device_jpeg))
            overflowed.clear()
            del fb
        # the bucket's ONE read-back of the fp16 split's range flag (the forwards above did not synchronise); all ranks decide alike
        def red(bad, _dev=hs.device):
            t = torch.tensor([1 if bad else 0], dtype=torch.int32, device=_dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return int(t.item()) != 0
        # The PNG writes of this bucket are already queued (they overlap the compute); the flag is read only now.  Out-of-range forwards
        # produced garbage images: with auto_fallback the restart overwrites every file, WITHOUT it check_range raises -- and the bucket's
        # files are removed first, so that a LamaRangeError never leaves bad output on disk.
        try:
            in_range = model.generator.check_range(hs.device, reduce=red if world > 1 else None)
        except L.LamaRangeError:
            drain()
            for pth in bucket_paths:
                if os.path.exists(pth):
                    os.remove(pth)
            raise
        if not in_range:
            drain()
            raise _RangeRestart()
        bucket_paths.clear()
        model.generator.drop_plan((batch_size, 4, Hp, Wp), hs.device)               # bucket done: free its buffers / graphs
        del hs, gathered, h_out
        r0 = r1
    drain()
    return written


def predict_refine(model, items: List[Tuple[str, str]], indir: str, outdir: str, cfg: dict, *, device='cuda', rank: int = 0,
                   world: int = 1) -> int:
    """``refine=True`` (bin/predict.py:75-81): one image at a time through lama_amd.refinement.refine_predict.  Each image's
    optimisation is sequential, so the ranks are plain replicas: rank r takes items r, r + world, ... and writes its own results
    (no collective on this path)."""
    from .refinement import refine_predict
    pad_mod = int(cfg['dataset.pad_out_to_modulo'])
    if int(cfg.get('refiner.batch_size', 1)) > 1:
        return _predict_refine_batched(model, items, indir, outdir, cfg, device=device, rank=rank, world=world)
    pool = ThreadPoolExecutor(4)
    futures, written = [], 0
    for i in range(rank, len(items), world):
        mask_path, img_path = items[i]
        image, mask, (h, w) = load_item(mask_path, img_path, pad_mod, cfg.get('dataset.scale_factor'))
        batch = dict(image=torch.from_numpy(image)[None].to(device), mask=torch.from_numpy(mask)[None].to(device),
                     unpad_to_size=[torch.tensor([h]), torch.tensor([w])])
        # bin/predict.py:75-81: the refine branch hands the RAW grayscale mask to refine_predict (line 84's binarisation belongs to the
        # plain branch only); the refiner thresholds it itself at every scale (refinement.py:212,304-305)
        cur_res = refine_predict(batch, model, gpu_ids=str(cfg['refiner.gpu_ids']), modulo=int(cfg['refiner.modulo']),
                                 n_iters=int(cfg['refiner.n_iters']), lr=float(cfg['refiner.lr']), min_side=int(cfg['refiner.min_side']),
                                 max_scales=int(cfg['refiner.max_scales']), px_budget=int(cfg['refiner.px_budget']))
        res = cur_res[0].permute(1, 2, 0).numpy()                                                          # bin/predict.py:80
        u8 = np.clip(res * 255, 0, 255).astype('uint8')                                                    # bin/predict.py:92
        rel = os.path.splitext(mask_path[len(indir):].lstrip(os.sep))[0] + cfg['out_ext']
        futures.append(pool.submit(_write_png, os.path.join(outdir, rel), u8))
        written += 1
    for f in futures:
        f.result()
    pool.shutdown()
    return written


def _predict_refine_batched(model, items: List[Tuple[str, str]], indir: str, outdir: str, cfg: dict, *, device='cuda', rank: int = 0,
                            world: int = 1) -> int:
    """``refine=True refiner.batch_size=N`` (N > 1; extension): the rank's share of the items (the same as predict_refine's) grouped by
    their size after ``dataset.scale_factor``, each group refined in chunks of at most N images through refine_predict_batch -- one
    batched optimisation per chunk, every image its own loss and Adam state.  The next chunk's PNGs load on the thread pool while the
    current chunk refines; the files written are those of predict_refine."""
    from PIL import Image
    from .refinement import refine_predict_batch
    pad_mod = int(cfg['dataset.pad_out_to_modulo'])
    n_max = int(cfg['refiner.batch_size'])
    scale_factor = cfg.get('dataset.scale_factor')
    mine = [items[i] for i in range(rank, len(items), world)]
    t0 = time.perf_counter()

    def header_size(item):
        with Image.open(item[1]) as im:
            w, h = im.size
        return (h, w) if scale_factor is None else scaled_size(h, w, scale_factor)

    groups: Dict[Tuple[int, int], List[Tuple[str, str]]] = {}
    for item in mine:
        groups.setdefault(header_size(item), []).append(item)
    chunks = [g[i:i + n_max] for g in groups.values() for i in range(0, len(g), n_max)]
    pool = ThreadPoolExecutor(4)

    def load(chunk):
        return [load_item(m, im, pad_mod, scale_factor) for m, im in chunk]

    futures, written = [], 0
    try:
        nxt = pool.submit(load, chunks[0]) if chunks else None
        for ci, chunk in enumerate(chunks):
            loaded = nxt.result()
            nxt = pool.submit(load, chunks[ci + 1]) if ci + 1 < len(chunks) else None
            hw = {tuple(hw_) for _, _, hw_ in loaded}
            if len(hw) != 1:
                raise L.LamaError(f'refiner.batch_size: the images of one chunk decode to different sizes {sorted(hw)}')
            h, w = hw.pop()
            B = len(chunk)
            batch = dict(image=torch.from_numpy(np.stack([a for a, _, _ in loaded])).to(device),
                         mask=torch.from_numpy(np.stack([m for _, m, _ in loaded])).to(device),
                         unpad_to_size=[torch.tensor([h] * B), torch.tensor([w] * B)])
            # the RAW grayscale masks, as in predict_refine (bin/predict.py:75-81)
            cur_res = refine_predict_batch(batch, model, gpu_ids=str(cfg['refiner.gpu_ids']), modulo=int(cfg['refiner.modulo']),
                                           n_iters=int(cfg['refiner.n_iters']), lr=float(cfg['refiner.lr']), min_side=int(cfg['refiner.min_side']),
                                           max_scales=int(cfg['refiner.max_scales']), px_budget=int(cfg['refiner.px_budget']))
            for b, (mask_path, _) in enumerate(chunk):
                u8 = np.clip(cur_res[b].permute(1, 2, 0).numpy() * 255, 0, 255).astype('uint8')
                rel = os.path.splitext(mask_path[len(indir):].lstrip(os.sep))[0] + cfg['out_ext']
                futures.append(pool.submit(_write_png, os.path.join(outdir, rel), u8))
                written += 1
        for f in futures:
            f.result()
    finally:
        pool.shutdown()
    dt = time.perf_counter() - t0
    print(f'rank {rank}: refined {written} images in {dt:.3f} s ({len(chunks)} batched optimisations of up to {n_max} images)')
    return written


def main(argv: Optional[Sequence[str]] = None) -> int:
    cfg = parse_overrides(sys.argv[1:] if argv is None else argv)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if not torch.cuda.is_available():
        raise L.LamaError('lama_amd.predict needs an MI355X: no GPU is visible (there is no CPU fallback)')
    device = torch.device('cuda', local)
    torch.cuda.set_device(device)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', device_id=device)
    train_config = lcfg.load_train_config(os.path.join(cfg['model.path'], 'config.yaml'))           # bin/predict.py:46-48
    ckpt = os.path.join(cfg['model.path'], 'models', cfg['model.checkpoint'])                       # bin/predict.py:55-57
    model = trainers.load_checkpoint(train_config, ckpt, strict=False, map_location=device)         # bin/predict.py:58
    model.freeze()
    model.generator.set_precision(L.PREC_NAMES[cfg['precision']])
    model.generator.use_graph = True
    indir = cfg['indir'] if cfg['indir'].endswith(os.sep) else cfg['indir'] + os.sep               # bin/predict.py:63-64
    items = list_dataset(indir, cfg['dataset.img_suffix'])
    if cfg.get('refine', False):                                                                    # bin/predict.py:75-81
        n = predict_refine(model, items, indir, cfg['outdir'], cfg, device=device, rank=rank, world=world)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        print(f'rank {rank}: wrote {n} refined images to {cfg["outdir"]}')
        return 0
    if cfg.get('profile', False):
        global PROFILE_SPANS
        PROFILE_SPANS = True
    t0 = time.perf_counter()
    n = predict(model, items, indir, cfg['outdir'], pad_mod=int(cfg['dataset.pad_out_to_modulo']), batch_size=int(cfg['batch_size']),
                out_ext=cfg['out_ext'], device=device, rank=rank, world=world, dist=dist, io_threads=int(cfg['io_threads']), out_key=cfg['out_key'],
                scale_factor=cfg.get('dataset.scale_factor'), paste_back=bool(cfg['paste_back']), device_png=bool(cfg['device_png']),
                device_jpeg=bool(cfg['device_jpeg']), jpeg_quality=cfg['jpeg_quality'], jpeg_subsampling=cfg['jpeg_subsampling'],
                crop_to_mask=bool(cfg['crop_to_mask']), crop_margin=int(cfg['crop_margin']), crop_step=int(cfg['crop_step']),
                crop_max_side=int(cfg['crop_max_side']))
    dt = time.perf_counter() - t0
    if rank == 0:
        # (the loop's own wall time: plan build + graph capture of every shape bucket, PNG decode, upload, compute, download, PNG encode + write)
        print(f'wrote {n} images to {cfg["outdir"]} in {dt:.3f} s ({n / max(dt, 1e-9):.1f} images/s, {world} rank(s), io_threads={int(cfg["io_threads"])})')
        if cfg['crop_to_mask']:
            print(f'crop_to_mask pre-pass: {LOOP_TIMES.get("crop_prepass", 0.0):.3f} s of the {dt:.3f} s (every mask decoded once more, on the I/O pool, for its window)')
        if cfg.get('profile', False):
            print('main-thread seconds per phase of the round loop: ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(LOOP_TIMES.items())))
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
