"""The entropy-coded scan of lama_jpeg_scan_u8_fwd (csrc/jpeg.hip), restated in numpy: the definition the kernel is held to byte for byte.
Integer arithmetic only; the tables come from lama_amd/jpeg.py, the one place jpeg_from_scan reads them from too.

  colour     Y  = (19595 R + 38470 G +  7471 B + 32768) >> 16
             Cb = ((-11059 R - 21709 G + 32768 B + 32767) >> 16) + 128      (>>: arithmetic, i.e. floor; 32767 keeps B = 255 at 255)
             Cr = (( 32768 R - 27439 G -  5329 B + 32767) >> 16) + 128
  edges      the last column / row repeated out to the MCU grid (8 x 8 for 4:4:4, 16 x 16 for 4:2:0)
  dummies    4:2:0 only: a Y block that lies wholly outside the image (8 bx >= w or 8 by >= h) is not transformed: its DC level is that of the
             block coded before it (the same MCU's previous Y block) and its AC levels are 0, so it costs a zero DC difference and an EOB
  4:2:0      chroma sample = (a + b + c + d + 2) >> 2 over each 2 x 2 of the full-size Cb / Cr
  DCT        s = sample - 128;  C[u][x] = round(2^13 alpha(u) cos((2x + 1) u pi / 16)), alpha(0) = sqrt(1/8), alpha(u) = 1/2
             rows     t[y][u] = (sum_x C[u][x] s[y][x] + 2^7)  >> 8       (5 fraction bits)
             columns  c[v][u] = (sum_y C[v][y] t[y][u] + 2^14) >> 15      (the coefficient times 8: 3 fraction bits, so that the
                                                                            quantiser rounds once, not twice)
  quantise   Q = clamp((base scale + 50) / 100, 1, 255), scale = 5000 / q (q < 50) or 200 - 2 q;  level = sign(c) ((|c| + 4 Q) / (8 Q))
  coding     zigzag, DC difference per component, (run, size) symbols with ZRL and EOB, Annex K.3 - K.6 codes, MSB first
  intervals  one MCU row each: DC predictors 0, bits padded with 1s to a byte, FF -> FF 00, RSTm (m = row mod 8) between two intervals"""
import functools

import numpy as np

from lama_amd import jpeg as J

J444, J420 = 0, 1
SEG_MCUS = {J444: 64, J420: 32}          # the MCUs a workgroup of jpeg.hip codes at a time (192 blocks either way)
BLOCK_MAX_BITS = 1660                    # DC: code <= 11 bits + 11; 63 AC of code <= 16 bits + 10
DCT_BOUND = 0.5                          # |integer DCT - fp64 DCT| of the same samples stays below this (the derivation: csrc/jpeg.hip)


@functools.lru_cache(maxsize=None)
def dct_table() -> np.ndarray:
    u, x = np.mgrid[:8, :8].astype(np.float64)
    alpha = np.where(u == 0, np.sqrt(1 / 8), 0.5)
    return np.rint(8192 * alpha * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)


def dct_matrix_f64() -> np.ndarray:
    u, x = np.mgrid[:8, :8].astype(np.float64)
    return np.where(u == 0, np.sqrt(1 / 8), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)


def mcu_size(ss: int) -> int:
    return 16 if ss == J420 else 8


def ycc_planes(img: np.ndarray, ss: int):
    """[h,w,3] u8 -> (Y, Cb, Cr) int64 sample planes on the MCU grid (Cb / Cr at half size for 4:2:0)."""
    h, w = img.shape[:2]
    m = mcu_size(ss)
    a = np.pad(img.astype(np.int64), ((0, -h % m), (0, -w % m), (0, 0)), mode='edge')
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = ((-11059 * r - 21709 * g + 32768 * b + 32767) >> 16) + 128
    cr = ((32768 * r - 27439 * g - 5329 * b + 32767) >> 16) + 128
    assert y.min() >= 0 and y.max() <= 255 and min(cb.min(), cr.min()) >= 0 and max(cb.max(), cr.max()) <= 255
    if ss == J420:
        cb, cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (cb, cr))
    return y, cb, cr


def blocks_of(plane: np.ndarray) -> np.ndarray:
    """[8a, 8b] -> [a, b, 8, 8]"""
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    return plane.reshape(a, 8, b, 8).transpose(0, 2, 1, 3)


def fdct(samples: np.ndarray) -> np.ndarray:
    """[..., 8(y), 8(x)] int64 samples (level shift NOT applied) -> [..., 8(v), 8(u)] coefficients times 8."""
    C = dct_table()
    s = samples - 128
    t = (np.einsum('ux,...yx->...yu', C, s) + (1 << 7)) >> 8
    return (np.einsum('vy,...yu->...vu', C, t) + (1 << 14)) >> 15


def quantise(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """[..., 8, 8] coefficients times 8 (fdct), q [64] natural order -> [..., 64] levels in zigzag order."""
    q = q.reshape(8, 8)
    lev = np.sign(coef) * ((np.abs(coef) + 4 * q) // (8 * q))
    return lev.reshape(*lev.shape[:-2], 64)[..., list(J.ZIGZAG)]


def levels_of(img: np.ndarray, quality: int, ss: int):
    """-> (Y levels [by, bx, 64], Cb levels, Cr levels), zigzag order."""
    y, cb, cr = ycc_planes(img, ss)
    ql, qc = J.quant_table(J.QUANT_LUMA, quality), J.quant_table(J.QUANT_CHROMA, quality)
    return quantise(fdct(blocks_of(y)), ql), quantise(fdct(blocks_of(cb)), qc), quantise(fdct(blocks_of(cr)), qc)


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code: int, n: int):
        self.acc = (self.acc << n) | code
        self.n += n


def _code_block(bw: _Bits, lev, pred: int, dc, ac, stats) -> int:
    d = int(lev[0]) - pred
    cat = abs(d).bit_length()
    c, n = dc[cat]
    bw.put(c, n)
    bw.put((d if d >= 0 else d - 1) & ((1 << cat) - 1), cat)
    stats['dc_cat'] = max(stats['dc_cat'], cat)
    stats['dc_zero'] += d == 0
    run = 0
    nz = np.flatnonzero(lev[1:]) + 1
    last = 0
    for k in nz:
        run = int(k) - last - 1
        while run >= 16:
            bw.put(*ac[0xf0])
            stats['zrl'] += 1
            run -= 16
        v = int(lev[k])
        cat = abs(v).bit_length()
        assert cat <= 10
        c, n = ac[(run << 4) | cat]
        bw.put(c, n)
        bw.put((v if v >= 0 else v - 1) & ((1 << cat) - 1), cat)
        stats['ac_cat'] = max(stats['ac_cat'], cat)
        last = int(k)
    if last < 63:
        bw.put(*ac[0x00])
        stats['eob_only'] += len(nz) == 0
    else:
        stats['no_eob'] += 1
    return int(lev[0])


def encode(img: np.ndarray, quality: int, ss: int):
    """-> (scan bytes, stats of the mechanisms the stream went through)."""
    assert img.ndim == 3 and img.shape[2] == 3 and img.dtype == np.uint8 and ss in (J444, J420)
    ly, lcb, lcr = levels_of(img, quality, ss)
    h, w = img.shape[:2]
    dcl, dcc, acl, acc = (J.huffman_codes(t) for t in (J.DC_LUMA, J.DC_CHROMA, J.AC_LUMA, J.AC_CHROMA))
    rows, mpr = lcb.shape[:2] if ss == J420 else ly.shape[:2]
    stats = dict(dc_cat=0, ac_cat=0, zrl=0, eob_only=0, no_eob=0, dc_zero=0, stuffed=0, pad_bits=0, dummies=0, carried=[], rows=rows, mcus_per_row=mpr, interval_bytes=[])
    out = bytearray()
    for r in range(rows):
        bw = _Bits()
        py = pcb = pcr = 0
        for m in range(mpr):
            if ss == J420:
                for k in range(4):
                    by, bx = 2 * r + (k >> 1), 2 * m + (k & 1)
                    lev = ly[by, bx]
                    if 8 * by >= h or 8 * bx >= w:
                        lev = np.zeros(64, np.int64)
                        lev[0] = py
                        stats['dummies'] += 1
                    py = _code_block(bw, lev, py, dcl, acl, stats)
            else:
                py = _code_block(bw, ly[r, m], py, dcl, acl, stats)
            pcb = _code_block(bw, lcb[r, m], pcb, dcc, acc, stats)
            pcr = _code_block(bw, lcr[r, m], pcr, dcc, acc, stats)
            if (m + 1) % SEG_MCUS[ss] == 0 and m + 1 < mpr:
                stats['carried'].append(bw.n % 8)          # the bits of an unfinished byte that a workgroup of jpeg.hip carries into its next segment
        pad = -bw.n % 8
        stats['pad_bits'] = max(stats['pad_bits'], pad)
        bw.put((1 << pad) - 1, pad)
        raw = bw.acc.to_bytes(bw.n // 8, 'big')
        stats['stuffed'] += raw.count(b'\xff')
        body = raw.replace(b'\xff', b'\xff\x00')
        stats['interval_bytes'].append(len(body))
        out += body
        if r < rows - 1:
            out += bytes([0xff, 0xd0 + (r & 7)])
    return bytes(out), stats


def scan_ref(img: np.ndarray, h: int, w: int, quality: int, ss: int) -> bytes:
    """The scan of the h x w top-left corner of ``img`` ([H,W,3] u8)."""
    return encode(np.ascontiguousarray(img[:h, :w]), quality, ss)[0]


def bound(h: int, w: int, ss: int) -> int:
    """lama_jpeg_scan_bound: every block at its longest code, every byte of an interval stuffed, the markers between the intervals."""
    if ss not in (J444, J420) or not (1 <= h <= 65535 and 1 <= w <= 65535):
        return 0
    m = mcu_size(ss)
    rows, mpr = -(-h // m), -(-w // m)
    per = 2 * ((mpr * (6 if ss == J420 else 3) * BLOCK_MAX_BITS + 7) // 8)
    return rows * per + 2 * (rows - 1)
