"""The numpy / pure-Python restatement of the device PNG stream (lama_png_deflate_u8_fwd, csrc/png.hip): ``deflate_ref`` defines the kernel's
output byte for byte.  The stream is this engine's own definition (a PNG encoder owes a decoder the pixels, not particular bytes):

  1. filtered bytes: per row the byte 1 (Sub), then w c bytes x[i] - x[i - c] mod 256 (the first pixel as is); row = 1 + w c
  2. chunks of R = max(1, chunk_bytes // row) whole rows (the last one may be shorter), each at most 65535 raw bytes
  3. a chunk = ONE dynamic-Huffman block (BFINAL 0, BTYPE 10, HLIT 0 = 257 codes, HDIST 0 = one distance code of length 0, HCLEN 15; the
     19 code-length-code lengths 4 for the symbols 0..15 and 0 for 16 / 17 / 18: every code length travels as 4 bits), the chunk's bytes as
     literals, symbol 256, then an empty stored block (000, pad to a byte, 00 00 FF FF): the chunk ends on a byte boundary
  4. code lengths: the depths of the Huffman tree over the used symbols (256 counts once) built by the two-queue merge over the symbols
     sorted by (count, symbol), a leaf before an internal node on ties; deeper than 15: every non-zero count n becomes (n + 1) >> 1 and the
     tree is built again.  Canonical codes, bit-reversed into the LSB-first stream
  5. a chunk whose dynamic form is not shorter than raw + 5 bytes is stored instead: 00, LEN, ~LEN (little endian), the raw bytes
  6. 78 01, the chunks, 01 00 00 FF FF, Adler-32 of the filtered bytes (big endian)
"""
import zlib

import numpy as np

DEFAULT_CHUNK = 24576
CLC_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
HEADER_BITS = 17 + 3 * 19 + 4 * 258            # 1106


def filtered(image: np.ndarray, h: int, w: int) -> np.ndarray:
    """[h, 1 + w c] u8: the Sub-filtered rows of the h x w crop of a [Hs, Ws] / [Hs, Ws, c] slot."""
    a = np.asarray(image)
    a = a[:, :, None] if a.ndim == 2 else a
    c = a.shape[2]
    flat = np.ascontiguousarray(a[:h, :w]).reshape(h, w * c)
    raw = np.empty((h, 1 + w * c), np.uint8)
    raw[:, 0] = 1
    raw[:, 1:1 + c] = flat[:, :c]
    raw[:, 1 + c:] = flat[:, c:] - flat[:, :-c]
    return raw


def rows_per_chunk(row: int, chunk_bytes: int) -> int:
    return max(1, chunk_bytes // row)


def n_chunks(h: int, w: int, c: int, chunk_bytes: int = DEFAULT_CHUNK) -> int:
    return 0 if h <= 0 or w <= 0 else -(-h // rows_per_chunk(1 + w * c, chunk_bytes))


def _depths(counts):
    """Leaf depths of the two-queue Huffman merge over the used symbols sorted by (count, symbol); a leaf before an internal node on ties."""
    order = sorted((s for s in range(257) if counts[s]), key=lambda s: (counts[s], s))
    n = len(order)
    assert n >= 2
    weight = [counts[s] for s in order] + [0] * (n - 1)          # nodes 0 .. n-1: leaves in sorted order; n .. 2n-2: internal, in creation order
    parent = [0] * (2 * n - 1)
    li, ii = 0, n
    for k in range(n, 2 * n - 1):
        pick = []
        for _ in range(2):
            if li < n and (ii >= k or weight[li] <= weight[ii]):
                pick.append(li)
                li += 1
            else:
                pick.append(ii)
                ii += 1
        weight[k] = weight[pick[0]] + weight[pick[1]]
        parent[pick[0]] = parent[pick[1]] = k
    depth = [0] * (2 * n - 1)
    for k in range(2 * n - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    return {order[i]: depth[i] for i in range(n)}


def code_lengths(counts):
    """257 code lengths (0 = unused) of at most 15 bits: step 4 of the stream."""
    counts = [int(v) for v in counts]
    while True:
        d = _depths(counts)
        if max(d.values()) <= 15:
            return [d.get(s, 0) for s in range(257)]
        counts = [(v + 1) >> 1 if v else 0 for v in counts]


def canonical(lengths):
    """RFC 1951 3.2.2 codes, bit-reversed (the form that goes into the LSB-first stream)."""
    bl = [0] * 16
    for l in lengths:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        if l:
            out.append(int(format(nxt[l], f'0{l}b')[::-1], 2))
            nxt[l] += 1
        else:
            out.append(0)
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def pad(self):
        if self.n:
            self.put(0, 8 - self.n)


def chunk_ref(raw: bytes) -> bytes:
    """One chunk of filtered bytes as whole bytes: the dynamic block + the empty stored block, or the stored form."""
    n = len(raw)
    assert 0 < n <= 65535
    counts = np.bincount(np.frombuffer(raw, np.uint8), minlength=257)
    counts[256] = 1
    lens = code_lengths(counts)
    codes = canonical(lens)
    bits = HEADER_BITS + sum(int(counts[s]) * lens[s] for s in range(257)) + 3
    if (bits + 7) // 8 + 4 >= n + 5:
        return bytes([0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + bytes(raw)
    b = _Bits()
    b.put(0, 1)
    b.put(2, 2)
    b.put(0, 5)
    b.put(0, 5)
    b.put(15, 4)
    for s in CLC_ORDER:
        b.put(4 if s < 16 else 0, 3)
    for l in lens + [0]:                        # the 257 literal / length code lengths and the one distance code length, 4 bits each, MSB first
        b.put(int(format(l, '04b')[::-1], 2), 4)
    for v in raw:
        b.put(codes[v], lens[v])
    b.put(codes[256], lens[256])
    b.put(0, 3)
    b.pad()
    out = bytes(b.out) + b'\x00\x00\xff\xff'
    assert len(out) == (bits + 7) // 8 + 4
    return out


def deflate_ref(image: np.ndarray, h: int, w: int, chunk_bytes: int = DEFAULT_CHUNK) -> bytes:
    """The zlib stream of the h x w crop of ``image`` ([Hs, Ws] or [Hs, Ws, c] u8); b'' for an empty crop."""
    if h <= 0 or w <= 0:
        return b''
    raw = filtered(image, h, w)
    R = rows_per_chunk(raw.shape[1], chunk_bytes)
    out = bytearray(b'\x78\x01')
    for y in range(0, h, R):
        out += chunk_ref(raw[y:y + R].tobytes())
    out += b'\x01\x00\x00\xff\xff'
    out += (zlib.adler32(raw.tobytes()) & 0xffffffff).to_bytes(4, 'big')
    return bytes(out)


def bound(h: int, w: int, c: int, chunk_bytes: int = DEFAULT_CHUNK) -> int:
    """lama_png_deflate_bound: every chunk in its stored form (the dynamic form is taken only where it is shorter), header, final block, Adler-32."""
    if h <= 0 or w <= 0:
        return 0
    return h * (1 + w * c) + 5 * n_chunks(h, w, c, chunk_bytes) + 11


def huffman_only_len(raw: bytes) -> int:
    """zlib level 1, Z_HUFFMAN_ONLY, of the same filtered bytes: what the size condition is held against."""
    co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    return len(co.compress(raw) + co.flush())
