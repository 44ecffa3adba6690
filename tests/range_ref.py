"""Test helper: the numpy statement of lama_range_stats_fwd and the planted inputs of its tests.

``stats(a, limit)``: a = float32 / float16 array [batch, C, H, W] (any strides: a channel slice is fine) -> (abs_max float32 [C], n_nan, n_inf,
n_over uint32 [C]).  Classification is on the bit patterns, as in the kernel: NaN / inf by the exponent field, "over" by the widened value
(float16 -> float32 is exact) against ``limit`` as a float32.
"""
import numpy as np

CHUNK_BYTES = 32768          # one workgroup of range_stats.hip covers this many bytes of one plane (RS_CHUNK_BYTES)


def stats(a: np.ndarray, limit: float):
    assert a.dtype in (np.float32, np.float16) and a.ndim == 4
    wide = np.ascontiguousarray(a).astype(np.float32)                 # exact for float16 (denormals included)
    bits = wide.view(np.uint32) & np.uint32(0x7fffffff)
    inf = np.uint32(0x7f800000)
    lim = np.array([limit], dtype=np.float32).view(np.uint32)[0]
    nan_m, inf_m = bits > inf, bits == inf
    fin_m = bits < inf
    over_m = fin_m & (bits > lim)
    red = (0, 2, 3)
    amax_bits = np.where(fin_m, bits, np.uint32(0)).max(axis=red).astype(np.uint32)
    return (amax_bits.view(np.float32), nan_m.sum(axis=red).astype(np.uint32), inf_m.sum(axis=red).astype(np.uint32),
            over_m.sum(axis=red).astype(np.uint32))


def planted(shape, dtype, c0=0, c=None, limit=65504.0, seed=0, scale=100.0):
    """(full array [B, Ct, H, W], limit): ``randn * scale`` with special values planted into the view of channels [c0, c0 + c), at the positions
    where the kernel changes path: the first / last element of the view, the last image, the elements in front of and behind the 16-byte
    aligned body of a plane, and both sides of every boundary between two workgroups' pieces.  Each kind of value goes into a channel of its
    own where the view has that many; otherwise the kinds that share a channel take turns over the positions (nothing is overwritten).  Views
    of four channels and more end in an all-zero and an all-NaN channel."""
    rng = np.random.default_rng(seed)
    B, Ct, H, W = shape
    c = Ct - c0 if c is None else c
    full = (rng.standard_normal(shape) * scale).astype(dtype)
    v = full[:, c0:c0 + c]                                            # the view (writes go through)
    n = H * W
    per = CHUNK_BYTES // np.dtype(dtype).itemsize                     # elements per piece
    vec = 16 // np.dtype(dtype).itemsize                              # elements per 16-byte load

    def bits(u, ut):
        return np.array([u], dtype=ut).view(dtype)[0]

    if dtype == np.float32:
        lim32 = np.float32(limit)
        kinds = [lim32,                                               # exactly limit: not over
                 np.nextafter(lim32, np.float32(np.inf)),             # the next float: over
                 np.float32(-2.0) * lim32,
                 np.float32(np.inf), np.float32(-np.inf),
                 bits(0x7fc00000, np.uint32),                         # quiet NaN
                 bits(0xff800123, np.uint32),                         # NaN with the sign bit and a payload
                 np.float32(-0.0),
                 bits(0x00000001, np.uint32)]                         # the smallest denormal
    else:
        kinds = [np.float16(65504.0),                                 # with limit = 65504: not over
                 np.float16(-65504.0),
                 np.float16(np.inf), np.float16(-np.inf),
                 bits(0x7e00, np.uint16),
                 bits(0xfc01, np.uint16),                             # NaN with the sign bit and a payload
                 np.float16(-0.0),
                 bits(0x0001, np.uint16)]                             # the smallest half denormal
    special = c >= 4                                                  # the last two channels: all zero, all NaN
    ck = c - 2 if special else c                                      # channels that take planted kinds
    turns = -(-len(kinds) // ck)                                      # kinds per channel
    pos = [0, n - 1] + [q for q in (1, 2, 3, vec - 1, vec, n - 2, n - 3, n - vec, n - vec - 1) if 0 < q < n - 1]
    for b in range(per, n, per):
        pos += [b - 1, b]
    if n > 2 * per + 3:
        pos += [2 * per + 1, 2 * per + 2]
    pos = list(dict.fromkeys(pos))
    if n == 1:                                                        # one element per (image, channel): the kinds go through the images
        for i, val in enumerate(kinds[:B * ck]):
            v[i % B, (i // B) % ck, 0, 0] = val
        kinds = []
    for i, val in enumerate(kinds):
        ch, turn = i % ck, i // ck
        for j, ps in enumerate(pos):
            if j % turns != turn:
                continue
            img = 0 if ps == 0 else (B - 1 if ps == n - 1 else (i + j) % B)      # the first image at the first position, the last at the last
            v[img, ch, ps // W, ps % W] = val
    if special:
        v[:, c - 2] = 0
        v[:, c - 1] = bits(0x7fc00000, np.uint32) if dtype == np.float32 else bits(0x7e00, np.uint16)
    return full, float(limit)


# ---- shared by the emulator and the GPU tests ---------------------------------------------------------------------------------------

# (full shape, first channel of the view, channels of the view)
VIEWS = [((1, 1, 1, 1), 0, None),
         ((2, 5, 7, 9), 1, 3),          # planes of 63 elements, element-aligned starts, batch_stride > C H W
         ((2, 6, 8, 5), 0, None),       # spectrum-shaped
         ((3, 70, 4, 4), 0, None),      # many channels, few pixels, three images
         ((8, 1, 1, 1), 0, None),
         # a plane of 90 300 elements: the kernel's piece is 32 KiB = 8 192 fp32 / 16 384 fp16 elements (range_ref.CHUNK_BYTES), so this plane
         # is 12 / 6 pieces and the planted values sit on both sides of every boundary
         ((1, 2, 300, 301), 0, None)]
IDS = ['1x1x1x1', '2x5x7x9[1:4]', '2x6x8x5', '3x70x4x4', '8x1x1x1', '1x2x300x301']


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_view(lib, full, c0, c, limit, device='cpu'):
    """range_stats on channels [c0, c0 + c) of ``full`` == range_ref.stats, all four fields, abs_max compared as bits."""
    import torch
    from lama_amd import _lib as L
    t = torch.from_numpy(full).to(device)
    v = L.view(t, c0, c)
    out = torch.full((v.C, 4), 0x5a5a5a5a, dtype=torch.int32, device=device)        # garbage: must be overwritten
    got_t = lib.range_stats(v, full.shape[0], limit, out=out, stream=lib.stream_of(t))
    assert got_t.data_ptr() == out.data_ptr()
    got = L.unpack_range_stats(out)
    ref = stats(full[:, c0:c0 + v.C], limit)
    for name, g, r in zip(('abs_max', 'n_nan', 'n_inf', 'n_over'), got, ref):
        assert g.shape == r.shape and np.array_equal(_bits(g), _bits(r)), (name, g, r)
    return out, ref


def check_rows_against_reference(rep, limit=65504.0):
    """With keep=True every row equals range_ref of its own tensor, bit for bit; the row's summary is the summary of those arrays."""
    assert set(rep.tensors) == {r.name for r in rep.rows if r.per_channel is not None}
    for r in rep.rows:
        t = rep.tensors[r.name]
        assert tuple(t.shape) == tuple(r.shape) and str(t.dtype).endswith(r.dtype)
        ref = stats(t.cpu().numpy(), limit)
        for g, w in zip(r.per_channel, ref):
            assert np.array_equal(_bits(g), _bits(w)), r.name
        ch = int(np.argmax(ref[0]))
        assert r.channel == ch and r.abs_max == float(ref[0][ch])
        assert (r.n_nan, r.n_inf, r.n_over) == tuple(int(a.sum()) for a in ref[1:])
