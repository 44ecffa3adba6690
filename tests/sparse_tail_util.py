"""Shared by tests/test_sparse_tail_emu.py and tests/test_sparse_tail_gpu.py: a plain torch restatement of the sparse tail's closure rule
(include/lama_hip.h, lama_tail_lists_build), the mask cases, and the drivers that run the list variants of the ConvTranspose2d and head kernels
beside their dense launches.

The restatement works on PIXEL maps, not on rectangle arithmetic: it paints what every listed unit reads and asks each upstream unit whether
any painted pixel lies in the rectangle it writes -- the rule as the issue states it, in another form than the kernel's."""
import torch

from lama_amd import _lib as L

HEAD_RS = 16
# (batch, H, W): the second with ragged last tiles (20 x 36, 10 x 18, 5 x 9 input planes) and a ragged last head part (40 = 2 x 16 + 8) and segment
PLANES = [(1, 64, 96), (2, 40, 72)]
UP_MG = [1, 2, 4]                      # big-lama: up3 128 -> 64, up2 256 -> 128, up1 512 -> 256
MASKS = ['zero', 'one', 'corner', 'seam', 'bench64']


def cd(a, b):
    return (a + b - 1) // b


def bench_mask(b, r, seed):
    """bench.synthetic_batch's mask: a centred rectangle of 25 % of the area + 3 random strokes per image."""
    mask = torch.zeros(b, 1, r, r)
    mask[:, :, r // 4: r // 4 + r // 2, r // 4: r // 4 + r // 2] = 1.0
    gs = torch.Generator().manual_seed(4321 + seed)
    for bi in range(b):
        for _ in range(3):
            y0, x0 = int(torch.randint(0, r, (1,), generator=gs)), int(torch.randint(0, r, (1,), generator=gs))
            ln = int(torch.randint(max(2, r // 8), max(3, r // 2), (1,), generator=gs))
            th = max(1, r // 32)
            if int(torch.randint(0, 2, (1,), generator=gs)):
                mask[bi, 0, y0:y0 + th, x0:x0 + ln] = 1.0
            else:
                mask[bi, 0, y0:y0 + ln, x0:x0 + th] = 1.0
    return mask


def make_mask(kind, B, H, W):
    m = torch.zeros(B, 1, H, W)
    if kind == 'one':
        m[:] = 1.0
    elif kind == 'corner':
        m[B - 1, 0, H - 1, W - 1] = 1.0
    elif kind == 'seam':
        m[0, 0, 16, 64] = 0.5        # first row of head part 1 and of an 8-row up tile, first column of a 64-column up tile: the grown rectangle crosses both seams
    elif kind == 'bench64':
        bm = bench_mask(B, 64, 1234)
        h, w = min(H, 64), min(W, 64)
        m[:, :, :h, :w] = bm[:, :, :h, :w]
    return m


def ref_lists(mask, rs, up_mg):
    """mask [B, 1, H, W] -> (head list, [up list per level]) as python lists in ascending order."""
    B, _, H, W = mask.shape
    need = mask[:, 0] != 0
    txh, ns = cd(W, 26), cd(H, rs)
    head, read = [], torch.zeros(B, H, W, dtype=torch.bool)
    for part in range(ns):
        for b in range(B):
            for c in range(txh):
                y0, y1, x0, x1 = part * rs, min(part * rs + rs, H), c * 26, min(c * 26 + 26, W)
                if bool(need[b, y0:y1, x0:x1].any()):
                    head.append(part * B * txh + b * txh + c)
                    read[b, max(0, y0 - 3):min(H, y1 + 3), max(0, x0 - 3):min(W, x1 + 3)] = True
    ups = []
    for i, mg in enumerate(up_mg):
        h, w = H >> (i + 1), W >> (i + 1)
        tyn, txn = cd(h, 4), cd(w, 32)
        nxt, lst = torch.zeros(B, h, w, dtype=torch.bool), []
        for b in range(B):
            for ty in range(tyn):
                for tx in range(txn):
                    if bool(read[b, 8 * ty:8 * ty + 8, 64 * tx:64 * tx + 64].any()):
                        lst += [((b * tyn + ty) * txn + tx) * mg + m for m in range(mg)]
                        nxt[b, 4 * ty:4 * ty + 5, 32 * tx:32 * tx + 33] = True
        ups.append(lst)
        read = nxt
    return head, ups


def check_lists(lib, kind, plane, dev):
    B, H, W = plane
    # the mask as the generator's input holds it: channel 3 of a 4-channel buffer (a view with a batch stride of four planes)
    x = torch.full((B, 4, H, W), 3.0)
    x[:, 3:] = make_mask(kind, B, H, W)
    want_head, want_ups = ref_lists(x[:, 3:], HEAD_RS, UP_MG)
    xd = x.to(dev)
    lists = lib.tail_lists_alloc(B, H, W, HEAD_RS, UP_MG, dev)
    for t in [lists['head'][0]] + [u[0] for u in lists['up']]:
        t.fill_(-7)                                    # what the build does not write stays
    st = torch.cuda.current_stream().cuda_stream if dev != 'cpu' else 0
    for _ in range(2):                                 # a second build over the same buffers: nothing accumulates
        lib.tail_lists_build(L.view(xd, 3, 1), lists, st)
    for name, (lst, cnt), want in [('head', lists['head'], want_head)] + [(f'up{i}', lists['up'][i], want_ups[i]) for i in range(len(UP_MG))]:
        n = int(cnt.cpu()[0])
        got = lst.cpu()[:n].tolist()
        assert n == len(want), (name, n, len(want))
        assert set(got) == set(want), name
        assert all(a < b for a, b in zip(got, got[1:])), name
        assert bool((lst.cpu()[n:] == -7).all()), name
    if kind == 'zero':
        assert want_head == [] and all(u == [] for u in want_ups)
    if kind == 'one':
        assert len(want_head) == lists['head'][0].numel() and all(len(u) == lists['up'][i][0].numel() for i, u in enumerate(want_ups))


# ---- the list variants beside the dense launches ---------------------------------------------------------------------------------------------
SENT = -123.0


def _pick(n, frac, seed):
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(n, generator=g) < frac
    return torch.nonzero(keep).flatten().to(torch.int32)


def check_convt_list(lib, dev, B, cin, cout, H, W, frac, prec, seed=0):
    """ConvTranspose2d + bias + ReLU over a list of ``frac`` of its tiles: the listed tiles' 8 x 64 output rectangles (their 64 channels) equal the dense
    launch bit for bit, everything else keeps the sentinel."""
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(B, cin, H, W, generator=g).to(dev)
    w = (torch.randn(cin, cout, 3, 3, generator=g) * (1.0 / (cin * 2.25) ** 0.5)).to(dev)
    bias = torch.randn(cout, generator=g).to(dev)
    wp = lib.pack_conv_weight(w, None, stride=2, transposed=True, precision=prec)
    st = torch.cuda.current_stream().cuda_stream if dev != 'cpu' else 0
    dense = torch.full((B, cout, 2 * H, 2 * W), SENT, device=dev)
    args = (L.view(x), wp, None, B, 3, 2, 1, L.PAD_ZERO, True, bias, L.ACT_RELU)
    lib.conv2d(*args[:2], L.view(dense), *args[3:], precision=prec, stream=st)
    tyn, txn, mg = cd(H, 4), cd(W, 32), cout // 64
    n = B * tyn * txn * mg
    lst = _pick(n, frac, seed)
    buf = torch.full((n,), n + 5, dtype=torch.int32)       # entries behind the count are never read (they would be clamped, and written)
    buf[:lst.numel()] = lst
    cnt = torch.tensor([lst.numel()], dtype=torch.int32)
    got = torch.full_like(dense, SENT)
    tl = (buf.to(dev), cnt.to(dev), HEAD_RS)
    assert lib.conv2d(*args[:2], L.view(got), *args[3:], precision=prec, stream=st, tile_list=tl, query=True) is True
    lib.conv2d(*args[:2], L.view(got), *args[3:], precision=prec, stream=st, tile_list=tl)
    want = torch.full_like(dense, SENT).cpu()
    dc = dense.cpu()
    assert bool((dc != SENT).all())
    for t in lst.tolist():
        m = t % mg
        tx = (t // mg) % txn
        ty = (t // (mg * txn)) % tyn
        b = t // (mg * txn * tyn)
        sl = (b, slice(64 * m, 64 * m + 64), slice(8 * ty, 8 * ty + 8), slice(64 * tx, 64 * tx + 64))
        want[sl] = dc[sl]
    assert torch.equal(got.cpu(), want)
    return lst.numel(), n


def check_head_list(lib, dev, B, H, W, frac, prec, rs=HEAD_RS, seed=0):
    """ReflectionPad2d(3) + 7x7 conv 64 -> 3 + sigmoid over a list of ``frac`` of its rs x 26 segments against the dense launch."""
    g = torch.Generator().manual_seed(200 + seed)
    x = torch.randn(B, 64, H, W, generator=g).to(dev)
    w = (torch.randn(3, 64, 7, 7, generator=g) * (1.0 / (64 * 49) ** 0.5)).to(dev)
    bias = torch.randn(3, generator=g).to(dev)
    wp = lib.pack_conv_weight(w, None, precision=prec)
    st = torch.cuda.current_stream().cuda_stream if dev != 'cpu' else 0
    dense = torch.full((B, 3, H, W), SENT, device=dev)
    args = (L.view(x), wp, None, B, 7, 1, 3, L.PAD_REFLECT, False, bias, L.ACT_SIGMOID)
    lib.conv2d(*args[:2], L.view(dense), *args[3:], precision=prec, stream=st)
    txh, ns = cd(W, 26), cd(H, rs)
    n = B * txh * ns
    lst = _pick(n, frac, seed)
    buf = torch.full((n,), -9, dtype=torch.int32)
    buf[:lst.numel()] = lst
    cnt = torch.tensor([lst.numel()], dtype=torch.int32)
    got = torch.full_like(dense, SENT)
    tl = (buf.to(dev), cnt.to(dev), rs)
    assert lib.conv2d(*args[:2], L.view(got), *args[3:], precision=prec, stream=st, tile_list=tl, query=True) is True
    lib.conv2d(*args[:2], L.view(got), *args[3:], precision=prec, stream=st, tile_list=tl)
    want = torch.full_like(dense, SENT).cpu()
    dc = dense.cpu()
    assert bool((dc != SENT).all())
    for s in lst.tolist():
        part, col = s // (B * txh), s % (B * txh)
        b, c = col // txh, col % txh
        sl = (b, slice(None), slice(part * rs, part * rs + rs), slice(26 * c, 26 * c + 26))
        want[sl] = dc[sl]
    assert torch.equal(got.cpu(), want)
    return lst.numel(), n


def check_head_list_reads_inside_closure(lib, dev, B, H, W, prec, rs=HEAD_RS, seed=0):
    """The closure invariant of the head's list variant on ragged planes: a listed segment reads nothing outside its output rectangle grown by 3
    and clamped to the plane -- lanes and rows that feed no stored pixel included, because what they load passes the range watch.  Every input
    pixel outside the grown rectangles of the listed segments is NaN; the range flag must stay down and the listed outputs must equal the
    dense launch on the clean input.  Listed: the last (ragged) column of segments of every part, i.e. the ragged last part too."""
    g = torch.Generator().manual_seed(300 + seed)
    x = torch.randn(B, 64, H, W, generator=g)
    w = (torch.randn(3, 64, 7, 7, generator=g) * (1.0 / (64 * 49) ** 0.5)).to(dev)
    bias = torch.randn(3, generator=g).to(dev)
    wp = lib.pack_conv_weight(w, None, precision=prec)
    st = torch.cuda.current_stream().cuda_stream if dev != 'cpu' else 0
    txh, ns = cd(W, 26), cd(H, rs)
    assert 1 <= W % 26 <= 13 and H % rs != 0
    lst = [part * B * txh + b * txh + (txh - 1) for part in range(ns) for b in range(B)]
    inside = torch.zeros(B, H, W, dtype=torch.bool)
    for s in lst:
        part, col = s // (B * txh), s % (B * txh)
        b, c = col // txh, col % txh
        y0, y1, x0, x1 = part * rs, min(part * rs + rs, H), c * 26, min(c * 26 + 26, W)
        inside[b, max(0, y0 - 3):min(H, y1 + 3), max(0, x0 - 3):min(W, x1 + 3)] = True
    xp = x.clone()
    xp[~inside[:, None].expand(-1, 64, -1, -1)] = float('nan')
    args = (None, wp, None, B, 7, 1, 3, L.PAD_REFLECT, False, bias, L.ACT_SIGMOID)
    dense = torch.empty(B, 3, H, W, device=dev)
    lib.conv2d(L.view(x.to(dev)), wp, L.view(dense), *args[3:], precision=prec, stream=st)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    got = torch.full((B, 3, H, W), SENT, device=dev)
    tl = (torch.tensor(lst, dtype=torch.int32).to(dev), torch.tensor([len(lst)], dtype=torch.int32).to(dev), rs)
    lib.conv2d(L.view(xp.to(dev)), wp, L.view(got), *args[3:], precision=prec, stream=st, tile_list=tl, range_flag=flag)
    want = torch.full((B, 3, H, W), SENT)
    dc = dense.cpu()
    for s in lst:
        part, col = s // (B * txh), s % (B * txh)
        b, c = col // txh, col % txh
        sl = (b, slice(None), slice(part * rs, part * rs + rs), slice(26 * c, 26 * c + 26))
        want[sl] = dc[sl]
    assert torch.equal(got.cpu(), want)              # (a NaN that reached a stored pixel would show here)
    if prec == L.PREC_F16X3:
        assert int(flag.cpu()[0]) == 0               # ... and one that reached only the range watch, here
        bad = xp.clone()                             # the watch itself works: a NaN INSIDE a grown rectangle raises it
        idx = torch.nonzero(inside)[0]
        bad[idx[0], 0, idx[1], idx[2]] = float('nan')
        lib.conv2d(L.view(bad.to(dev)), wp, L.view(got), *args[3:], precision=prec, stream=st, tile_list=tl, range_flag=flag)
        assert int(flag.cpu()[0]) != 0
