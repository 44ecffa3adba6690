"""Plain references for tests/test_refine_kernels_gpu.py: fp64 torch / numpy on the host, no project kernel anywhere.

Every reference is evaluated on the SAME fp32 inputs the kernel gets, with the same fp32 window / weights / constants promoted to fp64, so
that the only difference to the kernel is the kernel's own rounding.  ``*_abs`` variants are the same linear operator applied to ``|input|``:
with non-negative weights that is the sum of the absolute values of the products, the quantity a rounding bound scales with."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import refine_oracle as R

U = 2.0 ** -24                      # unit roundoff of fp32 (round to nearest)


def gamma(k: int) -> float:
    """Higham's gamma_k = k u / (1 - k u): the relative bound on a result that went through k fp32 roundings."""
    return k * U / (1.0 - k * U)


# -- image pyramid -------------------------------------------------------------------------------------------------------------------

def blur64(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """gaussian_blur2d of the top-left crop [0:H, 0:W], fp64, with the fp32 window of the oracle promoted to fp64."""
    return R.gaussian_blur2d(x.double()[:, :, :H, :W])


def resize64(x: torch.Tensor, size) -> torch.Tensor:
    return F.interpolate(x.double(), size=tuple(size), mode='bilinear', align_corners=False)


def vjp64(fn, x_shape, gy: torch.Tensor) -> torch.Tensor:
    """Adjoint of the linear map ``fn`` by fp64 autograd: d <fn(x), gy> / d x."""
    x = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    fn(x).backward(gy.double())
    return x.grad


# -- mask chain ----------------------------------------------------------------------------------------------------------------------

def make_masks(H: int, W: int):
    """The three mask families of the mask-chain tests, [1, 1, H, W] fp32 in {0, 1}: a rectangle, a union of discs, strokes 1-3 px wide."""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    rect = torch.zeros(H, W)
    rect[H // 5:H // 5 + H // 2 + 1, W // 7:W // 7 + W // 3] = 1.0
    g = torch.Generator().manual_seed(77)
    discs = torch.zeros(H, W)
    for _ in range(12):
        cy, cx = float(torch.rand(1, generator=g)) * H, float(torch.rand(1, generator=g)) * W
        r = 20.0 + float(torch.rand(1, generator=g)) * min(H, W) / 8
        discs[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1.0
    strokes = torch.zeros(H, W)
    for i, wd in enumerate((1, 2, 3, 1, 2, 3)):
        y0, x0 = H // 8 + i * H // 9, W // 9 + i * W // 8
        strokes[y0:y0 + wd, W // 10:W - W // 10] = 1.0                      # horizontal
        strokes[H // 10:H - H // 10, x0:x0 + wd] = 1.0                      # vertical
        d = torch.arange(min(H, W) - 40)
        for t in range(wd):                                                 # diagonal, wd px wide along x
            strokes[d + 20, (d + 20 + 37 * i + t) % W] = 1.0
    return {'rectangle': rect[None, None].contiguous(), 'discs': discs[None, None].contiguous(), 'strokes': strokes[None, None].contiguous()}



def threshold_ref(x: torch.Tensor, thr: float) -> torch.Tensor:
    """x >= (float)thr ? 1 : 0 -- the comparison in fp32, as the kernel gets ``thr`` as a float argument."""
    return (x >= float(np.float32(thr))).to(x.dtype)


def erode_ref(x: torch.Tensor, se: torch.Tensor, max_val: float = 1e4) -> torch.Tensor:
    """kornia.morphology.erosion (flat element, geodesic border) as a running minimum over the shifted members of the FLIPPED element: no
    unfold, so it runs at 2048^2.  A minimum of inputs: nothing is rounded, the dtype of ``x`` is kept."""
    kh, kw = se.shape
    oy, ox = kh // 2, kw // 2
    H, W = x.shape[-2:]
    sef = se.flip(0, 1)
    out = torch.full_like(x, max_val)
    for ky in range(kh):
        for kx in range(kw):
            if float(sef[ky, kx]) == 0.0:
                continue
            dy, dx = ky - oy, kx - ox                                   # out[y, x] = min(out[y, x], x[y + dy, x + dx]) where that is inside
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            o = out[..., y0:y1, x0:x1]
            torch.minimum(o, x[..., y0 + dy:y1 + dy, x0 + dx:x1 + dx], out=o)
    return out


# -- masked L1 -----------------------------------------------------------------------------------------------------------------------

def l1_select(mask: torch.Tensor, C: int, select_ge: bool, thr: float = 1e-8) -> torch.Tensor:
    """bool [B, C, H, W]: the elements the masked-L1 kernels select (a 1-channel mask is broadcast over the channels)."""
    m = mask.expand(mask.shape[0], C, *mask.shape[2:])
    t = float(np.float32(thr))
    return (m >= t) if select_ge else (m < t)


def l1_terms(pred: torch.Tensor, target: torch.Tensor, sel: torch.Tensor):
    """Per image (sum, count): |pred - target| formed in fp32, summed in fp64 over the selection."""
    d = (pred - target).abs().double() * sel
    return d.flatten(1).sum(1), sel.flatten(1).sum(1).double()


def l1_grad(pred: torch.Tensor, target: torch.Tensor, sel: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """scale_b * sign(pred - target) * selected, fp32; ``scale`` fp32 [B]."""
    return torch.sign(pred - target) * sel * scale.float().view(-1, 1, 1, 1)


# -- Adam ----------------------------------------------------------------------------------------------------------------------------

def adam_constants(lr: float, step: int, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8):
    """The fp32 constants lama_adam_step hands its kernel, as the host code forms them (float arguments, bias corrections in double, then
    rounded to float), promoted to python floats."""
    f = lambda v: float(np.float32(v))          # noqa: E731
    b1f, b2f = f(b1), f(b2)
    return dict(lr=f(lr), b1=b1f, b2=b2f, eps=f(eps), c1=f(np.float32(1.0) - np.float32(b1)), c2=f(np.float32(1.0) - np.float32(b2)),
                bc1=f(1.0 - b1f ** step), bc2s=f(np.sqrt(1.0 - b2f ** step)))


def adam_step64(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, k: dict):
    """One step of the kernel's expression in fp64 from fp32 state: returns (p, m, v, m_abs, upd_abs) -- m_abs = b1 |m| + c1 |g| (what the
    rounding of m scales with when the two terms cancel), upd_abs = (lr / bc1) m_abs / denom."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    m_abs = k['b1'] * m.abs() + k['c1'] * g.abs()
    m = k['b1'] * m + k['c1'] * g
    v = k['b2'] * v + k['c2'] * g * g
    denom = v.sqrt() / k['bc2s'] + k['eps']
    a = k['lr'] / k['bc1']
    return p - a * (m / denom), m, v, m_abs, a * (m_abs / denom)


# -- reflect-pad adjoint / ring ------------------------------------------------------------------------------------------------------

def fold64(gp: torch.Tensor, pad: int) -> torch.Tensor:
    """Adjoint of F.pad(mode='reflect') by fp64 autograd: gp [B, C, H + 2 pad, W + 2 pad] -> [B, C, H, W]."""
    B, C, Hp, Wp = gp.shape
    x = torch.zeros(B, C, Hp - 2 * pad, Wp - 2 * pad, dtype=torch.float64, requires_grad=True)
    F.pad(x, (pad,) * 4, mode='reflect').backward(gp.double())
    return x.grad


def ring64(gy: torch.Tensor, wd: torch.Tensor):
    """The one-pixel frame of gp = conv2d(zero_pad_2(gy), wd) (gy [B, Cin, H, W], wd = w' [Cout, Cin, 3, 3]) in fp64, from strips only:
    (top [B, Cout, W + 2], bottom, left [B, Cout, H], right) in the layout of lama_dgrad_ring_fwd."""
    g = F.pad(gy.double(), (2,) * 4)
    w = wd.double()
    top, bot = F.conv2d(g[:, :, :3], w)[:, :, 0], F.conv2d(g[:, :, -3:], w)[:, :, 0]
    left, right = F.conv2d(g[:, :, :, :3], w)[:, :, 1:-1, 0], F.conv2d(g[:, :, :, -3:], w)[:, :, 1:-1, 0]
    return top, bot, left, right


def assemble_padded(interior: torch.Tensor, top, bot, left, right) -> torch.Tensor:
    """[B, C, H + 2, W + 2] fp64 from its interior and its frame."""
    B, C, H, W = interior.shape
    gp = torch.zeros(B, C, H + 2, W + 2, dtype=torch.float64)
    gp[:, :, 1:-1, 1:-1] = interior.double()
    gp[:, :, 0], gp[:, :, -1] = top.double(), bot.double()
    gp[:, :, 1:-1, 0], gp[:, :, 1:-1, -1] = left.double(), right.double()
    return gp
