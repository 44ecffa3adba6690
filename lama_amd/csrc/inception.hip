// The kernels of the FID feature extractor (Inception-v3 up to pool3; saicinpainting/evaluation/losses/fid/inception.py) that the generator's
// library did not have: rectangular zero-padded convolutions, the two 3x3 poolings, the global average pool and the input resize.
//
// lama_conv2d_rect_fwd: implicit GEMM on the 16-bit MFMA with the 3-term split of conv_split3.inc (w x ~= wh xh + wh xl + wl xh, fp32 accumulation):
//   M = cout, N = B Ho Wo (the pixels of ALL images in one flat list: the planes are 35^2, 17^2, 8^2, a tile of one image's rows would be
//   mostly ragged edge), K = (tap, channel) with the channels of a tap padded to a multiple of 8, so that the 8 K elements a lane feeds to one
//   v_mfma_f32_32x32x16 (k = 8 (lane >> 5) + j) are 8 consecutive channels of ONE tap: one bounds test and one address per lane and k-step,
//   8 loads a plane apart, each coalesced over the 32 pixels of the half-wave.
//   * weights: pre-split and stored in A-fragment order by lama_conv2d_rect_pack_weight ([k-step][32-row fragment][hi | lo][lane][8 halves],
//     BatchNorm scale folded, M tail and K tail zero): a wave reads its fragments straight from L2, 16 bytes per lane, fully coalesced;
//   * activations: gathered from global memory by the wave that multiplies them, split once, one k-step ahead of the MFMAs; no LDS, no barrier;
//   * a wave owns TM x 1 fragments of 32 x 32 outputs, a workgroup WM x WN waves.  The host takes the largest tile that still gives every CU a
//     workgroup (8 x 8 planes at B = 16 are 1024 pixels: 32 x 32 tiles of a 384-channel layer are 384 workgroups); M and N are split, K never
//     is: every output is one accumulator's k-ordered sum, bit-identical run to run.
#include "common.h"

typedef float ic_f32x16 __attribute__((ext_vector_type(16)));
typedef float ic_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned ic_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short ic_u16x2 __attribute__((ext_vector_type(2)));

namespace {

template <bool F16> struct IcHalf { typedef __bf16 T; };
template <> struct IcHalf<true> { typedef _Float16 T; };

// (hi, lo) split of two floats into two packed 16-bit pairs (element 0 in the low half); rw: range watch of the f16 split (conv_split3.inc)
template <bool F16>
__device__ __forceinline__ void ic_split2(float a, float b, unsigned& hi, unsigned& lo, unsigned& rw) {
    typedef typename IcHalf<F16>::T __attribute__((ext_vector_type(2))) h2;
    ic_f32x2 v = {a, b};
    h2 h = __builtin_convertvector(v, h2);
    ic_f32x2 r = v - __builtin_convertvector(h, ic_f32x2);
    h2 l = __builtin_convertvector(r, h2);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
    if constexpr (F16)
        rw = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(ic_u16x2, rw), __builtin_bit_cast(ic_u16x2, hi & 0x7fff7fffu)));
}

template <bool F16>
__device__ __forceinline__ ic_f32x16 ic_mfma(ic_u32x4 a, ic_u32x4 b, ic_f32x16 c) {
    typedef typename IcHalf<F16>::T __attribute__((ext_vector_type(8))) h8;
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

struct RcParams {
    const float* x; long long x_bs;
    int C, H, W;
    const char* w;          // [k-step][fragment][hi | lo][lane][8 halves]
    int MF, KS;             // 32-row fragments, k-steps of 16
    const float* bias;
    float* y; long long y_bs;
    int M, Ho, Wo, Ntot;    // Ntot = B Ho Wo
    int kh, kw, stride, ph, pw, Cp;   // Cp = cin rounded up to 8
    int act, MT;
    unsigned* range_flag;
};

template <bool F16, int TM, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void rc_conv_kernel(RcParams p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave - wm * WN;
    const int kh8 = lane >> 5, l31 = lane & 31;
    const int L = lama_xcd_remap(blockIdx.x, gridDim.x);
    const int mt = L % p.MT, nt = L / p.MT;
    const int n = (nt * WN + wn) * 32 + l31;
    const bool nvalid = n < p.Ntot;
    const int HoWo = p.Ho * p.Wo, HW = p.H * p.W;
    const int b = nvalid ? n / HoWo : 0;
    const int rem = nvalid ? n - b * HoWo : 0;
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    const int iy0 = oy * p.stride - p.ph, ix0 = ox * p.stride - p.pw;
    const float* xb = p.x + (long long)b * p.x_bs;
    const ic_u32x4* wp = reinterpret_cast<const ic_u32x4*>(p.w);

    int F[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int f = (mt * WM + wm) * TM + i;
        F[i] = f < p.MF ? f : p.MF - 1;          // fragments past M: read a real one, never stored
    }
    ic_f32x16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    // K position of this lane's 8 elements: channels c0 .. c0 + 7 of tap (ky, kx); ky >= kh = the zero-filled K tail
    int c0 = 8 * kh8, ky = 0, kx = 0;
    auto norm = [&]() {
        while (c0 >= p.Cp) {
            c0 -= p.Cp;
            if (++kx == p.kw) { kx = 0; ++ky; }
        }
    };
    norm();
    float v[8];
    ic_u32x4 ah[TM], al[TM];
    auto load = [&](int ks) {
        const int iy = iy0 + ky, ix = ix0 + kx;
        const bool ok = nvalid && ky < p.kh && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        const int off = ok ? c0 * HW + iy * p.W + ix : 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (ok && c0 + j < p.C) ? xb[off + j * HW] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int o = ((ks * p.MF + F[i]) * 2) * 64 + lane;
            ah[i] = wp[o];
            al[i] = wp[o + 64];
        }
    };
    unsigned rw = 0;
    load(0);
    for (int ks = 0; ks < p.KS; ++ks) {
        unsigned hh[4], ll[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ic_split2<F16>(v[2 * e], v[2 * e + 1], hh[e], ll[e], rw);
        const ic_u32x4 bh = {hh[0], hh[1], hh[2], hh[3]}, bl = {ll[0], ll[1], ll[2], ll[3]};
        ic_u32x4 ch[TM], cl[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) { ch[i] = ah[i]; cl[i] = al[i]; }
        if (ks + 1 < p.KS) {                     // the next k-step's operands are in flight while this one multiplies
            c0 += 16;
            norm();
            load(ks + 1);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            acc[i] = ic_mfma<F16>(ch[i], bh, acc[i]);
            acc[i] = ic_mfma<F16>(ch[i], bl, acc[i]);
            acc[i] = ic_mfma<F16>(cl[i], bh, acc[i]);
        }
    }
    if constexpr (F16) {
        if (p.range_flag != nullptr && ((rw & 0xffffu) >= 0x7c00u || (rw >> 16) >= 0x7c00u)) atomicOr(p.range_flag, 1u);
    }

    // epilogue: D[row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)][col = lane & 31]
    if (!nvalid) return;
    float* yb = p.y + (long long)b * p.y_bs + rem;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int f = (mt * WM + wm) * TM + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = f * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh8;
            if (m < p.M) {
                float o = acc[i][r];
                if (p.bias) o += p.bias[m];
                if (p.act == LAMA_ACT_RELU) o = fmaxf(o, 0.0f);
                yb[(long long)m * HoWo] = o;
            }
        }
    }
}

struct RcPackParams {
    const float* w;         // [cout][cin][kh][kw]
    const float* scale;     // [cout] or null
    ic_u32x4* dst;
    int M, C, T, Cp, MF, KS;
};

template <bool F16>
__global__ __launch_bounds__(256) void rc_pack_kernel(RcPackParams p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.KS * p.MF * 64) return;
    const int lane = idx & 63, f = (idx >> 6) % p.MF, ks = (idx >> 6) / p.MF;
    const int row = f * 32 + (lane & 31), k0 = ks * 16 + 8 * (lane >> 5);
    const int t = k0 / p.Cp, c0 = k0 - t * p.Cp;
    const float sc = (p.scale && row < p.M) ? p.scale[row] : 1.0f;
    unsigned hh[4], ll[4], rw = 0;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        v[j] = (row < p.M && t < p.T && c < p.C) ? p.w[((long long)row * p.C + c) * p.T + t] * sc : 0.0f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) ic_split2<F16>(v[2 * e], v[2 * e + 1], hh[e], ll[e], rw);
    const int o = ((ks * p.MF + f) * 2) * 64 + lane;
    p.dst[o] = ic_u32x4{hh[0], hh[1], hh[2], hh[3]};
    p.dst[o + 64] = ic_u32x4{ll[0], ll[1], ll[2], ll[3]};
}

bool ic_view(const lama_tensor* t) {
    return t && t->ptr && t->dtype == LAMA_DT_F32 && t->C > 0 && t->H > 0 && t->W > 0 && t->batch_stride >= (int64_t)t->C * t->H * t->W;
}
bool rc_geom(int cout, int cin, int kh, int kw) { return cout >= 1 && cin >= 1 && kh >= 1 && kh <= 7 && kw >= 1 && kw <= 7; }
int rc_cp(int cin) { return lama_round_up(cin, 8); }
int64_t rc_ksteps(int cin, int kh, int kw) { return lama_ceil_div64((int64_t)rc_cp(cin) * kh * kw, 16); }

template <bool F16, int TM, int WM, int WN>
void rc_launch(hipStream_t st, RcParams& p) {
    p.MT = lama_ceil_div(p.MF, TM * WM);
    const int grid = p.MT * lama_ceil_div(p.Ntot, 32 * WN);
    hipLaunchKernelGGL((rc_conv_kernel<F16, TM, WM, WN>), dim3(grid), dim3(64 * WM * WN), 0, st, p);
}

template <bool F16>
void rc_dispatch(hipStream_t st, RcParams& p) {
    // the largest tile (rows x pixels) that does not exceed the layer's rows and still gives each of the 256 CUs a workgroup
    auto wgs = [&](int bm, int bn) { return (long long)lama_ceil_div(p.MF * 32, bm) * lama_ceil_div(p.Ntot, bn); };
    const int rows = p.MF * 32;
    if (rows >= 128 && wgs(128, 64) >= 256) rc_launch<F16, 2, 2, 2>(st, p);
    else if (rows >= 64 && wgs(64, 64) >= 256) rc_launch<F16, 1, 2, 2>(st, p);
    else if (wgs(32, 64) >= 256) rc_launch<F16, 1, 1, 2>(st, p);
    else rc_launch<F16, 1, 1, 1>(st, p);
}

// ---- 3x3 pooling -----------------------------------------------------------------------------------------------------------------------------
struct PoolParams {
    const float* x; long long x_bs;
    float* y; long long y_bs;
    int C, H, W, Ho, Wo, stride, pad, mode;
    long long total;
};

__global__ __launch_bounds__(256) void pool3x3_kernel(PoolParams p) {
    const long long per = (long long)p.C * p.Ho * p.Wo;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / per);
        const long long r = i - (long long)b * per;
        const int ox = (int)(r % p.Wo);
        const long long r2 = r / p.Wo;
        const int oy = (int)(r2 % p.Ho), c = (int)(r2 / p.Ho);
        const float* s = p.x + (long long)b * p.x_bs + (long long)c * p.H * p.W;
        const int y0 = oy * p.stride - p.pad, x0 = ox * p.stride - p.pad;
        float m = -INFINITY, sum = 0.0f;
        int cnt = 0;
        for (int ky = 0; ky < 3; ++ky) {           // one fixed order: rows, then columns
            const int iy = y0 + ky;
            if (iy < 0 || iy >= p.H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = x0 + kx;
                if (ix < 0 || ix >= p.W) continue;
                const float v = s[(long long)iy * p.W + ix];
                if (v > m || v != v) m = v;         // F.max_pool2d: a NaN in the window is the result
                sum += v;
                ++cnt;
            }
        }
        p.y[(long long)b * p.y_bs + r] = p.mode == LAMA_POOL_MAX ? m : sum / (float)cnt;
    }
}

// ---- global average pool: one thread per (image, channel), fp64 sum in index order, one rounding ---------------------------------------------
__global__ __launch_bounds__(256) void gap_kernel(const float* x, long long x_bs, float* y, int C, int plane, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int b = i / C, c = i - b * C;
    const float* s = x + (long long)b * x_bs + (long long)c * plane;
    double a = 0.0;
    for (int k = 0; k < plane; ++k) a += (double)s[k];
    y[i] = (float)(a / (double)plane);
}

// ---- FID input: bilinear resize (align_corners = False, no antialias) of pred | target into one batch, then 2 x - 1 ---------------------------
struct FidInParams {
    const float* x0; long long x0_bs;
    const float* x1; long long x1_bs;
    float* y; long long y_bs;
    int B, H, W, Ho, Wo, resize;
    float sy, sx;
    long long total;
};

// lama_bilinear_fwd's coordinates (refine.hip): src = max(0, (dst + 0.5) scale - 0.5), i1 = min(i0 + 1, n - 1)
__device__ __forceinline__ void fid_bilin_src(int o, float scale, int n, int& i0, int& i1, float& l) {
    // one rounding (fmaf), as hipcc contracts the same expression of lama_bilinear_fwd and as ATen's area_pixel_compute_source_index is compiled:
    // the unfused form moves the weights of an inexact ratio (64 / 299) by an ulp of the coordinate
    float s = fmaf((float)o + 0.5f, scale, -0.5f);
    s = s < 0.0f ? 0.0f : s;
    i0 = (int)s;
    if (i0 > n - 1) i0 = n - 1;
    i1 = i0 + 1 < n ? i0 + 1 : n - 1;
    l = s - (float)i0;
}

__global__ __launch_bounds__(256) void fid_input_kernel(FidInParams p) {
    const long long per = 3ll * p.Ho * p.Wo;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.total; i += (long long)gridDim.x * 256) {
        const int img = (int)(i / per);
        const long long r = i - (long long)img * per;
        const int xo = (int)(r % p.Wo);
        const long long r2 = r / p.Wo;
        const int yo = (int)(r2 % p.Ho), c = (int)(r2 / p.Ho);
        const float* s = (img < p.B ? p.x0 + (long long)img * p.x0_bs : p.x1 + (long long)(img - p.B) * p.x1_bs) + (long long)c * p.H * p.W;
        float v;
        if (p.resize) {
            int y0, y1, x0, x1;
            float ly, lx;
            fid_bilin_src(yo, p.sy, p.H, y0, y1, ly);
            fid_bilin_src(xo, p.sx, p.W, x0, x1, lx);
            const float v00 = s[(long long)y0 * p.W + x0], v01 = s[(long long)y0 * p.W + x1];
            const float v10 = s[(long long)y1 * p.W + x0], v11 = s[(long long)y1 * p.W + x1];
            v = (1.0f - ly) * ((1.0f - lx) * v00 + lx * v01) + ly * ((1.0f - lx) * v10 + lx * v11);
        } else {
            v = s[(long long)yo * p.W + xo];
        }
        p.y[(long long)img * p.y_bs + r] = 2.0f * v - 1.0f;
    }
}

int ic_grid(long long total) {
    const long long g = (total + 255) / 256;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}
}  // namespace

extern "C" int64_t lama_conv2d_rect_packed_weight_bytes(int32_t cout, int32_t cin, int32_t kh, int32_t kw, int32_t precision) {
    if (!rc_geom(cout, cin, kh, kw) || (precision != LAMA_PREC_F16X3 && precision != LAMA_PREC_BF16X3)) return 0;
    const int64_t bytes = rc_ksteps(cin, kh, kw) * lama_ceil_div(cout, 32) * 2048;
    return bytes < 0x7fffffff ? bytes : 0;
}

extern "C" int lama_conv2d_rect_pack_weight(void* stream, const float* w, const float* scale, int32_t cout, int32_t cin, int32_t kh, int32_t kw,
                                            int32_t precision, void* dst) {
    if (!w || !dst || !rc_geom(cout, cin, kh, kw)) return LAMA_ERR_BAD_ARG;
    if (lama_conv2d_rect_packed_weight_bytes(cout, cin, kh, kw, precision) <= 0) return LAMA_ERR_UNSUPPORTED;
    RcPackParams p = {w, scale, (ic_u32x4*)dst, cout, cin, kh * kw, rc_cp(cin), lama_ceil_div(cout, 32), (int)rc_ksteps(cin, kh, kw)};
    const int grid = lama_ceil_div(p.KS * p.MF * 64, 256);
    if (precision == LAMA_PREC_F16X3) hipLaunchKernelGGL(rc_pack_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(rc_pack_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" int lama_conv2d_rect_fwd(void* stream, const lama_conv2d_rect_args* a) {
    if (!a || !ic_view(&a->x) || !ic_view(&a->y) || !a->w_packed || a->batch <= 0 || a->pad_h < 0 || a->pad_w < 0) return LAMA_ERR_BAD_ARG;
    if (a->act != LAMA_ACT_NONE && a->act != LAMA_ACT_RELU) return LAMA_ERR_UNSUPPORTED;
    if (a->kh < 1 || a->kh > 7 || a->kw < 1 || a->kw > 7 || (a->stride != 1 && a->stride != 2) || a->pad_h > 7 || a->pad_w > 7) return LAMA_ERR_UNSUPPORTED;
    if (a->precision != LAMA_PREC_F16X3 && a->precision != LAMA_PREC_BF16X3) return LAMA_ERR_UNSUPPORTED;
    const int H = a->x.H, W = a->x.W, cin = a->x.C, cout = a->y.C;
    if (H + 2 * a->pad_h < a->kh || W + 2 * a->pad_w < a->kw) return LAMA_ERR_BAD_ARG;
    const int Ho = (H + 2 * a->pad_h - a->kh) / a->stride + 1, Wo = (W + 2 * a->pad_w - a->kw) / a->stride + 1;
    if (a->y.H != Ho || a->y.W != Wo) return LAMA_ERR_BAD_ARG;
    if (((uintptr_t)a->w_packed & 15) || ((uintptr_t)a->x.ptr & 3) || ((uintptr_t)a->y.ptr & 3)) return LAMA_ERR_BAD_ARG;
    // 32-bit offsets inside one image and over the flat pixel list
    if ((int64_t)rc_cp(cin) * H * W > 0x7fffffff || (int64_t)a->batch * Ho * Wo > 0x7fffffff - 64 || (int64_t)cout * Ho * Wo > 0x7fffffff)
        return LAMA_ERR_UNSUPPORTED;
    if (lama_conv2d_rect_packed_weight_bytes(cout, cin, a->kh, a->kw, a->precision) <= 0) return LAMA_ERR_UNSUPPORTED;
    RcParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const float*)a->x.ptr; p.x_bs = a->x.batch_stride;
    p.C = cin; p.H = H; p.W = W;
    p.w = (const char*)a->w_packed;
    p.MF = lama_ceil_div(cout, 32); p.KS = (int)rc_ksteps(cin, a->kh, a->kw);
    p.bias = a->bias;
    p.y = (float*)a->y.ptr; p.y_bs = a->y.batch_stride;
    p.M = cout; p.Ho = Ho; p.Wo = Wo; p.Ntot = a->batch * Ho * Wo;
    p.kh = a->kh; p.kw = a->kw; p.stride = a->stride; p.ph = a->pad_h; p.pw = a->pad_w; p.Cp = rc_cp(cin);
    p.act = a->act;
    p.range_flag = a->range_flag;
    if (a->precision == LAMA_PREC_F16X3) rc_dispatch<true>((hipStream_t)stream, p);
    else rc_dispatch<false>((hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" int lama_pool3x3_fwd(void* stream, const lama_tensor* x, const lama_tensor* y, int32_t batch, int32_t mode, int32_t stride, int32_t pad) {
    if (!ic_view(x) || !ic_view(y) || batch <= 0 || x->C != y->C) return LAMA_ERR_BAD_ARG;
    if ((mode != LAMA_POOL_MAX && mode != LAMA_POOL_AVG_EXCLUDE_PAD) || (stride != 1 && stride != 2) || (pad != 0 && pad != 1)) return LAMA_ERR_UNSUPPORTED;
    if (x->H + 2 * pad < 3 || x->W + 2 * pad < 3) return LAMA_ERR_BAD_ARG;
    const int Ho = (x->H + 2 * pad - 3) / stride + 1, Wo = (x->W + 2 * pad - 3) / stride + 1;
    if (y->H != Ho || y->W != Wo) return LAMA_ERR_BAD_ARG;
    PoolParams p = {(const float*)x->ptr, x->batch_stride, (float*)y->ptr, y->batch_stride, x->C, x->H, x->W, Ho, Wo, stride, pad, mode,
                    (long long)batch * x->C * Ho * Wo};
    hipLaunchKernelGGL(pool3x3_kernel, dim3(ic_grid(p.total)), dim3(256), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" int lama_global_avgpool_fwd(void* stream, const lama_tensor* x, float* y, int32_t batch) {
    if (!ic_view(x) || !y || batch <= 0) return LAMA_ERR_BAD_ARG;
    if ((int64_t)batch * x->C > 0x7fffffff - 256 || (int64_t)x->H * x->W > 0x7fffffff) return LAMA_ERR_UNSUPPORTED;
    const int total = batch * x->C;
    hipLaunchKernelGGL(gap_kernel, dim3(lama_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)x->ptr, (long long)x->batch_stride, y,
                       (int)x->C, (int)(x->H * x->W), total);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" int lama_fid_input_fwd(void* stream, const lama_tensor* pred, const lama_tensor* target, const lama_tensor* y, int32_t batch, int32_t resize) {
    if (!ic_view(pred) || !ic_view(target) || !ic_view(y) || batch <= 0) return LAMA_ERR_BAD_ARG;
    if (pred->C != 3 || target->C != 3 || y->C != 3 || pred->H != target->H || pred->W != target->W) return LAMA_ERR_BAD_ARG;
    if (!resize && (y->H != pred->H || y->W != pred->W)) return LAMA_ERR_BAD_ARG;
    FidInParams p = {(const float*)pred->ptr, pred->batch_stride, (const float*)target->ptr, target->batch_stride, (float*)y->ptr, y->batch_stride,
                     batch, pred->H, pred->W, y->H, y->W, resize != 0, (float)pred->H / (float)y->H, (float)pred->W / (float)y->W,
                     2ll * batch * 3 * y->H * y->W};
    hipLaunchKernelGGL(fid_input_kernel, dim3(ic_grid(p.total)), dim3(256), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}
