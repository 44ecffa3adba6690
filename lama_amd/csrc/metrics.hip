// Quality metrics of the evaluator: SSIM, saicinpainting/evaluation/losses/ssim.py:46-71.
//
//   mu = W * x (depthwise window_size x window_size gaussian, sigma 1.5, ZERO padding window_size / 2: F.conv2d(padding=...)),
//   sigma_xx = W * x^2 - mu_x^2, sigma_xy = W * xy - mu_x mu_y,
//   ssim = (2 mu_x mu_y + C1)(2 sigma_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(sigma_xx + sigma_yy + C2)),  C1 = 0.01^2, C2 = 0.03^2,
//   one value per image = mean over (C, H, W) (size_average=False: ssim_map.mean(1).mean(1).mean(1)).
//
// HBM-bound (two reads of each image, nothing written but one partial sum per tile): one workgroup = one 16 x 32 tile of one
// (image, channel) plane; the tile + halo of both images goes to LDS once, the window is applied separably (the reference's 2-D
// window IS the outer product of the normalised 1-D one) to the five maps x, y, x^2, y^2, xy -- horizontal pass into LDS, vertical
// pass in registers --, the tile's SSIM sum is reduced in the workgroup and written to a per-tile slot; a second launch adds the
// slots of an image in a fixed order (bit-reproducible, no atomics).
#include "common.h"

namespace {
constexpr int SS_TH = 16, SS_TW = 32, SS_MAXR = 7, SS_THREADS = 256;

struct SsimParams {
    const float* a; long long a_bs;
    const float* b; long long b_bs;
    float* partial;          // [B][C * tiles_y * tiles_x]
    int C, H, W, tiles_x, tiles_y, r;
    float g[2 * SS_MAXR + 1];
};

__global__ __launch_bounds__(SS_THREADS) void ssim_tile_kernel(SsimParams p) {
    // dynamic LDS (common.h: no static __shared__): [a tile + halo][b tile + halo][5 horizontally filtered maps][per-wave sums]
    constexpr int NPATCH = (SS_TH + 2 * SS_MAXR) * (SS_TW + 2 * SS_MAXR), NHZ = (SS_TH + 2 * SS_MAXR) * SS_TW;
    float* sa = reinterpret_cast<float*>(lama_smem);
    float* sb = sa + NPATCH;
    float (*hz)[NHZ] = reinterpret_cast<float (*)[NHZ]>(sb + NPATCH);
    float* red = sb + NPATCH + 5 * NHZ;
    const int r = p.r, PH = SS_TH + 2 * r, PW = SS_TW + 2 * r;
    int t = blockIdx.x;
    const int tx = t % p.tiles_x; t /= p.tiles_x;
    const int ty = t % p.tiles_y; t /= p.tiles_y;
    const int c = t % p.C, img = t / p.C;
    const float* pa = p.a + (long long)img * p.a_bs + (long long)c * p.H * p.W;
    const float* pb = p.b + (long long)img * p.b_bs + (long long)c * p.H * p.W;
    const int y0 = ty * SS_TH - r, x0 = tx * SS_TW - r;
    for (int i = threadIdx.x; i < PH * PW; i += SS_THREADS) {
        const int py = i / PW, px = i - py * PW;
        const int y = y0 + py, x = x0 + px;
        const bool in = y >= 0 && y < p.H && x >= 0 && x < p.W;
        sa[i] = in ? pa[(long long)y * p.W + x] : 0.0f;
        sb[i] = in ? pb[(long long)y * p.W + x] : 0.0f;
    }
    __syncthreads();
    const int K = 2 * r + 1;
    for (int i = threadIdx.x; i < PH * SS_TW; i += SS_THREADS) {   // horizontal pass
        const int py = i / SS_TW, ox = i - py * SS_TW;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
        for (int k = 0; k < K; ++k) {
            const float w = p.g[k], u = sa[py * PW + ox + k], v = sb[py * PW + ox + k];
            s0 += w * u; s1 += w * v; s2 += w * (u * u); s3 += w * (v * v); s4 += w * (u * v);
        }
        hz[0][i] = s0; hz[1][i] = s1; hz[2][i] = s2; hz[3][i] = s3; hz[4][i] = s4;
    }
    __syncthreads();
    float acc = 0.0f;
    for (int i = threadIdx.x; i < SS_TH * SS_TW; i += SS_THREADS) {   // vertical pass + the SSIM map
        const int oy = i / SS_TW, ox = i - oy * SS_TW;
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
        for (int k = 0; k < K; ++k) {
            const float w = p.g[k];
            const int j = (oy + k) * SS_TW + ox;
            m1 += w * hz[0][j]; m2 += w * hz[1][j]; e11 += w * hz[2][j]; e22 += w * hz[3][j]; e12 += w * hz[4][j];
        }
        const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
        const float s11 = e11 - m11, s22 = e22 - m22, s12 = e12 - m12;
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
        const float v = ((2.0f * m12 + C1) * (2.0f * s12 + C2)) / ((m11 + m22 + C1) * (s11 + s22 + C2));
        if (ty * SS_TH + oy < p.H && tx * SS_TW + ox < p.W) acc += v;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int w = 0; w < SS_THREADS / 64; ++w) s += red[w];
        p.partial[blockIdx.x] = s;
    }
}

// out[img] = (sum of the image's tile sums, pairwise in a fixed order) / (C * H * W)
__global__ __launch_bounds__(256) void ssim_reduce_kernel(const float* partial, float* out, int per_image, float inv_n) {
    double* red = reinterpret_cast<double*>(lama_smem);
    const float* src = partial + (long long)blockIdx.x * per_image;
    double s = 0.0;
    for (int i = threadIdx.x; i < per_image; i += 256) s += (double)src[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(red[0] * (double)inv_n);
}
}  // namespace

extern "C" size_t lama_ssim_workspace_bytes(int32_t batch, int32_t C, int32_t H, int32_t W) {
    if (batch <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)batch * C * lama_ceil_div(H, SS_TH) * lama_ceil_div(W, SS_TW) * sizeof(float);
}

extern "C" int lama_ssim_fwd(void* stream, const lama_tensor* img1, const lama_tensor* img2, int32_t batch, int32_t window_size,
                             const float* window1d, float* out, void* workspace, size_t workspace_bytes) {
    auto ok = [](const lama_tensor* t) {
        return t && t->ptr && t->dtype == LAMA_DT_F32 && t->C > 0 && t->H > 0 && t->W > 0 && t->batch_stride >= (int64_t)t->C * t->H * t->W;
    };
    if (!ok(img1) || !ok(img2) || batch <= 0 || !out || !window1d || img1->C != img2->C || img1->H != img2->H || img1->W != img2->W)
        return LAMA_ERR_BAD_ARG;
    if (window_size < 1 || window_size > 2 * SS_MAXR + 1 || (window_size & 1) == 0) return LAMA_ERR_UNSUPPORTED;   // odd windows up to 15
    if (!workspace || workspace_bytes < lama_ssim_workspace_bytes(batch, img1->C, img1->H, img1->W)) return LAMA_ERR_BAD_ARG;
    SsimParams p;
    memset(&p, 0, sizeof(p));
    p.a = (const float*)img1->ptr; p.a_bs = img1->batch_stride;
    p.b = (const float*)img2->ptr; p.b_bs = img2->batch_stride;
    p.partial = (float*)workspace;
    p.C = img1->C; p.H = img1->H; p.W = img1->W;
    p.tiles_x = lama_ceil_div(p.W, SS_TW); p.tiles_y = lama_ceil_div(p.H, SS_TH);
    p.r = window_size / 2;
    for (int i = 0; i < window_size; ++i) p.g[i] = window1d[i];   // HOST array: the normalised 1-D gaussian of ssim.py:36-40
    const int per_image = p.C * p.tiles_x * p.tiles_y;
    constexpr size_t tile_lds = ((size_t)2 * (SS_TH + 2 * SS_MAXR) * (SS_TW + 2 * SS_MAXR) + 5 * (SS_TH + 2 * SS_MAXR) * SS_TW + SS_THREADS / 64) * sizeof(float);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3(batch * per_image), dim3(SS_THREADS), tile_lds, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    hipLaunchKernelGGL(ssim_reduce_kernel, dim3(batch), dim3(256), 256 * sizeof(double), (hipStream_t)stream, (const float*)workspace, out, per_image,
                       1.0f / ((float)p.C * (float)p.H * (float)p.W));
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// ----------------------------------------------------------------------------------------------------------------------------
// LPIPS (VGG-16, net-lin), saicinpainting/evaluation/losses/lpips.py: the memory-bound part around the thirteen 3x3 convs.
//
//   scale:  y = ((2 x - 1) - shift_c) / scale_c of BOTH inputs into the two halves of one [2B, 3, H, W] tensor (lpips.py:603-610): the
//           backbone then runs pred and target as one batch.
//   layer:  acc[b] += (1 / (h w)) sum_pixels sum_c w_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2   (lpips.py:45-47, 578-586)
//           and, in the same launch, max_pool2d(., 2, 2) of both maps (the next slice's input): every feature value is read from HBM once.
//
// One thread = one 2 x 2 quad of pixels (the pool window), 64 quads per workgroup along the row-major quad order (loads coalesce along w),
// the channels dealt round-robin to the workgroup's four waves.  ONE pass over the channels with five running sums per pixel,
//   S0 = sum f0^2, S1 = sum f1^2, A = sum w f0^2, B = sum w f1^2, X = sum w f0 f1,   d = (A a^2 - X a b) + (B b^2 - X a b),  a = 1 / (sqrt S0 + eps),
// kept in fp64: the product of two fp32 values is exact in fp64, so what the expansion cancels when f0 ~ f1 is 2^-53 of the terms, not 2^-24
// (DESIGN.md), and with f0 == f1 the two brackets are bitwise 0.  The kernel is HBM-bound: the fp64 VALU work hides behind the loads.
// Per-workgroup sums go to a slot each; a second launch adds an image's slots in a fixed order (no atomics: two runs are bit-identical).
namespace {
constexpr int LP_QUADS = 64, LP_SLICES = 4, LP_THREADS = LP_QUADS * LP_SLICES, LP_NSUM = 20;

struct LpipsScaleParams {
    const float* x0; long long x0_bs;
    const float* x1; long long x1_bs;
    float* y; long long y_bs;
    int batch, plane, normalize;     // plane = H * W
    float shift[3], scale[3];
};

__global__ __launch_bounds__(256) void lpips_scale_kernel(LpipsScaleParams p) {
    const int img = blockIdx.y;                                  // 0 .. 2 batch - 1: first the images of x0, then those of x1
    const float* src = img < p.batch ? p.x0 + (long long)img * p.x0_bs : p.x1 + (long long)(img - p.batch) * p.x1_bs;
    float* dst = p.y + (long long)img * p.y_bs;
    const long long n = 3ll * p.plane;
    const long long base = (long long)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long i = base + 256 * k;
        if (i < n) {
            const int c = (int)(i / p.plane);
            float v = src[i];
            if (p.normalize) v = 2.0f * v - 1.0f;
            dst[i] = (v - p.shift[c]) / p.scale[c];
        }
    }
}

struct LpipsLayerParams {
    const float* f0; long long f0_bs;
    const float* f1; long long f1_bs;
    float* p0; long long p0_bs;      // null: no pooled output
    float* p1; long long p1_bs;
    const float* w;                  // [C]
    double* partial;                 // [batch][tiles]
    int C, H, W, qh, qw, tiles;
};

template <bool VEC2>
__device__ __forceinline__ void lpips_load_quad(const float* p, int o00, int W, bool v00, bool v01, bool v10, bool v11, float (&q)[4]) {
    if constexpr (VEC2) {            // W even, 8-byte aligned planes: a quad row is one 8-byte load (v01 == v00, v11 == v10)
        const float2 z = make_float2(0.0f, 0.0f);
        const float2 t = v00 ? *reinterpret_cast<const float2*>(p + o00) : z;
        const float2 u = v10 ? *reinterpret_cast<const float2*>(p + o00 + W) : z;
        q[0] = t.x; q[1] = t.y; q[2] = u.x; q[3] = u.y;
    } else {
        q[0] = v00 ? p[o00] : 0.0f;
        q[1] = v01 ? p[o00 + 1] : 0.0f;
        q[2] = v10 ? p[o00 + W] : 0.0f;
        q[3] = v11 ? p[o00 + W + 1] : 0.0f;
    }
}

template <bool VEC2>
__global__ __launch_bounds__(LP_THREADS) void lpips_layer_kernel(LpipsLayerParams p) {
    double* red = reinterpret_cast<double*>(lama_smem);          // [LP_SLICES - 1][LP_NSUM][LP_QUADS]
    const int lane = threadIdx.x & 63;
    const int slice = LAMA_WAVE_UNIFORM((int)(threadIdx.x >> 6));
    const int tile = blockIdx.x % p.tiles, img = blockIdx.x / p.tiles;
    const int q = tile * LP_QUADS + lane;
    const bool valid = q < p.qh * p.qw;
    const int qy = valid ? q / p.qw : 0, qx = valid ? q - (q / p.qw) * p.qw : 0;
    const int y0 = 2 * qy, x0 = 2 * qx;
    const bool v00 = valid, v01 = valid && x0 + 1 < p.W, v10 = valid && y0 + 1 < p.H, v11 = v01 && v10;
    const int o00 = y0 * p.W + x0;
    const long long plane = (long long)p.H * p.W;
    const int ph = p.H >> 1, pw = p.W >> 1;
    const long long pplane = (long long)ph * pw;
    const float* f0 = p.f0 + (long long)img * p.f0_bs;
    const float* f1 = p.f1 + (long long)img * p.f1_bs;
    float* o0 = p.p0 ? p.p0 + (long long)img * p.p0_bs + (long long)qy * pw + qx : nullptr;
    float* o1 = p.p1 ? p.p1 + (long long)img * p.p1_bs + (long long)qy * pw + qx : nullptr;
    double s[LP_NSUM];               // [pixel of the quad][S0, S1, A, B, X]
#pragma unroll
    for (int i = 0; i < LP_NSUM; ++i) s[i] = 0.0;
#pragma unroll 2
    for (int c = slice; c < p.C; c += LP_SLICES) {
        float a[4], b[4];
        lpips_load_quad<VEC2>(f0 + c * plane, o00, p.W, v00, v01, v10, v11, a);
        lpips_load_quad<VEC2>(f1 + c * plane, o00, p.W, v00, v01, v10, v11, b);
        const double w = (double)p.w[c];
        if (v11) {                   // a whole 2 x 2 window: floor semantics, an odd last row / column is in the distance but not in the pool
            if (o0) o0[c * pplane] = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
            if (o1) o1[c * pplane] = fmaxf(fmaxf(b[0], b[1]), fmaxf(b[2], b[3]));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {                            // pixels outside the plane were loaded as 0: they add nothing
            const double da = (double)a[k], db = (double)b[k], wa = w * da, wb = w * db;
            s[5 * k + 0] = fma(da, da, s[5 * k + 0]);
            s[5 * k + 1] = fma(db, db, s[5 * k + 1]);
            s[5 * k + 2] = fma(wa, da, s[5 * k + 2]);
            s[5 * k + 3] = fma(wb, db, s[5 * k + 3]);
            s[5 * k + 4] = fma(wa, db, s[5 * k + 4]);
        }
    }
    if (slice > 0) {
#pragma unroll
        for (int i = 0; i < LP_NSUM; ++i) red[((slice - 1) * LP_NSUM + i) * LP_QUADS + lane] = s[i];
    }
    __syncthreads();
    if (slice == 0) {
        for (int j = 0; j < LP_SLICES - 1; ++j) {                // fixed order: slice 0 + 1 + 2 + 3
#pragma unroll
            for (int i = 0; i < LP_NSUM; ++i) s[i] += red[(j * LP_NSUM + i) * LP_QUADS + lane];
        }
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // no contraction here: fma(A ia, ia, -x) would subtract the ROUNDED x from the exact product, and f0 == f1 would not give 0
#pragma clang fp contract(off)
            const double ia = 1.0 / (sqrt(s[5 * k + 0]) + 1e-10), ib = 1.0 / (sqrt(s[5 * k + 1]) + 1e-10);
            const double x = s[5 * k + 4] * ia * ib;
            v += (s[5 * k + 2] * ia * ia - x) + (s[5 * k + 3] * ib * ib - x);
        }
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) p.partial[blockIdx.x] = v;
    }
}

// acc[img] += (float)((sum of the image's workgroup sums, in a fixed order) / (h w))
__global__ __launch_bounds__(256) void lpips_reduce_kernel(const double* partial, float* acc, int per_image, double inv_n) {
    double* red = reinterpret_cast<double*>(lama_smem);
    const double* src = partial + (long long)blockIdx.x * per_image;
    double s = 0.0;
    for (int i = threadIdx.x; i < per_image; i += 256) s += src[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) acc[blockIdx.x] += (float)(red[0] * inv_n);
}

bool lpips_f32_view(const lama_tensor* t) {
    return t && t->ptr && t->dtype == LAMA_DT_F32 && t->C > 0 && t->H > 0 && t->W > 0 && t->batch_stride >= (int64_t)t->C * t->H * t->W;
}
}  // namespace

extern "C" int lama_lpips_scale_fwd(void* stream, const lama_tensor* x0, const lama_tensor* x1, const lama_tensor* y, int32_t batch,
                                    int32_t normalize, const float* shift, const float* scale) {
    if (!lpips_f32_view(x0) || !lpips_f32_view(x1) || !lpips_f32_view(y) || batch <= 0 || !shift || !scale) return LAMA_ERR_BAD_ARG;
    if (x0->C != 3 || x1->C != 3 || y->C != 3 || x0->H != y->H || x0->W != y->W || x1->H != y->H || x1->W != y->W) return LAMA_ERR_BAD_ARG;
    if (batch > 32767 || (int64_t)y->H * y->W > (int64_t)0x7fffffff / 3) return LAMA_ERR_UNSUPPORTED;
    LpipsScaleParams p;
    memset(&p, 0, sizeof(p));
    p.x0 = (const float*)x0->ptr; p.x0_bs = x0->batch_stride;
    p.x1 = (const float*)x1->ptr; p.x1_bs = x1->batch_stride;
    p.y = (float*)y->ptr; p.y_bs = y->batch_stride;
    p.batch = batch; p.plane = y->H * y->W; p.normalize = normalize != 0;
    for (int c = 0; c < 3; ++c) {
        if (!(scale[c] != 0.0f)) return LAMA_ERR_BAD_ARG;
        p.shift[c] = shift[c]; p.scale[c] = scale[c];            // HOST arrays: ScalingLayer.shift / .scale
    }
    hipLaunchKernelGGL(lpips_scale_kernel, dim3(lama_ceil_div(3 * p.plane, 1024), 2 * batch), dim3(256), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" size_t lama_lpips_layer_workspace_bytes(int32_t batch, int32_t C, int32_t H, int32_t W) {
    if (batch <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)batch * lama_ceil_div64((int64_t)lama_ceil_div(H, 2) * lama_ceil_div(W, 2), LP_QUADS) * sizeof(double);
}

extern "C" int lama_lpips_layer_fwd(void* stream, const lama_tensor* f0, const lama_tensor* f1, int32_t batch, const float* w, float* acc,
                                    const lama_tensor* pool0, const lama_tensor* pool1, void* workspace, size_t workspace_bytes) {
    if (!lpips_f32_view(f0) || !lpips_f32_view(f1) || batch <= 0 || !w || !acc || f0->C != f1->C || f0->H != f1->H || f0->W != f1->W)
        return LAMA_ERR_BAD_ARG;
    const int C = f0->C, H = f0->H, W = f0->W;
    const bool pool = pool0 && pool0->ptr;
    if (pool != (pool1 && pool1->ptr)) return LAMA_ERR_BAD_ARG;                       // both pooled maps or neither
    if (pool) {
        if (H < 2 || W < 2) return LAMA_ERR_BAD_ARG;                                  // max_pool2d(2, 2) of such a plane is empty
        for (const lama_tensor* t : {pool0, pool1})
            if (!lpips_f32_view(t) || t->C != C || t->H != H / 2 || t->W != W / 2) return LAMA_ERR_BAD_ARG;
    }
    if ((int64_t)H * W > 0x7fffffff) return LAMA_ERR_UNSUPPORTED;
    const int64_t tiles = lama_ceil_div64((int64_t)lama_ceil_div(H, 2) * lama_ceil_div(W, 2), LP_QUADS);
    if (tiles * batch > 0x7fffffff) return LAMA_ERR_UNSUPPORTED;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < lama_lpips_layer_workspace_bytes(batch, C, H, W)) return LAMA_ERR_WORKSPACE;
    LpipsLayerParams p;
    memset(&p, 0, sizeof(p));
    p.f0 = (const float*)f0->ptr; p.f0_bs = f0->batch_stride;
    p.f1 = (const float*)f1->ptr; p.f1_bs = f1->batch_stride;
    if (pool) {
        p.p0 = (float*)pool0->ptr; p.p0_bs = pool0->batch_stride;
        p.p1 = (float*)pool1->ptr; p.p1_bs = pool1->batch_stride;
    }
    p.w = w; p.partial = (double*)workspace;
    p.C = C; p.H = H; p.W = W; p.qh = lama_ceil_div(H, 2); p.qw = lama_ceil_div(W, 2); p.tiles = (int)tiles;
    constexpr size_t lds = (size_t)(LP_SLICES - 1) * LP_NSUM * LP_QUADS * sizeof(double);
    // 8-byte quad rows: even W (then every row and, with an even plane or batch stride, every plane starts on an even element) + aligned bases
    const bool vec2 = (W & 1) == 0 && (((uintptr_t)p.f0 | (uintptr_t)p.f1) & 7) == 0 && (((int64_t)H * W) & 1) == 0 && ((p.f0_bs | p.f1_bs) & 1) == 0;
    if (vec2)
        hipLaunchKernelGGL(lpips_layer_kernel<true>, dim3((unsigned)(tiles * batch)), dim3(LP_THREADS), lds, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(lpips_layer_kernel<false>, dim3((unsigned)(tiles * batch)), dim3(LP_THREADS), lds, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    hipLaunchKernelGGL(lpips_reduce_kernel, dim3(batch), dim3(256), 256 * sizeof(double), (hipStream_t)stream, (const double*)workspace, acc, (int)tiles,
                       1.0 / ((double)H * (double)W));
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}
