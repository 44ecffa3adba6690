// The two data movements of the local Fourier unit of SpectralTransform (saicinpainting/training/modules/ffc.py:148-159), with
//   x1 [B, C, h, h], q = C / 4, s = h / 2:
//   lama_lfu_gather_fwd:    y[b, (2 j + i) q + c, yy, xx] = x[b, c, i s + yy, j s + xx]      c < q;  i, j in {0, 1};  yy, xx < s
//                           (the reference concatenates the row split first: the row half i is the fast index, the column half j the slow one)
//   lama_lfu_tile_add_fwd:  out[b, c, y, x] = a[b, c, y, x] + xs[b, c, y mod s, x mod s]     (xs.repeat(1, 1, 2, 2) added to x + fu(x))
//
// Both are streaming kernels: every element is read once and written once, nothing is shared between lanes, no LDS, no atomics.  A row of
// the quadrant planes has s elements, so the unit of work is a VB-byte piece of such a row, VB = the widest of 16 / 8 / 4 / 2 bytes that
// divides the row's bytes, every base pointer and every batch stride (lfu_vec_bytes): 16-byte loads and stores wherever the shapes allow,
// element accesses where they do not (s = 3 or 5: consecutive rows are never 16-byte aligned).  One 256-thread workgroup walks LFU_UNROLL
// * 256 consecutive pieces of ONE (image, channel) plane of the LARGER tensor (x1's quarter / a) -- contiguous on that side, row halves of s
// elements on the smaller; image and channel are uniform per workgroup (scalar arithmetic), a lane divides once, by the pieces per row -- and has all its loads in flight before the first store (the loads are unconditional: a lane
// past the plane's end reads the last piece again and stores nothing).
// The tile-add is one fp32 add per element; fp16 elements are widened, added in fp32 and rounded once (the correctly rounded half sum).
// out may be a itself: a lane reads the piece it writes.
#include "common.h"

namespace {
constexpr int LFU_THREADS = 256, LFU_UNROLL = 4;

// (first-class vectors, not the uint4 / uint2 structs: an array of those, copied from a load to a store, stayed an alloca that hipcc moved to LDS)
typedef unsigned lfu_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned lfu_u32x2 __attribute__((ext_vector_type(2)));
template <int VB> struct LfuVec;
template <> struct LfuVec<16> { typedef lfu_u32x4 T; };
template <> struct LfuVec<8> { typedef lfu_u32x2 T; };
template <> struct LfuVec<4> { typedef uint32_t T; };
template <> struct LfuVec<2> { typedef uint16_t T; };

struct LfuGatherParams {
    const char* x;           // channel 0 of the [B, q, h, h] view
    char* y;                 // [B, 4 q, s, s]
    long long x_bs, y_bs;    // bytes between consecutive images
    int q, s, nv, chunks;    // nv = VB-byte pieces per row of s elements; chunks = workgroups per source plane
};

struct LfuTileAddParams {
    const char* a;           // [B, C, 2 s, 2 s]
    const char* xs;          // [B, C, s, s]
    char* out;               // [B, C, 2 s, 2 s], may be a
    long long a_bs, xs_bs, out_bs;
    int C, s, nv, chunks;    // chunks = workgroups per plane of a
};

template <int VB> __global__ __launch_bounds__(LFU_THREADS) void lfu_gather_kernel(LfuGatherParams p) {
    typedef typename LfuVec<VB>::T V;
    int blk = blockIdx.x;
    const int chunk = blk % p.chunks; blk /= p.chunks;
    const int c = blk % p.q, img = blk / p.q;
    const long long quad = (long long)p.s * p.nv * VB;                // bytes of one output plane = a quarter of the source plane
    const char* src = p.x + (long long)img * p.x_bs + (long long)c * 4 * quad;
    char* dst = p.y + (long long)img * p.y_bs + (long long)c * quad;
    const long long gstep = (long long)p.q * quad;                    // between the output planes of two quadrants of one source channel
    const int pv = 4 * p.s * p.nv, rv = 2 * p.nv;                     // pieces per source plane / per source row
    const int v0 = chunk * (LFU_THREADS * LFU_UNROLL) + threadIdx.x;
    V r[LFU_UNROLL];
#pragma unroll
    for (int k = 0; k < LFU_UNROLL; ++k) {                           // no branch around a load: a lane past the end re-reads the plane's last piece
        const int v = v0 + k * LFU_THREADS;
        const unsigned vc = (unsigned)(v < pv ? v : pv - 1);
        r[k] = *reinterpret_cast<const V*>(src + (long long)vc * VB);
    }
#pragma unroll
    for (int k = 0; k < LFU_UNROLL; ++k) {
        const int v = v0 + k * LFU_THREADS;
        if (v < pv) {
            unsigned yy = (unsigned)v / (unsigned)rv, xv = (unsigned)v - yy * (unsigned)rv;
            const unsigned i = yy >= (unsigned)p.s ? 1u : 0u, j = xv >= (unsigned)p.nv ? 1u : 0u;
            yy -= i * (unsigned)p.s;
            xv -= j * (unsigned)p.nv;
            *reinterpret_cast<V*>(dst + (long long)(2u * j + i) * gstep + ((long long)yy * p.nv + xv) * VB) = r[k];
        }
    }
}

// a + b element by element over one VB-byte piece: the fp32 sum, rounded once to the element type
template <bool H, int VB> __device__ __forceinline__ typename LfuVec<VB>::T lfu_add(typename LfuVec<VB>::T a, typename LfuVec<VB>::T b) {
    typedef typename LamaAct<H>::T E;
    constexpr int N = VB / LamaAct<H>::ES;
    E ea[N], eb[N];
    __builtin_memcpy(ea, &a, VB);
    __builtin_memcpy(eb, &b, VB);
#pragma unroll
    for (int k = 0; k < N; ++k) ea[k] = (E)((float)ea[k] + (float)eb[k]);
    typename LfuVec<VB>::T r;
    __builtin_memcpy(&r, ea, VB);
    return r;
}

template <bool H, int VB> __global__ __launch_bounds__(LFU_THREADS) void lfu_tile_add_kernel(LfuTileAddParams p) {
    typedef typename LfuVec<VB>::T V;
    int blk = blockIdx.x;
    const int chunk = blk % p.chunks; blk /= p.chunks;
    const int c = blk % p.C, img = blk / p.C;
    const long long plane = 4ll * p.s * p.nv * VB;                     // bytes of one plane of a
    const char* a = p.a + (long long)img * p.a_bs + (long long)c * plane;
    const char* xs = p.xs + (long long)img * p.xs_bs + (long long)c * (plane >> 2);
    char* out = p.out + (long long)img * p.out_bs + (long long)c * plane;
    const int pv = 4 * p.s * p.nv, rv = 2 * p.nv;                      // pieces per plane / per row of a
    const int v0 = chunk * (LFU_THREADS * LFU_UNROLL) + threadIdx.x;
    V ra[LFU_UNROLL], rx[LFU_UNROLL];
#pragma unroll
    for (int k = 0; k < LFU_UNROLL; ++k) {
        const int v = v0 + k * LFU_THREADS;
        const unsigned vc = (unsigned)(v < pv ? v : pv - 1);          // (no branch around a load, as in the gather)
        unsigned y = vc / (unsigned)rv, xv = vc - y * (unsigned)rv;
        y -= y >= (unsigned)p.s ? (unsigned)p.s : 0u;
        xv -= xv >= (unsigned)p.nv ? (unsigned)p.nv : 0u;
        ra[k] = *reinterpret_cast<const V*>(a + (long long)vc * VB);
        rx[k] = *reinterpret_cast<const V*>(xs + ((long long)y * p.nv + xv) * VB);
    }
#pragma unroll
    for (int k = 0; k < LFU_UNROLL; ++k) {
        const int v = v0 + k * LFU_THREADS;
        if (v < pv) *reinterpret_cast<V*>(out + (long long)v * VB) = lfu_add<H, VB>(ra[k], rx[k]);
    }
}

// the widest piece that divides a row of s elements and keeps every piece of every tensor aligned
int lfu_vec_bytes(int s, int es, const lama_tensor* const* ts, int n) {
    unsigned long long bits = (unsigned long long)s * es;
    for (int k = 0; k < n; ++k) bits |= (unsigned long long)ts[k]->ptr | ((unsigned long long)ts[k]->batch_stride * es);
    for (int vb = 16; vb > es; vb >>= 1)
        if (!(bits & (unsigned)(vb - 1))) return vb;
    return es;
}

// what both entries ask of their tensors; `full` is the [., ., h, h] one that decides h
int lfu_check(const lama_tensor* const* ts, int n, const lama_tensor* full, int32_t batch) {
    for (int k = 0; k < n; ++k)
        if (!ts[k] || !ts[k]->ptr || ts[k]->C <= 0 || ts[k]->H <= 0 || ts[k]->W <= 0) return LAMA_ERR_BAD_ARG;
    if (batch <= 0) return LAMA_ERR_BAD_ARG;
    const int dt = full->dtype;
    if (dt != LAMA_DT_F32 && dt != LAMA_DT_F16) return LAMA_ERR_UNSUPPORTED;         // LAMA_DT_SPLIT16 and unknown types
    for (int k = 0; k < n; ++k)
        if (ts[k]->dtype != dt) return LAMA_ERR_UNSUPPORTED;                         // mixed
    if (full->H != full->W || (full->H & 1)) return LAMA_ERR_UNSUPPORTED;            // the reference splits both axes by h / 2
    const int es = dt == LAMA_DT_F16 ? 2 : 4;
    for (int k = 0; k < n; ++k) {
        if (ts[k]->batch_stride < (int64_t)ts[k]->C * ts[k]->H * ts[k]->W) return LAMA_ERR_BAD_ARG;
        if ((unsigned long long)ts[k]->ptr & (unsigned)(es - 1)) return LAMA_ERR_BAD_ARG;
    }
    return LAMA_OK;
}
}  // namespace

extern "C" int lama_lfu_gather_fwd(void* stream, const lama_tensor* x, const lama_tensor* y, int32_t batch) {
    const lama_tensor* ts[2] = {x, y};
    const int rc = lfu_check(ts, 2, x, batch);
    if (rc != LAMA_OK) return rc;
    const int s = x->H / 2;
    if (y->H != s || y->W != s || (long long)y->C != 4ll * x->C) return LAMA_ERR_BAD_ARG;
    const int es = x->dtype == LAMA_DT_F16 ? 2 : 4;
    const int vb = lfu_vec_bytes(s, es, ts, 2);
    LfuGatherParams p;
    p.x = (const char*)x->ptr; p.y = (char*)y->ptr;
    p.x_bs = (long long)x->batch_stride * es; p.y_bs = (long long)y->batch_stride * es;
    p.q = x->C; p.s = s; p.nv = s * es / vb;
    const long long pv = 4ll * s * p.nv;
    const long long chunks = lama_ceil_div64(pv, LFU_THREADS * LFU_UNROLL);
    const long long nwg = (long long)batch * x->C * chunks;
    if (pv > 0x3fffffffll || nwg > 0x7fffffffll) return LAMA_ERR_UNSUPPORTED;          // 32-bit piece indices, one grid dimension
    p.chunks = (int)chunks;
    const dim3 grid((unsigned)nwg), block(LFU_THREADS);
    switch (vb) {
        case 16: hipLaunchKernelGGL(lfu_gather_kernel<16>, grid, block, 0, (hipStream_t)stream, p); break;
        case 8: hipLaunchKernelGGL(lfu_gather_kernel<8>, grid, block, 0, (hipStream_t)stream, p); break;
        case 4: hipLaunchKernelGGL(lfu_gather_kernel<4>, grid, block, 0, (hipStream_t)stream, p); break;
        default: hipLaunchKernelGGL(lfu_gather_kernel<2>, grid, block, 0, (hipStream_t)stream, p); break;
    }
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" int lama_lfu_tile_add_fwd(void* stream, const lama_tensor* a, const lama_tensor* xs, const lama_tensor* out, int32_t batch) {
    const lama_tensor* ts[3] = {a, xs, out};
    const int rc = lfu_check(ts, 3, a, batch);
    if (rc != LAMA_OK) return rc;
    const int s = a->H / 2;
    if (xs->H != s || xs->W != s || xs->C != a->C || out->H != a->H || out->W != a->W || out->C != a->C) return LAMA_ERR_BAD_ARG;
    const bool half = a->dtype == LAMA_DT_F16;
    const int es = half ? 2 : 4;
    const int vb = lfu_vec_bytes(s, es, ts, 3);
    LfuTileAddParams p;
    p.a = (const char*)a->ptr; p.xs = (const char*)xs->ptr; p.out = (char*)out->ptr;
    p.a_bs = (long long)a->batch_stride * es; p.xs_bs = (long long)xs->batch_stride * es; p.out_bs = (long long)out->batch_stride * es;
    p.C = a->C; p.s = s; p.nv = s * es / vb;
    const long long pv = 4ll * s * p.nv;
    const long long chunks = lama_ceil_div64(pv, LFU_THREADS * LFU_UNROLL);
    const long long nwg = (long long)batch * a->C * chunks;
    if (pv > 0x3fffffffll || nwg > 0x7fffffffll) return LAMA_ERR_UNSUPPORTED;
    p.chunks = (int)chunks;
    const dim3 grid((unsigned)nwg), block(LFU_THREADS);
#define LFU_LAUNCH(H, VB) hipLaunchKernelGGL((lfu_tile_add_kernel<H, VB>), grid, block, 0, (hipStream_t)stream, p)
    if (half) {
        switch (vb) {
            case 16: LFU_LAUNCH(true, 16); break;
            case 8: LFU_LAUNCH(true, 8); break;
            case 4: LFU_LAUNCH(true, 4); break;
            default: LFU_LAUNCH(true, 2); break;
        }
    } else {
        switch (vb) {
            case 16: LFU_LAUNCH(false, 16); break;
            case 8: LFU_LAUNCH(false, 8); break;
            default: LFU_LAUNCH(false, 4); break;
        }
    }
#undef LFU_LAUNCH
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}
