// Per-channel range statistics of a lama_tensor view (lama_range_stats_fwd): for every channel c of x [batch, C, H, W]
//   abs_max = the largest |e| over the FINITE elements (+0.0f if there are none), n_nan, n_inf, n_over = finite elements with |e| > limit.
// The diagnostic behind the range watch of the fp16 split: which tensor left |x| <= 65504, in which channel, by how much (lama_amd/probe.py).
//
// Everything is decided on BIT PATTERNS: a = bits & 0x7fffffff is a non-negative float pattern and unsigned compares of those are exact
// (NaN: a > 0x7f800000, inf: a == 0x7f800000, over: a > bits(limit), max: the unsigned maximum) -- no floating-point instruction touches an
// element, so denormals are never flushed and a signalling NaN stays a NaN.  fp16 elements are classified on their own 15-bit magnitude the
// same way (the order of half patterns is the order of the values they widen to); the host turns `limit` into the largest half magnitude that
// does not exceed it, and the fold kernel widens the channel's maximum to fp32 with integer arithmetic (exact for half denormals too).
//
// A pure streaming read in two launches:
//   1. partial: one 256-thread workgroup per RS_CHUNK_BYTES (32 KiB) piece of one (image, channel) plane -- the channel is uniform per
//      workgroup.  16-byte loads over the aligned body (RS_UNROLL = 4 per lane in flight before the first word is looked at: a whole piece
//      is two such rounds), element loads over the at most 15 bytes in front of it and behind it: a plane may start at any element and
//      have any size.  The four values are
//      reduced inside the wave with __shfl_xor, through LDS across the four waves, and one 16-byte partial per workgroup goes to the workspace
//      at [c][image][piece].
//   2. fold: one workgroup per channel reduces its batch * pieces partials and OVERWRITES out[c].
// Unsigned maximum and 32-bit integer addition are associative and commutative: the result does not depend on the reduction order and two runs
// give the same bytes.  No atomics, nothing to zero.
#include "common.h"

namespace {
constexpr int RS_THREADS = 256, RS_CHUNK_BYTES = 32768, RS_UNROLL = 4;

struct RangeStatsParams {
    const char* x;
    long long bs_bytes;      // bytes between consecutive images
    long long plane;         // H * W elements
    uint32_t* partial;       // [C][batch][chunks][4]
    int C, batch, chunks;
    uint32_t lim;            // bits of `limit` (fp32) or the largest half magnitude <= limit (fp16)
};

struct RsAcc { uint32_t amax, nan, inf, over; };

template <bool H> __device__ __forceinline__ void rs_classify(uint32_t a, uint32_t lim, RsAcc& s) {
    constexpr uint32_t INF = H ? 0x7c00u : 0x7f800000u;
    const bool fin = a < INF;
    s.nan += a > INF ? 1u : 0u;
    s.inf += a == INF ? 1u : 0u;
    s.over += (fin && a > lim) ? 1u : 0u;
    const uint32_t m = fin ? a : 0u;
    s.amax = m > s.amax ? m : s.amax;
}

// one 32-bit word of the stream: one fp32 element or two fp16 elements
template <bool H> __device__ __forceinline__ void rs_word(uint32_t w, uint32_t lim, RsAcc& s) {
    if (H) {
        rs_classify<true>(w & 0x7fffu, lim, s);
        rs_classify<true>((w >> 16) & 0x7fffu, lim, s);
    } else {
        rs_classify<false>(w & 0x7fffffffu, lim, s);
    }
}

template <bool H> __device__ __forceinline__ void rs_element(const char* p, uint32_t lim, RsAcc& s) {
    if (H) rs_classify<true>((uint32_t)(*reinterpret_cast<const uint16_t*>(p)) & 0x7fffu, lim, s);
    else rs_classify<false>(*reinterpret_cast<const uint32_t*>(p) & 0x7fffffffu, lim, s);
}

// reduce the four values over the workgroup; valid in thread 0 afterwards
__device__ __forceinline__ void rs_block_reduce(RsAcc& s) {
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t m = __shfl_xor(s.amax, off, 64);
        s.amax = m > s.amax ? m : s.amax;
        s.nan += __shfl_xor(s.nan, off, 64);
        s.inf += __shfl_xor(s.inf, off, 64);
        s.over += __shfl_xor(s.over, off, 64);
    }
    uint32_t* red = reinterpret_cast<uint32_t*>(lama_smem);      // [RS_THREADS / 64][4]
    if ((threadIdx.x & 63) == 0) {
        uint32_t* r = red + 4 * (threadIdx.x >> 6);
        r[0] = s.amax; r[1] = s.nan; r[2] = s.inf; r[3] = s.over;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RS_THREADS / 64; ++w) {
            const uint32_t* r = red + 4 * w;
            s.amax = r[0] > s.amax ? r[0] : s.amax;
            s.nan += r[1]; s.inf += r[2]; s.over += r[3];
        }
    }
}

template <bool H> __global__ __launch_bounds__(RS_THREADS) void range_stats_partial_kernel(RangeStatsParams p) {
    constexpr int ES = LamaAct<H>::ES;
    constexpr long long CH = RS_CHUNK_BYTES / ES;               // elements per piece
    int blk = blockIdx.x;
    const int chunk = blk % p.chunks; blk /= p.chunks;
    const int c = blk % p.C, img = blk / p.C;
    const long long e0 = (long long)chunk * CH;
    const long long left = p.plane - e0;
    const int nbytes = (int)(left < CH ? left : CH) * ES;        // 1 .. RS_CHUNK_BYTES
    const char* base = p.x + (long long)img * p.bs_bytes + ((long long)c * p.plane + e0) * ES;
    int head = (int)((16u - (unsigned)((unsigned long long)base & 15u)) & 15u);       // bytes in front of the first 16-byte boundary
    head = head < nbytes ? head : nbytes;
    const int nvec = (nbytes - head) >> 4;
    const int tail0 = head + (nvec << 4);
    const int tid = threadIdx.x;
    RsAcc s = {0u, 0u, 0u, 0u};
    const uint4* vp = reinterpret_cast<const uint4*>(base + head);
    for (int i0 = tid; i0 < nvec; i0 += RS_THREADS * RS_UNROLL) {
        uint4 v[RS_UNROLL];
#pragma unroll
        for (int k = 0; k < RS_UNROLL; ++k) {                    // every load of the round is in flight before the first word is looked at
            const int i = i0 + k * RS_THREADS;
            v[k] = i < nvec ? vp[i] : make_uint4(0u, 0u, 0u, 0u);   // +0.0 changes none of the four values
        }
#pragma unroll
        for (int k = 0; k < RS_UNROLL; ++k) {
            rs_word<H>(v[k].x, p.lim, s); rs_word<H>(v[k].y, p.lim, s); rs_word<H>(v[k].z, p.lim, s); rs_word<H>(v[k].w, p.lim, s);
        }
    }
    // at most 15 bytes on either side of the body: one element per lane
    if (tid * ES < head) rs_element<H>(base + tid * ES, p.lim, s);
    if (tail0 + tid * ES < nbytes) rs_element<H>(base + tail0 + tid * ES, p.lim, s);
    rs_block_reduce(s);
    if (tid == 0) {
        uint32_t* dst = p.partial + 4 * (((long long)c * p.batch + img) * p.chunks + chunk);
        dst[0] = s.amax; dst[1] = s.nan; dst[2] = s.inf; dst[3] = s.over;
    }
}

// the fp32 pattern of a finite half magnitude (15 bits): integer arithmetic only, exact for denormals
__host__ __device__ inline uint32_t rs_half_to_f32_bits(uint32_t h) {
    const uint32_t e = h >> 10, m = h & 0x3ffu;
    if (e) return ((e + 112u) << 23) | (m << 13);
    if (!m) return 0u;
    int top = 9;                                              // m * 2^-24 = 1.xxx * 2^(top - 24)
    while (!(m >> top)) --top;
    return ((uint32_t)(top - 24 + 127) << 23) | ((m << (23 - top)) & 0x7fffffu);
}

__global__ __launch_bounds__(RS_THREADS) void range_stats_fold_kernel(const uint32_t* partial, uint32_t* out, int per_channel, int half) {
    const uint32_t* src = partial + 4ll * blockIdx.x * per_channel;
    RsAcc s = {0u, 0u, 0u, 0u};
    for (int i = threadIdx.x; i < per_channel; i += RS_THREADS) {
        const uint32_t* r = src + 4ll * i;
        s.amax = r[0] > s.amax ? r[0] : s.amax;
        s.nan += r[1]; s.inf += r[2]; s.over += r[3];
    }
    rs_block_reduce(s);
    if (threadIdx.x == 0) {
        uint32_t* o = out + 4ll * blockIdx.x;                 // struct lama_range_stats
        o[0] = half ? rs_half_to_f32_bits(s.amax) : s.amax;
        o[1] = s.nan; o[2] = s.inf; o[3] = s.over;
    }
}

long long rs_chunks(long long plane, int es) {
    const long long ch = RS_CHUNK_BYTES / es;
    return (plane + ch - 1) / ch;
}
}  // namespace

extern "C" size_t lama_range_stats_workspace_bytes(int32_t batch, int32_t C, int32_t H, int32_t W) {
    if (batch <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    // the pieces are cut in BYTES: an fp32 plane has the most, so one size serves both element types
    return (size_t)batch * C * rs_chunks((long long)H * W, 4) * sizeof(lama_range_stats);
}

extern "C" int lama_range_stats_fwd(void* stream, const lama_tensor* x, int32_t batch, float limit, lama_range_stats* out, void* workspace,
                                    size_t workspace_bytes) {
    static_assert(sizeof(lama_range_stats) == 16, "one 16-byte record per channel");
    if (!x || !x->ptr || !out || !workspace || batch <= 0 || x->C <= 0 || x->H <= 0 || x->W <= 0) return LAMA_ERR_BAD_ARG;
    uint32_t lim_bits;
    memcpy(&lim_bits, &limit, 4);
    if (!(limit > 0.0f) || (lim_bits & 0x7fffffffu) >= 0x7f800000u) return LAMA_ERR_BAD_ARG;       // zero, negative, inf, NaN
    const long long plane = (long long)x->H * x->W;
    if (x->batch_stride < (int64_t)x->C * plane) return LAMA_ERR_BAD_ARG;
    if (x->dtype != LAMA_DT_F32 && x->dtype != LAMA_DT_F16) return LAMA_ERR_UNSUPPORTED;
    const bool half = x->dtype == LAMA_DT_F16;
    const int es = half ? 2 : 4;
    if (((unsigned long long)x->ptr & (unsigned)(es - 1)) || ((unsigned long long)out & 3u) || ((unsigned long long)workspace & 3u)) return LAMA_ERR_BAD_ARG;
    if ((long long)batch * plane >= (1ll << 32)) return LAMA_ERR_UNSUPPORTED;                   // the counters are 32-bit
    const long long chunks = rs_chunks(plane, es);
    const long long nwg = (long long)batch * x->C * chunks;
    if (nwg > 0x7fffffffll) return LAMA_ERR_UNSUPPORTED;                                           // one grid dimension
    if (workspace_bytes < (size_t)nwg * sizeof(lama_range_stats)) return LAMA_ERR_WORKSPACE;
    RangeStatsParams p;
    p.x = (const char*)x->ptr;
    p.bs_bytes = (long long)x->batch_stride * es;
    p.plane = plane;
    p.partial = (uint32_t*)workspace;
    p.C = x->C; p.batch = batch; p.chunks = (int)chunks;
    if (half) {
        // the largest finite half magnitude whose value does not exceed limit (0 = +0.0 always qualifies: limit > 0)
        uint32_t lo = 0u, hi = 0x7bffu;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1u) >> 1;
            if (rs_half_to_f32_bits(mid) <= lim_bits) lo = mid; else hi = mid - 1u;
        }
        p.lim = lo;
    } else {
        p.lim = lim_bits;
    }
    const size_t lds = (RS_THREADS / 64) * 4 * sizeof(uint32_t);
    if (half) hipLaunchKernelGGL(range_stats_partial_kernel<true>, dim3((unsigned)nwg), dim3(RS_THREADS), lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(range_stats_partial_kernel<false>, dim3((unsigned)nwg), dim3(RS_THREADS), lds, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    hipLaunchKernelGGL(range_stats_fold_kernel, dim3((unsigned)x->C), dim3(RS_THREADS), lds, (hipStream_t)stream, (const uint32_t*)workspace,
                       (uint32_t*)out, (int)(batch * chunks), half ? 1 : 0);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}
