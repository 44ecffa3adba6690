// Elementwise pre/post kernels of the inference path, the composite FourierUnit entry point and the
// misc C-ABI functions.
#include "common.h"
#include <initializer_list>

struct EwParams {
    const float* img;
    long long img_bs;
    const float* mask;
    long long mask_bs;
    const float* pred;
    long long pred_bs;
    float* out;
    long long out_bs;
    long long hw;
    int B;
};

// masked_img = cat(img*(1-mask), mask)  (trainers/default.py:59,67-68)
__global__ __launch_bounds__(LAMA_NTHREADS) void mask_compose_kernel(EwParams p) {
    long long total = (long long)p.B * p.hw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int b = (int)(i / p.hw);
        long long px = i - (long long)b * p.hw;
        float m = p.mask[b * p.mask_bs + px];
        const float* im = p.img + b * p.img_bs + px;
        float* o = p.out + b * p.out_bs + px;
        float k = 1.0f - m;
        o[0] = im[0] * k;
        o[p.hw] = im[p.hw] * k;
        o[2 * p.hw] = im[2 * p.hw] * k;
        o[3 * p.hw] = m;
    }
}

// One evaluation of mask * pred + (1 - mask) * img for every kernel that blends: left to the compiler, blend_kernel fused the first product
// and blend_quantize_u8_kernel the second, and a fractional mask then broke forward_u8's contract (its bytes = quantize_u8_hwc(blend(...)))
// in about one byte per million.  The first product rides in the FMA, the second is rounded on its own -- what blend_kernel compiled to.
__device__ __forceinline__ float ew_blend(float m, float k, float pred, float img) { return fmaf(m, pred, k * img); }

// inpainted = mask*pred + (1-mask)*img  (trainers/default.py:71)
__global__ __launch_bounds__(LAMA_NTHREADS) void blend_kernel(EwParams p) {
    long long total = (long long)p.B * p.hw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int b = (int)(i / p.hw);
        long long px = i - (long long)b * p.hw;
        float m = p.mask[b * p.mask_bs + px];
        float k = 1.0f - m;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            p.out[b * p.out_bs + c * p.hw + px] = ew_blend(m, k, p.pred[b * p.pred_bs + c * p.hw + px], p.img[b * p.img_bs + c * p.hw + px]);
    }
}

struct QuantParams {
    const float* src;
    long long src_bs;
    uint8_t* dst;
    int B, H, W, ch, cw;
};

// np.clip(x*255, 0, 255).astype('uint8') (truncation) of x.permute(1,2,0)[:ch,:cw]  (bin/predict.py:86-92)
__global__ __launch_bounds__(LAMA_NTHREADS) void quantize_u8_hwc_kernel(QuantParams p) {
    long long total = (long long)p.B * p.ch * p.cw * 3;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int c = (int)(i % 3);
        long long r = i / 3;
        int x = (int)(r % p.cw);
        r /= p.cw;
        int y = (int)(r % p.ch);
        int b = (int)(r / p.ch);
        float v = p.src[b * p.src_bs + ((long long)c * p.H + y) * p.W + x] * 255.0f;
        v = fminf(fmaxf(v, 0.0f), 255.0f);
        p.dst[i] = (uint8_t)v;
    }
}

// ---- round 6 (v110): the predict step fed with what is on disk -- u8 HWC image + u8 mask, unpadded -- instead of fp32 NCHW tensors the host
// converted and padded (33.6 MB instead of 8.4 MB over PCIe per 8 x 512^2 step, and a float conversion + np.pad per image on the host).
//   image / 255 in fp32 (evaluation/data.py:12-20: astype('float32') / 255 -- the same IEEE division), symmetric padding at the bottom / right
//   up to (Hp, Wp) (data.py:29-33: np.pad(mode='symmetric'), padded row h + i = row h - 1 - i, periodic beyond row 2 h), mask > 0 (bin/predict.py:84) or mask / 255.
struct U8Params {
    const uint8_t* img;      // [B][Hp][Wp][3], the valid part in the top-left h x w corner of each image's slot
    const uint8_t* mask;     // [B][Hp][Wp]
    const int32_t* sizes;    // [B][2] = (h, w) of each image, or null: every image is Hp x Wp
    const float* pred;       // blend: [B,3,Hp,Wp]
    long long pred_bs;
    float* out;              // compose: [B,4,Hp,Wp] fp32
    long long out_bs;
    uint8_t* out_u8;         // blend + quantise: [B][Hp][Wp][3]
    int B, Hp, Wp, binarize;
};
// np.pad(mode='symmetric') for any amount of padding: the mirror is periodic with period 2 n (an image may be smaller than its padding: 3 rows
// in an 8-row slot, or a scaled 5 x 7 at 0.5 -> 2 x 4 padded to 8 x 8).  Shared by the u8 predict-step ends and resize_u8_kernel.
__device__ __forceinline__ int ew_symmetric(int y, int n) {
    if (y < n) return y;                                 // inside the image (every pixel of a full slot): no division
    const int t = y % (2 * n);
    return t < n ? t : 2 * n - 1 - t;
}
__device__ __forceinline__ bool u8_src(const U8Params& p, int b, int y, int x, long long& pix) {
    int h = p.Hp, w = p.Wp;
    if (p.sizes) { h = p.sizes[2 * b]; w = p.sizes[2 * b + 1]; }
    if (h <= 0 || w <= 0) return false;                  // an empty slot of a partial batch: zeros
    if (h > p.Hp) h = p.Hp;                              // (never taken for sizes that fit the slot: keeps every read inside it)
    if (w > p.Wp) w = p.Wp;
    pix = ((long long)b * p.Hp + ew_symmetric(y, h)) * p.Wp + ew_symmetric(x, w);
    return true;
}
// masked_img = cat(img * (1 - mask), mask)  (trainers/default.py:59,67-68) from the u8 operands
__global__ __launch_bounds__(LAMA_NTHREADS) void mask_compose_u8_kernel(U8Params p) {
    const long long hw = (long long)p.Hp * p.Wp, total = (long long)p.B * hw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / hw);
        const long long px = i - (long long)b * hw;
        const int y = (int)(px / p.Wp), x = (int)(px - (long long)y * p.Wp);
        long long sp;
        float r = 0.f, g = 0.f, bl = 0.f, m = 0.f;
        if (u8_src(p, b, y, x, sp)) {
            const uint8_t* im = p.img + sp * 3;
            r = (float)im[0] / 255.0f; g = (float)im[1] / 255.0f; bl = (float)im[2] / 255.0f;
            const uint8_t mu = p.mask[sp];
            m = p.binarize ? (mu > 0 ? 1.0f : 0.0f) : (float)mu / 255.0f;
        }
        float* o = p.out + b * p.out_bs + px;
        const float k = 1.0f - m;
        o[0] = r * k;
        o[hw] = g * k;
        o[2 * hw] = bl * k;
        o[3 * hw] = m;
    }
}
// inpainted = mask * pred + (1 - mask) * img (default.py:71), then np.clip(x * 255, 0, 255).astype('uint8') in HWC order (bin/predict.py:86-92)
__global__ __launch_bounds__(LAMA_NTHREADS) void blend_quantize_u8_kernel(U8Params p) {
    const long long hw = (long long)p.Hp * p.Wp, total = (long long)p.B * hw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / hw);
        const long long px = i - (long long)b * hw;
        const int y = (int)(px / p.Wp), x = (int)(px - (long long)y * p.Wp);
        long long sp;
        float im[3] = {0.f, 0.f, 0.f}, m = 0.f;
        if (u8_src(p, b, y, x, sp)) {
            const uint8_t* s = p.img + sp * 3;
            im[0] = (float)s[0] / 255.0f; im[1] = (float)s[1] / 255.0f; im[2] = (float)s[2] / 255.0f;
            const uint8_t mu = p.mask[sp];
            m = p.binarize ? (mu > 0 ? 1.0f : 0.0f) : (float)mu / 255.0f;
        }
        const float k = 1.0f - m;
        uint8_t* d = p.out_u8 + i * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // pred is not read where the mask is 0 (the sparse tail leaves those pixels of the generator's output unwritten: DESIGN.md 4.17):
            // fmaf(0, pred, 1 * img) = img for every finite pred -- the same bytes
            const float pr = m != 0.0f ? p.pred[b * p.pred_bs + c * hw + px] : 0.0f;
            float v = ew_blend(m, k, pr, im[c]) * 255.0f;
            v = fminf(fmaxf(v, 0.0f), 255.0f);
            d[c] = (uint8_t)v;
        }
    }
}

// ---- work lists of the sparse tail (lama_tail_lists_build) --------------------------------------------------------------------
// The predict step keeps mask * pred + (1 - mask) * image: where the mask is 0 the generator's output is never read, and the last launches of the
// generator -- the ConvTranspose2d upsamplings (convt2_kernel: tiles of 4 x 32 input pixels x 64 output channels) and the 7x7 head (head7_ws_kernel:
// segments of rs rows x 26 columns) -- have receptive fields of 1 and 3 pixels.  Two launches list the work units the output needs:
//   tail_flags_kernel  one 64-thread workgroup per head segment: is any mask pixel of its output rectangle not 0?
//   tail_lists_kernel  ONE workgroup: the closures -- an up tile is needed when its output rectangle meets what a LISTED unit downstream reads (the
//     head segment's rectangle grown by 3 and clamped to the plane; the 5 x 33 input patch of an up tile clamped to the plane), i.e. at the
//     granularity of what is computed: a listed unit never reads a pixel that was not written in this step -- and the ordered compactions (a
//     prefix sum, no atomic append: the list is the dense order with holes, the same from run to run).
#define TAIL_MAX_UP 4
struct TailParams {
    const float* mask;            // [B][H][W] plane of the generator's input (channel 3), batch stride in elements
    long long mask_bs;
    int B, H, W;                  // the head's plane
    int txh, ns, rs;              // head: 26-column segments per row, parts per column, rows per part
    int n_up;
    int uh[TAIL_MAX_UP], uw[TAIL_MAX_UP], mg[TAIL_MAX_UP];   // level i (0 = feeds the head): its INPUT plane, Cout / 64
    int* head_flags;              // workspace: [ns][B * txh]
    int* up_flags[TAIL_MAX_UP];   // workspace: [B][tiles_y][tiles_x]
    int* head_list; int* head_count;
    int* up_list[TAIL_MAX_UP]; int* up_count[TAIL_MAX_UP];
};

__global__ __launch_bounds__(64) void tail_flags_kernel(TailParams p) {
    const int ncols = p.B * p.txh, g = blockIdx.x;
    const int part = g / ncols, col = g - part * ncols, b = col / p.txh, x0 = (col - b * p.txh) * 26;
    const int y0 = part * p.rs, y1 = y0 + p.rs < p.H ? y0 + p.rs : p.H, x1 = x0 + 26 < p.W ? x0 + 26 : p.W;
    const int w = x1 - x0, n = (y1 - y0) * w;
    const float* m = p.mask + (long long)b * p.mask_bs;
    bool any = false;
    for (int i = threadIdx.x; i < n; i += 64) {
        const int r = i / w, c = i - r * w;
        any = any || m[(long long)(y0 + r) * p.W + x0 + c] != 0.0f;
    }
    if (threadIdx.x == 0) p.head_flags[g] = 0;
    __syncthreads();
    if (any) p.head_flags[g] = 1;           // (every writer stores the same value)
}

// ordered compaction by the whole workgroup: item i of n with flags[i] != 0 becomes the list entries i * mg .. i * mg + mg - 1
__device__ void tail_compact(const int* flags, int n, int mg, int* list, int* count, int* lds) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int per = (n + nt - 1) / nt;
    const int i0 = tid * per < n ? tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    int c = 0;
    for (int i = i0; i < i1; ++i) c += flags[i] != 0;
    lds[tid] = c;
    __syncthreads();
    for (int d = 1; d < nt; d <<= 1) {
        const int v = tid >= d ? lds[tid - d] : 0;
        __syncthreads();
        lds[tid] += v;
        __syncthreads();
    }
    int pos = lds[tid] - c;
    for (int i = i0; i < i1; ++i)
        if (flags[i] != 0) {
            for (int m = 0; m < mg; ++m) list[pos * mg + m] = i * mg + m;
            ++pos;
        }
    if (tid == nt - 1) count[0] = lds[tid] * mg;
    __syncthreads();
}

#define TAIL_NT 1024   // one workgroup: its time is a chain of memory round trips per thread, so the widest workgroup is the shortest chain
__global__ __launch_bounds__(TAIL_NT) void tail_lists_kernel(TailParams p) {
    int* lds = reinterpret_cast<int*>(lama_smem);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int ncols = p.B * p.txh;
    tail_compact(p.head_flags, ncols * p.ns, 1, p.head_list, p.head_count, lds);
    for (int lv = 0; lv < p.n_up; ++lv) {
        const int ty_n = (p.uh[lv] + 3) / 4, tx_n = (p.uw[lv] + 31) / 32, nsp = p.B * ty_n * tx_n;
        const int Ho = 2 * p.uh[lv], Wo = 2 * p.uw[lv];
        for (int t = tid; t < nsp; t += nt) {
            const int tx = t % tx_n, ty = (t / tx_n) % ty_n, b = t / (tx_n * ty_n);
            const int y0 = 8 * ty, y1 = y0 + 8 < Ho ? y0 + 8 : Ho, x0 = 64 * tx, x1 = x0 + 64 < Wo ? x0 + 64 : Wo;   // this tile's output rectangle
            int need = 0;
            if (lv == 0) {       // read by: the rectangle of a listed head segment grown by the 3-pixel reflection pad, clamped to the plane
                int pa0 = (y0 - 3) / p.rs - 1, pa1 = (y1 + 3) / p.rs + 1, c0 = (x0 - 3) / 26 - 1, c1 = (x1 + 3) / 26 + 1;
                pa0 = pa0 < 0 ? 0 : pa0; pa1 = pa1 >= p.ns ? p.ns - 1 : pa1; c0 = c0 < 0 ? 0 : c0; c1 = c1 >= p.txh ? p.txh - 1 : c1;
                for (int pa = pa0; pa <= pa1; ++pa)
                    for (int c = c0; c <= c1; ++c) {
                        int ry0 = pa * p.rs, ry1 = ry0 + p.rs < p.H ? ry0 + p.rs : p.H, rx0 = c * 26, rx1 = rx0 + 26 < p.W ? rx0 + 26 : p.W;
                        ry0 = ry0 - 3 < 0 ? 0 : ry0 - 3; ry1 = ry1 + 3 > p.H ? p.H : ry1 + 3; rx0 = rx0 - 3 < 0 ? 0 : rx0 - 3; rx1 = rx1 + 3 > p.W ? p.W : rx1 + 3;
                        if (ry0 < y1 && y0 < ry1 && rx0 < x1 && x0 < rx1 && p.head_flags[pa * ncols + b * p.txh + c] != 0) need = 1;
                    }
            } else {             // read by: the 4 x 32 input pixels of a listed tile of the level downstream plus one row below and one column right
                const int Hd = p.uh[lv - 1], Wd = p.uw[lv - 1], tyd_n = (Hd + 3) / 4, txd_n = (Wd + 31) / 32;
                int a0 = y0 / 4 - 1, a1 = y1 / 4 + 1, c0 = x0 / 32 - 1, c1 = x1 / 32 + 1;
                a0 = a0 < 0 ? 0 : a0; a1 = a1 >= tyd_n ? tyd_n - 1 : a1; c0 = c0 < 0 ? 0 : c0; c1 = c1 >= txd_n ? txd_n - 1 : c1;
                for (int a = a0; a <= a1; ++a)
                    for (int c = c0; c <= c1; ++c) {
                        const int ry0 = 4 * a, ry1 = ry0 + 5 < Hd ? ry0 + 5 : Hd, rx0 = 32 * c, rx1 = rx0 + 33 < Wd ? rx0 + 33 : Wd;
                        if (ry0 < y1 && y0 < ry1 && rx0 < x1 && x0 < rx1 && p.up_flags[lv - 1][(b * tyd_n + a) * txd_n + c] != 0) need = 1;
                    }
            }
            p.up_flags[lv][t] = need;
        }
        __syncthreads();
        tail_compact(p.up_flags[lv], nsp, p.mg[lv], p.up_list[lv], p.up_count[lv], lds);
    }
}

// ---- the evaluator's loader on the device: a batch of DECODED u8 (ground truth, prediction, mask) triples in one launch --
//   PrecomputedInpaintingResultsDataset.__getitem__ (evaluation/data.py:110-124): image.astype('float32') / 255 of both images (data.py:16, the same
//   IEEE division as mask_compose_u8_kernel), pad_img_to_modulo's symmetric padding bottom / right (data.py:29-33), and the clamp of the ground
//   truth alone (evaluator.py:87-90).  The evaluator reads the mask only through its mean (evaluator.py:58,164): the float mask plane is never
//   formed, the launch leaves the exact integer sum of the padded u8 mask per image instead.
// The host has checked every size (the sizes ride in the kernel's argument block): 0 < h <= Hs, 0 < w <= Ws, padding <= extent, so a padded
// row Hp > y >= h mirrors to row 2 h - 1 - y >= 0 without the periodic form of ew_symmetric.
// Roles by workgroup: block b < B sums the mask of image b (its h x Ws bytes are one contiguous run: 16-byte loads, per-thread partial sums, one
// fixed-order pass over them in LDS -- integer adds, no atomics, no workspace); the others convert, one thread per 4 consecutive output pixels:
// 12 bytes in (three dword loads where the row pitch allows), one float4 per colour plane out (a wave writes 1 KB runs of each plane).
#define LAMA_EI_MAX_BATCH 64
struct EvalIngestParams {
    const uint8_t* gt;       // [B][Hs][Ws][3]
    const uint8_t* pred;     // [B][Hs][Ws][3]
    const uint8_t* mask;     // [B][Hs][Ws]
    float* out_img;          // [B,3,Hp,Wp]
    long long img_bs;
    float* out_pred;         // [B,3,Hp,Wp]
    long long pred_bs;
    long long* sums;         // [B]
    float lo, hi;
    int B, Hs, Ws, Hp, Wp, clamp, vec_ld, vec_st;
    int32_t sizes[LAMA_EI_MAX_BATCH][2];
};
typedef uint32_t __attribute__((may_alias)) ei_u32;
// Four HWC pixels are 12 bytes held in three little-endian dwords: byte k = 3 * j + c is channel c of pixel j (0..3).
__device__ __forceinline__ uint32_t u8_get(const uint32_t (&d)[3], int k) { return (d[k >> 2] >> (8 * (k & 3))) & 255u; }
__device__ __forceinline__ void u8_put(uint32_t (&d)[3], int k, uint32_t v) { d[k >> 2] |= v << (8 * (k & 3)); }   // (onto a zero byte)
__device__ __forceinline__ float ei_byte(const uint32_t (&d)[3], int k) { return (float)u8_get(d, k) / 255.0f; }
// The four pixels from column x0 of the slot row that starts at pixel `row`, and their mask bytes in m4.  vec: one dword of mask and three of RGB
// at row + x0.  Otherwise byte by byte, pixel j from row + col(x) with x = x0 + j clamped to W - 1 (a column past the edge re-reads the last
// one; it is never stored).  Every load is unconditional.
template <class Col> __device__ __forceinline__ void u8_load4(const uint8_t* img, const uint8_t* msk, long long row, int x0, int W, bool vec, Col col,
                                                              uint32_t& m4, uint32_t (&d)[3]) {
    if (vec) {
        const long long px = row + x0;
        m4 = *reinterpret_cast<const ei_u32*>(msk + px);
        const ei_u32* s = reinterpret_cast<const ei_u32*>(img + px * 3);
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
        return;
    }
    m4 = d[0] = d[1] = d[2] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long px = row + col(x0 + j < W ? x0 + j : W - 1);
        m4 |= (uint32_t)msk[px] << (8 * j);
#pragma unroll
        for (int c = 0; c < 3; ++c) u8_put(d, 3 * j + c, img[px * 3 + c]);
    }
}

__device__ __forceinline__ void ei_load4(const uint8_t* src, long long row, int x0, int w, int Wp, bool vec, float (&v)[3][4]) {
    if (vec && x0 + 4 <= w) {
        const ei_u32* s = reinterpret_cast<const ei_u32*>(src + (row + x0) * 3);
        const uint32_t d[3] = {s[0], s[1], s[2]};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][j] = ei_byte(d, 3 * j + c);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        if (x < Wp) {
            const uint8_t* s = src + (row + (x < w ? x : 2 * w - 1 - x)) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][j] = (float)s[c] / 255.0f;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][j] = 0.0f;
        }
    }
}
// four pixels of NP planes: one float4 per plane, or the columns below Wp one by one
template <int NP> __device__ __forceinline__ void ei_store4(float* o, long long hw, int x0, int Wp, bool vec, const float (&v)[NP][4]) {
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        if (vec) {
            *reinterpret_cast<float4*>(o + c * hw) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < Wp) o[c * hw + j] = v[c][j];
        }
    }
}

__global__ __launch_bounds__(LAMA_NTHREADS) void eval_ingest_u8_kernel(EvalIngestParams p) {
    if ((int)blockIdx.x < p.B) {
        // sum over the padded plane = sum over the h x w pixels, each counted once per padded position that mirrors onto it: rows / columns
        // from 2 n - Np on count twice
        const int b = blockIdx.x, h = p.sizes[b][0], w = p.sizes[b][1];
        const int y2 = 2 * h - p.Hp, x2 = 2 * w - p.Wp;
        const uint8_t* m = p.mask + (long long)b * p.Hs * p.Ws;
        const long long n = (long long)h * p.Ws;
        const long long mis = (long long)(reinterpret_cast<uintptr_t>(m) & 15);      // the run's first byte inside its 16-byte line
        const long long nchunks = (mis + n + 15) >> 4;
        unsigned long long acc = 0;
        for (long long ch = threadIdx.x; ch < nchunks; ch += LAMA_NTHREADS) {
            const long long f0 = ch * 16 - mis;
            uint32_t d[4] = {0u, 0u, 0u, 0u};
            const bool whole = f0 >= 0 && f0 + 16 <= n;
            if (whole) {
                const ei_u32* s = reinterpret_cast<const ei_u32*>(m + f0);
                d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
            } else {
                for (int k = 0; k < 16; ++k)
                    if (f0 + k >= 0 && f0 + k < n) d[k >> 2] |= (uint32_t)m[f0 + k] << (8 * (k & 3));
            }
            const long long fc = f0 < 0 ? 0 : f0;                                   // (bytes in front of the run are zero in d)
            int y = (int)(fc / p.Ws), x = (int)(fc - (long long)y * p.Ws);
            uint32_t part = 0;
            for (int k = (int)(fc - f0); k < 16; ++k) {
                const uint32_t u = (d[k >> 2] >> (8 * (k & 3))) & 255u;
                const uint32_t wt = x < w ? (x >= x2 ? 2u : 1u) * (y >= y2 ? 2u : 1u) : 0u;
                part += u * wt;
                if (++x == p.Ws) { x = 0; ++y; }
            }
            acc += part;
        }
        unsigned long long* red = reinterpret_cast<unsigned long long*>(lama_smem);
        red[threadIdx.x] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long s = 0;
            for (int t = 0; t < LAMA_NTHREADS; ++t) s += red[t];
            p.sums[b] = (long long)s;
        }
        return;
    }
    const int qpr = (p.Wp + 3) >> 2;
    const long long hw = (long long)p.Hp * p.Wp, total = (long long)p.B * p.Hp * qpr;
    const long long step = (long long)(gridDim.x - p.B) * LAMA_NTHREADS;
    for (long long i = (long long)(blockIdx.x - p.B) * LAMA_NTHREADS + threadIdx.x; i < total; i += step) {
        const int q = (int)(i % qpr);
        const long long r = i / qpr;
        const int y = (int)(r % p.Hp), b = (int)(r / p.Hp);
        const int h = p.sizes[b][0], w = p.sizes[b][1];
        const int x0 = 4 * q;
        const long long row = ((long long)b * p.Hs + (y < h ? y : 2 * h - 1 - y)) * p.Ws;
        const bool vst = p.vec_st && x0 + 4 <= p.Wp;
        float v[3][4];
        ei_load4(p.gt, row, x0, w, p.Wp, p.vec_ld != 0, v);
        if (p.clamp) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[c][j] = fminf(fmaxf(v[c][j], p.lo), p.hi);
        }
        ei_store4(p.out_img + b * p.img_bs + (long long)y * p.Wp + x0, hw, x0, p.Wp, vst, v);
        ei_load4(p.pred, row, x0, w, p.Wp, p.vec_ld != 0, v);
        ei_store4(p.out_pred + b * p.pred_bs + (long long)y * p.Wp + x0, hw, x0, p.Wp, vst, v);
    }
}

// ---- dataset.scale_factor on the device: the loader's chain for one batch of DECODED u8 images in one launch --
//   image.astype('float32') / 255 (evaluation/data.py:12-20), cv2.resize(fx = fy = factor) with INTER_AREA on the image and INTER_NEAREST on the
//   mask (data.py:42-55,74-77), pad_img_to_modulo's symmetric padding of the SCALED result (data.py:29-33), mask > 0 (bin/predict.py:84).
// The resize is lama_amd/predict.py's restatement of OpenCV's resize.cpp (_resize_area, _area_taps, _resize_nearest) and the contract is
// BIT-IDENTITY with it: the same IEEE operations in the same order.  Tap indices and weights are computed per output pixel in fp64 from the
// destination index, scale = 1.0 / factor and the image's OWN size (the images of one batch differ in size: no table can be precomputed), and
// rounded to fp32 where the Python rounds them.  Every function below switches floating-point contraction OFF (device and host compiler alike):
// buf + a * w must stay a multiply and an add, f1 + scale must not fuse with the multiply that made f1.
// Two simplifications that change no bit: sums start from +0 instead of from their first term (every term is non-negative and finite, +0 + x = x),
// and the zero-weight padding taps of the host's tables are not visited (x + 0 = x).
#define LAMA_RESIZE_AREA_INT 0      // scale = 1 / factor is an integer: resizeAreaFast
#define LAMA_RESIZE_AREA_FRAC 1     // scale > 1: computeResizeAreaTab + ResizeArea_Invoker
#define LAMA_RESIZE_LINEAR 2        // scale < 1: the linear path with area coefficients
struct ResizeParams {
    const uint8_t* img;          // [B][Hs][Ws][3], each image's h x w pixels in the top-left corner of its slot
    const uint8_t* mask;         // [B][Hs][Ws]
    const int32_t* src_sizes;    // [B][2] = (h, w); h = 0: an empty slot -> zeros
    const int32_t* dst_sizes;    // [B][2] = scaled_size(h, w, factor), from the host
    float* out_img;              // [B,3,Hp,Wp]
    long long img_bs;
    float* out_mask;             // [B,1,Hp,Wp]
    long long mask_bs;
    double factor, scale;        // scale = 1.0 / factor: one fp64 division on the host, as the Python does it
    float inv_area;              // integer shrink: float32(1.0 / (isc * isc))
    int B, Hs, Ws, Hp, Wp, binarize, regime, isc;
};
__device__ __forceinline__ float rz_px(const uint8_t* q) { return (float)q[0] / 255.0f; }
// one destination index of computeResizeAreaTab (_area_taps): an optional first tap s1 - 1 (wa), the whole cells s1 .. s2 - 1 (wm), an optional
// last tap s2 (wb)
struct AreaTaps {
    int s1, s2;
    float wa, wm, wb;
    bool first, last;
};
__device__ __forceinline__ AreaTaps rz_area_taps(int d, int ssize, double scale) {
#pragma clang fp contract(off)
    AreaTaps t;
    const double f1 = (double)d * scale;
    const double f2 = f1 + scale;
    const double rem = (double)ssize - f1;
    const double cell = rem < scale ? rem : scale;
    const double c1 = ceil(f1), c2 = floor(f2), last = (double)(ssize - 1);
    int s1 = (int)(c1 < last ? c1 : last), s2 = (int)(c2 < last ? c2 : last);       // s2 = min(s2, ssize - 1); s1 = min(s1, s2) below
    s1 = s1 < s2 ? s1 : s2;
    s1 = s1 > 0 ? s1 : 0;                                      // (never taken for sizes the host computed: keeps every read inside the image)
    s2 = s2 > 0 ? s2 : 0;
    const double da = (double)s1 - f1;
    double db = f2 - (double)s2;
    t.first = da > 1e-3 && s1 > 0;
    t.last = db > 1e-3;
    db = db < 1.0 ? db : 1.0;
    db = db < cell ? db : cell;
    t.s1 = s1; t.s2 = s2;
    t.wa = (float)(da / cell);
    t.wm = (float)(1.0 / cell);
    t.wb = (float)(db / cell);
    return t;
}
// the x pass of ResizeArea_Invoker over one source row, three channels: buf += S[sx] * alpha, taps in table order
__device__ __forceinline__ void rz_area_row(const uint8_t* row, const AreaTaps& t, float buf[3]) {
#pragma clang fp contract(off)
    buf[0] = buf[1] = buf[2] = 0.0f;
    if (t.first) {
        const uint8_t* q = row + (long long)(t.s1 - 1) * 3;
        for (int c = 0; c < 3; ++c) buf[c] = buf[c] + rz_px(q + c) * t.wa;
    }
    for (int sx = t.s1; sx < t.s2; ++sx) {
        const uint8_t* q = row + (long long)sx * 3;
        for (int c = 0; c < 3; ++c) buf[c] = buf[c] + rz_px(q + c) * t.wm;
    }
    if (t.last) {
        const uint8_t* q = row + (long long)t.s2 * 3;
        for (int c = 0; c < 3; ++c) buf[c] = buf[c] + rz_px(q + c) * t.wb;
    }
}
// enlarging (_resize_area's coef): sx = floor(d * scale), fx = float32((d + 1) - (sx + 1) * factor) kept in [0, 1)
struct LinTaps {
    int i0, i1;
    float a0, a1;
};
__device__ __forceinline__ LinTaps rz_lin_taps(int d, int ssize, double scale, double factor) {
#pragma clang fp contract(off)
    LinTaps t;
    int sx = (int)floor((double)d * scale);
    const double prod = (double)(sx + 1) * factor;
    float fx = (float)((double)(d + 1) - prod);
    fx = fx <= 0.0f ? 0.0f : fx - floorf(fx);
    if (sx < 0) { fx = 0.0f; sx = 0; }
    if (sx >= ssize - 1) { fx = 0.0f; sx = ssize - 1; }
    t.i0 = sx;
    t.i1 = sx + 1 < ssize - 1 ? sx + 1 : ssize - 1;
    t.a0 = 1.0f - fx;
    t.a1 = fx;
    return t;
}
__global__ __launch_bounds__(LAMA_NTHREADS) void resize_u8_kernel(ResizeParams p) {
#pragma clang fp contract(off)
    const long long hw = (long long)p.Hp * p.Wp, total = (long long)p.B * hw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / hw);
        const long long px = i - (long long)b * hw;
        const int y = (int)(px / p.Wp), x = (int)(px - (long long)y * p.Wp);
        const int h = p.src_sizes[2 * b], w = p.src_sizes[2 * b + 1], dh = p.dst_sizes[2 * b], dw = p.dst_sizes[2 * b + 1];
        float v[3] = {0.0f, 0.0f, 0.0f}, m = 0.0f;
        // an empty slot, or sizes that do not fit the slot / the output view (the host cannot see them without a synchronisation): zeros
        if (h > 0 && w > 0 && dh > 0 && dw > 0 && h <= p.Hs && w <= p.Ws && dh <= p.Hp && dw <= p.Wp) {
            const int ys = ew_symmetric(y, dh), xs = ew_symmetric(x, dw);
            const uint8_t* src = p.img + (long long)b * p.Hs * p.Ws * 3;
            const long long rs = (long long)p.Ws * 3;                              // bytes per source row of the slot
            if (p.regime == LAMA_RESIZE_AREA_INT) {
                const int isc = p.isc;
                const int dh2 = dh < h / isc ? dh : h / isc, dw2 = dw < w / isc ? dw : w / isc;
                if (ys < dh2 && xs < dw2) {                                          // resizeAreaFast: the box sy-major, four at a time, * float32(1 / area)
                    const uint8_t* base = src + (long long)ys * isc * rs + (long long)xs * isc * 3;
                    const int area = isc * isc;
                    int k = 0, sy = 0, sx = 0;
                    float t[4][3];
                    for (; k <= area - 4; k += 4) {
                        for (int j = 0; j < 4; ++j) {
                            const uint8_t* q = base + sy * rs + sx * 3;
                            for (int c = 0; c < 3; ++c) t[j][c] = rz_px(q + c);
                            if (++sx == isc) { sx = 0; ++sy; }
                        }
                        for (int c = 0; c < 3; ++c) v[c] = v[c] + (((t[0][c] + t[1][c]) + t[2][c]) + t[3][c]);
                    }
                    for (; k < area; ++k) {
                        const uint8_t* q = base + sy * rs + sx * 3;
                        for (int c = 0; c < 3; ++c) v[c] = v[c] + rz_px(q + c);
                        if (++sx == isc) { sx = 0; ++sy; }
                    }
                    for (int c = 0; c < 3; ++c) v[c] = v[c] * p.inv_area;
                } else {                                                             // its border loop: row-major sum of the pixels inside the image / their count
                    const long long ly0 = (long long)ys * isc, lx0 = (long long)xs * isc;
                    const int y0 = (int)(ly0 < h ? ly0 : h), x0 = (int)(lx0 < w ? lx0 : w);
                    const int y1 = ly0 + isc < h ? (int)(ly0 + isc) : h, x1 = lx0 + isc < w ? (int)(lx0 + isc) : w;
                    const int cnt = (y1 - y0) * (x1 - x0);
                    if (cnt > 0) {
                        for (int yy = y0; yy < y1; ++yy)
                            for (int xx = x0; xx < x1; ++xx) {
                                const uint8_t* q = src + yy * rs + (long long)xx * 3;
                                for (int c = 0; c < 3; ++c) v[c] = v[c] + rz_px(q + c);
                            }
                        for (int c = 0; c < 3; ++c) v[c] = v[c] / (float)cnt;
                    }
                }
            } else if (p.regime == LAMA_RESIZE_AREA_FRAC) {                          // the x pass of each source row this pixel needs, then the y pass over them
                const AreaTaps tx = rz_area_taps(xs, w, p.scale), ty = rz_area_taps(ys, h, p.scale);
                float buf[3];
                if (ty.first) {
                    rz_area_row(src + (long long)(ty.s1 - 1) * rs, tx, buf);
                    for (int c = 0; c < 3; ++c) v[c] = v[c] + buf[c] * ty.wa;
                }
                for (int sy = ty.s1; sy < ty.s2; ++sy) {
                    rz_area_row(src + sy * rs, tx, buf);
                    for (int c = 0; c < 3; ++c) v[c] = v[c] + buf[c] * ty.wm;
                }
                if (ty.last) {
                    rz_area_row(src + ty.s2 * rs, tx, buf);
                    for (int c = 0; c < 3; ++c) v[c] = v[c] + buf[c] * ty.wb;
                }
            } else {                                                                 // rows = a[x0] * ax0 + a[x1] * ax1, then the same in y
                const LinTaps tx = rz_lin_taps(xs, w, p.scale, p.factor), ty = rz_lin_taps(ys, h, p.scale, p.factor);
                const uint8_t* r0 = src + ty.i0 * rs;
                const uint8_t* r1 = src + ty.i1 * rs;
                for (int c = 0; c < 3; ++c) {
                    const float row0 = rz_px(r0 + tx.i0 * 3 + c) * tx.a0 + rz_px(r0 + tx.i1 * 3 + c) * tx.a1;
                    const float row1 = rz_px(r1 + tx.i0 * 3 + c) * tx.a0 + rz_px(r1 + tx.i1 * 3 + c) * tx.a1;
                    v[c] = row0 * ty.a0 + row1 * ty.a1;
                }
            }
            // INTER_NEAREST (_resize_nearest): tap min(floor(d * (1 / factor)), size - 1)
            const double fy = floor((double)ys * p.scale), fx = floor((double)xs * p.scale);
            const int my = fy < (double)(h - 1) ? (int)fy : h - 1, mx = fx < (double)(w - 1) ? (int)fx : w - 1;
            const uint8_t mu = p.mask[((long long)b * p.Hs + my) * p.Ws + mx];
            m = p.binarize ? (mu > 0 ? 1.0f : 0.0f) : (float)mu / 255.0f;
        }
        float* o = p.out_img + b * p.img_bs + px;
        o[0] = v[0];
        o[hw] = v[1];
        o[2 * hw] = v[2];
        p.out_mask[b * p.mask_bs + px] = m;
    }
}

// ---- the item walk of the kernels that rewrite a batch of u8 source slots (paste_back_u8_kernel, crop_paste_u8_kernel) --
// Streaming kernels: 7 bytes per source pixel (1 mask + 3 in + 3 out).  One work item = 4 consecutive pixels of a slot row: one dword of mask,
// three dwords of RGB in, three out (VEC: dword accesses, where Ws % 4 == 0 and the pointers allow; byte accesses otherwise).  A 256-thread
// workgroup takes U8_UNROLL * 256 items of ONE image, so what the policy loads per image is uniform (scalar loads, its divisions once per
// workgroup) -- ROW: 256 consecutive items of U8_UNROLL consecutive rows (slots of U8_ROW_MIN_ITEMS items per row or more: the row and what
// hangs on it are uniform too); otherwise consecutive items of the slot, a lane divides once per item by the items per row.  A lane has the
// streaming loads of all its items in flight before the policy's own reads, and every load before its first store; the loads are unconditional
// (a lane past the end re-reads the last item and stores nothing).  No LDS, no atomics.
// A kernel is this walk and a policy:
//   Policy(p, b)        the state of image b, loaded once per workgroup: ok (false: the slot becomes zeros), h, w (zeros outside h x w) and its own
//   row(y)              what one row of the image shares
//   pixel(r, x, mu, sb) the three bytes of pixel (y, x) in place of its source bytes sb, given its mask byte mu != 0: a pixel whose mask byte is 0
//                       keeps its source bytes without a call, so nothing but the streams is read for it
// Policies and their helpers do float arithmetic with contraction OFF (every operation rounded on its own); the walk itself does none.
#define U8_THREADS 256
#define U8_UNROLL 4
#define U8_ROW_MIN_ITEMS 192
struct U8WalkParams {
    const uint8_t* img;          // [B][Hs][Ws][3], each image's h x w pixels in the top-left corner of its slot
    const uint8_t* mask;         // [B][Hs][Ws]
    const int32_t* src_sizes;    // [B][2] = (h, w); h = 0: an empty slot
    uint8_t* out_u8;             // [B][Hs][Ws][3]: the slots the walk writes (crop_compose_u8_kernel: none)
    int Hs, Ws, binarize;        // (the ints follow the pointers, a kernel's own ints come first in its struct: the arguments load in wide runs)
    int qpr, chunks, ygroups;    // items per row; workgroups per row (ROW) / per image; groups of U8_UNROLL rows per slot (ROW)
};
// item k of a lane where a workgroup takes consecutive items of one image: (y, q) of the item, of the last one for a lane past the end (false)
__device__ __forceinline__ bool u8_item(int chunk, int k, int tid, int nitems, int qpr, int& y, int& q) {
    const int v = (chunk * U8_UNROLL + k) * U8_THREADS + tid;
    const unsigned vc = (unsigned)(v < nitems ? v : nitems - 1);
    y = (int)(vc / (unsigned)qpr); q = (int)(vc - (unsigned)y * (unsigned)qpr);
    return v < nitems;
}
template <bool VEC, bool ROW, class Policy> __device__ __forceinline__ void u8_slot_walk(const typename Policy::Params& p) {
    int blk = blockIdx.x;
    const int chunk = blk % p.chunks; blk /= p.chunks;
    const int yg = ROW ? blk % p.ygroups : 0, b = ROW ? blk / p.ygroups : blk;
    const int tid = threadIdx.x;
    const Policy pol(p, b);
    const long long slot = (long long)b * p.Hs * p.Ws;
    const uint8_t* img = p.img + slot * 3;
    const uint8_t* msk = p.mask + slot;
    uint8_t* out = p.out_u8 + slot * 3;
    const int nitems = p.Hs * p.qpr;

    int yy[U8_UNROLL], qq[U8_UNROLL];
    bool valid[U8_UNROLL];
    uint32_t m4[U8_UNROLL], d[U8_UNROLL][3];
#pragma unroll
    for (int k = 0; k < U8_UNROLL; ++k) {                 // the streaming loads of every item, none behind a branch
        int y, q;
        if (ROW) {
            y = yg * U8_UNROLL + k; q = chunk * U8_THREADS + tid;
            valid[k] = y < p.Hs && q < p.qpr;
            y = y < p.Hs ? y : p.Hs - 1; q = q < p.qpr ? q : p.qpr - 1;
        } else {
            valid[k] = u8_item(chunk, k, tid, nitems, p.qpr, y, q);
        }
        yy[k] = y; qq[k] = q;
        u8_load4(img, msk, (long long)y * p.Ws, 4 * q, p.Ws, VEC, [](int x) { return x; }, m4[k], d[k]);
    }
#pragma unroll
    for (int k = 0; k < U8_UNROLL; ++k) {                 // the bytes to store, in place of the bytes loaded
        uint32_t o[3] = {0u, 0u, 0u};
        const int y = yy[k], x0 = 4 * qq[k];
        if (valid[k] && pol.ok && y < pol.h) {
            const typename Policy::Row r = pol.row(y);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + j;
                if (x < pol.w) {
                    const uint32_t mu = (m4[k] >> (8 * j)) & 255u;
                    uint32_t sb[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) sb[c] = u8_get(d[k], 3 * j + c);
                    if (mu != 0u) pol.pixel(r, x, mu, sb);
#pragma unroll
                    for (int c = 0; c < 3; ++c) u8_put(o, 3 * j + c, sb[c]);
                }
            }
        }
        d[k][0] = o[0]; d[k][1] = o[1]; d[k][2] = o[2];
    }
#pragma unroll
    for (int k = 0; k < U8_UNROLL; ++k) {
        if (!valid[k]) continue;
        const long long px = (long long)yy[k] * p.Ws + 4 * qq[k];
        if (VEC) {
            ei_u32* s = reinterpret_cast<ei_u32*>(out + px * 3);
            s[0] = d[k][0]; s[1] = d[k][1]; s[2] = d[k][2];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * qq[k] + j < p.Ws) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) out[(px + j) * 3 + c] = (uint8_t)u8_get(d[k], 3 * j + c);
                }
        }
    }
}

// ---- paste_back: the scaled step's fp32 result resampled to the SOURCE grid and pasted into the decoded u8 original, in one launch --
//   out = source pixel where the mask is 0; elsewhere F.interpolate(lowres[:, :dh, :dw], size=(h, w), mode='bilinear', align_corners=False)
//   (index arithmetic of rf_bilin_src, csrc/refine.hip) blended as mask * v + (1 - mask) * image and quantised as clip(. * 255, 0, 255) truncated.
// This output has no counterpart in the reference (which writes the scaled image): the contract is BYTE-IDENTITY with the numpy restatement
// tests/paste_back_util.py::paste_back_ref -- every operation rounded on its own, as in resize_u8_kernel.  Where the mask byte is 0 both forms of
// the mask give the source byte back ((k / 255.f) * 255.f truncates to k for all 256 values): those pixels are copied.
// u8_slot_walk over the source slots; the policy is the bilinear gather from the low-resolution tensor, which is 1 / 16 of the streams at
// factor 0.25 and stays in L2 / the Infinity Cache.  Sizes that do not fit the slot / the low-resolution view (the host cannot see them
// without a synchronisation) make the slot zeros, as an empty slot is.
struct PasteParams : U8WalkParams {
    int LH, LW;
    const int32_t* dst_sizes;    // [B][2] = (dh, dw): the valid corner of lowres
    const float* low;            // [B,3,LH,LW]
    long long low_bs;
};
struct PbAxis {
    int i0, i1;
    float l;
};
// rf_bilin_src (csrc/refine.hip): src = max(0, (dst + 0.5) * scale - 0.5); i0 = (int)src; i1 = min(i0 + 1, n - 1); l = src - i0
__device__ __forceinline__ PbAxis pb_axis(int o, float scale, int n) {
#pragma clang fp contract(off)
    PbAxis a;
    float s = ((float)o + 0.5f) * scale - 0.5f;
    s = s < 0.0f ? 0.0f : s;
    a.i0 = (int)s;
    if (a.i0 > n - 1) a.i0 = n - 1;
    a.i1 = a.i0 + 1 < n ? a.i0 + 1 : n - 1;
    a.l = s - (float)a.i0;
    return a;
}
// np.clip(r * 255, 0, 255).astype('uint8') as blend_quantize_u8_kernel does it (a NaN becomes 0: fmaxf returns its other operand)
__device__ __forceinline__ uint32_t pb_quant(float r) {
#pragma clang fp contract(off)
    float t = r * 255.0f;
    t = fminf(fmaxf(t, 0.0f), 255.0f);
    return (uint32_t)(uint8_t)t;
}
struct PastePolicy {
    typedef PasteParams Params;
    struct Row {                 // the y taps: byte offsets of their rows inside a plane, the weights
        unsigned r0, r1;
        float l, hl;
    };
    bool ok;
    int h, w, dh, dw, binarize;
    float sy, sx;
    const char* low;
    long long plane;             // bytes of one low-resolution plane, < 2^32
    unsigned rowb;
    __device__ __forceinline__ PastePolicy() {}          // (ShrinkPastePolicy fills the state from a window)
    __device__ __forceinline__ PastePolicy(const PasteParams& p, int b) {
#pragma clang fp contract(off)
        h = p.src_sizes[2 * b]; w = p.src_sizes[2 * b + 1]; dh = p.dst_sizes[2 * b]; dw = p.dst_sizes[2 * b + 1];
        ok = h > 0 && w > 0 && dh > 0 && dw > 0 && h <= p.Hs && w <= p.Ws && dh <= p.LH && dw <= p.LW;
        sy = ok ? (float)dh / (float)h : 0.0f; sx = ok ? (float)dw / (float)w : 0.0f;
        low = reinterpret_cast<const char*>(p.low + (long long)b * p.low_bs);
        plane = 4ll * p.LH * p.LW;
        rowb = 4u * (unsigned)p.LW;
        binarize = p.binarize;
    }
    __device__ __forceinline__ Row row(int y) const {
#pragma clang fp contract(off)
        const PbAxis ay = pb_axis(y, sy, dh);
        Row r;
        r.r0 = (unsigned)ay.i0 * rowb; r.r1 = (unsigned)ay.i1 * rowb;
        r.l = ay.l; r.hl = 1.0f - ay.l;
        return r;
    }
    __device__ __forceinline__ void pixel(const Row& r, int x, uint32_t mu, uint32_t (&sb)[3]) const {
#pragma clang fp contract(off)
        const PbAxis ax = pb_axis(x, sx, dw);
        const float hx = 1.0f - ax.l;
        // byte offsets inside one plane in 32 bits (the entry has checked that they fit) on a plane pointer that is uniform
        const unsigned c0 = 4u * (unsigned)ax.i0, c1 = 4u * (unsigned)ax.i1;
        float t[3][4];                                    // the pixel's twelve taps in flight together, then the arithmetic
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const char* pl = low + c * plane;
            t[c][0] = *reinterpret_cast<const float*>(pl + (r.r0 + c0)); t[c][1] = *reinterpret_cast<const float*>(pl + (r.r0 + c1));
            t[c][2] = *reinterpret_cast<const float*>(pl + (r.r1 + c0)); t[c][3] = *reinterpret_cast<const float*>(pl + (r.r1 + c1));
        }
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = r.hl * (hx * t[c][0] + ax.l * t[c][1]) + r.l * (hx * t[c][2] + ax.l * t[c][3]);
        if (binarize) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sb[c] = pb_quant(v[c]);
        } else {
            const float m = (float)mu / 255.0f, km = 1.0f - m;
#pragma unroll
            for (int c = 0; c < 3; ++c) sb[c] = pb_quant(m * v[c] + km * ((float)sb[c] / 255.0f));
        }
    }
};
template <bool VEC, bool ROW> __global__ __launch_bounds__(U8_THREADS) void paste_back_u8_kernel(PasteParams p) {
    u8_slot_walk<VEC, ROW, PastePolicy>(p);
}

// ---- crop_to_mask: the step's two ends when the generator sees only a WINDOW (y0, x0, ch, cw) of each image's source slot --
//   crop_compose_u8_kernel = mask_compose_u8_kernel, crop_paste_u8_kernel = blend_quantize_u8_kernel on the slot batch that would hold
//   C = image[y0:y0+ch, x0:x0+cw] and M = mask[y0:y0+ch, x0:x0+cw] with sizes (ch, cw) -- BIT FOR BIT (tests/crop_util.py holds both to those
//   entries on host-cropped slots and to a numpy restatement), so the expressions below are theirs, with floating-point contraction OFF -- and
//   the paste writes every source byte outside the window (and inside it where the mask byte is 0: (k / 255.f) * 255.f truncates to k) as it is.
// Like paste_back this output has no counterpart in the reference.  The paste is u8_slot_walk over the source slots with the window test and the
// blend as its policy: it reads the prediction only under the mask, inside the window.  The compose walks the PADDED WINDOW instead, in the same
// items (u8_item, u8_load4: U8_UNROLL * 256 consecutive items of one image per workgroup, every load of a lane before its first store) and
// writes 16 bytes per window pixel (a float4 per plane and item) for 4 read.  No LDS, no atomics.
struct CropParams : U8WalkParams {   // (qpr, chunks: compose: of the padded window, paste: of the slot)
    int Hp, Wp;
    const int32_t* rects;        // [B][4] = (y0, x0, ch, cw): the window
    const float* pred;           // paste: [B,3,Hp,Wp]
    long long pred_bs;
    float* out;                  // compose: [B,4,Hp,Wp]
    long long out_bs;
    int vec_ld, vec_st;          // compose: dword loads from the slots (Ws % 4 == 0, aligned pointers) / float4 stores (Wp % 4 == 0, aligned view)
};
struct CropRect {
    int h, w, y0, x0, ch, cw;
    bool ok;
};
// An empty slot, or a rect that does not fit its image, the slot or the view (device data: the host cannot see it without a synchronisation).
// Every comparison is on values already known to be in range, so nothing overflows.
__device__ __forceinline__ CropRect crop_rect_load(const CropParams& p, int b) {
    CropRect r;
    r.h = p.src_sizes[2 * b]; r.w = p.src_sizes[2 * b + 1];
    r.y0 = p.rects[4 * b]; r.x0 = p.rects[4 * b + 1]; r.ch = p.rects[4 * b + 2]; r.cw = p.rects[4 * b + 3];
    r.ok = r.h > 0 && r.w > 0 && r.h <= p.Hs && r.w <= p.Ws && r.ch >= 1 && r.cw >= 1 && r.ch <= p.Hp && r.cw <= p.Wp && r.ch <= r.h && r.cw <= r.w &&
           r.y0 >= 0 && r.x0 >= 0 && r.y0 <= r.h - r.ch && r.x0 <= r.w - r.cw;
    return r;
}
// masked_img = cat(C / 255 * (1 - m), m) with the symmetric padding of C up to (Hp, Wp): mask_compose_u8_kernel on the window
__global__ __launch_bounds__(U8_THREADS) void crop_compose_u8_kernel(CropParams p) {
#pragma clang fp contract(off)
    const int b = blockIdx.x / p.chunks, chunk = blockIdx.x - b * p.chunks;
    const int tid = threadIdx.x;
    const CropRect r = crop_rect_load(p, b);
    // (a rect that does not fit reads pixel (0, 0) of its slot and writes zeros)
    const int y0 = r.ok ? r.y0 : 0, x0 = r.ok ? r.x0 : 0, ch = r.ok ? r.ch : 1, cw = r.ok ? r.cw : 1;
    const long long slot = (long long)b * p.Hs * p.Ws;
    const uint8_t* img = p.img + slot * 3;
    const uint8_t* msk = p.mask + slot;
    const long long hw = (long long)p.Hp * p.Wp;
    float* out = p.out + b * p.out_bs;
    const int nitems = p.Hp * p.qpr;
    const bool vld = p.vec_ld && (x0 & 3) == 0;          // the window's rows start on a dword of the slot

    int yy[U8_UNROLL], qq[U8_UNROLL];
    bool valid[U8_UNROLL];
    uint32_t m4[U8_UNROLL], d[U8_UNROLL][3];
#pragma unroll
    for (int k = 0; k < U8_UNROLL; ++k) {                 // the loads of every item: dwords for four pixels of the window itself, else mirrored bytes
        valid[k] = u8_item(chunk, k, tid, nitems, p.qpr, yy[k], qq[k]);
        const long long row = (long long)(y0 + ew_symmetric(yy[k], ch)) * p.Ws + x0;
        u8_load4(img, msk, row, 4 * qq[k], p.Wp, vld && 4 * qq[k] + 4 <= cw, [cw](int x) { return ew_symmetric(x, cw); }, m4[k], d[k]);
    }
#pragma unroll
    for (int k = 0; k < U8_UNROLL; ++k) {
        if (!valid[k]) continue;
        float v[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float rgb[3] = {0.f, 0.f, 0.f}, m = 0.f;
            if (r.ok) {
#pragma unroll
                for (int c = 0; c < 3; ++c) rgb[c] = ei_byte(d[k], 3 * j + c);
                const uint32_t mu = (m4[k] >> (8 * j)) & 255u;
                m = p.binarize ? (mu > 0 ? 1.0f : 0.0f) : (float)mu / 255.0f;
            }
            const float km = 1.0f - m;
            v[0][j] = rgb[0] * km; v[1][j] = rgb[1] * km; v[2][j] = rgb[2] * km; v[3][j] = m;
        }
        ei_store4(out + (long long)yy[k] * p.Wp + 4 * qq[k], hw, 4 * qq[k], p.Wp, p.vec_st != 0, v);
    }
}
// out = the source bytes, with blend_quantize_u8_kernel's bytes for (C, M, pred) inside the window; zeros outside h x w
struct CropPastePolicy : CropRect {
    typedef CropParams Params;
    struct Row {
        bool in;                 // the row crosses the window
        unsigned off;            // byte offset of its window row inside one plane in 32 bits (the entry has checked that it fits)
    };
    const char* pred;
    long long plane;             // bytes of one plane of the prediction, < 2^32
    int Wp, binarize;
    __device__ __forceinline__ CropPastePolicy(const CropParams& p, int b) : CropRect(crop_rect_load(p, b)) {
        pred = reinterpret_cast<const char*>(p.pred + (long long)b * p.pred_bs);
        plane = 4ll * p.Hp * p.Wp;
        Wp = p.Wp; binarize = p.binarize;
    }
    __device__ __forceinline__ Row row(int y) const {
        Row r;
        r.in = y >= y0 && y - y0 < ch;
        r.off = r.in ? 4u * (unsigned)(y - y0) * (unsigned)Wp : 0u;
        return r;
    }
    __device__ __forceinline__ void pixel(const Row& r, int x, uint32_t mu, uint32_t (&sb)[3]) const {
#pragma clang fp contract(off)
        if (!(r.in && x >= x0 && x - x0 < cw)) return;
        const unsigned off = r.off + 4u * (unsigned)(x - x0);
        float pr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) pr[c] = *reinterpret_cast<const float*>(pred + c * plane + off);
        const float m = binarize ? 1.0f : (float)mu / 255.0f, km = 1.0f - m;
#pragma unroll
        for (int c = 0; c < 3; ++c) sb[c] = pb_quant(ew_blend(m, km, pr[c], (float)sb[c] / 255.0f));
    }
};
template <bool VEC, bool ROW> __global__ __launch_bounds__(U8_THREADS) void crop_paste_u8_kernel(CropParams p) {
    u8_slot_walk<VEC, ROW, CropPastePolicy>(p);
}

// ---- crop_max_side: the two ends of a crop_to_mask step whose window is SHRUNK by a per-image integer k (1 .. LAMA_SHRINK_MAX) for the generator --
// THIS OUTPUT HAS NO COUNTERPART IN THE REFERENCE: it is this engine's own definition (tests/crop_shrink_util.py restates it in numpy).  With
// C, M the window of image b, dh = ceil(ch / k), dw = ceil(cw / k):
//   crop_shrink_compose_u8_kernel  out = cat(S * (1 - m), m) after the symmetric padding of the dh x dw planes up to (Hp, Wp).  S is the integer
//     shrink of resize_u8_kernel on C, the same operations in the same order: a whole k x k box is summed row-major, four pixels at a time as
//     acc + (((a + b) + c) + d), the rest one by one, times float32(1 / k^2); a box cut by the window's bottom / right edge is that kernel's
//     border loop, the row-major sum of the pixels inside over their count.  The MASK is the MAX of the box's bytes, cut boxes included (not
//     INTER_NEAREST as dataset.scale_factor: a one-pixel stroke must stay a hole for the generator while the paste still replaces it; dh is a
//     ceiling so that every window pixel lies in a box); m = max > 0 (binarize) or max / 255.f.
//   crop_shrink_paste_u8_kernel    paste_back_u8_kernel's bytes for (C, M, lowres, (dh, dw)) on window coordinates (y - y0, x - x0), the source
//     bytes everywhere else: the pixels under the mask are a k-fold bilinear UPSAMPLING of the generator's output.  u8_slot_walk with the window
//     test in front of PastePolicy's gather.
// A work item of the compose is four consecutive pixels of a row of the padded low-resolution view (u8_item, a float4 store per plane): its four
// boxes are one run of 12 k bytes per source row, neighbouring lanes read neighbouring runs, the window is read once and nothing goes through an
// fp32 image / mask in memory.  Where the slots take dword accesses the run is read as aligned dwords, whatever x0 is (ShrinkDwords); byte by
// byte otherwise.  k is uniform in a workgroup.  No LDS, no atomics, no workspace.
#define LAMA_SHRINK_MAX 16       // (1.0 / (1.0 / k) == k in fp64 up to 48: the pin against the host's resize with factor 1 / k relies on it)
struct ShrinkParams : CropParams {   // (pred: the low-resolution result [B,3,Hp,Wp]; Hp, Wp: the padded LOW-RESOLUTION view)
    const int32_t* shrinks;      // [B] = k
    float inv_area[LAMA_SHRINK_MAX + 1];   // float32(1.0 / (k * k)), rounded once from fp64 on the host as resize_u8's inv_area is
};
struct ShrinkRect : CropRect {
    int k, dh, dw;
};
// crop_rect_load's conditions with the low-resolution size in place of the window's, and k in 1 .. LAMA_SHRINK_MAX
__device__ __forceinline__ ShrinkRect shrink_rect_load(const ShrinkParams& p, int b) {
    ShrinkRect r;
    r.h = p.src_sizes[2 * b]; r.w = p.src_sizes[2 * b + 1];
    r.y0 = p.rects[4 * b]; r.x0 = p.rects[4 * b + 1]; r.ch = p.rects[4 * b + 2]; r.cw = p.rects[4 * b + 3];
    r.k = p.shrinks[b];
    r.ok = r.h > 0 && r.w > 0 && r.h <= p.Hs && r.w <= p.Ws && r.ch >= 1 && r.cw >= 1 && r.ch <= r.h && r.cw <= r.w && r.y0 >= 0 && r.x0 >= 0 &&
           r.y0 <= r.h - r.ch && r.x0 <= r.w - r.cw && r.k >= 1 && r.k <= LAMA_SHRINK_MAX;
    r.dh = r.ok ? (r.ch - 1) / r.k + 1 : 0; r.dw = r.ok ? (r.cw - 1) / r.k + 1 : 0;
    r.ok = r.ok && r.dh <= p.Hp && r.dw <= p.Wp;
    return r;
}
// The source pixels of one box row in x order, byte by byte ...
struct ShrinkBytes {
    const uint8_t* pi;
    const uint8_t* pm;
    __device__ __forceinline__ void row(const uint8_t* img, const uint8_t* msk, long long px) { pi = img + px * 3; pm = msk + px; }
    __device__ __forceinline__ void next(float (&t)[3], uint32_t& mu) {
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = rz_px(pi + c);
        const uint32_t m = *pm;
        mu = mu > m ? mu : m;
        pi += 3; ++pm;
    }
};
// ... and from the aligned dwords that hold them (the slots take dword accesses, so every dword that holds a byte of a slot lies inside it): a
// row starts `skip` bytes into its first dword, a dword is loaded only when the next pixel needs a byte of it.  Lanes of one j differ by
// multiples of 12 k bytes (4 k of mask), so a wave refills in step.
struct ShrinkDwords {
    const ei_u32* wi;
    const ei_u32* wm;
    unsigned si, sm, vi, vm;     // bytes to skip in the next dword / bytes held
    uint64_t bi;
    uint32_t bm;
    __device__ __forceinline__ void row(const uint8_t* img, const uint8_t* msk, long long px) {
        const uint8_t* a = img + px * 3;
        const uint8_t* m = msk + px;
        si = (unsigned)(reinterpret_cast<uintptr_t>(a) & 3); sm = (unsigned)(reinterpret_cast<uintptr_t>(m) & 3);
        wi = reinterpret_cast<const ei_u32*>(a - si); wm = reinterpret_cast<const ei_u32*>(m - sm);
        vi = vm = 0u; bi = 0ull; bm = 0u;
    }
    __device__ __forceinline__ void next(float (&t)[3], uint32_t& mu) {
        while (vi < 3u) {
            const uint64_t w = (uint64_t)(*wi++) >> (8u * si);
            bi |= w << (8u * vi);
            vi += 4u - si; si = 0u;
        }
        if (vm == 0u) {
            bm = *wm++ >> (8u * sm);
            vm = 4u - sm; sm = 0u;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = (float)(uint32_t)((bi >> (8 * c)) & 255u) / 255.0f;
        const uint32_t m = bm & 255u;
        mu = mu > m ? mu : m;
        bi >>= 24; vi -= 3u; bm >>= 8; --vm;
    }
};
// S and the mask's max of the box of bh x bw pixels (k x k: whole) whose top-left pixel is `base`; rs: pixels per slot row
template <class Stream> __device__ __forceinline__ void shrink_box(const uint8_t* img, const uint8_t* msk, long long base, long long rs, int bh, int bw, int k,
                                                                   float inv_area, float (&v)[3], uint32_t& mu) {
#pragma clang fp contract(off)
    Stream st;
    v[0] = v[1] = v[2] = 0.0f;
    mu = 0u;
    st.row(img, msk, base);
    if (bh == k && bw == k) {                             // resizeAreaFast: the box sy-major, four at a time, * float32(1 / area)
        const int area = k * k;
        int n = 0, sx = 0;
        float t[4][3];
        for (; n <= area - 4; n += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                st.next(t[j], mu);
                if (++sx == k) { sx = 0; base += rs; st.row(img, msk, base); }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = v[c] + (((t[0][c] + t[1][c]) + t[2][c]) + t[3][c]);
        }
        for (; n < area; ++n) {
            st.next(t[0], mu);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = v[c] + t[0][c];
            if (++sx == k) { sx = 0; base += rs; st.row(img, msk, base); }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = v[c] * inv_area;
    } else {                                              // its border loop: row-major sum of the pixels inside the window / their count
        float t[3];
        for (int yy = 0; yy < bh; ++yy) {
            for (int xx = 0; xx < bw; ++xx) {
                st.next(t, mu);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = v[c] + t[c];
            }
            base += rs;
            st.row(img, msk, base);
        }
        const float cnt = (float)(bh * bw);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = v[c] / cnt;
    }
}
template <bool VEC> __global__ __launch_bounds__(U8_THREADS) void crop_shrink_compose_u8_kernel(ShrinkParams p) {
#pragma clang fp contract(off)
    const int b = blockIdx.x / p.chunks, chunk = blockIdx.x - b * p.chunks;
    const int tid = threadIdx.x;
    const ShrinkRect r = shrink_rect_load(p, b);
    // (a rect that does not fit reads pixel (0, 0) of its slot and writes zeros)
    const int k = r.ok ? r.k : 1, y0 = r.ok ? r.y0 : 0, x0 = r.ok ? r.x0 : 0, ch = r.ok ? r.ch : 1, cw = r.ok ? r.cw : 1;
    const int dh = r.ok ? r.dh : 1, dw = r.ok ? r.dw : 1;
    const float inv_area = p.inv_area[k];
    const long long slot = (long long)b * p.Hs * p.Ws;
    const uint8_t* img = p.img + slot * 3;
    const uint8_t* msk = p.mask + slot;
    const long long hw = (long long)p.Hp * p.Wp;
    float* out = p.out + b * p.out_bs;
    const int nitems = p.Hp * p.qpr;
#pragma unroll 1
    for (int it = 0; it < U8_UNROLL; ++it) {
        int y, q;
        if (!u8_item(chunk, it, tid, nitems, p.qpr, y, q)) continue;
        const int by = ew_symmetric(y, dh) * k, bh = k < ch - by ? k : ch - by;
        const long long row = (long long)(y0 + by) * p.Ws + x0;
        float v[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = 4 * q + j < p.Wp ? 4 * q + j : p.Wp - 1;                   // (a column past the view repeats the last one; it is never stored)
            const int bx = ew_symmetric(x, dw) * k, bw = k < cw - bx ? k : cw - bx;
            float s[3], m = 0.0f;
            uint32_t mu;
            if (VEC) shrink_box<ShrinkDwords>(img, msk, row + bx, p.Ws, bh, bw, k, inv_area, s, mu);
            else shrink_box<ShrinkBytes>(img, msk, row + bx, p.Ws, bh, bw, k, inv_area, s, mu);
            if (r.ok) m = p.binarize ? (mu > 0u ? 1.0f : 0.0f) : (float)mu / 255.0f;
            else s[0] = s[1] = s[2] = 0.0f;
            const float km = 1.0f - m;
            v[0][j] = s[0] * km; v[1][j] = s[1] * km; v[2][j] = s[2] * km; v[3][j] = m;
        }
        ei_store4(out + (long long)y * p.Wp + 4 * q, hw, 4 * q, p.Wp, p.vec_st != 0, v);
    }
}
// out = the source bytes, with paste_back_u8_kernel's bytes for (C, M, lowres, (dh, dw)) inside the window; zeros outside h x w
struct ShrinkPastePolicy : PastePolicy {
    typedef ShrinkParams Params;
    struct Row : PastePolicy::Row {
        bool in;                 // the row crosses the window
    };
    int y0, x0, ch, cw;
    __device__ __forceinline__ ShrinkPastePolicy(const ShrinkParams& p, int b) {
#pragma clang fp contract(off)
        const ShrinkRect r = shrink_rect_load(p, b);
        ok = r.ok; h = r.h; w = r.w; dh = r.dh; dw = r.dw;
        y0 = r.y0; x0 = r.x0; ch = r.ch; cw = r.cw;
        sy = ok ? (float)dh / (float)ch : 0.0f; sx = ok ? (float)dw / (float)cw : 0.0f;
        low = reinterpret_cast<const char*>(p.pred + (long long)b * p.pred_bs);
        plane = 4ll * p.Hp * p.Wp;
        rowb = 4u * (unsigned)p.Wp;
        binarize = p.binarize;
    }
    __device__ __forceinline__ Row row(int y) const {
        Row r;
        r.in = y >= y0 && y - y0 < ch;
        static_cast<PastePolicy::Row&>(r) = PastePolicy::row(r.in ? y - y0 : 0);
        return r;
    }
    __device__ __forceinline__ void pixel(const Row& r, int x, uint32_t mu, uint32_t (&sb)[3]) const {
        if (r.in && x >= x0 && x - x0 < cw) PastePolicy::pixel(r, x - x0, mu, sb);
    }
};
template <bool VEC, bool ROW> __global__ __launch_bounds__(U8_THREADS) void crop_shrink_paste_u8_kernel(ShrinkParams p) {
    u8_slot_walk<VEC, ROW, ShrinkPastePolicy>(p);
}

struct AffineParams {
    const float* x;
    long long x_bs;
    const float* scale;
    const float* shift;
    float* y;
    long long y_bs;
    long long hw;
    int C, B, act;
};

// y = act(x*scale[c] + shift[c]): stand-alone BatchNorm2d(eval) / ReLU / Sigmoid / Tanh layers
// (generator.model[25], [26], [35] ... when a caller runs the Sequential layer by layer)
__global__ __launch_bounds__(LAMA_NTHREADS) void affine_act_kernel(AffineParams p) {
    long long per = (long long)p.C * p.hw, total = per * p.B;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int b = (int)(i / per);
        long long r = i - (long long)b * per;
        int c = (int)(r / p.hw);
        float v = p.x[b * p.x_bs + r];
        if (p.scale) v = v * p.scale[c] + p.shift[c];
        if (p.act == LAMA_ACT_RELU) v = fmaxf(v, 0.0f);
        else if (p.act == LAMA_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
        else if (p.act == LAMA_ACT_TANH) v = tanhf(v);
        p.y[b * p.y_bs + r] = v;
    }
}

struct PadParams {
    const float* x;
    long long x_bs;
    float* y;
    long long y_bs;
    int C, B, H, W, pad;
};

// nn.ReflectionPad2d(pad) as a stand-alone layer (generator.model[0], [33])
__global__ __launch_bounds__(LAMA_NTHREADS) void reflect_pad_kernel(PadParams p) {
    const int Ho = p.H + 2 * p.pad, Wo = p.W + 2 * p.pad;
    long long per = (long long)p.C * Ho * Wo, total = per * p.B;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int b = (int)(i / per);
        long long r = i - (long long)b * per;
        int xo = (int)(r % Wo);
        long long r2 = r / Wo;
        int yo = (int)(r2 % Ho);
        int c = (int)(r2 / Ho);
        int yi = yo - p.pad, xi = xo - p.pad;
        if (yi < 0) yi = -yi;
        if (yi >= p.H) yi = 2 * (p.H - 1) - yi;
        if (xi < 0) xi = -xi;
        if (xi >= p.W) xi = 2 * (p.W - 1) - xi;
        p.y[b * p.y_bs + r] = p.x[b * p.x_bs + ((long long)c * p.H + yi) * p.W + xi];
    }
}

namespace {
int ew_grid(long long total) {
    long long g = (total + LAMA_NTHREADS - 1) / LAMA_NTHREADS;
    return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g));
}
bool same_hw(const lama_tensor* a, const lama_tensor* b) { return a->H == b->H && a->W == b->W; }
// the glue kernels around the generator (image / mask side) are fp32 only; the fp16 activation path (LAMA_DT_F16) starts at the
// stem's output and ends at the head's input
bool all_f32(std::initializer_list<const lama_tensor*> ts) {
    for (const lama_tensor* t : ts)
        if (t && t->ptr && t->dtype != LAMA_DT_F32) return false;
    return true;
}
}  // namespace

extern "C" int lama_version(void) { return LAMA_HIP_VERSION; }

extern "C" const char* lama_error_string(int code) {
    switch (code) {
        case LAMA_OK: return "ok";
        case LAMA_ERR_BAD_ARG: return "bad argument";
        case LAMA_ERR_UNSUPPORTED: return "unsupported shape or option";
        case LAMA_ERR_WORKSPACE: return "workspace missing or too small";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

extern "C" int lama_mask_compose_fwd(void* stream, const lama_tensor* image, const lama_tensor* mask,
                                     const lama_tensor* out, int32_t batch) {
    if (!image || !mask || !out || !image->ptr || !mask->ptr || !out->ptr || batch <= 0) return LAMA_ERR_BAD_ARG;
    if (image->C != 3 || mask->C != 1 || out->C != 4 || !same_hw(image, mask) || !same_hw(image, out)) return LAMA_ERR_BAD_ARG;
    if (!all_f32({image, mask, out})) return LAMA_ERR_UNSUPPORTED;
    EwParams p;
    memset(&p, 0, sizeof(p));
    p.img = (const float*)image->ptr; p.img_bs = image->batch_stride;
    p.mask = (const float*)mask->ptr; p.mask_bs = mask->batch_stride;
    p.out = (float*)out->ptr; p.out_bs = out->batch_stride;
    p.hw = (long long)image->H * image->W;
    p.B = batch;
    hipLaunchKernelGGL(mask_compose_kernel, dim3(ew_grid(p.B * p.hw)), dim3(LAMA_NTHREADS), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" int lama_blend_fwd(void* stream, const lama_tensor* image, const lama_tensor* mask, const lama_tensor* pred,
                              const lama_tensor* out, int32_t batch) {
    if (!image || !mask || !pred || !out || !image->ptr || !mask->ptr || !pred->ptr || !out->ptr || batch <= 0) return LAMA_ERR_BAD_ARG;
    if (image->C != 3 || mask->C != 1 || pred->C != 3 || out->C != 3) return LAMA_ERR_BAD_ARG;
    if (!same_hw(image, mask) || !same_hw(image, pred) || !same_hw(image, out)) return LAMA_ERR_BAD_ARG;
    if (!all_f32({image, mask, pred, out})) return LAMA_ERR_UNSUPPORTED;
    EwParams p;
    memset(&p, 0, sizeof(p));
    p.img = (const float*)image->ptr; p.img_bs = image->batch_stride;
    p.mask = (const float*)mask->ptr; p.mask_bs = mask->batch_stride;
    p.pred = (const float*)pred->ptr; p.pred_bs = pred->batch_stride;
    p.out = (float*)out->ptr; p.out_bs = out->batch_stride;
    p.hw = (long long)image->H * image->W;
    p.B = batch;
    hipLaunchKernelGGL(blend_kernel, dim3(ew_grid(p.B * p.hw)), dim3(LAMA_NTHREADS), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" int lama_quantize_u8_hwc_fwd(void* stream, const lama_tensor* src, uint8_t* dst, int32_t batch,
                                        int32_t crop_h, int32_t crop_w) {
    if (!src || !src->ptr || !dst || batch <= 0 || src->C != 3) return LAMA_ERR_BAD_ARG;
    if (crop_h <= 0 || crop_w <= 0 || crop_h > src->H || crop_w > src->W) return LAMA_ERR_BAD_ARG;
    if (!all_f32({src})) return LAMA_ERR_UNSUPPORTED;
    QuantParams p;
    p.src = (const float*)src->ptr; p.src_bs = src->batch_stride;
    p.dst = dst;
    p.B = batch; p.H = src->H; p.W = src->W; p.ch = crop_h; p.cw = crop_w;
    hipLaunchKernelGGL(quantize_u8_hwc_kernel, dim3(ew_grid((long long)batch * crop_h * crop_w * 3)), dim3(LAMA_NTHREADS), 0,
                       (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// (v110) the two ends of the predict step on u8 operands: see mask_compose_u8_kernel / blend_quantize_u8_kernel
extern "C" int lama_mask_compose_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* sizes, const lama_tensor* out,
                                        int32_t batch, int32_t binarize) {
    if (!image_hwc || !mask || !out || !out->ptr || batch <= 0 || out->C != 4 || out->H <= 0 || out->W <= 0) return LAMA_ERR_BAD_ARG;
    if (!all_f32({out})) return LAMA_ERR_UNSUPPORTED;
    U8Params p;
    memset(&p, 0, sizeof(p));
    p.img = image_hwc; p.mask = mask; p.sizes = sizes;
    p.out = (float*)out->ptr; p.out_bs = out->batch_stride;
    p.B = batch; p.Hp = out->H; p.Wp = out->W; p.binarize = binarize;
    hipLaunchKernelGGL(mask_compose_u8_kernel, dim3(ew_grid((long long)batch * out->H * out->W)), dim3(LAMA_NTHREADS), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" int lama_blend_quantize_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* sizes, const lama_tensor* pred,
                                          uint8_t* dst_hwc, int32_t batch, int32_t binarize) {
    if (!image_hwc || !mask || !pred || !pred->ptr || !dst_hwc || batch <= 0 || pred->C != 3 || pred->H <= 0 || pred->W <= 0) return LAMA_ERR_BAD_ARG;
    if (!all_f32({pred})) return LAMA_ERR_UNSUPPORTED;
    U8Params p;
    memset(&p, 0, sizeof(p));
    p.img = image_hwc; p.mask = mask; p.sizes = sizes;
    p.pred = (const float*)pred->ptr; p.pred_bs = pred->batch_stride;
    p.out_u8 = dst_hwc;
    p.B = batch; p.Hp = pred->H; p.Wp = pred->W; p.binarize = binarize;
    hipLaunchKernelGGL(blend_quantize_u8_kernel, dim3(ew_grid((long long)batch * pred->H * pred->W)), dim3(LAMA_NTHREADS), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// work lists of the sparse tail: see tail_flags_kernel / tail_lists_kernel
static bool tail_geometry(const lama_tensor* mask, int32_t batch, const lama_tail_lists* l, TailParams* p) {
    if (!mask || !l || batch <= 0 || mask->H <= 0 || mask->W <= 0 || l->n_up < 0 || l->n_up > TAIL_MAX_UP || l->head_rs < 8 || l->head_rs % 8 != 0) return false;
    memset(p, 0, sizeof(*p));
    p->B = batch; p->H = mask->H; p->W = mask->W;
    p->txh = lama_ceil_div(mask->W, 26); p->rs = l->head_rs; p->ns = lama_ceil_div(mask->H, l->head_rs);
    p->n_up = l->n_up;
    int H = mask->H, W = mask->W;
    for (int i = 0; i < l->n_up; ++i) {          // level i writes the plane level i - 1 (the head for i = 0) reads: twice its own input plane
        if (H % 2 != 0 || W % 2 != 0 || l->up_mg[i] < 1) return false;
        H /= 2; W /= 2;
        p->uh[i] = H; p->uw[i] = W; p->mg[i] = l->up_mg[i];
    }
    long long total = (long long)batch * p->txh * p->ns;
    for (int i = 0; i < l->n_up; ++i) total += (long long)batch * lama_ceil_div(p->uh[i], 4) * lama_ceil_div(p->uw[i], 32) * p->mg[i];
    return total < (1ll << 24);                  // one workgroup closes and compacts every list
}
extern "C" size_t lama_tail_lists_workspace_bytes(int32_t batch, int32_t H, int32_t W, const lama_tail_lists* lists) {
    lama_tensor m;
    memset(&m, 0, sizeof(m));
    m.H = H; m.W = W;
    TailParams p;
    if (!tail_geometry(&m, batch, lists, &p)) return 0;
    size_t n = (size_t)batch * p.txh * p.ns;
    for (int i = 0; i < p.n_up; ++i) n += (size_t)batch * lama_ceil_div(p.uh[i], 4) * lama_ceil_div(p.uw[i], 32);
    return n * sizeof(int32_t);
}
extern "C" int lama_tail_lists_build(void* stream, const lama_tensor* mask, int32_t batch, const lama_tail_lists* lists, void* workspace,
                                     size_t workspace_bytes) {
    TailParams p;
    if (!mask || !mask->ptr || mask->C != 1 || !tail_geometry(mask, batch, lists, &p)) return LAMA_ERR_BAD_ARG;
    if (!all_f32({mask})) return LAMA_ERR_UNSUPPORTED;
    if (!lists->head_list || !lists->head_count) return LAMA_ERR_BAD_ARG;
    for (int i = 0; i < p.n_up; ++i)
        if (!lists->up_list[i] || !lists->up_count[i]) return LAMA_ERR_BAD_ARG;
    if (!workspace || ((uintptr_t)workspace & 3) != 0 || workspace_bytes < lama_tail_lists_workspace_bytes(batch, mask->H, mask->W, lists)) return LAMA_ERR_WORKSPACE;
    p.mask = (const float*)mask->ptr; p.mask_bs = mask->batch_stride;
    int* ws = (int*)workspace;
    p.head_flags = ws;
    ws += (size_t)batch * p.txh * p.ns;
    p.head_list = lists->head_list; p.head_count = lists->head_count;
    for (int i = 0; i < p.n_up; ++i) {
        p.up_flags[i] = ws;
        ws += (size_t)batch * lama_ceil_div(p.uh[i], 4) * lama_ceil_div(p.uw[i], 32);
        p.up_list[i] = lists->up_list[i]; p.up_count[i] = lists->up_count[i];
    }
    hipLaunchKernelGGL(tail_flags_kernel, dim3(batch * p.txh * p.ns), dim3(64), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    hipLaunchKernelGGL(tail_lists_kernel, dim3(1), dim3(TAIL_NT), TAIL_NT * sizeof(int), (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// the evaluator's loader on u8 operands: see eval_ingest_u8_kernel
extern "C" int lama_eval_ingest_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* pred_hwc, const uint8_t* mask, const int32_t* sizes,
                                       int32_t Hs, int32_t Ws, int32_t pad_mod, int32_t clamp, float clamp_lo, float clamp_hi,
                                       const lama_tensor* out_image, const lama_tensor* out_pred, int64_t* mask_sum, int32_t batch) {
    if (!image_hwc || !pred_hwc || !mask || !out_image || !out_pred || !out_image->ptr || !out_pred->ptr || !mask_sum) return LAMA_ERR_BAD_ARG;
    if (batch <= 0 || Hs <= 0 || Ws <= 0 || pad_mod <= 0) return LAMA_ERR_BAD_ARG;
    if (out_image->C != 3 || out_pred->C != 3 || out_image->H <= 0 || out_image->W <= 0 || !same_hw(out_image, out_pred)) return LAMA_ERR_BAD_ARG;
    if (clamp && !(clamp_lo <= clamp_hi)) return LAMA_ERR_BAD_ARG;
    if (((uintptr_t)out_image->ptr & 3) || ((uintptr_t)out_pred->ptr & 3) || ((uintptr_t)mask_sum & 7)) return LAMA_ERR_BAD_ARG;
    if (!all_f32({out_image, out_pred})) return LAMA_ERR_UNSUPPORTED;
    const int Hp = out_image->H, Wp = out_image->W;
    const auto ceil_mod = [pad_mod](long long v) { return (v + pad_mod - 1) / pad_mod * pad_mod; };           // data.py:23-26
    bool small = false;
    for (int b = 0; b < batch; ++b) {
        const int h = sizes ? sizes[2 * b] : Hs, w = sizes ? sizes[2 * b + 1] : Ws;
        if (h <= 0 || w <= 0 || h > Hs || w > Ws) return LAMA_ERR_BAD_ARG;
        if (ceil_mod(h) != Hp || ceil_mod(w) != Wp) return LAMA_ERR_BAD_ARG;          // one padded size per launch: the outputs are one tensor
        small = small || Hp - h > h || Wp - w > w;
    }
    if (small) return LAMA_ERR_UNSUPPORTED;                   // padding beyond the image's own extent (np.pad's periodic mirror) is not served
    const size_t slot = (size_t)Hs * Ws;
    for (int b0 = 0; b0 < batch; b0 += LAMA_EI_MAX_BATCH) {   // the sizes ride in the argument block: LAMA_EI_MAX_BATCH images per launch
        EvalIngestParams p;
        memset(&p, 0, sizeof(p));
        p.B = batch - b0 < LAMA_EI_MAX_BATCH ? batch - b0 : LAMA_EI_MAX_BATCH;
        p.gt = image_hwc + b0 * slot * 3; p.pred = pred_hwc + b0 * slot * 3; p.mask = mask + b0 * slot;
        p.out_img = (float*)out_image->ptr + b0 * out_image->batch_stride; p.img_bs = out_image->batch_stride;
        p.out_pred = (float*)out_pred->ptr + b0 * out_pred->batch_stride; p.pred_bs = out_pred->batch_stride;
        p.sums = (long long*)mask_sum + b0;
        p.lo = clamp_lo; p.hi = clamp_hi; p.clamp = clamp != 0;
        p.Hs = Hs; p.Ws = Ws; p.Hp = Hp; p.Wp = Wp;
        p.vec_ld = Ws % 4 == 0 && !((uintptr_t)p.gt & 3) && !((uintptr_t)p.pred & 3);
        p.vec_st = Wp % 4 == 0 && !((uintptr_t)p.out_img & 15) && !((uintptr_t)p.out_pred & 15) && p.img_bs % 4 == 0 && p.pred_bs % 4 == 0;
        for (int b = 0; b < p.B; ++b) {
            p.sizes[b][0] = sizes ? sizes[2 * (b0 + b)] : Hs;
            p.sizes[b][1] = sizes ? sizes[2 * (b0 + b) + 1] : Ws;
        }
        const int grid = p.B + ew_grid((long long)p.B * Hp * ((Wp + 3) / 4));
        hipLaunchKernelGGL(eval_ingest_u8_kernel, dim3(grid), dim3(LAMA_NTHREADS), LAMA_NTHREADS * sizeof(unsigned long long), (hipStream_t)stream,
                           p);
        LAMA_CHECK_LAUNCH();
    }
    return LAMA_OK;
}

// dataset.scale_factor inside the u8 predict step: see resize_u8_kernel
extern "C" int lama_resize_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes, const int32_t* dst_sizes,
                                  int32_t Hs, int32_t Ws, double factor, const lama_tensor* out_image, const lama_tensor* out_mask, int32_t batch,
                                  int32_t binarize) {
    if (!image_hwc || !mask || !src_sizes || !dst_sizes || !out_image || !out_mask || !out_image->ptr || !out_mask->ptr) return LAMA_ERR_BAD_ARG;
    if (batch <= 0 || Hs <= 0 || Ws <= 0 || !(factor > 0.0) || !(factor <= 1.0e9)) return LAMA_ERR_BAD_ARG;
    if (out_image->C != 3 || out_mask->C != 1 || out_image->H <= 0 || out_image->W <= 0 || !same_hw(out_image, out_mask)) return LAMA_ERR_BAD_ARG;
    const double scale = 1.0 / factor;
    if (!(scale <= 1.0e9)) return LAMA_ERR_BAD_ARG;
    if (!all_f32({out_image, out_mask})) return LAMA_ERR_UNSUPPORTED;
    ResizeParams p;
    memset(&p, 0, sizeof(p));
    p.img = image_hwc; p.mask = mask; p.src_sizes = src_sizes; p.dst_sizes = dst_sizes;
    p.out_img = (float*)out_image->ptr; p.img_bs = out_image->batch_stride;
    p.out_mask = (float*)out_mask->ptr; p.mask_bs = out_mask->batch_stride;
    p.factor = factor; p.scale = scale;
    p.B = batch; p.Hs = Hs; p.Ws = Ws; p.Hp = out_image->H; p.Wp = out_image->W; p.binarize = binarize;
    p.regime = LAMA_RESIZE_LINEAR;
    p.isc = 1;
    if (scale >= 1.0) {                                   // _resize_area: isc = int(round(scale)) (half to even), integer when |scale - isc| < eps
        const double r = nearbyint(scale);
        p.isc = (int)r;
        p.regime = fabs(scale - r) < 2.220446049250313e-16 ? LAMA_RESIZE_AREA_INT : LAMA_RESIZE_AREA_FRAC;
        if (p.regime == LAMA_RESIZE_AREA_INT && p.isc > 32768) return LAMA_ERR_UNSUPPORTED;      // (isc * isc is an int)
        p.inv_area = (float)(1.0 / ((double)p.isc * p.isc));
    }
    hipLaunchKernelGGL(resize_u8_kernel, dim3(ew_grid((long long)batch * p.Hp * p.Wp)), dim3(LAMA_NTHREADS), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// The launch plan of the u8 item kernels (see u8_slot_walk) for `batch` images of H x W pixels: fills p.qpr, p.chunks and -- with `rows`, where
// a row has U8_ROW_MIN_ITEMS items or more -- p.ygroups.  vec: the slots (p.img, p.mask, p.out_u8 where there is one) take dword accesses.
// 64-bit arithmetic throughout: W + 3, H + 3 may not fit an int.
struct U8Plan {
    bool vec, row;
    unsigned nwg;
};
static int u8_walk_plan(U8WalkParams& p, int H, int W, int batch, bool rows, U8Plan& pl) {
    p.qpr = (int)lama_ceil_div64(W, 4);
    pl.vec = p.Ws % 4 == 0 && !(((uintptr_t)p.img | (uintptr_t)p.mask | (uintptr_t)p.out_u8) & 3);
    pl.row = rows && p.qpr >= U8_ROW_MIN_ITEMS;
    long long nwg;
    if (pl.row) {
        p.chunks = (int)lama_ceil_div64(p.qpr, U8_THREADS);
        p.ygroups = (int)lama_ceil_div64(H, U8_UNROLL);
        nwg = (long long)batch * p.ygroups * p.chunks;
    } else {
        const long long n = (long long)H * p.qpr;
        if (n > 0x3fffffffll) return LAMA_ERR_UNSUPPORTED;            // 32-bit item indices
        p.chunks = (int)lama_ceil_div64(n, U8_THREADS * U8_UNROLL);
        nwg = (long long)batch * p.chunks;
    }
    if (nwg > 0x7fffffffll) return LAMA_ERR_UNSUPPORTED;              // one grid dimension
    pl.nwg = (unsigned)nwg;
    return LAMA_OK;
}
// the VEC x ROW instantiation of a walk kernel that a plan asks for
#define U8_LAUNCH1(KERNEL, V, R, pl, stream, p) hipLaunchKernelGGL((KERNEL<V, R>), dim3((pl).nwg), dim3(U8_THREADS), 0, (hipStream_t)(stream), p)
#define U8_LAUNCH(KERNEL, pl, stream, p)                                                                                            \
    do {                                                                                                                            \
        if ((pl).vec) { if ((pl).row) U8_LAUNCH1(KERNEL, true, true, pl, stream, p); else U8_LAUNCH1(KERNEL, true, false, pl, stream, p); } \
        else { if ((pl).row) U8_LAUNCH1(KERNEL, false, true, pl, stream, p); else U8_LAUNCH1(KERNEL, false, false, pl, stream, p); } \
    } while (0)
// an fp32 view of three planes that a paste gathers from with 32-bit byte offsets inside a plane
static int u8_check_rgb_view(const lama_tensor* t) {
    if (!t || !t->ptr || t->C != 3 || t->H <= 0 || t->W <= 0 || t->batch_stride < (int64_t)3 * t->H * t->W) return LAMA_ERR_BAD_ARG;
    if (!all_f32({t})) return LAMA_ERR_UNSUPPORTED;
    if ((uintptr_t)t->ptr & 3) return LAMA_ERR_BAD_ARG;
    if ((long long)t->H * t->W > 0x3fffffffll) return LAMA_ERR_UNSUPPORTED;
    return LAMA_OK;
}

// the scaled step's result pasted back into the source image: see paste_back_u8_kernel
extern "C" int lama_paste_back_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes, const int32_t* dst_sizes,
                                      int32_t Hs, int32_t Ws, const lama_tensor* lowres, uint8_t* out_hwc, int32_t batch, int32_t binarize) {
    if (!image_hwc || !mask || !src_sizes || !dst_sizes || !out_hwc || out_hwc == image_hwc) return LAMA_ERR_BAD_ARG;
    if (batch <= 0 || Hs <= 0 || Ws <= 0) return LAMA_ERR_BAD_ARG;
    if (const int e = u8_check_rgb_view(lowres)) return e;
    PasteParams p;
    memset(&p, 0, sizeof(p));
    p.img = image_hwc; p.mask = mask; p.src_sizes = src_sizes; p.dst_sizes = dst_sizes;
    p.low = (const float*)lowres->ptr; p.low_bs = lowres->batch_stride;
    p.out_u8 = out_hwc;
    p.Hs = Hs; p.Ws = Ws; p.LH = lowres->H; p.LW = lowres->W; p.binarize = binarize != 0;
    U8Plan pl;
    if (const int e = u8_walk_plan(p, Hs, Ws, batch, true, pl)) return e;
    U8_LAUNCH(paste_back_u8_kernel, pl, stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// crop_to_mask: the generator's input from a window of each source slot, and its result pasted into the source: see crop_compose_u8_kernel
extern "C" int lama_crop_compose_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes, const int32_t* rects,
                                        int32_t Hs, int32_t Ws, const lama_tensor* out, int32_t batch, int32_t binarize) {
    if (!image_hwc || !mask || !src_sizes || !rects || !out || !out->ptr) return LAMA_ERR_BAD_ARG;
    if (batch <= 0 || Hs <= 0 || Ws <= 0 || out->C != 4 || out->H <= 0 || out->W <= 0) return LAMA_ERR_BAD_ARG;
    if (out->batch_stride < (int64_t)4 * out->H * out->W) return LAMA_ERR_BAD_ARG;
    if (!all_f32({out})) return LAMA_ERR_UNSUPPORTED;
    if ((uintptr_t)out->ptr & 3) return LAMA_ERR_BAD_ARG;
    CropParams p;
    memset(&p, 0, sizeof(p));
    p.img = image_hwc; p.mask = mask; p.src_sizes = src_sizes; p.rects = rects;
    p.out = (float*)out->ptr; p.out_bs = out->batch_stride;
    p.Hs = Hs; p.Ws = Ws; p.Hp = out->H; p.Wp = out->W; p.binarize = binarize != 0;
    U8Plan pl;                                                        // the items of the padded window, never by rows
    if (const int e = u8_walk_plan(p, out->H, out->W, batch, false, pl)) return e;
    p.vec_ld = pl.vec;
    p.vec_st = out->W % 4 == 0 && out->batch_stride % 4 == 0 && !((uintptr_t)out->ptr & 15);
    hipLaunchKernelGGL(crop_compose_u8_kernel, dim3(pl.nwg), dim3(U8_THREADS), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" int lama_crop_paste_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes, const int32_t* rects,
                                      int32_t Hs, int32_t Ws, const lama_tensor* pred, uint8_t* out_hwc, int32_t batch, int32_t binarize) {
    if (!image_hwc || !mask || !src_sizes || !rects || !out_hwc || out_hwc == image_hwc) return LAMA_ERR_BAD_ARG;
    if (batch <= 0 || Hs <= 0 || Ws <= 0) return LAMA_ERR_BAD_ARG;
    if (const int e = u8_check_rgb_view(pred)) return e;
    CropParams p;
    memset(&p, 0, sizeof(p));
    p.img = image_hwc; p.mask = mask; p.src_sizes = src_sizes; p.rects = rects;
    p.pred = (const float*)pred->ptr; p.pred_bs = pred->batch_stride;
    p.out_u8 = out_hwc;
    p.Hs = Hs; p.Ws = Ws; p.Hp = pred->H; p.Wp = pred->W; p.binarize = binarize != 0;
    U8Plan pl;
    if (const int e = u8_walk_plan(p, Hs, Ws, batch, true, pl)) return e;
    U8_LAUNCH(crop_paste_u8_kernel, pl, stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// crop_max_side: the same two ends with the window shrunk by shrinks[b] for the generator: see crop_shrink_compose_u8_kernel
static void shrink_params(ShrinkParams& p, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes, const int32_t* rects,
                          const int32_t* shrinks, int32_t Hs, int32_t Ws, const lama_tensor* view, int32_t binarize) {
    memset(&p, 0, sizeof(p));
    p.img = image_hwc; p.mask = mask; p.src_sizes = src_sizes; p.rects = rects; p.shrinks = shrinks;
    p.Hs = Hs; p.Ws = Ws; p.Hp = view->H; p.Wp = view->W; p.binarize = binarize != 0;
    for (int k = 1; k <= LAMA_SHRINK_MAX; ++k) p.inv_area[k] = (float)(1.0 / ((double)k * k));
}
extern "C" int lama_crop_shrink_compose_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes,
                                               const int32_t* rects, const int32_t* shrinks, int32_t Hs, int32_t Ws, const lama_tensor* out,
                                               int32_t batch, int32_t binarize) {
    if (!image_hwc || !mask || !src_sizes || !rects || !shrinks || !out || !out->ptr) return LAMA_ERR_BAD_ARG;
    if (batch <= 0 || Hs <= 0 || Ws <= 0 || out->C != 4 || out->H <= 0 || out->W <= 0) return LAMA_ERR_BAD_ARG;
    if (out->batch_stride < (int64_t)4 * out->H * out->W) return LAMA_ERR_BAD_ARG;
    if (!all_f32({out})) return LAMA_ERR_UNSUPPORTED;
    if ((uintptr_t)out->ptr & 3) return LAMA_ERR_BAD_ARG;
    ShrinkParams p;
    shrink_params(p, image_hwc, mask, src_sizes, rects, shrinks, Hs, Ws, out, binarize);
    p.out = (float*)out->ptr; p.out_bs = out->batch_stride;
    U8Plan pl;                                                        // the items of the padded low-resolution view, never by rows
    if (const int e = u8_walk_plan(p, out->H, out->W, batch, false, pl)) return e;
    p.vec_ld = pl.vec;
    p.vec_st = out->W % 4 == 0 && out->batch_stride % 4 == 0 && !((uintptr_t)out->ptr & 15);
    if (pl.vec) hipLaunchKernelGGL(crop_shrink_compose_u8_kernel<true>, dim3(pl.nwg), dim3(U8_THREADS), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(crop_shrink_compose_u8_kernel<false>, dim3(pl.nwg), dim3(U8_THREADS), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" int lama_crop_shrink_paste_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes,
                                             const int32_t* rects, const int32_t* shrinks, int32_t Hs, int32_t Ws, const lama_tensor* lowres,
                                             uint8_t* out_hwc, int32_t batch, int32_t binarize) {
    if (!image_hwc || !mask || !src_sizes || !rects || !shrinks || !out_hwc || out_hwc == image_hwc) return LAMA_ERR_BAD_ARG;
    if (batch <= 0 || Hs <= 0 || Ws <= 0) return LAMA_ERR_BAD_ARG;
    if (const int e = u8_check_rgb_view(lowres)) return e;
    ShrinkParams p;
    shrink_params(p, image_hwc, mask, src_sizes, rects, shrinks, Hs, Ws, lowres, binarize);
    p.pred = (const float*)lowres->ptr; p.pred_bs = lowres->batch_stride;
    p.out_u8 = out_hwc;
    U8Plan pl;
    if (const int e = u8_walk_plan(p, Hs, Ws, batch, true, pl)) return e;
    U8_LAUNCH(crop_shrink_paste_u8_kernel, pl, stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" int lama_affine_act_fwd(void* stream, const lama_tensor* x, const float* scale, const float* shift, int32_t act,
                                   const lama_tensor* y, int32_t batch) {
    if (!x || !y || !x->ptr || !y->ptr || batch <= 0) return LAMA_ERR_BAD_ARG;
    if (x->C != y->C || !same_hw(x, y) || ((scale == nullptr) != (shift == nullptr))) return LAMA_ERR_BAD_ARG;
    if (!all_f32({x, y})) return LAMA_ERR_UNSUPPORTED;
    AffineParams p;
    p.x = (const float*)x->ptr; p.x_bs = x->batch_stride;
    p.scale = scale; p.shift = shift;
    p.y = (float*)y->ptr; p.y_bs = y->batch_stride;
    p.hw = (long long)x->H * x->W;
    p.C = x->C; p.B = batch; p.act = act;
    hipLaunchKernelGGL(affine_act_kernel, dim3(ew_grid(p.hw * p.C * p.B)), dim3(LAMA_NTHREADS), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

extern "C" int lama_reflect_pad_fwd(void* stream, const lama_tensor* x, int32_t pad, const lama_tensor* y, int32_t batch) {
    if (!x || !y || !x->ptr || !y->ptr || batch <= 0 || pad < 0) return LAMA_ERR_BAD_ARG;
    if (x->C != y->C || y->H != x->H + 2 * pad || y->W != x->W + 2 * pad || pad >= x->H || pad >= x->W) return LAMA_ERR_BAD_ARG;
    if (!all_f32({x, y})) return LAMA_ERR_UNSUPPORTED;
    PadParams p;
    p.x = (const float*)x->ptr; p.x_bs = x->batch_stride;
    p.y = (float*)y->ptr; p.y_bs = y->batch_stride;
    p.C = x->C; p.B = batch; p.H = x->H; p.W = x->W; p.pad = pad;
    hipLaunchKernelGGL(reflect_pad_kernel, dim3(ew_grid((long long)batch * y->C * y->H * y->W)), dim3(LAMA_NTHREADS), 0, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// ---- FourierUnit.forward (ffc.py:76-113) as three launches over caller workspace ------------------
// bytes of one spectrum slot of the FourierUnit's workspace: [batch, 2C, h, w/2+1] fp32, rounded up to 256
static size_t fu_spec_bytes(int32_t batch, int32_t C, int32_t h, int32_t w) {
    return ((size_t)batch * 2 * C * h * (w / 2 + 1) * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" size_t lama_fourier_unit_workspace_bytes(int32_t batch, int32_t C, int32_t h, int32_t w) {
    if (batch <= 0 || C <= 0 || h <= 0 || w <= 0) return 0;
    return 2 * fu_spec_bytes(batch, C, h, w) + lama_fft_workspace_bytes(batch, C, h, w);
}

// The ONE statement of the FourierUnit's workspace layout: spec_in (the operand of the spectral 1x1) | spec_out (after BN + ReLU), each
// [batch, 2C, h, w/2+1] in the activation dtype inside a 256-byte aligned slot sized for fp32, then the FFT workspace.
extern "C" int lama_fourier_unit_workspace_views(int32_t batch, int32_t C, int32_t h, int32_t w, int32_t dtype, void* workspace, size_t workspace_bytes,
                                                 lama_tensor* spec_in, lama_tensor* spec_out) {
    if (batch <= 0 || C <= 0 || h <= 0 || w <= 0 || !spec_in || !spec_out) return LAMA_ERR_BAD_ARG;
    if (dtype != LAMA_DT_F32 && dtype != LAMA_DT_F16) return LAMA_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < lama_fourier_unit_workspace_bytes(batch, C, h, w)) return LAMA_ERR_WORKSPACE;
    const int wf = w / 2 + 1;
    char* ws = (char*)workspace;
    *spec_in = lama_tensor{ws, (int64_t)2 * C * h * wf, 2 * C, h, wf, dtype};
    *spec_out = lama_tensor{ws + fu_spec_bytes(batch, C, h, w), (int64_t)2 * C * h * wf, 2 * C, h, wf, dtype};
    return LAMA_OK;
}

static int fourier_unit_impl(void* stream, const lama_tensor* x, const void* w_packed, const float* bias,
                             const lama_tensor* y, int32_t batch, int32_t add_input, int32_t precision,
                             void* workspace, size_t workspace_bytes, uint32_t* range_flag,
                             const lama_conv2d_args* wino_args, void* wino_ws, size_t wino_ws_bytes, int32_t flags = 0) {
    if (!x || !y || !x->ptr || !y->ptr || !w_packed || batch <= 0) return LAMA_ERR_BAD_ARG;
    if (x->C != y->C || x->H != y->H || x->W != y->W) return LAMA_ERR_BAD_ARG;
    const int C = x->C, h = x->H, w = x->W;
    if (!workspace || workspace_bytes < lama_fourier_unit_workspace_bytes(batch, C, h, w)) return LAMA_ERR_WORKSPACE;
    const size_t spec_bytes = fu_spec_bytes(batch, C, h, w);
    char* ws = (char*)workspace;
    if (x->dtype != y->dtype) return LAMA_ERR_UNSUPPORTED;
    lama_tensor s1, s2;
    int rc = lama_fourier_unit_workspace_views(batch, C, h, w, x->dtype, workspace, workspace_bytes, &s1, &s2);
    if (rc) return rc;
    void* fws = ws + 2 * spec_bytes;
    size_t fws_bytes = workspace_bytes - 2 * spec_bytes;
    if (wino_args) {      // the deferred output transform of the Winograd conv of the layer before: inside the rfft2 launch where a kernel does that
        rc = lama_rfft2_winograd_out_fwd(stream, x, &s1, batch, fws, fws_bytes, wino_args, wino_ws, wino_ws_bytes);
        if (rc == LAMA_ERR_UNSUPPORTED) {
            rc = lama_winograd_out_fwd(stream, wino_args, wino_ws, wino_ws_bytes);
            if (rc) return rc;
            rc = lama_rfft2_fwd(stream, x, &s1, batch, fws, fws_bytes);
        }
    } else {
        rc = lama_rfft2_fwd(stream, x, &s1, batch, fws, fws_bytes);
    }
    if (rc) return rc;
    lama_conv2d_args a;
    memset(&a, 0, sizeof(a));
    a.x = s1;
    a.w_packed = w_packed;
    a.kh = a.kw = 1;
    a.stride = 1;
    a.bias = bias;
    a.act = LAMA_ACT_RELU;
    a.y = s2;
    a.batch = batch;
    a.precision = precision;
    a.range_flag = range_flag;
    a.flags = flags & LAMA_CONV_SIBLINGS_MASK;      // a part of the batch beside its siblings: the whole batch's kernel (v109)
    rc = lama_conv2d_fwd(stream, &a);
    if (rc) return rc;
    return lama_irfft2_fwd(stream, &s2, add_input ? x : nullptr, y, batch, fws, fws_bytes);
}

extern "C" int lama_fourier_unit_fwd(void* stream, const lama_tensor* x, const void* w_packed, const float* bias,
                                     const lama_tensor* y, int32_t batch, int32_t add_input, int32_t precision,
                                     void* workspace, size_t workspace_bytes, uint32_t* range_flag) {
    return fourier_unit_impl(stream, x, w_packed, bias, y, batch, add_input, precision, workspace, workspace_bytes, range_flag, nullptr, nullptr, 0);
}

// (v108) FourierUnit.forward of layer l + 1 that also finishes the Winograd local conv of layer l (lama_winograd_conv3x3_fwd with
// LAMA_CONV_DEFER_OUT): its output transform rides in the rfft2 launch (lama_rfft2_winograd_out_fwd) or, where no kernel does that, runs first
extern "C" int lama_fourier_unit_winograd_out_fwd(void* stream, const lama_tensor* x, const void* w_packed, const float* bias,
                                                  const lama_tensor* y, int32_t batch, int32_t add_input, int32_t precision,
                                                  void* workspace, size_t workspace_bytes, uint32_t* range_flag,
                                                  const lama_conv2d_args* wino_args, void* wino_workspace, size_t wino_workspace_bytes) {
    if (!wino_args || !wino_workspace) return LAMA_ERR_BAD_ARG;
    return fourier_unit_impl(stream, x, w_packed, bias, y, batch, add_input, precision, workspace, workspace_bytes, range_flag, wino_args,
                             wino_workspace, wino_workspace_bytes);
}

// (v109) both of the above + the LAMA_CONV_* flags of the spectral 1x1 launch
extern "C" int lama_fourier_unit_ex_fwd(void* stream, const lama_tensor* x, const void* w_packed, const float* bias, const lama_tensor* y,
                                        int32_t batch, int32_t add_input, int32_t precision, void* workspace, size_t workspace_bytes,
                                        uint32_t* range_flag, int32_t flags, const lama_conv2d_args* wino_args, void* wino_workspace,
                                        size_t wino_workspace_bytes) {
    if (wino_args && !wino_workspace) return LAMA_ERR_BAD_ARG;
    return fourier_unit_impl(stream, x, w_packed, bias, y, batch, add_input, precision, workspace, workspace_bytes, range_flag, wino_args,
                             wino_workspace, wino_workspace_bytes, flags);
}

