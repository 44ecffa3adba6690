// Fused implicit-GEMM convolution on the gfx950 16-bit matrix cores with a 3-term split that keeps
// fp32-class accuracy (LAMA_PREC_BF16X3 / LAMA_PREC_F16X3).  This body is compiled twice, by conv_bf16x3.hip
// (CB_F16 = 0: __bf16, v_mfma_f32_32x32x16_bf16) and conv_f16x3.hip (CB_F16 = 1: _Float16, v_mfma_f32_32x32x16_f16):
//
//   x = xh + xl,  w = wh + wl   (xh = half(x) RNE, xl = half(x - xh); same for w)
//   w*x ~= wh*xh + wh*xl + wl*xh          (dropped wl*xl term: 2^-16 relative for bf16, 2^-22 for f16; the
//                                          representation itself carries 16 / 22 mantissa bits)
//
// with fp32 accumulation: three MFMAs per product at 16x the rate of the exact v_mfma_f32_32x32x2_f32 path
// (conv_mfma.hip).  f16 is the more accurate split (measured 2-4x lower end-to-end error) and the default; bf16 keeps
// the fp32 exponent range for activations beyond 65504.  Same fused math as the f32 path:
//
//   y[b,o,p] = act( sum_{c,t} W1[o,c,t] x[b,c,tap_t(p)] [+ sum_c W2[o,c] x2[b,c,p]] + bias[o] ) [+ resid[b,o,p]]
//
// GEMM view per image: M = output channels, N = output pixels (the contiguous NCHW axis -> MFMA
// columns, coalesced loads / stores with no layout transform in HBM), K = (channel chunk, tap).
//
// Workgroup = 512 threads = 8 waves (2 per SIMD), output tile BM channels x BN pixels (BN = 128, a
// TH x TW rectangle; BM = 32 uses 8 waves along N, BN = 256).  K is walked in *stages* of TG taps x
// 16*KS channels (TG*KS MFMA k-steps of 16):
//   * weights: pre-split into (hi, lo) bf16 and pre-packed in MFMA A-fragment order by
//     lama_conv2d_pack_weight, so a stage is ONE contiguous image that is copied L2 -> registers -> LDS with
//     fully coalesced 16-byte accesses (no VALU) and read back with linear, conflict-free ds_read_b128;
//     three LDS buffers, the copy runs two to three stages ahead of the MFMAs;
//   * activations: the input *patch* of a channel chunk (tile + halo, reflection / zero padding
//     applied, stride-2 columns parity-split) is loaded fp32 from HBM/L2 one chunk ahead into
//     registers, split into hi/lo bf16 ONCE per element (v_cvt_pk_bf16_f32) and written to LDS as
//     [channel octet][pixel][8 x bf16] planes: a B fragment (8 consecutive channels of one pixel) is
//     one ds_read_b128, consecutive lanes = consecutive pixels = conflict free for every tap; the
//     9x / 49x im2col reuse never leaves the CU; two patch buffers, ONE barrier per stage.
// A second K segment (1x1 over x2) chains into the same accumulators:
//   out_xg = convl2g(x_l) + convg2g.conv2(x1 + fu(x1))  (ffc.py:161,223) + BN shift + ReLU + residual.
#include "common.h"
#include <stdlib.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
// CB_HALF (f16 back end only): this translation unit holds the LAMA_PREC_F16 launches (fp16 tensors, one product per MAC:
// conv_f16.hip) instead of the fp32-I/O 3-term ones (conv_f16x3.hip) -- two TUs so that hipcc compiles them in parallel
#ifndef CB_HALF
#define CB_HALF 0
#endif
// LAMA_PREC_F16 keeps the lo parts of the WEIGHTS (round 3): two products per MAC, w_hi * x + w_lo * x (the fp16 activation is its own hi
// part).  The packing always held them; the weights live in registers / LDS, so the HBM traffic of the path does not change.  Rounding the
// weights to fp16 was half of the path's error against the fp32 oracle (5.4e-3 of 1.0e-2 max-abs at 512^2).  0 = the round-2 one-product form.
#ifndef CB_HF_W2
#define CB_HF_W2 1
#endif
#if CB_F16
typedef _Float16 cb_half_t;
#define CB_MFMA __builtin_amdgcn_mfma_f32_32x32x16_f16
#if CB_HALF
#define CB_NAME(x) x##_f16
#else
#define CB_NAME(x) x##_f16x3
#endif
#else
typedef __bf16 cb_half_t;
#define CB_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16
#define CB_NAME(x) x##_bf16x3
#endif
typedef cb_half_t bf16x2 __attribute__((ext_vector_type(2)));   // (historic names: 2 / 8 x the 16-bit operand type)
typedef cb_half_t bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

namespace CB_NAME(cbns) {   // the two instantiations of this body must not share type / template names

#define CB_THREADS 512
#define CB_MAX_TAPS 49

// element types of a launch (lama_tensor.dtype of x / x2 and of y / resid): LAMA_PREC_F16 runs on the f16 back end only
// bit 0: x is fp16, bit 1: y / resid are fp16, bit 2: x2 is fp16 (the resnet blocks keep their residual stream fp32, everything
// else of the fp16 path is fp16 -- so the two big convs of a block read or write one fp32 tensor)
// bits 3 / 4 (3-term split precisions only): x / y is LAMA_DT_SPLIT16 -- pre-split (hi, lo) parts in staging order (lama_hip.h); only the
// stem kernel (y) and the 4 x 1 stride-2 launch (x, y) know them, nothing else is ever launched with them
enum { CB_IO_F32 = 0, CB_IO_F16_F32 = 1, CB_IO_F32_F16 = 2, CB_IO_F16 = 3, CB_IO_X2H = 4, CB_IO_XS = 8, CB_IO_YS = 16 };

struct CbSeg {
    const float* x;
    long long bstride;
    int C, H, W;
    const char* w;       // packed weights of this sub-convolution: [stage][k-step][32-row fragment F][hi|lo][lane][8 x bf16]
    int mft;             // fragments per k-step = ceil(M / 32); a k-step image is mft * 2048 bytes
    int nchunk, NG;      // channel chunks (16*KS channels each), tap groups (TG taps each) per chunk
    int stride, pad_mode;
    int dy0, dx0;        // patch origin relative to (gy*stride, gx*stride)
    int PH, PW;          // patch rows / cols (real pixels)
    int PWs, PWh;        // LDS row pitch in pixels; parity-split half width (stride 2) or 0
    int npix;            // pixels per LDS octet plane
    int tapoff[CB_MAX_TAPS];  // LDS pixel offset of tap t inside the patch
    int vpad;                 // MODE 1 / 2: horizontal padding of the folded 7x7 (the 7 horizontal taps are not in the tap list)
};

struct CbParams {
    CbSeg s1, s2;
    const float* bias;
    const float* resid;
    long long resid_bstride;
    float* y;
    long long y_bstride;
    int M, MT;
    int Ho, Wo;
    int GH, GW, oy0, ox0, ostep;
    long long* trace;    // profiling tools only (LAMA_CW_TRACE): 32 int64 per workgroup
    // fused SpectralTransform.conv1 of the NEXT layer (12 x 1 weights-in-registers launch only, conv_wreg_dev.inc): packed 1x1 weights
    // 384 -> 192 with the channel order of the accumulator layout, their BatchNorm shift, and the output x1 [B, 192, Ho, Wo] fp32
    const char* f1_w;
    const float* f1_bias;
    float* f1_y;
    long long f1_y_bstride;
    int TWlog, tiles_x, tiles_y, B;
    int act;
    int wbytes, pbytes;  // bytes of ONE weight-stage buffer / ONE patch buffer (hi + lo planes)
    int nwbuf;           // weight-stage buffers in LDS: min(3, stages)
    unsigned* range_flag;   // lama_conv2d_args.range_flag (f16 split only; may be null)
};

// MODE: 0 = plain convolution; 1 / 2 = the two 7x7 layers of the generator folded into 7-tap (vertical) convolutions so that
// the MFMA K / M dimension is not mostly padding:
//   1 (stem, cin <= 4):  the 7 horizontal taps become virtual input channels cc = c*7 + kx (28 of 32 useful instead of 4 of 16),
//                        generated by shifted loads while the patch is staged;
//   2 (head, cout <= 4): the 7 horizontal taps become virtual OUTPUT rows m' = o*7 + kx (21 of 32 useful instead of 3 of 32):
//                        z[o,kx][y][x'] = sum_{c,ky} W[o,c,ky,kx] x[c][y+ky-pad][x'],  y[o][y][x] = sum_kx z[o,kx][y][x+kx-pad];
//                        the second sum runs in the epilogue through LDS, a 32-column tile yields 26 output columns.
template <int BM, int NACC = 1, int MODE = 0>
struct CbGeom {
    // BM <= 64: all 8 waves along N (256 pixels), 64 rows -> TM = 2; the fused transposed kernel (4 accumulator sets) and the
    // stem (4 channel octets per pixel to stage) keep 2 x 4 waves at BM = 64 (TM = 1, 128 pixels)
    static constexpr int WAVES_M = (BM >= 128 || ((NACC == 4 || MODE == 1) && BM == 64)) ? 2 : 1;
    static constexpr int WAVES_N = 8 / WAVES_M;
    static constexpr int BN = WAVES_N * 32;
    static constexpr int TM = BM / WAVES_M / 32;  // 32-row fragments per wave (BM = 192 -> 3)
    static constexpr int MF = BM / 32;            // fragments per M tile
};

__device__ __forceinline__ int cb_src_coord(int i, int n, int pad_mode) {
    if (pad_mode == LAMA_PAD_REFLECT) {
        if (i < 0) i = -i;
        if (i >= n) i = 2 * (n - 1) - i;
        if (i < 0) i = 0;  // only reachable for pixels of a ragged tile that are never stored
        if (i >= n) i = n - 1;
        return i;
    }
    return (i < 0 || i >= n) ? -1 : i;
}

// (hi, lo) bf16 split of two floats, packed as two dwords (element 0 in the low half)
__device__ __forceinline__ void cb_split2(float a, float b, unsigned& hi, unsigned& lo) {
    f32x2 v = {a, b};
    bf16x2 h = __builtin_convertvector(v, bf16x2);
    f32x2 r = v - __builtin_convertvector(h, f32x2);
    bf16x2 l = __builtin_convertvector(r, bf16x2);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}

// the same split with the residuals formed AND rounded by v_fma_mixlo_f16 / v_fma_mixhi_f16 (f16 back end: 3 instead of 6 VALU instructions per pair --
// round 3's v_fma_mix_f32 form had 4; bit-identical for every fp32 bit pattern: LAMA_F16_SPLIT_LO, common.h).  Used where the split sits in a wave's
// MFMA shadow and VALU issue is what binds (the Winograd staging transform, the spectral GEMM's staging): same-box -0.5 % of the step
// (profiles/r06_ab_split3.txt).  NOT the general cb_split2: in the staging code of the other kernels the inline asm costs the compiler's scheduling more
// than the three instructions save (+0.3 % of the step, the outer layers +1 %: same file).
__device__ __forceinline__ void cb_split2_mix(float a, float b, unsigned& hi, unsigned& lo) {
#if CB_F16
    f32x2 v = {a, b};
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    LAMA_F16_SPLIT_LO(lo, hi, a, b);
#else
    cb_split2(a, b, hi, lo);
#endif
}

// Range watch of the f16 split (CB_F16 only -- bf16 keeps the fp32 exponent range).  An activation beyond 65504 rounds to inf in
// the hi term (and its lo term to -inf / NaN): the 3-term product is then garbage.  Every site that splits ACTIVATIONS keeps a
// per-lane running maximum of the |hi| bit patterns (two 16-bit fields: one v_and + one v_pk_max_u16 per element pair); a field
// >= 0x7c00 at the end of the kernel (inf, or a NaN that came in) raises the caller's flag (lama_conv2d_args.range_flag) and the
// host re-runs the forward with LAMA_PREC_BF16X3 (lama_amd/ffc.py).
typedef unsigned short cb_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void cb_split2(float a, float b, unsigned& hi, unsigned& lo, unsigned& rw) {
    cb_split2(a, b, hi, lo);
#if CB_F16
    rw = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(cb_u16x2, rw), __builtin_bit_cast(cb_u16x2, hi & 0x7fff7fffu)));
#endif
}
// the same watch on a word that already holds two fp16 activations (LAMA_DT_F16 inputs)
__device__ __forceinline__ void cb_range_watch(unsigned packed, unsigned& rw) {
#if CB_F16
    rw = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(cb_u16x2, rw), __builtin_bit_cast(cb_u16x2, packed & 0x7fff7fffu)));
#endif
}
__device__ __forceinline__ void cb_range_report(unsigned rw, unsigned* flag) {
#if CB_F16
    if (flag != nullptr && ((rw & 0xffffu) >= 0x7c00u || (rw >> 16) >= 0x7c00u)) atomicOr(flag, 1u);
#endif
}

// three ints selected by a (possibly runtime) index without dynamic register indexing (an indexed array would go to scratch)
struct CbInt3 {
    int v0, v1, v2;
    __device__ __forceinline__ void set(int i, int x) {
        if (i == 0) v0 = x;
        else if (i == 1) v1 = x;
        else v2 = x;
    }
    __device__ __forceinline__ int get(int i) const { return i == 1 ? v1 : (i == 2 ? v2 : v0); }
};

template <int V>
struct CbTag {
    static constexpr int value = V;
};

// A / B fragments of one MFMA k-step (16 channels of one tap) for this wave
template <int TM>
struct CbFrag {
    bf16x8 ah[TM], al[TM], bh, bl;
};

// One K segment: accumulate into acc.
//   LDS: three weight-stage buffers (the DMA runs two stages ahead, so the first k-step of stage s+1 can
//   be fetched into registers BEFORE the barrier that ends stage s) and two patch buffers.
//   Registers: two fragment sets -- the ds_read_b128 of k-step k+1 are in flight under the MFMAs of k-step k.
// ABL: timing-only ablations selected by the environment variable LAMA_CB_ABLATE for the profiling tools (results are
// WRONG for ABL != 0): bit 0 = no MFMA, bit 1 = no fragment ds_reads in the loop, bit 2 = no staging, bit 3 = no barriers,
// bit 4 = no patch staging, bit 5 = no weight staging.
// NACC = 4: fused ConvTranspose2d(k3, s2, p1, op1) -- the 9 taps are walked like a 3x3 convolution over a (tile + 1) patch,
// tap (ky, kx) accumulates into the accumulator set of its output-parity class (ky != 1, kx != 1), and the epilogue writes
// complete 2x2 output blocks (one launch and full cache lines instead of four strided launches).
// HI: the input tensor of this segment is fp16 (LAMA_DT_F16); NP1: one MFMA product per MAC (LAMA_PREC_F16: weights hi only, the
// activation's hi part only -- exact for an fp16 input, a rounding to fp16 for the fp32 input of the stem).
template <int T, int TG, int KS, int BM, int MAXU, int ABL = 0, int NACC = 1, int MODE = 0, bool HI = false, bool NP1 = false>
__device__ __forceinline__ void cb_segment(const CbSeg& s, int mt, int b, int gy0, int gx0, int TWlog, char* wbuf0, int wbytes,
                                           char* pbuf0, int pbytes, f32x16 (&acc)[NACC][CbGeom<BM, NACC, MODE>::TM], unsigned& rw) {
    using G = CbGeom<BM, NACC, MODE>;
    constexpr int NG = T / TG;                      // stages per channel chunk
    constexpr int NKK = TG * KS;                    // MFMA k-steps per stage
    constexpr bool XPF = (NG >= 2) && (MAXU <= NG - 1);  // next chunk's patch complete (and behind a barrier) before the
                                                     // chunk's last stage -> its first B fragment can be prefetched across
    constexpr int NOCT = 2 * KS;                    // channel octets per chunk
    constexpr int BKC = 16 * KS;                    // channels per chunk
    constexpr int NPIECE = NKK * G::MF * 2;         // 1-KiB fragment images per weight stage
    constexpr int WROUNDS = (NPIECE + 7) / 8;
    constexpr int WST = NPIECE * 1024;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / G::WAVES_N, wn = wave % G::WAVES_N;
    const int khalf = lane >> 5, l31 = lane & 31;
    const int TW = 1 << TWlog;
    const int HW = s.H * s.W;
    const int NPR = s.PH * s.PW;
    const int nunits = NPR * NOCT;
    const int plo = NOCT * s.npix * 16;             // byte offset of the lo planes inside a patch buffer

    // per-thread staging units: (patch pixel, channel octet) -> element offset in the chunk, LDS byte offset
    static_assert(MAXU <= 3, "staging units per thread");
    CbInt3 ubase = {0, 0, 0}, lds_off = {-1, -1, -1}, uq8 = {0, 0, 0}, uvalid = {0, 0, 0}, ucol = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < MAXU; ++i) {
        int u = i * CB_THREADS + tid;
        int so = 0, lo = -1, q = 0;
        int ok = 0;
        if (u < nunits) {
            q = u / NPR;
            int pp = u - q * NPR;
            int py = pp / s.PW, px = pp - py * s.PW;
            int iy = cb_src_coord(gy0 * s.stride + s.dy0 + py, s.H, s.pad_mode);
            int ix = cb_src_coord(gx0 * s.stride + s.dx0 + px, s.W, s.pad_mode);
            if (iy >= 0 && ix >= 0) { so = iy * s.W + ix; ok = 1; }
            if (MODE == 1) {   // virtual channels shift the column per element: only the ROW decides whether the unit is padding
                so = (iy < 0 ? 0 : iy) * s.W;
                ok = iy >= 0;
                ucol.set(i, gx0 + s.dx0 + px);
            }
            int lidx = py * s.PWs + (s.PWh ? (px & 1) * s.PWh + (px >> 1) : px);
            lo = (q * s.npix + lidx) * 16;
        }
        ubase.set(i, (MODE == 1 ? 0 : q * 8 * HW) + so);   // always an in-bounds element of the chunk (zero padding is applied at write time)
        lds_off.set(i, lo);
        uq8.set(i, q * 8);
        uvalid.set(i, ok);
    }
    // B-fragment base: this lane's pixel inside the patch, octet plane khalf
    int boff;
    {
        int n = wn * 32 + l31;
        int ty = n >> TWlog, tx = n & (TW - 1);
        int pixoff = ty * s.stride * s.PWs + (s.PWh ? tx : tx * s.stride);
        boff = (khalf * s.npix + pixoff) * 16;
    }
    const int aoff = (wm * G::TM * 2) * 1024 + lane * 16;  // A fragments of this wave inside a k-step image

    using XT = typename LamaAct<HI>::T;
    const XT* xb = reinterpret_cast<const XT*>(s.x) + (long long)b * s.bstride;
    const int S = s.nchunk * NG;

    // Patch staging keeps ONE unit (8 channels of one pixel) per thread in flight: unit u of chunk ch+1 is written to LDS in
    // stage u of chunk ch and the following unit is requested right after, so a kernel with a large halo (MAXU = 3: stride 2,
    // 7x7) needs no more staging registers than the bottleneck 3x3 (MAXU = 1).
    constexpr int UF = (NG >= MAXU) ? 1 : MAXU;   // units in flight: all of them when a chunk has fewer stages than units
    // 1x1 / transposed-class kernels (one stage per chunk, one unit per thread) are bound by HBM latency, not by the MFMAs:
    // they keep PF chunks in flight (chunk c lives in register slot c % PF; the chunk loop is unrolled PF times so the slot
    // index is a compile-time constant).
    constexpr int PF = (NG == 1 && MAXU == 1) ? 4 : 1;
    float preg[UF * PF][8];
    auto usel = [&](const CbInt3& arr, int u) { return MAXU == 1 ? arr.v0 : arr.get(u); };
    auto load_unit = [&](int ch, int u, int slot = 0) {
        const XT* xc = xb + (long long)ch * BKC * HW;
        const int crem = s.C - ch * BKC;
        const int ub = usel(ubase, u);
        if constexpr (MODE == 1) {   // virtual channel cc = c*7 + kx: real channel c, column shifted by kx - pad (dx0 = -pad is in ucol)
            const int q8 = usel(uq8, u), col = usel(ucol, u);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                int cc = q8 + e;
                int c = cc / 7, kx = cc - c * 7;
                int ix = cb_src_coord(col + kx - s.vpad, s.W, s.pad_mode);
                int cr = c < s.C ? c : s.C - 1;
                float v = (float)xb[(unsigned)(cr * HW + ub + (ix < 0 ? 0 : ix))];
                preg[slot][e] = (c < s.C && ix >= 0) ? v : 0.0f;
            }
        } else if (crem >= BKC) {  // (uniform) every channel of the chunk exists: unconditional loads, no per-element branches
#pragma unroll
            for (int e = 0; e < 8; ++e) preg[slot][e] = (float)xc[(unsigned)(ub + e * HW)];   // SGPR base + 32-bit lane offset
        } else {            // channel tail: clamp the address, zero the value (the packed weights are zero there too)
            const int q8 = usel(uq8, u);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                int c = q8 + e;
                int back = c < crem ? 0 : (c - (crem - 1)) * HW;
                float v = (float)xc[(unsigned)(ub + e * HW - back)];
                preg[slot][e] = c < crem ? v : 0.0f;
            }
        }
    };
    auto write_unit = [&](char* pb, int u, int slot = 0) {
        const int lo = usel(lds_off, u);
        if (lo >= 0) {
            unsigned hh[4], ll[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (NP1) {   // hi part only (v_cvt_pk: exact for values that came from fp16)
                    f32x2 v2 = {preg[slot][2 * e], preg[slot][2 * e + 1]};
                    hh[e] = __builtin_bit_cast(unsigned, __builtin_convertvector(v2, bf16x2));
                    cb_range_watch(hh[e], rw);
                    ll[e] = 0u;
                } else cb_split2(preg[slot][2 * e], preg[slot][2 * e + 1], hh[e], ll[e], rw);
            }
            u32x4 h = {hh[0], hh[1], hh[2], hh[3]}, l = {ll[0], ll[1], ll[2], ll[3]};
            if (!usel(uvalid, u)) { h = u32x4{0, 0, 0, 0}; l = h; }   // zero padding
            *reinterpret_cast<u32x4*>(pb + lo) = h;
            if constexpr (!NP1) *reinterpret_cast<u32x4*>(pb + plo + lo) = l;
        }
    };
    // stage g of chunk ch: write the unit(s) of chunk ch+1 that belong to this stage, keep the next one in flight
    // With a single unit and >= 3 stages per chunk the two waves of a SIMD stage their unit in DIFFERENT stages (waves 0-3 in
    // stage 0, waves 4-7 in stage 1), so the split / address VALU work of one runs under the MFMAs of the other.
    const int gskew = (MAXU == 1 && NG >= 3) ? (wave >> 2) : 0;
    auto stage_patch = [&](int ch, int g, char* pbn, int slot1) {   // slot1 = register slot of chunk ch+1 (PF > 1 only)
        if (ch + 1 >= s.nchunk) return;
        if constexpr (PF > 1) {
            write_unit(pbn, 0, slot1);
            if (ch + 1 + PF < s.nchunk) load_unit(ch + 1 + PF, 0, slot1);
        } else if constexpr (NG >= MAXU) {
            if (MAXU == 1) {
                if (g == gskew) {
                    write_unit(pbn, 0);
                    if (ch + 2 < s.nchunk) load_unit(ch + 2, 0);
                }
            } else if (g < MAXU) {
                write_unit(pbn, g);
                if (g + 1 < MAXU) load_unit(ch + 1, g + 1);
                else if (ch + 2 < s.nchunk) load_unit(ch + 2, 0);
            }
        } else {   // fewer stages than units: every unit has its own register slot and all are written / reloaded in stage 0
            if (g == 0) {
#pragma unroll
                for (int u = 0; u < MAXU; ++u) write_unit(pbn, u, u);
                if (ch + 2 < s.nchunk) {
#pragma unroll
                    for (int u = 0; u < MAXU; ++u) load_unit(ch + 2, u, u);
                }
            }
        }
    };
    // weight stage st: global (L2-resident packed image) -> registers; written to LDS a stage later.  Plain loads + ds_write
    // instead of global_load_lds DMA: with a DMA in flight hipcc degrades every s_waitcnt to lgkmcnt(0)/vmcnt(0), which
    // serialises the ds_read prefetch below; 16 B per lane per round keeps the loads fully coalesced.
    u32x4 wreg[WROUNDS];
    constexpr int WITEMS = NPIECE * 64;   // 16-byte items per stage image
    // The packed layout does not depend on the M-tile height: this workgroup copies fragments [mt*MF, mt*MF + MF) of each
    // k-step (one contiguous MF*2 KiB run per k-step; fragments past the last one are clamped, their rows are never stored).
    auto load_w = [&](int st) {
        const u32x4* g = reinterpret_cast<const u32x4*>(s.w) + (long long)st * NKK * s.mft * 128;
#pragma unroll
        for (int r = 0; r < WROUNDS; ++r) {
            int idx = r * CB_THREADS + tid;
            if ((r + 1) * CB_THREADS > WITEMS) idx = idx < WITEMS ? idx : WITEMS - 1;   // partial last round: clamp, never branch
            const int kk = idx / (G::MF * 128), rem = idx - kk * (G::MF * 128);
            int F = mt * G::MF + (rem >> 7);
            F = F < s.mft ? F : s.mft - 1;
            wreg[r] = g[(kk * s.mft + F) * 128 + (rem & 127)];
        }
    };
    auto write_w = [&](char* wb) {
        u32x4* d = reinterpret_cast<u32x4*>(wb);
#pragma unroll
        for (int r = 0; r < WROUNDS; ++r) {
            int idx = r * CB_THREADS + tid;
            if ((r + 1) * CB_THREADS <= WITEMS || idx < WITEMS) d[idx] = wreg[r];
        }
    };
    using Frag = CbFrag<G::TM>;
    auto read_a = [&](Frag& f, const char* wb, int kk) {
#pragma unroll
        for (int i = 0; i < G::TM; ++i) {
            const char* ap = wb + (kk * G::MF * 2 + i * 2) * 1024 + aoff;
            f.ah[i] = *reinterpret_cast<const bf16x8*>(ap);
            if constexpr (!NP1 || CB_HF_W2) f.al[i] = *reinterpret_cast<const bf16x8*>(ap + 1024);
        }
    };
    // LDS offset of tap (g*TG + tgi) = tgoff[tgi] + g * grow: one kernel row (or the whole transposed-class tap list) per stage,
    // so the stage loop needs no scalar loads (an SMEM load in flight would force lgkmcnt(0) on every ds_read wait)
    // (the fully unrolled kernels keep all <= 9 tap offsets in scalar registers and index them at compile time)
    constexpr bool FLAT = (NG <= 3) && (MAXU == 1 || NACC == 4);
    constexpr int NTOFF = FLAT ? T : TG;
    int tgoff[NTOFF];
#pragma unroll
    for (int i = 0; i < NTOFF; ++i) tgoff[i] = s.tapoff[i] * 16;
    const int grow = (!FLAT && NG > 1) ? (s.tapoff[TG] - s.tapoff[0]) * 16 : 0;
    auto read_b = [&](Frag& f, const char* pb, int g, int tgi, int ks) {
        const char* bp = pb + (ks * 2 * s.npix) * 16 + (FLAT ? tgoff[g * TG + tgi] : tgoff[tgi] + g * grow) + boff;
        f.bh = *reinterpret_cast<const bf16x8*>(bp);
        if constexpr (!NP1) f.bl = *reinterpret_cast<const bf16x8*>(bp + plo);
    };

    // prologue: weight stages 0 and 1 and the chunk-0 patch in LDS; stage 2 / chunk 1 in flight to registers
    load_w(0);
    load_unit(0, 0);
    write_w(wbuf0);
    if (S > 1) load_w(1);               // in flight while the first patch unit is converted
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
        write_unit(pbuf0, u);
        if (u + 1 < MAXU) load_unit(0, u + 1);
    }
    if (s.nchunk > 1) {
        if constexpr (PF > 1) {
#pragma unroll
            for (int c = 1; c <= PF; ++c)
                if (c < s.nchunk) load_unit(c, 0, c % PF);
        } else if constexpr (UF == 1) load_unit(1, 0);
        else {
#pragma unroll
            for (int u = 0; u < MAXU; ++u) load_unit(1, u, u);
        }
    }
    if (S > 1) write_w(wbuf0 + wbytes);
    if (S > 2) load_w(2);
    __syncthreads();
    Frag fr[2];   // fragment sets, indexed with compile-time parity only (two k-steps in flight, no register copies)
    read_a(fr[0], wbuf0, 0);
    read_b(fr[0], pbuf0, 0, 0, 0);

    int st = 0, wi = 0;  // wi = st % 3
    // one channel chunk = NG stages = NG*NKK k-steps; PAR = parity of the fragment set holding its first k-step
    // FLAT: stages of a chunk fully unrolled and the fragment-set parity carried at compile time (the bottleneck kernels);
    // otherwise (7x7 kernels, big staging footprints) a rolled stage loop that realigns the parity with one register copy
    // per stage, which keeps code size and register pressure down.
    static_assert(NACC == 1 || (FLAT && T == 9 && TG == 3), "fused transposed classes need the unrolled 3x3 structure");
    auto stage = [&](int ch, int g, auto par_tag, auto slot_tag, auto g_tag) {
        constexpr int PAR = decltype(par_tag)::value;
        constexpr int SLOT1 = decltype(slot_tag)::value;
        constexpr int GC = decltype(g_tag)::value;   // compile-time copy of g for the unrolled kernels (-1 otherwise)
        const char* pb = pbuf0 + (ch & 1) * pbytes;
        char* pbn = pbuf0 + ((ch + 1) & 1) * pbytes;
        const char* wb = wbuf0 + wi * wbytes;
        const int wi1 = wi == 2 ? 0 : wi + 1, wi2 = wi1 == 2 ? 0 : wi1 + 1;
        const char* wbn = wbuf0 + wi1 * wbytes;
        if constexpr (!(ABL & 4) && !(ABL & 16)) stage_patch(ch, g, pbn, SLOT1);
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            Frag& cur = fr[(PAR + kk) & 1];
            Frag& nxt = fr[(PAR + kk + 1) & 1];
            if constexpr (ABL & 2) {
                if (kk + 1 == NKK && !(ABL & 4) && !(ABL & 32) && st + 2 < S) write_w(wbuf0 + wi2 * wbytes);
                nxt = cur;
            } else if (kk + 1 < NKK) {
                const int tgi = (kk + 1) / KS, ks = (kk + 1) % KS;
                read_a(nxt, wb, kk + 1);
                read_b(nxt, pb, g, tgi, ks);
            } else {
                if (st + 1 < S) {
                    // first k-step of the next stage: its weights were written before the previous barrier
                    read_a(nxt, wbn, 0);
                    if (g + 1 < NG) read_b(nxt, pb, g + 1, 0, 0);
                    else if (XPF) read_b(nxt, pbn, 0, 0, 0);   // next chunk's patch is complete and visible
                }
                // stage st+2 (in registers since the end of stage st-1) -> the buffer stage st-1 was read from
                if (!(ABL & 4) && !(ABL & 32) && st + 2 < S) write_w(wbuf0 + wi2 * wbytes);
            }
            // pin the order: the ds_reads of the NEXT k-step are issued before this k-step's MFMAs and are only
            // waited for after them (hipcc otherwise sinks the reads next to their use and exposes the LDS latency)
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (ABL & 1) {
#pragma unroll
                for (int i = 0; i < G::TM; ++i) { LAMA_KEEP_LIVE(cur.ah[i]); LAMA_KEEP_LIVE(cur.al[i]); LAMA_KEEP_LIVE(cur.bh); LAMA_KEEP_LIVE(cur.bl); }
            } else {
                const int CLS = NACC == 4 ? ((GC != 1) ? 2 : 0) + (((kk / KS) != 1) ? 1 : 0) : 0;
#pragma unroll
                for (int i = 0; i < G::TM; ++i) {
                    acc[CLS][i] = CB_MFMA(cur.ah[i], cur.bh, acc[CLS][i], 0, 0, 0);
                    if constexpr (!NP1) {
                        acc[CLS][i] = CB_MFMA(cur.ah[i], cur.bl, acc[CLS][i], 0, 0, 0);
                        acc[CLS][i] = CB_MFMA(cur.al[i], cur.bh, acc[CLS][i], 0, 0, 0);
                    } else if constexpr (CB_HF_W2) {
                        acc[CLS][i] = CB_MFMA(cur.al[i], cur.bh, acc[CLS][i], 0, 0, 0);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!(ABL & 4) && !(ABL & 32) && st + 3 < S) load_w(st + 3);   // registers are free again: fetch three stages ahead
        if constexpr (!(ABL & 8)) __syncthreads();
        if (!XPF && g == NG - 1 && st + 1 < S) read_b(fr[(PAR + NKK) & 1], pbn, 0, 0, 0);   // chunk boundary: new patch visible only now
        wi = wi1;
        ++st;
    };
    if constexpr (FLAT) {
        // one chunk = NG*NKK k-steps; an odd count flips the parity for the next chunk -> unroll two chunks
        auto chunk = [&](int ch, auto par_tag) {
            constexpr int PAR = decltype(par_tag)::value;
            stage(ch, 0, CbTag<PAR & 1>{}, CbTag<0>{}, CbTag<0>{});
            if constexpr (NG > 1) stage(ch, 1, CbTag<(PAR + NKK) & 1>{}, CbTag<0>{}, CbTag<1>{});
            if constexpr (NG > 2) stage(ch, 2, CbTag<(PAR + 2 * NKK) & 1>{}, CbTag<0>{}, CbTag<2>{});
        };
        if constexpr (PF > 1) {
            static_assert(PF == 4 && NKK % 2 == 0, "slot unroll");
            for (int ch = 0; ch < s.nchunk; ch += PF) {   // chunk ch+j+1 lives in slot (j+1) % PF
                stage(ch, 0, CbTag<0>{}, CbTag<1>{}, CbTag<0>{});
                if (ch + 1 < s.nchunk) stage(ch + 1, 0, CbTag<0>{}, CbTag<2>{}, CbTag<0>{});
                if (ch + 2 < s.nchunk) stage(ch + 2, 0, CbTag<0>{}, CbTag<3>{}, CbTag<0>{});
                if (ch + 3 < s.nchunk) stage(ch + 3, 0, CbTag<0>{}, CbTag<0>{}, CbTag<0>{});
            }
        } else if constexpr ((NG * NKK) % 2 == 0) {
            for (int ch = 0; ch < s.nchunk; ++ch) chunk(ch, CbTag<0>{});
        } else {
            for (int ch = 0; ch < s.nchunk; ch += 2) {
                chunk(ch, CbTag<0>{});
                if (ch + 1 < s.nchunk) chunk(ch + 1, CbTag<1>{});
            }
        }
    } else {
        for (int ch = 0; ch < s.nchunk; ++ch) {
#pragma unroll 1
            for (int g = 0; g < NG; ++g) {
                stage(ch, g, CbTag<0>{}, CbTag<0>{}, CbTag<-1>{});
                if constexpr (NKK % 2 == 1) fr[0] = fr[1];   // realign: the next stage's first k-step was fetched into set 1
            }
        }
    }
}

// IOM = CB_IO_* (element types of x / x2 and of y / resid); any fp16 tensor means LAMA_PREC_F16 = one product per MAC
template <int T1, int TG1, int KS1, int T2, int TG2, int KS2, int BM, int MAXU, int ABL = 0, int NACC = 1, int MODE = 0, int IOM = 0>
__global__ __launch_bounds__(CB_THREADS) void CB_NAME(conv_kernel)(CbParams p) {
    using G = CbGeom<BM, NACC, MODE>;
    constexpr bool HI = (IOM & 1) != 0, HO = (IOM & 2) != 0, HI2 = (IOM & CB_IO_X2H) != 0, NP1 = IOM != CB_IO_F32;
    using YT = typename LamaAct<HO>::T;
    const YT* const yresid = reinterpret_cast<const YT*>(p.resid);
    YT* const yout = reinterpret_cast<YT*>(p.y);
    char* wbuf0 = lama_smem;
    char* pbuf0 = lama_smem + p.nwbuf * p.wbytes;

    const int L = lama_xcd_remap(blockIdx.x, gridDim.x);
    const int mt = L % p.MT;
    int tile = L / p.MT;
    const int tix = tile % p.tiles_x;
    tile /= p.tiles_x;
    const int tiy = tile % p.tiles_y;
    const int b = tile / p.tiles_y;
    const int TW = 1 << p.TWlog, TH = G::BN >> p.TWlog;
    // MODE 2: a 32-column tile of z produces 26 output columns, tiles overlap by the 6-column halo
    const int gy0 = tiy * TH, gx0 = MODE == 2 ? tix * 26 - p.s1.vpad : tix * TW;

    f32x16 acc[NACC][G::TM];
#pragma unroll
    for (int c = 0; c < NACC; ++c)
#pragma unroll
        for (int i = 0; i < G::TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][i][r] = 0.0f;

    unsigned rw = 0;   // range watch of the f16 split
    cb_segment<T1, TG1, KS1, BM, MAXU, ABL, NACC, MODE, HI, NP1>(p.s1, mt, b, gy0, gx0, p.TWlog, wbuf0, p.wbytes, pbuf0, p.pbytes, acc, rw);
    if constexpr (TG2 > 0) cb_segment<T2, TG2, KS2, BM, MAXU, 0, NACC, 0, HI2, NP1>(p.s2, mt, b, gy0, gx0, p.TWlog, wbuf0, p.wbytes, pbuf0, p.pbytes, acc, rw);
    cb_range_report(rw, p.range_flag);

    // epilogue: D[row = (r&3) + 8*(r>>2) + 4*(lane>>5)][col = lane&31]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / G::WAVES_N, wn = wave % G::WAVES_N;
    const long long plane = (long long)p.Ho * p.Wo;
    const int n = wn * 32 + (lane & 31);
    const int gy = gy0 + (n >> p.TWlog), gx = gx0 + (n & (TW - 1));
    if constexpr (MODE == 2) {
        // z fragment (rows m' = o*7 + kx, 32 columns x' = gx0 + j of tile row wn) -> this wave's LDS slab -> horizontal 7-tap sum
        static_assert(G::TM == 1 && NACC == 1, "head mode geometry");
        float* zb = reinterpret_cast<float*>(lama_smem) + wave * 1024;   // the weight buffers are free after the last barrier
#pragma unroll
        for (int r = 0; r < 16; ++r) zb[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 32 + (lane & 31)] = acc[0][0][r];
        __syncthreads();
        const int j = lane & 31, oc = p.M / 7;
        const int oy = gy0 + wn, ox = gx0 + p.s1.vpad + j;
        if (lane < 26 && oy < p.GH && ox < p.GW) {
            for (int o = 0; o < oc; ++o) {
                float v = 0.0f;
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) v += zb[(o * 7 + kx) * 32 + j + kx];
                if (p.bias) v += p.bias[o];
                if (p.act == LAMA_ACT_RELU) v = fmaxf(v, 0.0f);
                else if (p.act == LAMA_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
                else if (p.act == LAMA_ACT_TANH) v = tanhf(v);
                long long off = o * plane + (long long)oy * p.Wo + ox;
                if (p.resid) v += (float)yresid[(long long)b * p.resid_bstride + off];
                yout[(long long)b * p.y_bstride + off] = (YT)v;
            }
        }
        return;
    }
    const bool pv = gy < p.GH && gx < p.GW;
    const int gyc = gy < p.GH ? gy : p.GH - 1, gxc = gx < p.GW ? gx : p.GW - 1;
    // On gfx9 a store counts in vmcnt until L2 acknowledges it, so a load issued right behind a store waits for that round trip
    // (the original per-element "load bias, load residual, store" sequence paid it 16 times per fragment).  Fragments
    // (accumulator set c, 32-row block i) are walked in order; the bias / residual values of fragment f+1 are requested BEFORE
    // the 16 stores of fragment f, with clamped (always valid) addresses instead of branches.
    // Addresses: uniform 64-bit row base (scalar registers) + ONE 32-bit lane offset per fragment, so the 16 stores / loads of a
    // fragment need no per-element address registers.
    int khalf4 = 4 * (lane >> 5);
    LAMA_OPAQUE(khalf4);   // keeps the epilogue loads behind the main loop
    const int wmu = LAMA_WAVE_UNIFORM(wm);
    constexpr int NF = NACC * G::TM;
    constexpr bool DB = NF * 16 <= 96;   // the fused transposed kernels (128 accumulator registers) cannot afford the second value set
    float bv[DB ? 2 : 1][16], rv[DB ? 2 : 1][16];
    auto row0_of = [&](int i) { return mt * BM + (wmu * G::TM + i) * 32; };          // uniform
    auto pix_off = [&](int c) {
        // NACC == 4: accumulator set c holds output pixel (2*gy + (c >> 1), 2*gx + (c & 1))
        return (gyc * p.ostep + (NACC == 4 ? (c >> 1) : p.oy0)) * p.Wo + (gxc * p.ostep + (NACC == 4 ? (c & 1) : p.ox0));
    };
    const int kplane = khalf4 * (int)plane;
    auto load_frag = [&](int f, int slot) {
        const int c = f / G::TM, i = f % G::TM;
        const int po = pix_off(c);
        const int row0 = row0_of(i);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mu = row0 + (r & 3) + 8 * (r >> 2);                             // uniform part of the row
            const int muc = mu < p.M ? mu : p.M - 1;                                  // rows past M: a valid address, never stored
            const int m = mu + khalf4;
            bv[slot][r] = p.bias ? p.bias[m < p.M ? m : p.M - 1] : 0.0f;
            rv[slot][r] = p.resid ? (float)(yresid + (long long)b * p.resid_bstride + (long long)muc * plane)[(unsigned)(po + (m < p.M ? kplane : 0))] : 0.0f;
        }
    };
    if (DB) load_frag(0, 0);
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int c = f / G::TM, i = f % G::TM;
        if (!DB) load_frag(f, 0);
        else if (f + 1 < NF) load_frag(f + 1, (f + 1) & 1);
        const unsigned lo = (unsigned)(pix_off(c) + kplane);
        const int row0 = row0_of(i);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mu = row0 + (r & 3) + 8 * (r >> 2);
            float v = acc[c][i][r] + bv[DB ? (f & 1) : 0][r];
            if (p.act == LAMA_ACT_RELU) v = fmaxf(v, 0.0f);
            else if (p.act == LAMA_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
            else if (p.act == LAMA_ACT_TANH) v = tanhf(v);
            v += rv[DB ? (f & 1) : 0][r];
            if (pv && mu + khalf4 < p.M) (yout + (long long)b * p.y_bstride + (long long)mu * plane)[lo] = (YT)v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// weight packing: reference layout fp32 -> [stage][k-step kk = tgi*KS + ks][32-row fragment F][hi|lo][lane][8 x bf16]
//   (hi, lo) bf16 A fragments; independent of the M-tile height the launch later picks:
//   lane l of fragment F holds output channel m = F*32 + (l&31),
//   input channels c = ch*16*KS + ks*16 + 8*(l>>5) + e  (e = 0..7), tap t = g*TG + tgi
// ------------------------------------------------------------------------------------------------
struct CbPackParams {
    const float* w;
    const float* scale;
    char* dst;
    int M, C, MFT, TG, KS, NG, nchunk;   // M / C: real output / input channels of the reference weight tensor
    int kh, kw, transposed, mode;
    int tap_ky[CB_MAX_TAPS], tap_kx[CB_MAX_TAPS];
};

__global__ void CB_NAME(conv_pack_kernel)(CbPackParams p) {
    const int NKK = p.TG * p.KS;
    const long long total = (long long)p.nchunk * p.NG * NKK * p.MFT * 64;  // (stage, kk, F, lane) items; each writes hi and lo 16 B
    for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (long long)gridDim.x * blockDim.x) {
        int lane = (int)(it & 63);
        long long r = it >> 6;
        int F = (int)(r % p.MFT);
        r /= p.MFT;
        int kk = (int)(r % NKK);
        r /= NKK;
        int g = (int)(r % p.NG);
        int ch = (int)(r / p.NG);
        int tgi = kk / p.KS, ks = kk - tgi * p.KS;
        int t = g * p.TG + tgi;
        int m = F * 32 + (lane & 31);
        int c0 = ch * 16 * p.KS + ks * 16 + 8 * (lane >> 5);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int c = c0 + e;
            float x = 0.0f;
            int mm = m, cc = c, kxo = -1;
            if (p.mode == 1) { cc = c / 7; kxo = c - cc * 7; }         // virtual input channel c = cc*7 + kx
            else if (p.mode == 2) { mm = m / 7; kxo = m - mm * 7; }    // virtual output row m = mm*7 + kx
            if (mm < p.M && cc < p.C) {
                int ky = p.tap_ky[t], kx = kxo >= 0 ? kxo : p.tap_kx[t];
                const int m = mm, c = cc;
                long long src = p.transposed ? (((long long)c * p.M + m) * p.kh + ky) * p.kw + kx
                                             : (((long long)m * p.C + c) * p.kh + ky) * p.kw + kx;
                x = p.w[src];
                if (p.scale) x *= p.scale[m];
            }
            v[e] = x;
        }
        unsigned hh[4], ll[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) cb_split2(v[2 * e], v[2 * e + 1], hh[e], ll[e]);
        long long stage = (long long)ch * p.NG + g;
        char* base = p.dst + (((stage * NKK + kk) * p.MFT + F) * 2) * 1024 + lane * 16;
        *reinterpret_cast<u32x4*>(base) = u32x4{hh[0], hh[1], hh[2], hh[3]};
        *reinterpret_cast<u32x4*>(base + 1024) = u32x4{ll[0], ll[1], ll[2], ll[3]};
    }
}

#include "conv_wreg_dev.inc"
#include "conv_ws_dev.inc"
#include "gemm_wk_dev.inc"
#include "conv_stem_dev.inc"
#include "conv_head_dev.inc"
#if !CB_HALF
#include "wino_dev.inc"
#include "convt_dev.inc"
#include "mdconv_dev.inc"
#endif

// ------------------------------------------------------------------------------------------------
// host side: plan, pack, launch
// ------------------------------------------------------------------------------------------------
namespace {

struct CbPlan {
    int mode;  // 0 plain, 1 stem-folded 7x7 (virtual input channels), 2 head-folded 7x7 (virtual output rows)
    int rows;  // GEMM rows (= cout, or cout*7 in mode 2)
    int mft;   // 32-row fragments = ceil(rows / 32)
    int nseg;  // packed sub-convolutions: 1, or 5 for ConvTranspose2d (0 = the fused 3x3 tap list, 1..4 = its output-parity classes)
    int T[5], TG[5], KS[5];
    int ky[5][CB_MAX_TAPS], kx[5][CB_MAX_TAPS];  // weight tap
    int dy[5][CB_MAX_TAPS], dx[5][CB_MAX_TAPS];  // input offset of the tap
    int oy0[5], ox0[5];
    int nchunk[5];
    long long cls_bytes[5], woff[5];
    long long total_bytes;
};

// M-tile height, chosen per launch (the packed weights do not depend on it).  One workgroup per CU is resident, so the cost
// of a launch is ~ rounds * (BM + fixed per-workgroup overhead): 192-row tiles win when they save a round or the 25 % padding
// of a second 128-row tile (M = 192: 1 x 192 instead of 2 x 128; M = 384 at 256 pixel tiles: 2 rounds instead of 3).
int cb_pick_bm(int M, int T, int stride, int batch, int GH, int GW) {
    if (M <= 32) return 32;
    if (M <= 64 || T == 49) return 64;       // 7x7 kernels keep their 7-tap weight stages small
    const long long tiles = (long long)batch * lama_ceil_div64((long long)GH * GW, 128);
    long long best = 0;
    int bm = 128;
    for (int cand : {128, 192}) {
        long long rounds = lama_ceil_div64(tiles * lama_ceil_div(M, cand), 256);
        long long cost = rounds * (cand + 24);
        if (best == 0 || cost < best) { best = cost; bm = cand; }
    }
    return bm;
}

bool cb_stage_shape(int T, int mode, int* TG, int* KS) {
    if (mode) { *TG = 7; *KS = mode == 1 ? 2 : 1; return T == 7; }
    switch (T) {
        case 1: *TG = 1; *KS = 2; return true;
        case 2: *TG = 2; *KS = 1; return true;
        case 4: *TG = 4; *KS = 1; return true;
        case 9: *TG = 3; *KS = 1; return true;
        case 49: *TG = 7; *KS = 1; return true;
    }
    return false;
}

bool cb_make_plan(int cout, int cin, int kh, int kw, int stride, int pad, int transposed, CbPlan* pl) {
    pl->mode = 0;
    if (!transposed && kh == 7 && kw == 7 && stride == 1) pl->mode = (cin * 7 <= 32) ? 1 : ((cout * 7 <= 32) ? 2 : 0);
    pl->rows = pl->mode == 2 ? cout * 7 : cout;
    pl->mft = lama_ceil_div(pl->rows, 32);
    if (transposed) {
        // ConvTranspose2d(k3, s2, p1, op1): y[2g + py, 2g' + px] += W[ky, kx] x[g + dy, g' + dx] with
        //   ky = 1 -> py = 0, dy = 0;  ky = 0 -> py = 1, dy = 1;  ky = 2 -> py = 1, dy = 0   (same for kx / px / dx)
        // walked as ONE 3x3 tap list; the kernel routes tap (ky, kx) to the accumulators of class (ky != 1, kx != 1).
        if (kh != 3 || kw != 3 || stride != 2 || pad != 1) return false;
        pl->nseg = 1;
        int t = 0;
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) {
                pl->ky[0][t] = a; pl->kx[0][t] = c;
                pl->dy[0][t] = (a == 0) ? 1 : 0; pl->dx[0][t] = (c == 0) ? 1 : 0;
                ++t;
            }
        pl->T[0] = 9;
        pl->oy0[0] = pl->ox0[0] = 0;
        // ... and packed a second time class by class for convt2_kernel (ct_route / ct_launch, conv_wreg_host.inc): output
        // parity (py, px) is a stride-1 convolution of the input with the 1, 2 or 4 taps that reach it, stored with step 2 from
        // (py, px); heaviest class first
        pl->nseg = 5;
        for (int cls = 1; cls < 5; ++cls) {
            const int py = cls <= 2 ? 1 : 0, px = (cls == 1 || cls == 3) ? 1 : 0;     // (1,1) (1,0) (0,1) (0,0)
            int n = 0;
            for (int a = 0; a < 3; ++a)
                for (int c = 0; c < 3; ++c) {
                    if ((a != 1) != (py == 1) || (c != 1) != (px == 1)) continue;
                    pl->ky[cls][n] = a; pl->kx[cls][n] = c;
                    pl->dy[cls][n] = (a == 0) ? 1 : 0; pl->dx[cls][n] = (c == 0) ? 1 : 0;
                    ++n;
                }
            pl->T[cls] = n;
            pl->oy0[cls] = py; pl->ox0[cls] = px;
        }
    } else {
        if (!((kh == 1 && kw == 1) || (kh == 3 && kw == 3) || (kh == 7 && kw == 7))) return false;
        if (stride != 1 && stride != 2) return false;
        pl->nseg = 1;
        int t = 0;
        for (int a = 0; a < kh; ++a)
            for (int c = 0; c < (pl->mode ? 1 : kw); ++c) {   // folded 7x7: the tap list holds the 7 vertical taps only
                pl->ky[0][t] = a; pl->kx[0][t] = c;
                pl->dy[0][t] = a - pad; pl->dx[0][t] = pl->mode ? 0 : c - pad;
                ++t;
            }
        pl->T[0] = t;
        pl->oy0[0] = pl->ox0[0] = 0;
    }
    long long off = 0;
    for (int cls = 0; cls < pl->nseg; ++cls) {
        if (!cb_stage_shape(pl->T[cls], pl->mode, &pl->TG[cls], &pl->KS[cls])) return false;
        pl->nchunk[cls] = lama_ceil_div(pl->mode == 1 ? cin * 7 : cin, 16 * pl->KS[cls]);
        pl->cls_bytes[cls] = (long long)pl->nchunk[cls] * pl->T[cls] * pl->KS[cls] * pl->mft * 2048;
        pl->woff[cls] = off;
        off += pl->cls_bytes[cls];
    }
    pl->total_bytes = off;
    return true;
}

// fill one segment for a tile of TH x TW output pixels; returns the staging units it needs
int cb_fill_seg(CbSeg* s, const lama_tensor& x, const char* w, const CbPlan& pl, int cls, int stride, int pad_mode, int TH, int TW,
                bool flat) {
    const int T = pl.T[cls];
    s->x = (const float*)x.ptr;
    s->bstride = x.batch_stride;
    s->C = x.C;
    s->H = flat ? 1 : x.H;
    s->W = flat ? x.H * x.W : x.W;
    s->w = w;
    s->mft = pl.mft;
    s->vpad = 0;
    s->nchunk = pl.nchunk[cls];
    s->NG = T / pl.TG[cls];
    s->stride = stride;
    s->pad_mode = pad_mode;
    int dymin = 1 << 30, dymax = -(1 << 30), dxmin = 1 << 30, dxmax = -(1 << 30);
    for (int t = 0; t < T; ++t) {
        dymin = pl.dy[cls][t] < dymin ? pl.dy[cls][t] : dymin;
        dymax = pl.dy[cls][t] > dymax ? pl.dy[cls][t] : dymax;
        dxmin = pl.dx[cls][t] < dxmin ? pl.dx[cls][t] : dxmin;
        dxmax = pl.dx[cls][t] > dxmax ? pl.dx[cls][t] : dxmax;
    }
    s->dy0 = dymin;
    s->dx0 = dxmin;
    s->PH = (TH - 1) * stride + (dymax - dymin) + 1;
    s->PW = (TW - 1) * stride + (dxmax - dxmin) + 1;
    if (stride == 2) {
        s->PWh = (s->PW + 1) / 2;
        s->PWs = 2 * s->PWh;
    } else {
        s->PWh = 0;
        s->PWs = s->PW;
    }
    s->npix = s->PH * s->PWs;
    for (int t = 0; t < T; ++t) {
        int ry = pl.dy[cls][t] - dymin, rx = pl.dx[cls][t] - dxmin;
        s->tapoff[t] = ry * s->PWs + (s->PWh ? (rx & 1) * s->PWh + (rx >> 1) : rx);
    }
    return s->PH * s->PW * 2 * pl.KS[cls];
}

// The LDS-staged launcher: the instantiation tables of conv_kernel, fed by cb_route() (conv_wreg_host.inc: lds_has_kernel states their conditions).
// CB_ERR_ROUTE (hipErrorUnknown): a launcher met a route cb_route() does not produce -- a bug, never a reason to fall through to another kernel.
#define CB_ERR_ROUTE 999

template <int T1, int TG1, int KS1, int T2, int TG2, int KS2, int BM, int IOM>
int cb_launch_u_io(hipStream_t st, const CbParams& p, int maxu, int grid, size_t shmem) {
#ifdef CB_DEV_NO_GENERIC   // kernel-development builds (tools/kres.py): skip the LDS-staged instantiations, 10x shorter compile
    return CB_ERR_ROUTE;
#endif
    if (maxu <= 1) hipLaunchKernelGGL((CB_NAME(conv_kernel)<T1, TG1, KS1, T2, TG2, KS2, BM, 1, 0, 1, 0, IOM>), dim3(grid), dim3(CB_THREADS), shmem, st, p);
    else if (maxu <= 3) hipLaunchKernelGGL((CB_NAME(conv_kernel)<T1, TG1, KS1, T2, TG2, KS2, BM, 3, 0, 1, 0, IOM>), dim3(grid), dim3(CB_THREADS), shmem, st, p);
    else return CB_ERR_ROUTE;
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// io: CB_IO_* bits of the launch (x, y / resid, x2).  LAMA_PREC_F16 launches exist for the element-type mixes the fp16 path produces:
// all fp16, fp32 in -> fp16 out, fp16 in -> fp32 out (the residual stream of the resnet blocks is fp32), x2 (= t) always fp16.
template <int T1, int TG1, int KS1, int T2, int TG2, int KS2, int BM>
int cb_launch_u(hipStream_t st, const CbParams& p, int maxu, int grid, size_t shmem, int io) {
#if !CB_HALF
    if (io == CB_IO_F32) return cb_launch_u_io<T1, TG1, KS1, T2, TG2, KS2, BM, CB_IO_F32>(st, p, maxu, grid, shmem);
#else
    constexpr int X2 = T2 > 0 ? CB_IO_X2H : 0;
    switch (io & 3) {
        case CB_IO_F16: return cb_launch_u_io<T1, TG1, KS1, T2, TG2, KS2, BM, CB_IO_F16 | X2>(st, p, maxu, grid, shmem);
        case CB_IO_F32_F16: return cb_launch_u_io<T1, TG1, KS1, T2, TG2, KS2, BM, CB_IO_F32_F16 | X2>(st, p, maxu, grid, shmem);
        case CB_IO_F16_F32: return cb_launch_u_io<T1, TG1, KS1, T2, TG2, KS2, BM, CB_IO_F16_F32 | X2>(st, p, maxu, grid, shmem);
    }
#endif
    return CB_ERR_ROUTE;
}

template <int T1, int TG1, int KS1, int T2, int TG2, int KS2>
int cb_launch_bm(hipStream_t st, const CbParams& p, int BM, int maxu, int grid, size_t shmem, int io) {
    switch (BM) {
        case 192: return cb_launch_u<T1, TG1, KS1, T2, TG2, KS2, 192>(st, p, maxu, grid, shmem, io);
        case 128: return cb_launch_u<T1, TG1, KS1, T2, TG2, KS2, 128>(st, p, maxu, grid, shmem, io);
        case 64: return cb_launch_u<T1, TG1, KS1, T2, TG2, KS2, 64>(st, p, maxu, grid, shmem, io);
        case 32: return cb_launch_u<T1, TG1, KS1, T2, TG2, KS2, 32>(st, p, maxu, grid, shmem, io);
    }
    return CB_ERR_ROUTE;
}

template <int BM, int IOM>
int cb_launch_trf_io(hipStream_t st, const CbParams& p, int maxu, int grid, size_t shmem) {
#ifdef CB_DEV_NO_GENERIC   // kernel-development builds (tools/kres.py): skip the LDS-staged instantiations, 10x shorter compile
    return CB_ERR_ROUTE;
#endif
    if (maxu <= 1) hipLaunchKernelGGL((CB_NAME(conv_kernel)<9, 3, 1, 0, 0, 0, BM, 1, 0, 4, 0, IOM>), dim3(grid), dim3(CB_THREADS), shmem, st, p);
    else if (maxu <= 3) hipLaunchKernelGGL((CB_NAME(conv_kernel)<9, 3, 1, 0, 0, 0, BM, 3, 0, 4, 0, IOM>), dim3(grid), dim3(CB_THREADS), shmem, st, p);
    else return CB_ERR_ROUTE;
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

template <int BM>
int cb_launch_trf_u(hipStream_t st, const CbParams& p, int maxu, int grid, size_t shmem, int io) {
#if !CB_HALF
    if (io == CB_IO_F32) return cb_launch_trf_io<BM, CB_IO_F32>(st, p, maxu, grid, shmem);
#else
    if (io == CB_IO_F16) return cb_launch_trf_io<BM, CB_IO_F16>(st, p, maxu, grid, shmem);
    if (io == CB_IO_F32_F16) return cb_launch_trf_io<BM, CB_IO_F32_F16>(st, p, maxu, grid, shmem);   // the first upsample reads the fp32 residual stream
    if (io == CB_IO_F16_F32) return cb_launch_trf_io<BM, CB_IO_F16_F32>(st, p, maxu, grid, shmem);
#endif
    return CB_ERR_ROUTE;
}

int cb_launch_folded7(hipStream_t st, const CbParams& p, int mode, int BM, int maxu, int grid, size_t shmem, int io) {
#ifdef CB_DEV_NO_GENERIC   // kernel-development builds (tools/kres.py): skip the LDS-staged instantiations, 10x shorter compile
    return CB_ERR_ROUTE;
#endif
#if CB_HALF
    // LAMA_PREC_F16: the stem reads the fp32 network input and writes fp16, the head reads fp16 and writes the fp32 image
    if (io == CB_IO_F32_F16 && mode == 1 && BM == 64) {
        hipLaunchKernelGGL((CB_NAME(conv_kernel)<7, 7, 2, 0, 0, 0, 64, 3, 0, 1, 1, CB_IO_F32_F16>), dim3(grid), dim3(CB_THREADS), shmem, st, p);
        LAMA_CHECK_LAUNCH();
        return LAMA_OK;
    }
    if (io == CB_IO_F16_F32 && mode == 2 && BM == 32) {
        hipLaunchKernelGGL((CB_NAME(conv_kernel)<7, 7, 1, 0, 0, 0, 32, 3, 0, 1, 2, CB_IO_F16_F32>), dim3(grid), dim3(CB_THREADS), shmem, st, p);
        LAMA_CHECK_LAUNCH();
        return LAMA_OK;
    }
    return CB_ERR_ROUTE;
#else
    if (io != CB_IO_F32) return CB_ERR_ROUTE;
    if (mode == 2 && BM == 32) hipLaunchKernelGGL((CB_NAME(conv_kernel)<7, 7, 1, 0, 0, 0, 32, 3, 0, 1, 2>), dim3(grid), dim3(CB_THREADS), shmem, st, p);
    else if (mode == 1 && BM == 64) hipLaunchKernelGGL((CB_NAME(conv_kernel)<7, 7, 2, 0, 0, 0, 64, 3, 0, 1, 1>), dim3(grid), dim3(CB_THREADS), shmem, st, p);
    else if (mode == 1 && BM == 128) hipLaunchKernelGGL((CB_NAME(conv_kernel)<7, 7, 2, 0, 0, 0, 128, 3, 0, 1, 1>), dim3(grid), dim3(CB_THREADS), shmem, st, p);
    else if (mode == 1 && BM == 32) hipLaunchKernelGGL((CB_NAME(conv_kernel)<7, 7, 2, 0, 0, 0, 32, 3, 0, 1, 1>), dim3(grid), dim3(CB_THREADS), shmem, st, p);
    else return CB_ERR_ROUTE;
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
#endif
}

int cb_launch(hipStream_t st, const CbParams& p, int T1, int T2, int BM, int maxu, bool trf, int mode, int io, int grid, size_t shmem) {
    if (grid <= 0) return LAMA_OK;
    if (mode) return cb_launch_folded7(st, p, mode, BM, maxu, grid, shmem, io);
    if (trf) {
        switch (BM) {
            case 128: return cb_launch_trf_u<128>(st, p, maxu, grid, shmem, io);
            case 64: return cb_launch_trf_u<64>(st, p, maxu, grid, shmem, io);
            case 32: return cb_launch_trf_u<32>(st, p, maxu, grid, shmem, io);
        }
        return CB_ERR_ROUTE;
    }
#if defined(LAMA_PROFILING) && !CB_HALF
    if (!CB_F16 && T1 == 9 && T2 == 0 && BM == 128 && maxu <= 1) {   // profiling tools only: timing ablations of the bottleneck 3x3 kernel
        static const int abl = lama_env_int("LAMA_CB_ABLATE", 0);   // read once
#define CB_ABL(v) \
    if (abl == v) { hipLaunchKernelGGL((CB_NAME(conv_kernel)<9, 3, 1, 0, 0, 0, 128, 1, v>), dim3(grid), dim3(CB_THREADS), shmem, st, p); LAMA_CHECK_LAUNCH(); return LAMA_OK; }
        CB_ABL(1) CB_ABL(2) CB_ABL(4) CB_ABL(6) CB_ABL(8) CB_ABL(14) CB_ABL(15) CB_ABL(16) CB_ABL(32)
#undef CB_ABL
    }
#endif
#define CB_CASE(t1, g1, k1, t2, g2, k2) \
    if (T1 == t1 && T2 == t2) return cb_launch_bm<t1, g1, k1, t2, g2, k2>(st, p, BM, maxu, grid, shmem, io);
    CB_CASE(9, 3, 1, 0, 0, 0)
    CB_CASE(9, 3, 1, 1, 1, 2)
    CB_CASE(1, 1, 2, 0, 0, 0)
    CB_CASE(49, 7, 1, 0, 0, 0)
    CB_CASE(2, 2, 1, 0, 0, 0)
    CB_CASE(4, 4, 1, 0, 0, 0)
#undef CB_CASE
    return CB_ERR_ROUTE;
}

#include "conv_wreg_host.inc"

}  // namespace

}  // namespace CB_NAME(cbns)
using namespace CB_NAME(cbns);

int64_t CB_NAME(lama_cb_packed_weight_bytes)(int cout, int cin, int kh, int kw, int stride, int transposed) {
    CbPlan pl;
    if (!cb_make_plan(cout, cin, kh, kw, stride, transposed ? 1 : kh / 2, transposed, &pl)) return LAMA_ERR_UNSUPPORTED;
    return pl.total_bytes;
}

int CB_NAME(lama_cb_pack_weight)(hipStream_t stream, const float* w, const float* scale, int cout, int cin, int kh, int kw, int stride,
                        int transposed, void* dst) {
    CbPlan pl;
    if (!cb_make_plan(cout, cin, kh, kw, stride, transposed ? 1 : kh / 2, transposed, &pl)) return LAMA_ERR_UNSUPPORTED;
    for (int cls = 0; cls < pl.nseg; ++cls) {
        CbPackParams pp;
        memset(&pp, 0, sizeof(pp));
        pp.w = w;
        pp.scale = scale;
        pp.dst = (char*)dst + pl.woff[cls];
        pp.M = cout;
        pp.C = cin;
        pp.MFT = pl.mft;
        pp.mode = pl.mode;
        pp.TG = pl.TG[cls];
        pp.KS = pl.KS[cls];
        pp.NG = pl.T[cls] / pl.TG[cls];
        pp.nchunk = pl.nchunk[cls];
        pp.kh = kh;
        pp.kw = kw;
        pp.transposed = transposed;
        for (int t = 0; t < pl.T[cls]; ++t) { pp.tap_ky[t] = pl.ky[cls][t]; pp.tap_kx[t] = pl.kx[cls][t]; }
        long long total = pl.cls_bytes[cls] / 32;  // items of 2 x 16 B
        int grid = (int)((total + 255) / 256);
        if (grid > 4096) grid = 4096;
        hipLaunchKernelGGL(CB_NAME(conv_pack_kernel), dim3(grid), dim3(256), 0, stream, pp);
        LAMA_CHECK_LAUNCH();
    }
    return LAMA_OK;
}

// arguments were validated by lama_conv2d_fwd (conv_mfma.hip).  ``tl``: the work list of lama_conv2d_list_fwd.  ``query`` (lama_conv2d_route_query):
// nothing is launched; the code is the launch's, query[0] the family and query[1] its geometry (cb_route_geometry).
int CB_NAME(lama_cb_conv2d_fwd)(hipStream_t stream, const lama_conv2d_args* a, int Ho, int Wo, const LamaTileList* tl, int32_t* query) {
    CbPlan pl, pl2;
    if (!cb_make_plan(a->y.C, a->x.C, a->kh, a->kw, a->stride, a->pad, a->transposed, &pl)) return LAMA_ERR_UNSUPPORTED;
    const bool has2 = a->x2.ptr != nullptr;
    if (has2 && (!cb_make_plan(a->y.C, a->x2.C, 1, 1, 1, 0, 0, &pl2) || pl.mode)) return LAMA_ERR_UNSUPPORTED;
    int io = (a->x.dtype == LAMA_DT_F16 ? 1 : 0) | (a->y.dtype == LAMA_DT_F16 ? 2 : 0) | ((has2 && a->x2.dtype == LAMA_DT_F16) ? CB_IO_X2H : 0);   // CB_IO_*
    if ((io != CB_IO_F32) != (CB_HALF != 0)) return LAMA_ERR_UNSUPPORTED;   // fp16 tensors <-> the LAMA_PREC_F16 translation unit
    // LAMA_DT_SPLIT16 (validated by lama_conv2d_fwd: split precisions, no x2 / resid / fuse1)
    io |= (a->x.dtype == LAMA_DT_SPLIT16 ? CB_IO_XS : 0) | (a->y.dtype == LAMA_DT_SPLIT16 ? CB_IO_YS : 0);
    const CbPlan* p2 = has2 ? &pl2 : nullptr;
    CbRoute r;
    const int rc = cb_route(a, pl, p2, Ho, Wo, io, tl, &r);
    if (query && rc == LAMA_OK) { query[0] = r.family; query[1] = cb_route_geometry(r); }
    if (query || rc != LAMA_OK) return rc;
    const long long HW = (long long)Ho * Wo;
    switch (r.family) {
        case CB_FAM_WK: return wk_launch(stream, a, pl, HW, r);
        case CB_FAM_W4: return w4_launch(stream, a, pl, HW, r);
        case CB_FAM_WS: return ws_launch(stream, a, pl, HW, r);
        case CB_FAM_WR: return wr_launch(stream, a, pl, p2, Ho, Wo, r);
        case CB_FAM_CT: return ct_launch(stream, a, pl, tl, r);
        case CB_FAM_STEM: return stem_launch(stream, a, pl, Ho, Wo, r);
        case CB_FAM_HEAD: return head_launch(stream, a, pl, Ho, Wo, tl, r);
        case CB_FAM_LDS: {
            CbParams p;
            lds_fill(&p, a, pl, p2, Ho, Wo, r);
            return cb_launch(stream, p, pl.T[0], has2 ? 1 : 0, r.BM, r.maxu, r.trf, r.mode, io, r.grid, r.shmem);
        }
    }
    return CB_ERR_ROUTE;
}

#if !CB_HALF
// Multi-dilated 3x3 reflect convolution (mdconv_dev.inc); arguments were validated by lama_multidilated_conv3x3_fwd (conv_mfma.hip):
// w_packed is the lama_conv2d_pack_weight image of the group weights concatenated along Cin
int CB_NAME(lama_cb_mdconv_fwd)(hipStream_t stream, const lama_conv2d_args* a, int groups, int min_dilation) {
    const int cout = a->y.C, cin = a->x.C, H = a->x.H, W = a->x.W;
    const int dmax = min_dilation << (groups - 1);
    if (dmax > MD_MAX_DIL || cout % 32 != 0 || cin % (16 * groups) != 0) return LAMA_ERR_UNSUPPORTED;
    if ((long long)cin * H * W >= (1ll << 31) || (long long)cout * H * W >= (1ll << 31)) return LAMA_ERR_UNSUPPORTED;   // 32-bit element offsets inside one image
    MdParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const float*)a->x.ptr;
    p.x_bstride = a->x.batch_stride;
    p.C = cin; p.H = H; p.W = W;
    p.w = (const char*)a->w_packed;
    p.mft = cout / 32;
    p.bias = a->bias;
    p.resid = (const float*)a->resid.ptr;
    p.resid_bstride = a->resid.batch_stride;
    p.y = (float*)a->y.ptr;
    p.y_bstride = a->y.batch_stride;
    p.M = cout;
    p.MT = lama_ceil_div(cout, 128);
    p.B = a->batch;
    p.TWlog = W <= 8 ? 3 : 4;      // the squarer tile: 8 rows x 16 columns (the halo of d = 8 costs 24 x 32 patch pixels; 4 x 32 would cost 20 x 48)
    const int TW = 1 << p.TWlog, TH = 128 >> p.TWlog;
    p.tiles_x = lama_ceil_div(W, TW);
    p.tiles_y = lama_ceil_div(H, TH);
    p.act = a->act;
    p.gchunks = cin / groups / 16;
    p.dmin = min_dilation;
    p.pbytes = 2 * 2 * (TH + 2 * dmax) * (TW + 2 * dmax) * 16;
    p.range_flag = a->range_flag;
    const size_t shmem = 2 * (size_t)MD_WBYTES + 2 * (size_t)p.pbytes;
    if (shmem > 160 * 1024) return LAMA_ERR_UNSUPPORTED;
    const long long grid = (long long)p.B * p.tiles_x * p.tiles_y * p.MT;
    if (grid <= 0 || grid >= (1ll << 31)) return grid <= 0 ? LAMA_OK : LAMA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(CB_NAME(mdconv_kernel), dim3((unsigned)grid), dim3(MD_THREADS), shmem, stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}
#endif

// ------------------------------------------------------------------------------------------------
// Winograd F(2x2, 3x3) form of the stride-1 3x3 reflect convolution (wino_dev.inc): pack + two launches
// ------------------------------------------------------------------------------------------------
#if !CB_HALF
namespace {
// the tile geometry of a plane (wino_dev.inc): the exact geometries of round 3 -- tile columns W / 2 = 16, 32, 64 or 128 and H a multiple of the band
// height -- or, for any other H >= 4, W >= 8, rows cut into overlapping segments of QR = 8 / 16 / 32 column quads (the fewest lanes per tile row win)
struct WgGeo { int TCL, RB, bands, nseg, QS, VR, QL, vc, generic; };
bool wg_shape(int cout, int cin, int H, int W, WgGeo* g) {
    if (cout <= 0 || cin <= 0 || cout % 128 != 0 || cin % 32 != 0) return false;
    if (H < 4 || W < 8) return false;
    if ((long long)cin * H * W * 4 >= (1ll << 31)) return false;      // 32-bit byte offsets inside one image
    g->QL = (W - 1) >> 2;
    g->vc = W - 4 * g->QL;
    if (W == 32 || W == 64 || W == 128 || W == 256) {
        const int TCL = lama_ilog2(W / 2), RB = 128 >> TCL;
        if (H >= 2 * RB && H % (2 * RB) == 0) {
            g->TCL = TCL; g->RB = RB; g->bands = H / (2 * RB);
            g->nseg = 1; g->QS = W / 4; g->VR = H / 2; g->generic = 0;
            return true;
        }
    }
    const int force_qr = lama_env_int("LAMA_WG_QR", 0);               // profiling build / emulator tests: 8 / 16 / 32 force the segment width (read per call)
    const int QW = (W + 3) >> 2, TR = (H + 1) >> 1;
    int best = 0, best_cost = 0;
    for (int QR = 32; QR >= 8; QR >>= 1) {
        if (force_qr && QR != force_qr) continue;
        const int nseg = QW <= QR ? 1 : (QW - 1 + QR - 2) / (QR - 1);
        const int cost = nseg * QR;
        if (!best || cost < best_cost) { best = QR; best_cost = cost; }
    }
    if (!best) return false;
    const int QR = best;
    g->nseg = QW <= QR ? 1 : (QW - 1 + QR - 2) / (QR - 1);
    g->QS = g->nseg > 1 ? QR - 1 : QR;
    g->TCL = lama_ilog2(2 * QR);
    g->RB = 64 / QR;
    g->VR = TR * g->nseg;
    g->bands = lama_ceil_div(g->VR, g->RB);
    g->generic = 1;
    return true;
}
}  // namespace

int64_t CB_NAME(lama_cb_wino_packed_weight_bytes)(int cout, int cin) {
    if (cout <= 0 || cin <= 0 || cout % 128 != 0 || cin % 32 != 0) return LAMA_ERR_UNSUPPORTED;
    return (int64_t)(cin / 16) * 16 * (cout / 32) * 2048;
}

int CB_NAME(lama_cb_wino_pack_weight)(hipStream_t stream, const float* w, const float* scale, int cout, int cin, void* dst) {
    if (CB_NAME(lama_cb_wino_packed_weight_bytes)(cout, cin) < 0) return LAMA_ERR_UNSUPPORTED;
    WgPackParams pp;
    pp.w = w;
    pp.scale = scale;
    pp.dst = (char*)dst;
    pp.M = cout;
    pp.C = cin;
    pp.MFT = cout / 32;
    const long long total = (long long)(cin / 16) * 16 * pp.MFT * 64;
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(CB_NAME(wino_pack_kernel), dim3(grid), dim3(256), 0, stream, pp);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// every bound lama_cb_wino_fwd enforces, with the real channel count (the 32-bit byte offsets inside one image depend on it)
bool CB_NAME(lama_cb_wino_shape_ok)(int cout, int cin, int H, int W) {
    WgGeo g;
    return wg_shape(cout, cin, H, W, &g);
}

// split-K of small launches (round 4): (image, band, xi, row group) units on 256 CUs -- below 128 of them the input channels are dealt to 2, below 64 to 4
// workgroups per unit (1 x 512^2 has 32 units: the launch took 41 us on an eighth of the chip)
static inline int wg_ksplit(int batch, int bands, int MG) {
    const long long units = (long long)batch * bands * 4 * MG;
    if (units <= 256) return units >= 128 ? 1 : (units >= 64 ? 2 : 4);
    // round 6: launches of a little more than a whole number of rounds (135 x 240: 272 units = two rounds for 1.06 rounds of work): halves / quarters
    // of the K loop round up less.  Cost model of one workgroup (us): 8 + 45 / KS (prologue + exchange, K loop), + 5 per extra slice the output transform adds
    int best = 1;
    double best_t = 0;
    for (int ks = 1; ks <= 4; ks *= 2) {
        const double t = (double)((units * ks + 255) / 256) * (8.0 + 45.0 / ks) + 5.0 * (ks - 1);
        if (ks == 1 || t < best_t - 1e-9) { best = ks; best_t = t; }
    }
    return best;
}

// round 6: is the Winograd form of this launch expected to beat the direct kernel?  The exact geometries: yes (measured, round 3).  The any-size
// geometry pays for lanes outside the plane and -- like every one-workgroup-per-CU launch -- for whole rounds: a little more than a round of units
// is two rounds (1 x 135 x 240: 272 units: 113 us against ~95 for 255 direct tiles; 1 x 168 x 168: 252 units: 65 against 92).  Cost model in us,
// constants from profiles/r06_winograd_any_size.txt: a round of workgroups 8 + 45 / KS, the output transform 14 (+ 5 per extra slice) per 32768
// pixels, a round of the direct kernel 92 (fitted at 128 output rows, MG = 1; wider launches have constants of their own, below).
bool CB_NAME(lama_cb_wino_preferred)(int batch, int cout, int cin, int H, int W) {
    WgGeo g;
    if (!wg_shape(cout, cin, H, W, &g)) return false;
    if (!g.generic) return true;
    const int MG = cout / 128, KS = wg_ksplit(batch, g.bands, MG);
    const long long units = (long long)batch * g.bands * 4 * MG;
    const double px = (double)batch * H * W / 32768.0;
    const double wino = (double)((units * KS + 255) / 256) * (8.0 + 45.0 / KS) + px * (14.0 + 5.0 * (KS - 1));
    long long tiles = 0;
    for (int tl = 5; tl >= 3; --tl) {
        const long long nt = (long long)batch * lama_ceil_div(W, 1 << tl) * lama_ceil_div(H, 128 >> tl);
        if (!tiles || (nt + 255) / 256 < (tiles + 255) / 256) tiles = nt;
    }
    if (MG > 1) {
        // more than one 128-row group (the 512 -> 512 convs of the pix2pixhd_global blocks), refitted on 12 plane shapes timed both ways
        // (profiles/regular_conv512.txt): a round of Winograd workgroups costs 58-65 us at KS = 1 (8 + 52 / KS), a round of the direct kernel
        // 82-94 (88); with both constants fitted at this width the rule needs no safety margin
        const double wino_m = (double)((units * KS + 255) / 256) * (8.0 + 52.0 / KS) + px * (14.0 + 5.0 * (KS - 1));
        return wino_m < (double)((tiles * MG + 255) / 256) * 88.0;
    }
    const double direct = (double)((tiles * MG + 255) / 256) * 92.0;
    return wino < 0.92 * direct;
}

int64_t CB_NAME(lama_cb_wino_workspace_bytes)(int batch, int cout, int H, int W) {
    WgGeo g;
    if (batch <= 0 || !wg_shape(cout, 32, H, W, &g)) return 0;
    return (int64_t)wg_ksplit(batch, g.bands, cout / 128) * batch * g.bands * 8 * cout * 128 * (int64_t)sizeof(float);
}

// arguments were validated by lama_winograd_conv3x3_fwd (conv_mfma.hip)
int CB_NAME(lama_cb_wino_fwd)(hipStream_t stream, const lama_conv2d_args* a, void* workspace, size_t workspace_bytes) {
    const int cout = a->y.C, cin = a->x.C, H = a->x.H, W = a->x.W;
    WgGeo g;
    if (!wg_shape(cout, cin, H, W, &g)) return LAMA_ERR_UNSUPPORTED;
    const int TCL = g.TCL, RB = g.RB, bands = g.bands;
    if (!g.generic && ((((uintptr_t)a->x.ptr | (uintptr_t)a->y.ptr | (uintptr_t)a->resid.ptr) & 15) != 0 || a->x.batch_stride % 4 != 0 || a->y.batch_stride % 4 != 0 ||
                       (a->resid.ptr && a->resid.batch_stride % 4 != 0)))
        return LAMA_ERR_UNSUPPORTED;      // 16-byte accesses of the exact geometries: such views keep lama_conv2d_fwd
    if (!workspace || (int64_t)workspace_bytes < CB_NAME(lama_cb_wino_workspace_bytes)(a->batch, cout, H, W)) return LAMA_ERR_WORKSPACE;
    WgParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const float*)a->x.ptr;
    p.x_bstride = a->x.batch_stride;
    p.C = cin; p.H = H; p.W = W;
    p.w = (const char*)a->w_packed;
    p.mft = cout / 32;
    p.part = (float*)workspace;
    p.M = cout; p.B = a->batch;
    p.TCL = TCL; p.RB = RB; p.bands = bands; p.MG = cout / 128;
    p.nseg = g.nseg; p.QS = g.QS; p.VR = g.VR; p.QL = g.QL; p.vc = g.vc;
    p.zpad = a->pad_mode == LAMA_PAD_ZERO;
    p.KS = wg_ksplit(a->batch << LAMA_CONV_SIBLINGS_LOG2(a->flags), bands, p.MG);      // (v109) a part of a batch beside its siblings: the whole batch's rule
    { const int alone = wg_ksplit(a->batch, bands, p.MG); if (p.KS > alone) p.KS = alone; }   // (never more slices than the workspace was sized for)
    { const int force = lama_env_int("LAMA_WG_KS", 0); if (force > 0) p.KS = force < p.KS ? force : p.KS; }   // profiling build / emulator tests: cap the split (the workspace is sized for the rule's)
    while (p.KS > 1 && (cin / 32) % p.KS != 0) p.KS >>= 1;
    p.range_flag = a->range_flag;
    const int grid = a->batch * bands * 4 * p.MG * p.KS;
    // GEO 1 of wino_gemm_kernel: a tile row = one 16-lane DPP row (64-column planes in the exact geometry, reflect padding); LAMA_WG_GEO=0 (profiling build) keeps GEO 0
    bool rows16 = !g.generic && W == 64 && TCL == 5 && g.nseg == 1 && g.QS == 16 && g.vc == 4 && !p.zpad;
#if defined(LAMA_PROFILING)
    { const int geo = lama_env_int("LAMA_WG_GEO", 1); if (!geo) rows16 = false; }   // read per launch: the forced-path test switches it between two launches
#endif
#if defined(LAMA_PROFILING)
    {   // profiling tools only: per-workgroup timeline, LAMA_WG_TRACE = device address of grid * 16 int64
        static const unsigned long long tr = lama_env_u64("LAMA_WG_TRACE");
        static const int abl = lama_env_int("LAMA_WG_ABLATE", 0);     // timing-only ablations (results wrong)
        if (tr) {
            p.trace = reinterpret_cast<long long*>(tr);
            if (rows16) hipLaunchKernelGGL((CB_NAME(wino_gemm_kernel)<true, 0, 1>), dim3(grid), dim3(WG_THREADS), WG_LDS_BYTES, stream, p);
            else hipLaunchKernelGGL((CB_NAME(wino_gemm_kernel)<true>), dim3(grid), dim3(WG_THREADS), WG_LDS_BYTES, stream, p);
        }
#define WG_ABL(v) else if (CB_F16 && abl == v) hipLaunchKernelGGL((CB_NAME(wino_gemm_kernel)<false, v>), dim3(grid), dim3(WG_THREADS), WG_LDS_BYTES, stream, p)
        WG_ABL(1); WG_ABL(2); WG_ABL(29); WG_ABL(31); WG_ABL(32); WG_ABL(64); WG_ABL(96); WG_ABL(34);
#undef WG_ABL
        else if (rows16) hipLaunchKernelGGL((CB_NAME(wino_gemm_kernel)<false, 0, 1>), dim3(grid), dim3(WG_THREADS), WG_LDS_BYTES, stream, p);
        else hipLaunchKernelGGL((CB_NAME(wino_gemm_kernel)<false>), dim3(grid), dim3(WG_THREADS), WG_LDS_BYTES, stream, p);
    }
#else
    if (rows16) hipLaunchKernelGGL((CB_NAME(wino_gemm_kernel)<false, 0, 1>), dim3(grid), dim3(WG_THREADS), WG_LDS_BYTES, stream, p);
    else hipLaunchKernelGGL((CB_NAME(wino_gemm_kernel)<false>), dim3(grid), dim3(WG_THREADS), WG_LDS_BYTES, stream, p);
#endif
    LAMA_CHECK_LAUNCH();
    if (a->flags & LAMA_CONV_DEFER_OUT) return LAMA_OK;      // the caller owes lama_winograd_out_fwd / lama_rfft2_winograd_out_fwd with the same arguments
    return CB_NAME(lama_cb_wino_out_fwd)(stream, a, workspace, workspace_bytes);
}

// the second launch's parameters from the same arguments (precision-independent; `out` is a WoParams)
int CB_NAME(lama_cb_wino_out_params)(const lama_conv2d_args* a, void* workspace, size_t workspace_bytes, void* out) {
    const int cout = a->y.C, cin = a->x.C, H = a->x.H, W = a->x.W;
    WgGeo g;
    if (!wg_shape(cout, cin, H, W, &g)) return LAMA_ERR_UNSUPPORTED;
    const int TCL = g.TCL, RB = g.RB, bands = g.bands;
    if (!g.generic && ((((uintptr_t)a->y.ptr | (uintptr_t)a->resid.ptr) & 15) != 0 || a->y.batch_stride % 4 != 0 || (a->resid.ptr && a->resid.batch_stride % 4 != 0)))
        return LAMA_ERR_UNSUPPORTED;
    if (!workspace || (int64_t)workspace_bytes < CB_NAME(lama_cb_wino_workspace_bytes)(a->batch, cout, H, W)) return LAMA_ERR_WORKSPACE;
    int KS = wg_ksplit(a->batch << LAMA_CONV_SIBLINGS_LOG2(a->flags), bands, cout / 128);
    { const int alone = wg_ksplit(a->batch, bands, cout / 128); if (KS > alone) KS = alone; }
    { const int force = lama_env_int("LAMA_WG_KS", 0); if (force > 0) KS = force < KS ? force : KS; }
    while (KS > 1 && (cin / 32) % KS != 0) KS >>= 1;
    WoParams o;
    memset(&o, 0, sizeof(o));
    o.part = (const float*)workspace;
    o.bias = a->bias;
    o.resid = (const float*)a->resid.ptr;
    o.resid_bstride = a->resid.batch_stride;
    o.y = (float*)a->y.ptr;
    o.y_bstride = a->y.batch_stride;
    o.M = cout; o.B = a->batch; o.H = H; o.W = W; o.TCL = TCL; o.RB = RB; o.bands = bands; o.act = a->act; o.KS = KS;
    o.nseg = g.generic ? g.nseg : 0; o.QS = g.QS; o.VR = g.VR;
    o.vec = (W % 4 == 0) && ((((uintptr_t)a->y.ptr | (uintptr_t)a->resid.ptr) & 15) == 0) && a->y.batch_stride % 4 == 0 && (!a->resid.ptr || a->resid.batch_stride % 4 == 0);
    memcpy(out, &o, sizeof(o));
    return LAMA_OK;
}

int CB_NAME(lama_cb_wino_out_fwd)(hipStream_t stream, const lama_conv2d_args* a, void* workspace, size_t workspace_bytes) {
    WoParams o;
    const int rc = CB_NAME(lama_cb_wino_out_params)(a, workspace, workspace_bytes, &o);
    if (rc) return rc;
    const long long total = (long long)o.B * o.bands * o.M * 64;
    long long g2 = (total + 255) / 256;
    if (g2 > 16384) g2 = 16384;
    hipLaunchKernelGGL(CB_NAME(wino_out_kernel), dim3((int)g2), dim3(256), 0, stream, o);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}
#endif
