// Dedicated kernel for the stem of the generator: ReflectionPad2d(3) + 7x7 conv (cin <= 4) -> 33..64 channels + BN + ReLU
// (ffc.py:315-317), for the 3-term split precisions (included by conv_split3.inc, device part).
//
// The layer writes the largest tensor of the network ([8,64,512,512] = 537 MB) from a 33 MB input with a K of only 7 x 32
// (the 7 horizontal taps folded into 28 virtual input channels, conv_split3.inc MODE 1).  In the LDS-staged kernel a workgroup
// spends ~1 us of MFMA time inside ~10 us of prologue (patch + 57 KB of weights), seven barrier-separated stages and a 32 KB
// store tail, one workgroup per CU: 630-650 us.  Here, as in conv_ws_dev.inc:
//
//   * weights stationary: a wave owns one 32-row fragment and keeps all 14 k-steps (7 vertical taps x 2) of its packed weights,
//     hi + lo, in 112 VGPRs for the whole launch (the packed layout of MODE 1 is used as it is);
//   * a wave walks DOWN a column of 32-pixel row segments with a rolling window of 7 input rows x 4 channels x 38 columns in a
//     wave-private LDS ring (8 row slots, 5 KB, elements already split to (hi, lo) and packed in one dword): a new output row
//     costs ONE new input row (3 coalesced loads per lane, requested a whole tile ahead) instead of 112 shifted dword loads
//     (the first version of this kernel, TA-bound at 438 us); no workgroup barrier anywhere, the hand-off between the lanes of
//     the wave is LAMA_WAVE_SYNC;
//   * a lane's 8 K-values of a k-step are 8 (channel, kx) pairs of its pixel = 8 ds_read_b32 at lane-constant offsets + the
//     row slot, re-packed with two integer ops per pair; reflection is applied when a row / column is loaded, never in the loop;
//   * persistent 4-wave workgroups, two per CU; the two waves of a pixel column (the two row fragments) keep private windows.

struct StemParams {
    const float* x;
    long long x_bstride;
    int C, H, W;
    const char* w;       // MODE 1 packed weights: [k-step 2 ky + ks][32-row fragment][hi|lo][lane][8 halves], virtual channel c = cc * 7 + kx
    int mft;
    const float* bias;
    float* y;
    long long y_bstride;
    int M, B, act;
    int tx;              // 32-pixel segments per row
    int ns, rs;          // vertical parts per column of segments, rows per part
    int nseg;            // B * tx * ns
    unsigned* range_flag;   // lama_conv2d_args.range_flag (f16 split only; may be null)
};

#define STEM_WIN 40                      // dwords per (row slot, channel): 38 window columns, padded
#define STEM_SLOT (4 * STEM_WIN)         // dwords per row slot
#define STEM_WAVE_LDS (8 * STEM_SLOT + 64)   // + 64 dump dwords for the lanes without an element in the row load
#define STEM_LDS_BYTES (4 * STEM_WAVE_LDS * 4)

// packed (hi | lo << 16) halves of two floats
__device__ __forceinline__ void stem_pack2(float a, float b, unsigned& pa, unsigned& pb, unsigned& rw) {
    unsigned hi, lo;
    cb_split2(a, b, hi, lo, rw);
    pa = __builtin_amdgcn_perm(lo, hi, 0x05040100u);       // (hi & 0xffff) | (lo << 16): one v_perm_b32 each
    pb = __builtin_amdgcn_perm(lo, hi, 0x07060302u);       // (hi >> 16) | (lo & 0xffff0000)
}

// HO (f16 back end, LAMA_PREC_F16): the output is fp16 (half of this kernel's HBM traffic, which is all stores) and the contraction is
// one product per MAC (hi parts only).
// YS (3-term split only): the output is LAMA_DT_SPLIT16 -- the (hi, lo) parts the next stride-2 conv would form while it stages, stored in
// its staging order, [channel octet][hi | lo][H][W][8 halves] (four bytes per element, as fp32); this kernel then watches the range of what
// it stores (lama_hip.h).  M % 8 == 0 (the host checks).
template <bool HO = false, bool YS = false>
__global__ __launch_bounds__(256, 2) void CB_NAME(stem7_ws_kernel)(StemParams p) {
    static_assert(!(HO && YS), "pre-split output: the 3-term split precisions only");
    constexpr int ESO = HO ? 2 : 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = LAMA_WAVE_UNIFORM(tid >> 6);
    const int F = wave & 1, half = wave >> 1;
    const int khalf = lane >> 5, l31 = lane & 31;
    const int H = p.H, W = p.W, HW = H * W;
    const int strip = blockIdx.x * 2 + half, nstrips = gridDim.x * 2;
    unsigned* const win = reinterpret_cast<unsigned*>(lama_smem) + wave * STEM_WAVE_LDS;
    unsigned rw = 0;   // range watch of the f16 split

    // the window starts as zeros: channels past C are never loaded and virtual channels 28..31 read a real one (zero weights)
    for (int i = lane; i < STEM_WAVE_LDS; i += 64) win[i] = 0u;

    // this wave's weights: fragment F, k-steps 0..13
    constexpr bool ALO = !HO || CB_HF_W2;   // fp16 output (LAMA_PREC_F16): a_hi x b_hi + a_lo x b_hi
    u32x4 ah[14], al[ALO ? 14 : 1];
    {
        const lama_buf_t wres = LAMA_BUF_RSRC(p.w, (long long)14 * p.mft * 2048);
        const int Fc = F < p.mft ? F : p.mft - 1;
#pragma unroll
        for (int s = 0; s < 14; ++s) {
            ah[s] = __builtin_bit_cast(u32x4, LAMA_BUF_LOAD_B128(wres, lane * 16, (s * p.mft + Fc) * 2048));
            if constexpr (ALO) al[s] = __builtin_bit_cast(u32x4, LAMA_BUF_LOAD_B128(wres, lane * 16 + 1024, (s * p.mft + Fc) * 2048));
        }
    }
    // bias of the 16 rows this lane holds: row = F * 32 + (r & 3) + 8 (r >> 2) + 4 khalf
    float bv[16];
    {
        const lama_buf_t bres = LAMA_BUF_RSRC(p.bias, p.bias ? (long long)p.M * 4 : 0ll);
#pragma unroll
        for (int r = 0; r < 16; ++r) bv[r] = __builtin_bit_cast(float, LAMA_BUF_LOAD_B32(bres, (F * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf) * 4, 0));
    }
    // window index (dwords inside a row slot) of this lane's 16 K-values per vertical tap: virtual channel c = 16 ks + 8 khalf + e
    // = (channel cc, horizontal tap kx) -> cc * STEM_WIN + l31 + kx; virtual channels 28..31 (zero weights) read channel 0
    int widx[2][8];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = 16 * ks + 8 * khalf + e;
            const int cc = c / 7, kx = c - cc * 7;
            widx[ks][e] = c < 28 ? cc * STEM_WIN + l31 + kx : l31;
        }
    // row load: element id = lane + 64 i -> (channel id / 38, window column id % 38), i = 0..2 (152 elements)
    int lcc[3], lj[3], lw[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int id = lane + 64 * i;
        lcc[i] = id / 38;
        lj[i] = id - lcc[i] * 38;
        lw[i] = id < 152 ? lcc[i] * STEM_WIN + lj[i] : -1;      // -1: no element, the (zero) value goes to the dump dwords
    }
    LAMA_WAVE_SYNC();

#pragma unroll 1
    for (int g = strip; g < p.nseg; g += nstrips) {
        const int col = g / p.ns, part = g - col * p.ns;
        const int b = col / p.tx, px0 = (col - b * p.tx) * 32;
        const int y0 = part * p.rs, y1 = (y0 + p.rs < H) ? y0 + p.rs : H;
        const lama_buf_t xres = LAMA_BUF_RSRC(p.x + (long long)b * p.x_bstride, (long long)p.C * HW * 4);
        const lama_buf_t yres = LAMA_BUF_RSRC(reinterpret_cast<char*>(p.y) + (long long)b * p.y_bstride * ESO, (long long)p.M * HW * ESO);
        int coloff[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            int ix = px0 - 3 + lj[i];
            ix = ix < 0 ? -ix : ix;
            ix = ix >= W ? 2 * (W - 1) - ix : ix;
            ix = ix < 0 ? 0 : (ix >= W ? W - 1 : ix);           // columns past a ragged last segment (never used by a stored pixel)
            coloff[i] = (lw[i] >= 0 && lcc[i] < p.C) ? (lcc[i] * HW + ix) * 4 : 0x7ffffff0;
        }
        auto row_off = [&](int u) {                             // virtual row u (may be outside the image) -> byte offset of the input row
            int iy = u < 0 ? -u : u;
            iy = iy >= H ? 2 * (H - 1) - iy : iy;
            iy = iy < 0 ? 0 : (iy >= H ? H - 1 : iy);
            return iy * W * 4;
        };
        float nr[3];
        auto request_row = [&](int u) {
            const int ro = row_off(u);
#pragma unroll
            for (int i = 0; i < 3; ++i) nr[i] = __builtin_bit_cast(float, LAMA_BUF_LOAD_B32(xres, coloff[i], ro));
        };
        auto deposit_row = [&](int u) {                         // split, pack and store the requested row into slot (u + 8) & 7
            unsigned pk[4];
            stem_pack2(nr[0], nr[1], pk[0], pk[1], rw);
            stem_pack2(nr[2], 0.0f, pk[2], pk[3], rw);
            unsigned* slot = win + ((u + 8) & 7) * STEM_SLOT;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                if (lw[i] >= 0) slot[lw[i]] = pk[i];
                else win[8 * STEM_SLOT + lane] = pk[i];
            }
        };
        // fill the window with the 7 rows of the first output row of this part
        for (int u = y0 - 3; u <= y0 + 3; ++u) {
            request_row(u);
            deposit_row(u);
        }
        LAMA_WAVE_SYNC();

#pragma unroll 1
        for (int y = y0; y < y1; ++y) {
            request_row(y + 4);                                 // the one new row of the NEXT output row, a whole tile ahead
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            // the 8 ds_read_b32 of k-step s + 1 are issued before the (serially dependent) MFMAs of k-step s
            unsigned d[2][8];
            auto read_k = [&](auto s_tag) {
                constexpr int s = decltype(s_tag)::value;
                const unsigned* slot = win + ((y + (s >> 1) + 5) & 7) * STEM_SLOT;      // virtual row y + ky - 3
#pragma unroll
                for (int e = 0; e < 8; ++e) d[s & 1][e] = slot[widx[s & 1][e]];
            };
            auto mma_k = [&](auto s_tag) {
                constexpr int s = decltype(s_tag)::value;
                if constexpr (s + 1 < 14) read_k(CbTag<(s + 1 < 14 ? s + 1 : 0)>{});
                unsigned hh[4], ll[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // (d0 & 0xffff) | (d1 << 16) and (d0 >> 16) | (d1 & 0xffff0000) as ONE v_perm_b32 each (round 6, fourth session: the compiler emitted
                    // v_and + v_lshl_or and v_lshrrev + v_and_or -- 211 of the 301 VALU instructions between a row's 42 MFMAs, in a kernel whose two waves per
                    // SIMD are bound by instruction issue: profiles/r06_sq_counters.txt)
                    hh[e] = __builtin_amdgcn_perm(d[s & 1][2 * e + 1], d[s & 1][2 * e], 0x05040100u);
                    ll[e] = __builtin_amdgcn_perm(d[s & 1][2 * e + 1], d[s & 1][2 * e], 0x07060302u);
                }
                const bf16x8 bh = __builtin_bit_cast(bf16x8, u32x4{hh[0], hh[1], hh[2], hh[3]});
                const bf16x8 bl = __builtin_bit_cast(bf16x8, u32x4{ll[0], ll[1], ll[2], ll[3]});
                __builtin_amdgcn_sched_barrier(0);
                acc = CB_MFMA(__builtin_bit_cast(bf16x8, ah[s]), bh, acc, 0, 0, 0);
                if constexpr (!HO) acc = CB_MFMA(__builtin_bit_cast(bf16x8, ah[s]), bl, acc, 0, 0, 0);
                if constexpr (ALO) acc = CB_MFMA(__builtin_bit_cast(bf16x8, al[s]), bh, acc, 0, 0, 0);
            };
            read_k(CbTag<0>{});
            mma_k(CbTag<0>{}); mma_k(CbTag<1>{}); mma_k(CbTag<2>{}); mma_k(CbTag<3>{}); mma_k(CbTag<4>{}); mma_k(CbTag<5>{}); mma_k(CbTag<6>{});
            mma_k(CbTag<7>{}); mma_k(CbTag<8>{}); mma_k(CbTag<9>{}); mma_k(CbTag<10>{}); mma_k(CbTag<11>{}); mma_k(CbTag<12>{}); mma_k(CbTag<13>{});
            // the slot of virtual row y - 4 is free (this output row read y - 3 .. y + 3): the new row goes there
            LAMA_WAVE_SYNC();
            deposit_row(y + 4);
            LAMA_WAVE_SYNC();
            // bias, activation, store (rows past M are out of range of the buffer, pixels past W get an out-of-range offset)
            const int px = px0 + l31;
            const int eoff = (px < W && F < p.mft) ? ((F * 32 + 4 * khalf) * HW + y * W + px) * ESO : 0x7ffffff0;
            float ov[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) ov[r] = acc[r] + bv[r];
            if (p.act == LAMA_ACT_RELU) {
#pragma unroll
                for (int r = 0; r < 16; ++r) ov[r] = fmaxf(ov[r], 0.0f);
            } else if (p.act == LAMA_ACT_SIGMOID) {
#pragma unroll
                for (int r = 0; r < 16; ++r) ov[r] = 1.0f / (1.0f + expf(-ov[r]));
            } else if (p.act == LAMA_ACT_TANH) {
#pragma unroll
                for (int r = 0; r < 16; ++r) ov[r] = tanhf(ov[r]);
            }
            if constexpr (YS) {
                // registers 4 g .. 4 g + 3 = channels 4 khalf .. 4 khalf + 3 of octet 4 F + g: 8 bytes of the pixel's hi slot, 8 of its lo slot
                // (a wave stores 512 contiguous bytes per plane).  Split, then the watch of what IS stored (a ragged last segment's lanes past W and
                // octets past M are not), then the stores.
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    unsigned h0, h1, l0, l1;
                    cb_split2(ov[4 * g], ov[4 * g + 1], h0, l0);
                    cb_split2(ov[4 * g + 2], ov[4 * g + 3], h1, l1);
                    const int oct = F * 4 + g;
                    const bool stored = px < W && oct * 8 < p.M;
                    if (stored) {
                        cb_range_watch(h0, rw);
                        cb_range_watch(h1, rw);
                    }
                    const int voff = stored ? (y * W + px) * 16 + 8 * khalf : 0x7ffffff0;   // (not stored: past the buffer's range, dropped)
                    LAMA_BUF_STORE_B64(yres, (u32x2{h0, h1}), voff, oct * 2 * HW * 16);
                    LAMA_BUF_STORE_B64(yres, (u32x2{l0, l1}), voff, (oct * 2 + 1) * HW * 16);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if constexpr (HO) LAMA_BUF_STORE_B16(yres, __builtin_bit_cast(unsigned short, (_Float16)ov[r]), eoff, ((r & 3) + 8 * (r >> 2)) * HW * ESO);
                    else LAMA_BUF_STORE_B32(yres, __builtin_bit_cast(unsigned, ov[r]), eoff, ((r & 3) + 8 * (r >> 2)) * HW * ESO);
                }
            }
        }
        LAMA_WAVE_SYNC();   // the next part refills the window
    }
    cb_range_report(rw, p.range_flag);
}
