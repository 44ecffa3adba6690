// Dedicated kernel for the head of the generator: ReflectionPad2d(3) + 7x7 conv 64 -> (<= 4) channels + bias + sigmoid
// (ffc.py:360-363), for the 3-term split precisions (included by conv_split3.inc, device part).
//
// The layer reads the largest tensor of the network ([8,64,512,512] = 537 MB) for a 25 MB output.  GEMM view as in MODE 2 of
// conv_split3.inc: the 7 horizontal taps become virtual output rows m' = o * 7 + kx (21 of 32 rows useful),
//     z[m'][Y][X'] = sum_{c, ky} W[o, c, ky, kx] x[c][Y + ky - 3][X'],      y[o][Y][X] = sum_kx z[o * 7 + kx][Y][X + kx - 3],
// K = 7 vertical taps x 64 channels = 28 k-steps, and the MODE 2 weight packing is used as it is.  The LDS-staged kernel runs it
// in 500-515 us (patch with a 2.5x vertical halo per 4-row tile, one workgroup per CU).  Here:
//
//   * a 4-wave workgroup walks DOWN a column of 32 input columns (26 output columns); wave q owns channels 16 q .. 16 q + 15:
//     its weights (7 k-steps, hi + lo) stay in 56 VGPRs, and its B operands are lane-private -- lane (khalf, column) needs the 8
//     channels 16 q + 8 khalf .. + 7 of its column for the 7 rows Y - 3 .. Y + 3, so the 7-row window is a REGISTER ring
//     of 8 slots x 8 VGPRs -- the 7 rows of the window as (hi, lo) halves plus the row in flight as the 8 requested floats (a
//     row is requested one output row before it is needed and converted in place); the loop over rows is unrolled by 8
//     so that the ring slots are compile-time, and a new output row costs 8 coalesced dword loads per lane: no LDS and no
//     address arithmetic in the K loop (21 MFMAs per wave and row);
//   * the four channel-group partial sums and the 7-tap horizontal sum meet in LDS (double-buffered, one barrier per row): every
//     thread finishes at most one output pixel (28 LDS reads), bias + sigmoid + store.
//   * persistent workgroups, three per CU (they cover each other's load latency).

struct HeadParams {
    const float* x;
    long long x_bstride;
    int C, H, W;         // C == 64
    const char* w;       // MODE 2 packed weights: [channel group ch][ky][hi|lo][lane][8 halves], virtual row m' = o * 7 + kx
    const float* bias;
    float* y;
    long long y_bstride;
    int M, B, act;       // M <= 4 output channels
    int tx;              // 26-column output segments per row
    int ns, rs;          // vertical parts per column of segments, rows per part (a multiple of HEAD_R = 8)
    int nseg;            // B * tx * ns
    unsigned* range_flag;   // lama_conv2d_args.range_flag (f16 split only; may be null)
    const int* list;        // LIST instantiation (lama_conv2d_list_fwd): the dense segment indices to walk, in ascending order ...
    const int* count;       // ... and how many of them (device int, written by lama_tail_lists_build earlier in the same stream)
};

#define HEAD_ZP 33                                  // floats per z row in LDS (32 columns, padded)
#define HEAD_ZR 28                                  // virtual rows kept per channel group (7 M, M <= 4)
#define HEAD_ZBUF (4 * HEAD_ZR * HEAD_ZP)           // one z buffer: 4 channel groups x 28 virtual rows
#define HEAD_LDS_BYTES (2 * HEAD_ZBUF * 4)

#define HEAD_D 1                                    // input rows in flight beyond the 7-row window (5 rows / 12 slots / two
                                                    // workgroups per CU measured slower: 356 vs 317 us)
#define HEAD_R (7 + HEAD_D)                         // register ring slots = rows the row loop is unrolled by
#ifndef HEAD_ABL
#define HEAD_ABL 0                                  // stand-alone harness only (results WRONG): 1 no MFMA, 2 no input loads, 4 no finisher, 8 no z exchange / barrier
#endif
#ifndef HEAD_LATE
#define HEAD_LATE 1                                 // 0: the round-2 order (the row in flight is converted at the top of the output row)
#endif

// HI (f16 back end, LAMA_PREC_F16): the input is fp16 (half of this kernel's HBM traffic, which is all loads): a requested row is 8
// 16-bit patterns that pack into the four hi dwords without any conversion; one product per MAC.  The output image stays fp32.
// LIST: the workgroups walk the p.count[0] segment indices of p.list (segments that hold a needed output pixel: sparse tail, DESIGN.md 4.17) instead
// of 0 .. nseg - 1; list order = dense order with holes, so neighbouring entries are still neighbouring columns wherever both are listed.
template <bool HI = false, bool LIST = false>
__global__ __launch_bounds__(256, 3) void CB_NAME(head7_ws_kernel)(HeadParams p) {
    constexpr int ESI = HI ? 2 : 4;
    const int tid = threadIdx.x, lane = tid & 63, q = LAMA_WAVE_UNIFORM(tid >> 6);
    const int khalf = lane >> 5, l31 = lane & 31;
    const int H = p.H, W = p.W, HW = H * W;
    float* const zlds = reinterpret_cast<float*>(lama_smem);
    unsigned rw = 0;   // range watch of the f16 split

    // this wave's weights: channel group q, k-steps ky = 0..6
    constexpr bool ALO = !HI || CB_HF_W2;   // fp16 input: a_lo x b is the second product (weights keep 22 bits)
    u32x4 ah[7], al[ALO ? 7 : 1];
    {
        const lama_buf_t wres = LAMA_BUF_RSRC(p.w, (long long)28 * 2048);
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            ah[ky] = __builtin_bit_cast(u32x4, LAMA_BUF_LOAD_B128(wres, lane * 16, (q * 7 + ky) * 2048));
            if constexpr (ALO) al[ky] = __builtin_bit_cast(u32x4, LAMA_BUF_LOAD_B128(wres, lane * 16 + 1024, (q * 7 + ky) * 2048));
        }
    }
    // the output pixel this thread finishes: (o, j) = (tid / 26, tid % 26) for tid < 26 * M
    const int fo = tid / 26, fj = tid - fo * 26;
    const bool finisher = fo < p.M;
    const float fbias = (finisher && p.bias) ? p.bias[fo] : 0.0f;

    // Segment order: neighbouring COLUMNS (same vertical part) on neighbouring workgroups of one XCD.  The 32 input columns of a
    // segment start at x0 - 3, so every 128-byte row piece straddles two lines and the second one is the first of the next column's
    // segment: walked at the same time behind the same L2 it is fetched from HBM once (column-major order put the two on
    // different XCDs: 2.09x the algorithmic traffic, profiles/r02_pmc.json).
    const int ncols = p.B * p.tx;
    int nseg = p.nseg;
    if constexpr (LIST) { const int n = p.count[0]; nseg = n < nseg ? (n > 0 ? n : 0) : nseg; }   // (never more entries than the list holds)
#pragma unroll 1
    for (int gi = lama_xcd_remap(blockIdx.x, gridDim.x); gi < nseg; gi += gridDim.x) {
        int g = gi;
        if constexpr (LIST) { g = p.list[gi]; g = g < 0 ? 0 : (g >= p.nseg ? p.nseg - 1 : g); }   // (an entry is a segment of this plane whatever the buffer holds)
        const int part = g / ncols, col = g - part * ncols;
        const int b = col / p.tx, x0 = (col - b * p.tx) * 26;
        const int y0 = part * p.rs, y1 = (y0 + p.rs < H) ? y0 + p.rs : H;
        const lama_buf_t xres = LAMA_BUF_RSRC(reinterpret_cast<const char*>(p.x) + (long long)b * p.x_bstride * ESI, (HEAD_ABL & 2) ? 0ll : (long long)p.C * HW * ESI);
        const lama_buf_t yres = LAMA_BUF_RSRC(p.y + (long long)b * p.y_bstride, (long long)p.M * HW * 4);
        // this lane's input column X' = x0 - 3 + l31 (reflected) and channel plane
        int ix = x0 - 3 + l31;
        ix = ix < 0 ? -ix : ix;
        ix = ix >= W ? 2 * (W - 1) - ix : ix;
        ix = ix < 0 ? 0 : (ix >= W ? W - 1 : ix);               // columns of a ragged last segment that no stored pixel uses
        // LIST: what this segment may read is its output rectangle grown by 3 and clamped to the plane -- all the list build closes over.  The
        // columns / rows that stored pixels use lie inside it (reflection included); the lanes of a ragged last segment and the rows of a ragged
        // last part that feed no stored pixel would reflect out of it (W % 26 in 1..13: columns left of x0 - 3), into tiles nobody wrote, and
        // what they load passes the range watch: keep them inside.
        const int rx0 = x0 - 3 < 0 ? 0 : x0 - 3, rx1 = (x0 + 26 < W ? x0 + 26 : W) + 2 < W ? (x0 + 26 < W ? x0 + 26 : W) + 2 : W - 1;
        const int ry0 = y0 - 3 < 0 ? 0 : y0 - 3, ry1 = y1 + 2 < H ? y1 + 2 : H - 1;
        if constexpr (LIST) ix = ix < rx0 ? rx0 : (ix > rx1 ? rx1 : ix);
        const int coloff = ((16 * q + 8 * khalf) * HW + ix) * ESI;
        auto row_off = [&](int u) {                             // virtual row u (may be outside the image) -> byte offset of the input row
            int iy = u < 0 ? -u : u;
            iy = iy >= H ? 2 * (H - 1) - iy : iy;
            iy = iy < 0 ? 0 : (iy >= H ? H - 1 : iy);
            if constexpr (LIST) iy = iy < ry0 ? ry0 : (iy > ry1 ? ry1 : iy);
            return iy * W * ESI;
        };
        // register ring: slot (u - (y0 - 3)) % HEAD_R holds virtual row u of this lane's 8 channels, first as the 8 requested
        // floats, from the row that needs it on as (hi[4], lo[4]) halves
        unsigned ring[HEAD_R][8];
        auto request = [&](int u, auto slot_tag) {
            constexpr int SL = decltype(slot_tag)::value;
            const int ro = row_off(u);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if constexpr (HI) ring[SL][e] = (unsigned)LAMA_BUF_LOAD_B16(xres, coloff, ro + e * HW * ESI);
                else ring[SL][e] = LAMA_BUF_LOAD_B32(xres, coloff, ro + e * HW * ESI);
            }
        };
        auto convert = [&](auto slot_tag) {   // 8 floats -> hi halves in ring[][0..3], lo halves in ring[][4..7]
            constexpr int SL = decltype(slot_tag)::value;
            unsigned hh[4], ll[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (HI) { hh[e] = ring[SL][2 * e] | (ring[SL][2 * e + 1] << 16); cb_range_watch(hh[e], rw); ll[e] = 0u; }
                else cb_split2(__builtin_bit_cast(float, ring[SL][2 * e]), __builtin_bit_cast(float, ring[SL][2 * e + 1]), hh[e], ll[e], rw);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) { ring[SL][e] = hh[e]; ring[SL][4 + e] = ll[e]; }
        };
        // rows y0 - 3 .. y0 + 2 of the first window converted, rows y0 + 3 .. y0 + 2 + HEAD_D in flight
        request(y0 - 3, CbTag<0>{}); request(y0 - 2, CbTag<1>{}); request(y0 - 1, CbTag<2>{}); request(y0, CbTag<3>{});
        request(y0 + 1, CbTag<4>{}); request(y0 + 2, CbTag<5>{}); request(y0 + 3, CbTag<6>{});
        static_assert(HEAD_D == 1, "prologue requests rows y0 - 3 .. y0 + 2 + HEAD_D");
        convert(CbTag<0>{}); convert(CbTag<1>{}); convert(CbTag<2>{}); convert(CbTag<3>{}); convert(CbTag<4>{}); convert(CbTag<5>{});

        // one output row; J = (Y - y0) % HEAD_R is compile-time: virtual row Y + ky - 3 sits in slot (J + ky) % HEAD_R
        auto row = [&](int Y, auto j_tag) {
            constexpr int J = decltype(j_tag)::value;
            // HEAD_LATE: the row requested HEAD_D output rows ago (virtual row Y + 3) is the LAST tap of this output row: the six taps whose
            // rows are already converted run first, so the request has most of another row's MFMAs (three waves per SIMD: ~1 us) to come back
            // from HBM before its wait -- a deeper ring does not fit the 168 registers of three waves per SIMD (HEAD_D = 2 spills 11)
            if constexpr (!HEAD_LATE) convert(CbTag<(J + 6) % HEAD_R>{});  // virtual row Y + 3, requested HEAD_D rows ago
            request(Y + 3 + HEAD_D, CbTag<(J + HEAD_R - 1) % HEAD_R>{});   // into the slot of virtual row Y - 4
            __builtin_amdgcn_sched_barrier(0);
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int ky = 0; ky < 7; ++ky) {
                const int SL = (J + ky) % HEAD_R;   // compile-time after unrolling
                if constexpr (HEAD_LATE) {
                    if (ky == 6) {
                        __builtin_amdgcn_sched_barrier(0);
                        convert(CbTag<(J + 6) % HEAD_R>{});
                    }
                }
                const bf16x8 bh = __builtin_bit_cast(bf16x8, u32x4{ring[SL][0], ring[SL][1], ring[SL][2], ring[SL][3]});
                const bf16x8 bl = __builtin_bit_cast(bf16x8, u32x4{ring[SL][4], ring[SL][5], ring[SL][6], ring[SL][7]});
                if constexpr (HEAD_ABL & 1) { LAMA_KEEP_LIVE(bh); LAMA_KEEP_LIVE(bl); acc[ky] += 1.0f; }
                else {
                    acc = CB_MFMA(__builtin_bit_cast(bf16x8, ah[ky]), bh, acc, 0, 0, 0);
                    if constexpr (!HI) acc = CB_MFMA(__builtin_bit_cast(bf16x8, ah[ky]), bl, acc, 0, 0, 0);
                    if constexpr (ALO) acc = CB_MFMA(__builtin_bit_cast(bf16x8, al[ky]), bh, acc, 0, 0, 0);
                }
            }
            // partial z of this channel group -> LDS buffer (Y - y0) & 1: rows m' = (r & 3) + 8 (r >> 2) + 4 khalf < 28, column l31
            float* zb = zlds + ((Y - y0) & 1) * HEAD_ZBUF + q * (HEAD_ZR * HEAD_ZP);
            if constexpr (HEAD_ABL & 8) { LAMA_KEEP_LIVE(acc); }
            else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = (r & 3) + 8 * (r >> 2) + 4 * khalf;
                    if (m < HEAD_ZR) zb[m * HEAD_ZP + l31] = acc[r];
                }
                __syncthreads();
            }
            // y[o][Y][x0 + j] = sum over channel groups and kx of z[o * 7 + kx][j + kx]  (z column index = X' - (x0 - 3))
            if (finisher && !(HEAD_ABL & 4)) {   // waves 0 and 1 only (26 M <= 104 threads)
                const float* zr = zlds + ((Y - y0) & 1) * HEAD_ZBUF + fo * 7 * HEAD_ZP + fj;
                float v = fbias;
#pragma unroll
                for (int qq = 0; qq < 4; ++qq)
#pragma unroll
                    for (int kx = 0; kx < 7; ++kx) v += zr[qq * (HEAD_ZR * HEAD_ZP) + kx * HEAD_ZP + kx];
                if (p.act == LAMA_ACT_RELU) v = fmaxf(v, 0.0f);
                else if (p.act == LAMA_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
                else if (p.act == LAMA_ACT_TANH) v = tanhf(v);
                const int X = x0 + fj;
                const int eo = (X < W && Y < y1) ? (fo * HW + Y * W + X) * 4 : 0x7ffffff0;
                LAMA_BUF_STORE_B32(yres, __builtin_bit_cast(unsigned, v), eo, 0);
            }
        };
#pragma unroll 1
        for (int Y = y0; Y < y1; Y += HEAD_R) {                 // rs is a multiple of HEAD_R; rows past y1 are computed and dropped
            row(Y + 0, CbTag<0>{}); row(Y + 1, CbTag<1>{}); row(Y + 2, CbTag<2>{}); row(Y + 3, CbTag<3>{});
            row(Y + 4, CbTag<4>{}); row(Y + 5, CbTag<5>{}); row(Y + 6, CbTag<6>{}); row(Y + 7, CbTag<7>{});
        }
        static_assert(HEAD_R == 8, "row loop unrolled by HEAD_R");
        __syncthreads();   // the last row's finishers read buffer 0 / 1 while the next part would already write into it
    }
    cb_range_report(rw, p.range_flag);
}
