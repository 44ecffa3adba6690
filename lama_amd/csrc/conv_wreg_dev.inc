// "Weights in registers" variant of the 3-term split convolution (included by conv_split3.inc, device part).
//
// The LDS-staged kernel above moves BOTH GEMM operands through LDS; at the bottleneck shapes of the generator (3x3 / 1x1,
// stride 1, 128-384 output channels over 64x64 planes) its LDS pipe (fragment reads + ds_write of the weight stages) is as busy
// as the matrix cores.  Here the packed weights -- already stored in MFMA A-fragment order,
// [k-step][32-row fragment][hi|lo][lane][8 halves] -- never touch LDS: every wave owns ONE 32-row fragment and loads its
// (hi, lo) A operands straight from L2 into registers (two fully coalesced 1-KiB buffer loads per k-step, a RING of k-steps
// ahead), and covers 128 pixels (4 B fragments, 4 accumulators), so one A fragment feeds 12 MFMAs and the only LDS traffic
// is the 8 ds_read_b128 of the B fragments per 12 MFMAs (the activation patch: fp32 -> (hi, lo) split once, 9x tap reuse).
//
//   workgroup = WMV M-waves x KG K-groups; output tile 32*WMV channels x 128 pixels (TH x TW rectangle):
//     <4, 2>  512 threads: 128 channels; the two K-groups split every channel chunk between them (3x3: 32-channel chunks, group g
//             takes channels 16g..16g+15 with all 9 taps; 1x1: 64-channel chunks, group g takes k-steps 2g, 2g+1) -> two waves
//             per SIMD although a batch of 8 x 64 x 64 pixels x 128 channels has only four 32x32 accumulator fragments per
//             SIMD; the partial sums meet in the epilogue through LDS, each group storing half of the tile;
//     <4, 1>  256 threads, TWO workgroups per CU (the stride-2 downsampling convs: short K loops, many tiles): every wave walks all of K
//             over 16-channel chunks, no K-group exchange; the two resident workgroups run out of phase, so the prologue (first patch
//             from HBM), the staging and the store tail of one sit under the MFMAs of the other;
//     <12, 1> 768 threads: all 384 channels of the global branch in ONE workgroup per pixel tile (three waves per SIMD, the patch
//             is staged once instead of once per 128-channel tile, one launch round on 256 CUs);
//   Patch staging as in the LDS-staged kernel (unit = 8 channels of one pixel, two units per thread and chunk, loaded one
//   chunk or two chunks ahead); ONE barrier per chunk; no branch inside a chunk (out-of-range buffer loads return 0).
//   Every request for the following k-steps is slotted into the shadow of one of the current k-step's MFMAs
//   (sched_group_barrier), so a wave never has a pure memory phase.

template <int T, int KSC, int WMV, int KG>
struct CwShape {
    static_assert((T == 9 && (KSC == 2 || (KSC == 1 && KG == 1))) || (T == 1 && KSC == 4),
                  "3x3 over 32-channel chunks (16-channel chunks in the 4 x 1 geometry) or 1x1 over 64-channel chunks");
    static_assert(KG == 1 || KG == 2, "K-groups");
    static constexpr int THREADS = 64 * WMV * KG;
    static constexpr int NKG = T * KSC / KG;                   // k-steps per wave and chunk: 9 / 18 (3x3), 2 / 4 (1x1)
    static constexpr int WPS = WMV * KG / 4;                   // waves per SIMD
    // chunks the patch loads run ahead: a 1x1 chunk of a K-split workgroup is too short to cover the HBM latency
    static constexpr int PFD = (T == 1 && KG == 2) ? 2 : 1;
    // A-operand register ring (k-steps); loads run RING-1 k-steps ahead
    // 3x3 at two waves per SIMD (256 registers): a ring of a whole chunk (9 k-steps).  vmcnt retires in order, so waiting for an
    // A fragment (L2) also waits for every patch load (HBM) requested before it: with the A requests 8 k-steps ahead, the only
    // A fragment that was requested behind a chunk's patch loads is the one needed at that chunk's last k-step, where the patch is
    // needed anyway (ring of 3: the wait at k-step 2 gave the patch loads two k-steps to come back from HBM)
#ifndef LAMA_CW_RING9
#define LAMA_CW_RING9 0   // measured on MI355X: no gain (convA 105.8 -> 104.3 us in isolation, end to end flat) for 44 more VGPRs
#endif
    // (the experimental one-wave-per-SIMD local conv, <9, 2, 4, 1>, has nobody to cover a late A fragment: a ring of six k-steps -- nine spill)
    static constexpr int RING = (T == 9) ? ((LAMA_CW_RING9 && KG == 2 && WPS <= 2) ? 9 : ((KSC == 2 && WMV == 4 && KG == 1) ? 6 : 3)) : ((WPS >= 3) ? 2 : 4);
    // two B fragment sets (next k-step's reads under this k-step's MFMAs) while the register budget allows: 3 waves per SIMD
    // leave 168 VGPRs and hide the LDS latency behind the other two waves instead
    static constexpr bool BDB = WPS <= 2;
    static constexpr int NOCT = 2 * KSC;                       // channel octets per chunk
    static_assert((PFD * NKG) % RING == 0, "ring slot must be a compile-time function of the unrolled position");
};

struct CwFrag {
    bf16x8 bh[4], bl[4];
};

// ABL: timing-only ablations for the profiling tools (LAMA_CW_ABLATE; results are WRONG for ABL != 0): bit 0 = no A loads in
// the loop, bit 1 = no B fragment reads in the loop, bit 2 = no patch staging in the loop, bit 3 = no MFMA, bit 4 = patch loads
// but no LDS writes, bit 5 = LDS writes but no patch loads, bit 6 = (results stay correct) thread 0 of every workgroup writes a
// timeline (100 MHz ticks: start, after the prologue barrier, after every chunk barrier, end) to the buffer in trace
// HF: LAMA_PREC_F16 (f16 back end only) -- ONE MFMA per (A, B) fragment pair instead of three: no lo planes in LDS, no lo weights in
// registers.  HI: this segment's input tensor is fp16 (LAMA_DT_F16: the element is its own hi part, no conversion); with HF && !HI
// the input is fp32 (the residual stream of the resnet blocks stays fp32) and is rounded to its hi part while it is staged.
// ROLL (3x3 with 32-pixel-wide tile rows, i.e. pixel fragment j = tile row j): tap (ky, kx) of fragment j reads patch row j + ky
// shifted by kx, so the k-steps are walked kx-major and the SIX patch rows of one (16-channel group, kx) are read once for the three
// ky taps: 12 ds_read_b128 per 36 MFMAs instead of 24 (the fragment reads of 8 waves kept the LDS pipe 2/3 as busy as the matrix
// cores).  Eight row slots: rows 0, 1, 4, 5 have fixed slots, rows 2, 3 alternate between two pairs from one (group, kx) set to the
// next, so that the next set's rows 0..3 are requested while the current set's ky = 1, 2 taps still run on rows 1..5.
// NU: staging units (8 channels of one patch pixel) per thread and chunk -- 2 for the stride-1 tiles, 5 for the (2 TH + 1) x (2 TW + 1)
// patch of a stride-2 3x3 (columns parity-split in LDS, so that the B fragments of every tap stay 32 consecutive 16-byte slots)
// XS: this segment's input tensor is LAMA_DT_SPLIT16 (3-term split only): the producer stored the (hi, lo) parts in staging order, per image
// [channel octet][hi | lo][H][W][8 halves], so a unit is two 16-byte buffer loads and two 16-byte LDS writes -- no conversion, no split, no range
// watch (the producer watched what it stored); padding, the parity split of the columns and the dump slot are untouched, and the LDS image is
// the one the fp32 form gives bit for bit.
template <int T, int KSC, int WMV, int KG, int ABL = 0, int SCH = 2, bool HF = false, bool HI = HF, bool ROLL = false, int NU = 2, bool XS = false>
__device__ __forceinline__ void cw_segment(const CbSeg& s, int F, int b, int gy0, int gx0, int TWlog, char* pbuf0, int pbytes,
                                           f32x16 (&acc)[4], unsigned& rw, long long* trace = nullptr) {
    using S = CwShape<T, KSC, WMV, KG>;
    // (measured, round 4: the stride-2 convs with their patch requests TWO chunks ahead -- 80 staging registers -- run 1.5x slower:
    // profiles/r04_ab_down_pfd2.txt)
    constexpr int NKG = S::NKG, PFD = S::PFD, RING = S::RING, NOCT = S::NOCT, D = RING - 1, THREADS = S::THREADS;
    constexpr bool BDB = S::BDB;
    constexpr int BKC = 16 * KSC;
    constexpr int ES = HI ? 2 : 4;   // bytes per activation element
    static_assert(!XS || (!HF && !HI), "pre-split input: the 3-term split precisions only");
    constexpr int NLD = XS ? 2 * NU : 8 * NU;   // patch requests per thread and chunk
    const int tid = threadIdx.x, lane = tid & 63, wave = LAMA_WAVE_UNIFORM(tid >> 6);
    const int kg = KG == 1 ? 0 : wave / WMV;
    const int khalf = lane >> 5, l31 = lane & 31;
    const int TW = 1 << TWlog;
    const int HW = s.H * s.W;
    const int NPR = s.PH * s.PW;
    const int nunits = NPR * NOCT;
    const int pdump = NOCT * s.npix * 16;            // 16-byte dump slot behind the hi planes (and behind the lo planes)
    const int plo = pdump + 16;                      // byte offset of the lo planes inside a patch buffer
    const int nchunk = s.C / BKC;                    // the host only takes this path when C is a multiple of the chunk

    // staging units of this thread: (patch pixel, channel octet) -> element offset inside a chunk, LDS byte offset
    int ubase[NU], lds_off[NU], uvalid[NU];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const int u = i * THREADS + tid;
        int so = 0, lo = pdump, ok = 0, q = 0;   // threads without a unit write zeros to the dump slot: no branch in the loop
        if (u < nunits) {
            q = u / NPR;
            const int pp = u - q * NPR;
            const int py = pp / s.PW, px = pp - py * s.PW;
            const int iy = cb_src_coord(gy0 * s.stride + s.dy0 + py, s.H, s.pad_mode);
            const int ix = cb_src_coord(gx0 * s.stride + s.dx0 + px, s.W, s.pad_mode);
            if (iy >= 0 && ix >= 0) { so = iy * s.W + ix; ok = 1; }
            lo = (q * s.npix + py * s.PWs + (s.PWh ? (px & 1) * s.PWh + (px >> 1) : px)) * 16;
        }
        // byte offset inside a chunk; always in bounds (zero padding is applied at write time).  XS: the hi plane of octet q, the lo plane HW * 16 behind
        ubase[i] = XS ? (q * 2 * HW + so) * 16 : (q * 8 * HW + so) * ES;
        lds_off[i] = lo;
        uvalid[i] = ok;
    }
    // one buffer resource per image: lane offset = unit, scalar offset = (chunk, channel) -> no per-element address registers
    const lama_buf_t xres = LAMA_BUF_RSRC(reinterpret_cast<const char*>(s.x) + (long long)b * s.bstride * ES, (long long)s.C * HW * ES);
    float preg[PFD][NU][8];   // HF: the raw 16-bit patterns (zero-extended)
    auto load_units = [&](int ch, auto slot_tag) {
        constexpr int SL = decltype(slot_tag)::value;
        if constexpr (XS) {   // a chunk is BKC channels = BKC / 8 octets of 2 * HW * 16 bytes = the same BKC * HW * 4 bytes as in fp32
#pragma unroll
            for (int hl = 0; hl < 2; ++hl)
#pragma unroll
                for (int i = 0; i < NU; ++i) {
                    const u32x4 v = __builtin_bit_cast(u32x4, LAMA_BUF_LOAD_B128(xres, ubase[i], ch * BKC * HW * 4 + hl * HW * 16));
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned ve = v[e];   // (a named scalar: __builtin_bit_cast of the vector ELEMENT expression reads element 0 for every e)
                        preg[SL][i][4 * hl + e] = __builtin_bit_cast(float, ve);
                    }
                }
            return;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int so = (ch * BKC + e) * HW * ES;
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                if constexpr (HI) preg[SL][i][e] = __builtin_bit_cast(float, (unsigned)LAMA_BUF_LOAD_B16(xres, ubase[i], so));
                else preg[SL][i][e] = __builtin_bit_cast(float, LAMA_BUF_LOAD_B32(xres, ubase[i], so));
            }
        }
    };
    auto write_units = [&](char* pb, auto slot_tag) {
        constexpr int SL = decltype(slot_tag)::value;
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            unsigned hh[4], ll[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (XS) {
                    hh[e] = __builtin_bit_cast(unsigned, preg[SL][i][e]);
                    ll[e] = __builtin_bit_cast(unsigned, preg[SL][i][4 + e]);
                } else if constexpr (HI) {
                    hh[e] = __builtin_bit_cast(unsigned, preg[SL][i][2 * e]) | (__builtin_bit_cast(unsigned, preg[SL][i][2 * e + 1]) << 16);
                    cb_range_watch(hh[e], rw);
                    ll[e] = 0u;
                } else if constexpr (HF) {   // fp32 input, hi part only
                    f32x2 v2 = {preg[SL][i][2 * e], preg[SL][i][2 * e + 1]};
                    hh[e] = __builtin_bit_cast(unsigned, __builtin_convertvector(v2, bf16x2));
                    cb_range_watch(hh[e], rw);
                    ll[e] = 0u;
                } else cb_split2(preg[SL][i][2 * e], preg[SL][i][2 * e + 1], hh[e], ll[e], rw);
            }
            u32x4 h = {hh[0], hh[1], hh[2], hh[3]}, l = {ll[0], ll[1], ll[2], ll[3]};
            if (!uvalid[i]) { h = u32x4{0, 0, 0, 0}; l = h; }
            *reinterpret_cast<u32x4*>(pb + lds_off[i]) = h;
            if constexpr (!HF) *reinterpret_cast<u32x4*>(pb + plo + lds_off[i]) = l;
        }
    };

    // k-step kk of a chunk (compile time) -> 16-channel group inside the chunk
    auto c16_of = [&](int kk) { return T == 9 ? (KG == 2 ? kg : kk / 9) : (KG == 2 ? 2 * kg + kk : kk); };
    // B fragments: pixel n = j*32 + (lane & 31) of the tile, octet plane 2 * c16 + khalf (the K-group part of c16 is in boff)
    int boff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = j * 32 + l31;
        const int ty = n >> TWlog, tx = n & (TW - 1);
        boff[j] = (((KG == 2 ? (T == 9 ? 2 * kg : 4 * kg) : 0) + khalf) * s.npix + ty * s.stride * s.PWs + tx) * 16;
    }
    int tgoff[T];
#pragma unroll
    for (int t = 0; t < T; ++t) tgoff[t] = s.tapoff[t] * 16;
    auto read_bj = [&](CwFrag& f, const char* pb, int kk, int j, bool hi, bool lo) {
        const int koct = T == 9 ? (KG == 2 ? 0 : kk / 9) : kk;   // 16-channel group of this k-step beyond the K-group part
        const char* bp = pb + tgoff[T == 1 ? 0 : kk % T] + koct * 2 * s.npix * 16 + boff[j];
        if (hi) f.bh[j] = *reinterpret_cast<const bf16x8*>(bp);
        if constexpr (!HF) { if (lo) f.bl[j] = *reinterpret_cast<const bf16x8*>(bp + plo); }
    };
    auto read_b = [&](CwFrag& f, const char* pb, int kk) {
#pragma unroll
        for (int j = 0; j < 4; ++j) read_bj(f, pb, kk, j, true, true);
    };

    // A operands: packed k-step q of fragment F = 2 KiB at (q * mft + F) * 2048: [hi | lo][lane][8 halves]
    const int kbytes = s.mft * 2048;
    const lama_buf_t wres = LAMA_BUF_RSRC(s.w, (long long)(s.C / 16) * T * kbytes);
    const int aoff = F * 2048 + lane * 16;
    constexpr bool ALO = !HF || CB_HF_W2;               // the lo weights are loaded (3-term split, or the two-product fp16 path)
    u32x4 ah[RING], al[ALO ? RING : 1];
    // ROLL walks the taps kx-major: position s of a 9-k-step group is tap (ky, kx) = (s % 3, s / 3) = packed tap ky * 3 + kx
    auto tap_of = [&](int sx) { return ROLL ? (sx % 3) * 3 + sx / 3 : sx; };
    auto kstep_q = [&](int c, int kk) { return (T == 9) ? (KSC * c + c16_of(kk)) * 9 + tap_of(kk % 9) : 4 * c + c16_of(kk); };
    auto load_a = [&](int R, int q) {   // R is a compile-time constant at every (unrolled) call site
        ah[R] = __builtin_bit_cast(u32x4, LAMA_BUF_LOAD_B128(wres, aoff, q * kbytes));
        if constexpr (ALO) al[R] = __builtin_bit_cast(u32x4, LAMA_BUF_LOAD_B128(wres, aoff + 1024, q * kbytes));
    };

    // prologue: chunk 0's patch in LDS, the first RING-1 k-steps of A and (PFD = 2) chunk 1's units in flight
    load_units(0, CbTag<0>{});
#pragma unroll
    for (int i = 0; i < D; ++i) load_a(i, kstep_q(i / NKG, i % NKG));
    write_units(pbuf0, CbTag<0>{});
    if constexpr (PFD == 2) load_units(1, CbTag<1>{});
    __syncthreads();
    if constexpr (ABL & 64) { if (threadIdx.x == 0) trace[1] = LAMA_CLOCK(); }

    auto chunk = [&](int c, auto slot_tag) {
        constexpr int SLOT = decltype(slot_tag)::value;
        const char* pb = pbuf0 + (c & 1) * pbytes;
        char* pbn = pbuf0 + ((c + 1) & 1) * pbytes;
        CwFrag fr[BDB ? 2 : 1];
        read_b(fr[0], pb, 0);
        auto kstep = [&](auto kk_tag) {
            constexpr int kk = decltype(kk_tag)::value;
            constexpr int RS = (SLOT * NKG + kk) % RING;          // ring slot of this k-step
            constexpr int CUR = BDB ? (kk & 1) : 0, NXT = BDB ? ((kk + 1) & 1) : 0;
            if constexpr (SCH == 2) __builtin_amdgcn_sched_barrier(0);
            // past the last chunk / k-step the buffer loads are out of range and return 0: no branches in the chunk body
            constexpr bool LDU = !(ABL & 4) && !(ABL & 32) && kk == 0;
            constexpr bool WRU = !(ABL & 4) && !(ABL & 16) && kk == NKG - 1;
            constexpr bool RDB = (kk + 1 < NKG) && !(ABL & 2);
            if constexpr (LDU) load_units(c + PFD, CbTag<SLOT>{});
            if constexpr (!(ABL & 1)) {   // A operands RING-1 k-steps ahead (into the slot the previous k-step just released)
                constexpr int n2 = kk + D;
                load_a((RS + D) % RING, kstep_q(c + n2 / NKG, n2 % NKG));
            }
            if constexpr (BDB && kk + 1 < NKG) {
                if constexpr (ABL & 2) fr[NXT] = fr[CUR];
                else read_b(fr[NXT], pb, kk + 1);
            }
            if constexpr ((ABL & 16) && kk == NKG - 1) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
#pragma unroll
                    for (int i = 0; i < NU; ++i) LAMA_KEEP_LIVE(preg[0][i][e]);
            }
            if constexpr (WRU) write_units(pbn, CbTag<(SLOT + 1) % PFD>{});
            // SCH 1: two phases per k-step (requests for the following k-steps, then this k-step's MFMAs);
            // SCH 2: one scheduling region per k-step with every request slotted into the shadow of one of its MFMAs
            if constexpr (SCH == 1) __builtin_amdgcn_sched_barrier(0);
            const bf16x8 a_hi = __builtin_bit_cast(bf16x8, ah[RS]), a_lo = __builtin_bit_cast(bf16x8, al[ALO ? RS : 0]);
            CwFrag& f = fr[CUR];
            if constexpr (HF) {
                if constexpr (CB_HF_W2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = CB_MFMA(a_hi, f.bh[j], acc[j], 0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[j] = CB_MFMA(CB_HF_W2 ? a_lo : a_hi, f.bh[j], acc[j], 0, 0, 0);
                    if constexpr (!BDB && RDB) read_bj(f, pb, kk + 1, j, true, false);
                }
            } else if constexpr (ABL & 8) {
                LAMA_KEEP_LIVE(a_hi); LAMA_KEEP_LIVE(a_lo);
#pragma unroll
                for (int j = 0; j < 4; ++j) { LAMA_KEEP_LIVE(f.bh[j]); LAMA_KEEP_LIVE(f.bl[j]); }
            } else if constexpr (BDB) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = CB_MFMA(a_hi, f.bh[j], acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = CB_MFMA(a_hi, f.bl[j], acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = CB_MFMA(a_lo, f.bh[j], acc[j], 0, 0, 0);
            } else {
                // one fragment set: the lo fragments are released by the second product, the hi fragments by the third; the next
                // k-step's fragment j is requested right behind the MFMA that read the old one for the last time
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = CB_MFMA(a_hi, f.bh[j], acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[j] = CB_MFMA(a_hi, f.bl[j], acc[j], 0, 0, 0);
                    if constexpr (RDB) read_bj(f, pb, kk + 1, j, false, true);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[j] = CB_MFMA(a_lo, f.bh[j], acc[j], 0, 0, 0);
                    if constexpr (RDB) read_bj(f, pb, kk + 1, j, true, false);
                }
            }
            if constexpr (SCH == 1) __builtin_amdgcn_sched_barrier(0);
            if constexpr (SCH == 2 && !(ABL & 8) && !HF) {
                constexpr int NVM = ((ABL & 1) ? 0 : 2) + (LDU ? NLD : 0);                    // VMEM reads of this region
                auto grp = [&](auto i_tag) {
                    constexpr int i = decltype(i_tag)::value;
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                     // MFMA
                    if constexpr (BDB) {
                        if constexpr (RDB && i < 8) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // DS read
                        constexpr int nv = (i >= 8) ? (NVM + 11 - i) / 4 : 0;                              // VMEM reads behind the last four
                        if constexpr (nv > 0) __builtin_amdgcn_sched_group_barrier(0x020, nv, 0);
                        if constexpr (WRU && i >= 8) __builtin_amdgcn_sched_group_barrier(0x200, (2 * NU + 11 - i) / 4, 0);   // DS writes
                    } else {
                        constexpr int nv = (i < 4) ? (NVM + 3 - i) / 4 : 0;                                // VMEM reads behind the first four
                        if constexpr (nv > 0) __builtin_amdgcn_sched_group_barrier(0x020, nv, 0);
                        if constexpr (WRU && i < 4) __builtin_amdgcn_sched_group_barrier(0x200, (2 * NU + 3 - i) / 4, 0);     // DS writes
                        if constexpr (RDB && i >= 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);    // DS read (program order)
                    }
                };
                grp(CbTag<0>{}); grp(CbTag<1>{}); grp(CbTag<2>{}); grp(CbTag<3>{}); grp(CbTag<4>{}); grp(CbTag<5>{});
                grp(CbTag<6>{}); grp(CbTag<7>{}); grp(CbTag<8>{}); grp(CbTag<9>{}); grp(CbTag<10>{}); grp(CbTag<11>{});
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        static_assert(NKG == 2 || NKG == 4 || NKG == 9 || NKG == 18, "k-steps per chunk");
        kstep(CbTag<0>{});
        kstep(CbTag<1>{});
        if constexpr (NKG > 2) { kstep(CbTag<2>{}); kstep(CbTag<3>{}); }
        if constexpr (NKG > 4) {
            kstep(CbTag<4>{}); kstep(CbTag<5>{}); kstep(CbTag<6>{}); kstep(CbTag<7>{}); kstep(CbTag<8>{});
        }
        if constexpr (NKG > 9) {
            kstep(CbTag<9>{}); kstep(CbTag<10>{}); kstep(CbTag<11>{}); kstep(CbTag<12>{}); kstep(CbTag<13>{}); kstep(CbTag<14>{});
            kstep(CbTag<15>{}); kstep(CbTag<16>{}); kstep(CbTag<17>{});
        }
        __syncthreads();
        if constexpr (ABL & 64) { if (threadIdx.x == 0 && c < 28) trace[2 + c] = LAMA_CLOCK(); }
    };
    struct CwRow { bf16x8 h, l; };
    [[maybe_unused]] int rowoff[6];
    if constexpr (ROLL) {
#pragma unroll
        for (int r = 0; r < 6; ++r) rowoff[r] = (((KG == 2 ? 2 * kg : 0) + khalf) * s.npix + r * s.PWs + l31) * 16;
    }
    [[maybe_unused]] auto read_row = [&](CwRow& d, const char* pb, int g, int kx, int r) {
        const char* bp = pb + (g * 2 * s.npix + kx) * 16 + rowoff[r];
        d.h = *reinterpret_cast<const bf16x8*>(bp);
        if constexpr (!HF) d.l = *reinterpret_cast<const bf16x8*>(bp + plo);
    };
    [[maybe_unused]] auto chunk_roll = [&](int c, auto) {   // generic: only instantiated for ROLL
        static_assert(!ROLL || (T == 9 && PFD == 1 && NKG % 9 == 0), "ROLL: 3x3 only");
        const char* pb = pbuf0 + (c & 1) * pbytes;
        char* pbn = pbuf0 + ((c + 1) & 1) * pbytes;
        constexpr int NSET = NKG / 3;
        CwRow rows[8];
        [[maybe_unused]] long long tks[NKG + 1];   // ABL & 64: shader-clock stamp of every k-step of chunk 8 (wave 0)
#pragma unroll
        for (int r = 0; r < 4; ++r) read_row(rows[r], pb, 0, 0, r);
        auto kstep = [&](auto kk_tag) {
            constexpr int kk = decltype(kk_tag)::value;
            constexpr int g = kk / 9, kx = (kk % 9) / 3, ky = kk % 3, si = kk / 3, par = si & 1;
            constexpr int RS = kk % RING;
            constexpr bool more = si + 1 < NSET;
            constexpr int gn = (3 * (si + 1)) / 9, kxn = ((3 * (si + 1)) % 9) / 3;    // the next set
            constexpr int S2 = par ? 6 : 2, S3 = par ? 7 : 3, S2n = par ? 2 : 6, S3n = par ? 3 : 7;   // slots of rows 2, 3 (this set, next set)
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (ABL & 64) { if (c == 8 && wave == 0) tks[kk] = LAMA_CYCLES(); }
            constexpr bool LDU = !(ABL & 4) && !(ABL & 32) && kk == 0;
            constexpr bool WRU = !(ABL & 4) && !(ABL & 16) && kk == NKG - 1;
            constexpr int NDS = (ABL & 2) ? 0 : ((ky == 0 || more) ? (HF ? 2 : 4) : 0);
            if constexpr (LDU) load_units(c + PFD, CbTag<0>{});
            if constexpr (!(ABL & 1)) {
                constexpr int n2 = kk + D;
                load_a((RS + D) % RING, kstep_q(c + n2 / NKG, n2 % NKG));
            }
            if constexpr (NDS > 0) {
                if constexpr (ky == 0) { read_row(rows[4], pb, g, kx, 4); read_row(rows[5], pb, g, kx, 5); }
                else if constexpr (ky == 1) { read_row(rows[0], pb, gn, kxn, 0); read_row(rows[S2n], pb, gn, kxn, 2); }
                else { read_row(rows[1], pb, gn, kxn, 1); read_row(rows[S3n], pb, gn, kxn, 3); }
            }
            if constexpr ((ABL & 16) && kk == NKG - 1) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
#pragma unroll
                    for (int i = 0; i < NU; ++i) LAMA_KEEP_LIVE(preg[0][i][e]);
            }
            if constexpr (WRU) write_units(pbn, CbTag<0>{});
            const bf16x8 a_hi = __builtin_bit_cast(bf16x8, ah[RS]), a_lo = __builtin_bit_cast(bf16x8, al[ALO ? RS : 0]);
            auto slot = [&](int r) { return r == 2 ? S2 : (r == 3 ? S3 : r); };
            if constexpr (ABL & 8) {
                LAMA_KEEP_LIVE(a_hi); LAMA_KEEP_LIVE(a_lo);
#pragma unroll
                for (int j = 0; j < 4; ++j) { LAMA_KEEP_LIVE(rows[slot(ky + j)].h); LAMA_KEEP_LIVE(rows[slot(ky + j)].l); }
            } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = CB_MFMA(a_hi, rows[slot(ky + j)].h, acc[j], 0, 0, 0);
            }
            if constexpr (!HF && !(ABL & 8)) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = CB_MFMA(a_hi, rows[slot(ky + j)].l, acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = CB_MFMA(a_lo, rows[slot(ky + j)].h, acc[j], 0, 0, 0);
            } else if constexpr (HF && CB_HF_W2 && !(ABL & 8)) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = CB_MFMA(a_lo, rows[slot(ky + j)].h, acc[j], 0, 0, 0);
            }
            if constexpr (SCH == 2 && !HF && !(ABL & 8)) {
                constexpr int NVM = ((ABL & 1) ? 0 : 2) + (LDU ? NLD : 0);
                auto grp = [&](auto i_tag) {
                    constexpr int i = decltype(i_tag)::value;
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                     // MFMA
                    if constexpr (i < NDS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);              // DS read
                    constexpr int nv = (i >= 8) ? (NVM + 11 - i) / 4 : 0;                                  // VMEM reads behind the last four
                    if constexpr (nv > 0) __builtin_amdgcn_sched_group_barrier(0x020, nv, 0);
                    if constexpr (WRU && i >= 8) __builtin_amdgcn_sched_group_barrier(0x200, (2 * NU + 11 - i) / 4, 0);   // DS writes
                };
                grp(CbTag<0>{}); grp(CbTag<1>{}); grp(CbTag<2>{}); grp(CbTag<3>{}); grp(CbTag<4>{}); grp(CbTag<5>{});
                grp(CbTag<6>{}); grp(CbTag<7>{}); grp(CbTag<8>{}); grp(CbTag<9>{}); grp(CbTag<10>{}); grp(CbTag<11>{});
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        kstep(CbTag<0>{}); kstep(CbTag<1>{}); kstep(CbTag<2>{}); kstep(CbTag<3>{}); kstep(CbTag<4>{});
        kstep(CbTag<5>{}); kstep(CbTag<6>{}); kstep(CbTag<7>{}); kstep(CbTag<8>{});
        if constexpr (NKG > 9) {
            kstep(CbTag<9>{}); kstep(CbTag<10>{}); kstep(CbTag<11>{}); kstep(CbTag<12>{}); kstep(CbTag<13>{}); kstep(CbTag<14>{});
            kstep(CbTag<15>{}); kstep(CbTag<16>{}); kstep(CbTag<17>{});
        }
        if constexpr (ABL & 64) { if (c == 8 && wave == 0) tks[NKG] = LAMA_CYCLES(); }
        if constexpr (!(ABL & 128)) __syncthreads();   // bit 7: no barrier (timing only)
        if constexpr (ABL & 64) {
            if (threadIdx.x == 0 && c < 16) trace[2 + c] = LAMA_CLOCK();
            if (threadIdx.x == 0 && c == 8 && NKG == 9) {
#pragma unroll
                for (int i = 0; i <= NKG; ++i) trace[18 + i] = tks[i];
                trace[28] = LAMA_CYCLES();
            }
        }
    };
    if constexpr (ROLL) {
        for (int c = 0; c < nchunk; ++c) chunk_roll(c, CbTag<0>{});
    } else if constexpr (PFD == 1) {
        for (int c = 0; c < nchunk; ++c) chunk(c, CbTag<0>{});
    } else {
        for (int c = 0; c < nchunk; c += 2) {
            chunk(c, CbTag<0>{});
            if (c + 1 < nchunk) chunk(c + 1, CbTag<1>{});
        }
    }
}

// HF: LAMA_PREC_F16 (one product per MAC); HI1 / HI2 / HO: x, x2 and y / resid are fp16 (any mix: the resnet blocks keep their
// residual stream fp32 and everything else fp16)
template <int T1, int KSC1, int T2, int KSC2, int WMV = 4, int KG = 2, int ABL = 0, int SCH = 2, bool HF = false, bool HI1 = HF, bool HI2 = HF,
          bool HO = HF, bool ROLL = false, int NU = 2, bool FUSE1 = false, bool XS = false, bool YS = false>
__global__ __launch_bounds__(64 * WMV * KG, (WMV * KG == 4) ? 2 : 1) void CB_NAME(conv_wr_kernel)(CbParams p) {
    // XS / YS (the 4 x 1 stride-2 launch of the 3-term split): x / y is LAMA_DT_SPLIT16 -- cw_segment stages pre-split units, the epilogue
    // splits, watches and stores what the next stride-2 conv would otherwise split while it stages
    static_assert(!(XS || YS) || (KG == 1 && T2 == 0 && !HF && !HO && !FUSE1), "pre-split tensors: plain one-segment launches without K-groups");
    using AT = typename LamaAct<HO>::T;   // element type of resid / y
    const int L = lama_xcd_remap(blockIdx.x, gridDim.x);
    const int mt = L % p.MT;
    int tile = L / p.MT;
    const int tix = tile % p.tiles_x;
    tile /= p.tiles_x;
    const int tiy = tile % p.tiles_y;
    const int b = tile / p.tiles_y;
    const int TW = 1 << p.TWlog, TH = 128 >> p.TWlog;
    const int gy0 = tiy * TH, gx0 = tix * TW;
    const int tid = threadIdx.x, lane = tid & 63, wave = LAMA_WAVE_UNIFORM(tid >> 6);
    const int kg = wave / WMV, wm = wave % WMV;
    const int F = mt * WMV + wm;                                   // this wave's 32-row fragment
    const int Fc = F < p.s1.mft ? F : p.s1.mft - 1;               // past the last fragment: clamp (rows are never stored)

    long long* trace = nullptr;
    if constexpr (ABL & 64) {   // profiling tools only: 32 slots per workgroup (0 start, 1 prologue, 2.. chunks of segment 1, 9.. of segment 2, 30 end)
        trace = p.trace + (long long)blockIdx.x * 32;
        if (threadIdx.x == 0) trace[0] = LAMA_CLOCK();
    }
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

    unsigned rw = 0;   // range watch of the f16 split
    // ABL bit 8 (profiling tools, timing only, results WRONG): waves F >= 6 stream the weight fragments of wave F - 6 -- the SAME number of
    // requests per CU, half the distinct bytes from L2: what a 256-pixel tile shared by two half-row workgroups could gain at best (DESIGN.md 9.2)
    const int Fw = (ABL & 256) ? Fc % 6 : Fc;
    cw_segment<T1, KSC1, WMV, KG, (ABL & 255), SCH, HF, HI1, ROLL && T1 == 9, NU, XS>(p.s1, Fw, b, gy0, gx0, p.TWlog, lama_smem, p.pbytes, acc, rw, trace);
    if constexpr (T2 > 0) cw_segment<T2, KSC2, WMV, KG, (ABL & 65), SCH, HF, HI2>(p.s2, Fw, b, gy0, gx0, p.TWlog, lama_smem, p.pbytes, acc, rw, (ABL & 64) ? trace + 7 : nullptr);
    cb_range_report(rw, p.range_flag);

    const long long plane = (long long)p.Ho * p.Wo;
    // On gfx9 a store counts in vmcnt until L2 acknowledges it, so a load issued behind a store waits for that round trip: all
    // loads of a fragment (bias once per wave, then the 16 residual values) are issued BEFORE its 16 stores, with clamped
    // (always valid) addresses instead of branches.
    // Addresses: uniform 64-bit row base (scalar registers) + ONE 32-bit lane offset per fragment.
    const int khalf4 = 4 * (lane >> 5);
    const int kplane = khalf4 * (int)plane;
    auto row_u = [&](int r) { return F * 32 + (r & 3) + 8 * (r >> 2); };   // uniform part of row r of this wave's fragment
    float bv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bv[r] = p.bias ? p.bias[row_u(r) + khalf4 < p.M ? row_u(r) + khalf4 : p.M - 1] : 0.0f;
    constexpr int NRV = (WMV * KG / 4 >= 3) ? 1 : 2;   // residual value sets: one at three waves per SIMD (168 registers)
    float rv[NRV][16];
    auto frag_off = [&](int j, bool& pv) {
        const int n = j * 32 + (lane & 31);
        const int gy = gy0 + (n >> p.TWlog), gx = gx0 + (n & (TW - 1));
        pv = gy < p.GH && gx < p.GW;
        return (gy < p.GH ? gy : p.GH - 1) * p.Wo + (gx < p.GW ? gx : p.GW - 1);
    };
    auto load_resid = [&](int j, int slot) {   // residual values of pixel fragment j (zeros without a residual operand)
        bool pv;
        const int po = frag_off(j, pv);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mu = row_u(r), muc = mu < p.M ? mu : p.M - 1;   // rows past M: a valid address, never stored
            rv[slot][r] = p.resid ? (float)(reinterpret_cast<const AT*>(p.resid) + (long long)b * p.resid_bstride + (long long)muc * plane)[(unsigned)(po + (mu + khalf4 < p.M ? kplane : 0))] : 0.0f;
        }
    };
    auto store_frag = [&](int j, const f32x16& v16, int slot) {   // bias, activation, residual, store
        bool pv;
        const int po = frag_off(j, pv);
        const unsigned lo = (unsigned)(po + kplane);
        [[maybe_unused]] float vs[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mu = row_u(r);
            float v = v16[r] + bv[r];
            if (p.act == LAMA_ACT_RELU) v = fmaxf(v, 0.0f);
            else if (p.act == LAMA_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
            else if (p.act == LAMA_ACT_TANH) v = tanhf(v);
            v += rv[slot][r];
            if constexpr (YS) vs[r] = v;
            else if (pv && mu + khalf4 < p.M) (reinterpret_cast<AT*>(p.y) + (long long)b * p.y_bstride + (long long)mu * plane)[lo] = (AT)v;
        }
        if constexpr (YS) {
            // LAMA_DT_SPLIT16: registers 4 g .. 4 g + 3 are channels 4 khalf .. 4 khalf + 3 of octet 4 F + g -> 8 bytes of the pixel's hi slot and
            // 8 of its lo slot; the two half-waves fill the 16 bytes, 32 pixels of a tile row are 512 contiguous bytes per plane.  Split, THEN the
            // watch -- of what is stored and nothing else (lanes of a ragged tile outside the plane hold garbage) --, then plain vector stores.
            char* const yb = reinterpret_cast<char*>(p.y) + (long long)b * p.y_bstride * 4;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                unsigned h0, h1, l0, l1;
                cb_split2(vs[4 * g], vs[4 * g + 1], h0, l0);
                cb_split2(vs[4 * g + 2], vs[4 * g + 3], h1, l1);
                const int oct = F * 4 + g;
                if (pv && oct * 8 < p.M) {
                    cb_range_watch(h0, rw);
                    cb_range_watch(h1, rw);
                    char* const d = yb + ((long long)oct * 2 * plane + po) * 16 + 2 * khalf4;
                    *reinterpret_cast<u32x2*>(d) = u32x2{h0, h1};
                    *reinterpret_cast<u32x2*>(d + plane * 16) = u32x2{l0, l1};
                }
            }
        }
    };
    if constexpr (FUSE1) {
        // ------------------------------------------------------------------------------------------------------------------
        // Epilogue with SpectralTransform.conv1 of the NEXT layer (ffc.py:128-133,145: x1 = ReLU(BN(conv1x1 384 -> 192 (x_g)))).
        // This workgroup holds all 384 channels of its 128-pixel tile of the new x_g, and the matrix cores idle while the tile drains at
        // the HBM rate (17 us with every CU in the same phase): the 192 x 384 GEMM over exactly this tile runs here instead of as a
        // launch of its own.  Two passes of two pixel fragments: every wave finishes its fragments (bias, activation, residual, store --
        // as below), splits the results into (hi, lo) and leaves them in LDS as the B operands of ITS two k-steps (the accumulator
        // layout of a 32-row fragment IS the B layout of two 16-channel k-steps once conv1's input channels are packed in that order:
        // lama_conv2d_args.fuse1_w); then wave (F', g) = (wave % 6, wave / 6) multiplies row fragment F' of conv1 with k-steps
        // 12 g .. 12 g + 11 for both pixel fragments, the two K halves meet through LDS, and each wave finishes one fragment of x1.
        // ------------------------------------------------------------------------------------------------------------------
        static_assert(WMV == 12 && KG == 1 && !HF, "fused conv1: the 12 x 1 geometry of the 3-term split only");
        const int F1 = wave % 6, g1 = wave / 6;
        const lama_buf_t w1res = LAMA_BUF_RSRC(p.f1_w, (long long)24 * 6 * 2048);
        char* const lb = lama_smem;                                   // B operands: [k-step 24][pixel fragment 2][hi | lo][lane][16 bytes] = 96 KiB
        // conv1's A operands: a ring of six k-steps (hi + lo: 48 registers -- the accumulators of the main loops are gone by now),
        // requested six k-steps (36 MFMAs) ahead: the L2 latency of a fragment is longer than three k-steps of this short GEMM
        constexpr int R1 = 6;
        u32x4 wh[R1], wl[R1];
        auto load_w1 = [&](int slot, int kk) {   // slot and kk are compile-time at every call site
            const int so = ((12 * g1 + kk) * 6 + F1) * 2048;
            wh[slot] = __builtin_bit_cast(u32x4, LAMA_BUF_LOAD_B128(w1res, lane * 16, so));
            wl[slot] = __builtin_bit_cast(u32x4, LAMA_BUF_LOAD_B128(w1res, lane * 16 + 1024, so));
        };
        // 1. all four pixel fragments: bias, activation, residual, store (one unbroken HBM-bound phase, as in the plain epilogue); the
        //    finished values replace the accumulators as packed (hi, lo) halves = the B operands of this wave's two k-steps
        u32x4 bq[4][2][2];                                            // [pixel fragment][k-step of this wave][hi | lo]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            load_resid(j, 0);
            bool pv;
            const unsigned lo = (unsigned)(frag_off(j, pv) + kplane);
            float vv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int mu = row_u(r);
                float v = acc[j][r] + bv[r];
                if (p.act == LAMA_ACT_RELU) v = fmaxf(v, 0.0f);
                else if (p.act == LAMA_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
                else if (p.act == LAMA_ACT_TANH) v = tanhf(v);
                v += rv[0][r];
                vv[r] = v;
                if (pv && mu + khalf4 < p.M) (reinterpret_cast<AT*>(p.y) + (long long)b * p.y_bstride + (long long)mu * plane)[lo] = (AT)v;
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                unsigned hh[4], ll[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) cb_split2(vv[8 * ks + 2 * e], vv[8 * ks + 2 * e + 1], hh[e], ll[e], rw);
                bq[j][ks][0] = u32x4{hh[0], hh[1], hh[2], hh[3]};
                bq[j][ks][1] = u32x4{ll[0], ll[1], ll[2], ll[3]};
            }
        }
        // 2. two passes of two pixel fragments through LDS (96 KiB of B operands per pass)
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int i = 0; i < R1; ++i) load_w1(i, i);
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    char* dst = lb + ((((2 * F + ks) * 2 + jj) * 2) * 64 + lane) * 16;
                    *reinterpret_cast<u32x4*>(dst) = bq[2 * pass + jj][ks][0];
                    *reinterpret_cast<u32x4*>(dst + 1024) = bq[2 * pass + jj][ks][1];
                }
            __syncthreads();
            f32x16 a2[2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int r = 0; r < 16; ++r) a2[jj][r] = 0.0f;
            bf16x8 xh[2][2], xl[2][2];                                // [buffer][pixel fragment]: the next k-step's B operands are read under this one's MFMAs
            auto read_x = [&](int buf, int kk) {
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const char* src = lb + ((((12 * g1 + kk) * 2 + jj) * 2) * 64 + lane) * 16;
                    xh[buf][jj] = *reinterpret_cast<const bf16x8*>(src);
                    xl[buf][jj] = *reinterpret_cast<const bf16x8*>(src + 1024);
                }
            };
            read_x(0, 0);
#pragma unroll
            for (int kk = 0; kk < 12; ++kk) {
                const bf16x8 w_hi = __builtin_bit_cast(bf16x8, wh[kk % R1]), w_lo = __builtin_bit_cast(bf16x8, wl[kk % R1]);
                if (kk + 1 < 12) read_x((kk + 1) & 1, kk + 1);
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    a2[jj] = CB_MFMA(w_hi, xh[kk & 1][jj], a2[jj], 0, 0, 0);
                    a2[jj] = CB_MFMA(w_hi, xl[kk & 1][jj], a2[jj], 0, 0, 0);
                    a2[jj] = CB_MFMA(w_lo, xh[kk & 1][jj], a2[jj], 0, 0, 0);
                }
                if (kk + R1 < 12) load_w1(kk % R1, kk + R1);          // into the slot this k-step just released
            }
            {   // the two K halves: wave (F1, g1) finishes pixel fragment g1 of this pass and hands the other one to (F1, 1 - g1) through
                // an exchange area BEHIND the B operands (48 KiB): no barrier between the GEMM and the hand-over, and the one barrier of
                // the hand-over also tells every wave that the B operands of this pass have been read
                typedef float f32x4 __attribute__((ext_vector_type(4)));
                f32x4* xw = reinterpret_cast<f32x4*>(lama_smem + 96 * 1024) + wave * 256;
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const f32x16& o = g1 == 0 ? a2[1] : a2[0];
                    xw[r4 * 64 + lane] = f32x4{o[4 * r4], o[4 * r4 + 1], o[4 * r4 + 2], o[4 * r4 + 3]};
                }
                __syncthreads();
                const f32x4* xr = reinterpret_cast<const f32x4*>(lama_smem + 96 * 1024) + (F1 + 6 * (1 - g1)) * 256;
                f32x16 sum = g1 == 0 ? a2[0] : a2[1];
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const f32x4 o = xr[r4 * 64 + lane];
#pragma unroll
                    for (int e = 0; e < 4; ++e) sum[4 * r4 + e] += o[e];
                }
                bool pv;
                const unsigned lo1 = (unsigned)(frag_off(2 * pass + g1, pv) + kplane);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int mu1 = F1 * 32 + (r & 3) + 8 * (r >> 2);
                    const float v = fmaxf(sum[r] + (p.f1_bias ? p.f1_bias[mu1 + khalf4] : 0.0f), 0.0f);
                    if (pv) (p.f1_y + (long long)b * p.f1_y_bstride + (long long)mu1 * plane)[lo1] = v;
                }
            }
            // (no barrier here: the next pass writes B operands that every wave finished reading before the hand-over barrier, and its
            // own hand-over writes come after ITS first barrier, which every wave reaches only after reading this pass's hand-over)
        }
        cb_range_report(rw, p.range_flag);
    } else if constexpr (KG == 1) {
        if (NRV == 2) load_resid(0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (NRV == 1) load_resid(j, 0);
            else if (j + 1 < 4) load_resid(j + 1, (j + 1) & 1);
            store_frag(j, acc[j], NRV == 1 ? 0 : (j & 1));
        }
        if constexpr (YS) cb_range_report(rw, p.range_flag);   // the producer-side watch of what this workgroup stored
    } else {
        // K-group exchange (the patch buffers are free after the last barrier): group 0 finishes pixel fragments 0-1, group 1
        // fragments 2-3; each wave hands the other two to its partner (same fragment, other group) as [fragment][r / 4][lane][4 floats]
        if (kg == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float t0 = acc[0][r], t1 = acc[1][r];
                acc[0][r] = acc[2][r]; acc[1][r] = acc[3][r];
                acc[2][r] = t0; acc[3][r] = t1;
            }
        }
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        f32x4* xw = reinterpret_cast<f32x4*>(lama_smem) + wave * 512;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4)
                xw[(jj * 4 + r4) * 64 + lane] = f32x4{acc[2 + jj][4 * r4], acc[2 + jj][4 * r4 + 1], acc[2 + jj][4 * r4 + 2], acc[2 + jj][4 * r4 + 3]};
        __syncthreads();
        const f32x4* xr = reinterpret_cast<const f32x4*>(lama_smem) + ((1 - kg) * WMV + wm) * 512;
        if constexpr (NRV == 2) {
            load_resid(2 * kg, 0);
            load_resid(2 * kg + 1, 1);
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            if constexpr (NRV == 1) load_resid(2 * kg + jj, 0);
            f32x16 sum = acc[jj];
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const f32x4 o = xr[(jj * 4 + r4) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[4 * r4 + e] += o[e];
            }
            store_frag(2 * kg + jj, sum, NRV == 1 ? 0 : jj);
        }
    }
    if constexpr (ABL & 64) { if (threadIdx.x == 0) { trace[30] = LAMA_CLOCK(); trace[31] = L; } }
}
