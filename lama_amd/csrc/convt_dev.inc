// ConvTranspose2d(k3, s2, p1, op1) + folded BatchNorm + ReLU (the three upsampling layers, ffc.py:348-354) as ONE launch with the weights in
// registers (included by conv_split3.inc; 3-term split precisions, fp32 tensors).
//
// Output pixel (2i + py, 2j + px) of a transposed 3x3 / stride 2 conv is a small stride-1 conv of the input around (i, j) with the
// (1 + py)(1 + px) taps that reach its parity class: class (1,1) 4 taps, (1,0) and (0,1) 2 taps, (0,0) 1 tap, input offsets in
// {0, 1}^2, zero beyond the bottom / right edge.  History: round 1's fused LDS-staged launch walks all nine taps into four accumulator sets
// per workgroup (bound by its weight stream through LDS, 1.24 ms per step); round 2's four per-class launches of conv_wr_kernel lost to it;
// round 3's convt_kernel (wave = (class, row fragment), column parities exchanged through LDS; 0.99 ms per step) is in the git history;
// round 4's convt2_kernel below replaced it (0.79 ms per step).
//
// Shapes: Cin % 32 == 0, Cout % 64 == 0, W % 32 == 0, H % 4 == 0, no residual, identity / ReLU epilogue (up1 / up2 / up3 of big-lama at
// power-of-two inputs); anything else returns LAMA_ERR_UNSUPPORTED and the fused LDS-staged launch runs.

struct CtParams {
    const float* x;
    long long x_bstride;
    int C, H, W;
    const char* w[4];        // packed weights of class c: k-step (16-channel group g, tap t) at ((g * T + t) * mft + F) * 2048
    int T[4];
    int off[4][4];           // patch pixel offset (dy * CT_PWS + dx) of tap t of class c
    int py[4], px[4];
    int mft;
    const float* bias;
    float* y;
    long long y_bstride;
    int M, B, act;
    int tiles_x, tiles_y, MG;
    unsigned* range_flag;
    int abl;                 // profiling tools only (LAMA_CT_ABLATE, results WRONG): bit 0 = no global stores, bit 1 = no epilogue at all
    const int* list;         // LIST instantiation (lama_conv2d_list_fwd): the dense tile indices to walk, in ascending order ...
    const int* count;        // ... and how many of them (device int, written by lama_tail_lists_build earlier in the same stream)
};

#define CT_PWS 34                                   // LDS row pitch of the 5 x 33 patch (pixels)
#define CT_NPIX (5 * CT_PWS)

// ------------------------------------------------------------------------------------------------------------------------------------
// Round 4: ALL FOUR parity classes in one wave (convt2_kernel).
//
// What held round 3's convt_kernel at 0.23-0.37 of its ceiling (profiles/r03_convt.txt): (1) a wave per (class, row fragment) reads its own B
// fragments -- 8 ds_read_b128 per 12 MFMAs although the four classes read the SAME input pixels; (2) the two column parities of an output
// row live in different waves and meet through 64 KB of LDS behind two workgroup barriers per tile; (3) the stores of a tile sit on the
// in-order vmcnt chain of the next tile's A-fragment loads, and with one 8-wave workgroup per CU every wave of the CU is in that phase at
// the same time -- the tile is K loop + exchange + store drain, none of it overlapped.  Here:
//
//   * wave = (row fragment f, input-row pair pp): TWO pixel fragments (input rows 2 pp, 2 pp + 1 of a 4 x 32 tile) x ALL FOUR classes =
//     8 accumulators.  The nine (class, tap) products of a 16-channel k-group read only SIX distinct B fragments (input rows 2 pp .. 2 pp + 2 at
//     column shifts 0 / 1; hi + lo): 12 ds_read_b128 per 54 MFMAs instead of 36, and an A fragment (hi, lo from L2) feeds 6 MFMAs;
//   * a lane then holds BOTH column parities of its pixel for both row parities: the epilogue is wave-local -- bias, activation, one 8-byte
//     store per (channel, output row): 32 lanes x 8 bytes = a 256-byte run of an output row -- no exchange, no barrier;
//   * workgroup = 4 waves (f x pp: a 4 x 32 input tile x 64 output channels, the 5 x 33 patch of a 16-channel sub-chunk staged once for all of
//     them), TWO persistent workgroups per CU, each walking its own tiles: they drift out of phase, so the store drain (and the A waits
//     behind it) of one sits under the MFMAs of the other -- the arrangement of the stride-2 downsampling convs (conv_wreg_dev.inc <4, 1>).
//
// Packed weights: CbPlan classes 1..4 (class by class, k-step (16-channel group, tap)).
// The tap geometry is a compile-time table here (the B fragments are shared by position): the host checks the plan against it.
// ------------------------------------------------------------------------------------------------------------------------------------
#define C2_THREADS 256
// Measured on MI355X (stand-alone harness tools/ubench/mk_ct_bench.sh, profiles/r04_convt2.txt; up1 / up2 / up3 in us, same box): C2_KG x C2_AR =
// 1 x 3: 257 / 297 / 370 (the default: no spilled register), 1 x 6: 268 / 307 / 389, 2 x 3: 256 / 314 / 372, 2 x 6: 283 / 322 / 407; round 3's
// convt_kernel: 325 / 369 / 466.  Ablations at up3 say what is left: the three request streams of a wave -- A fragments (L2: 79 us alone = the
// 116 GB/s a CU draws from L2), patch (HBM latency chain: 109 us alone), stores (100 us alone = the HBM write rate) -- and the MFMAs (98 us
// exposed) ADD UP (291 us without MFMA, 370 with): one in-order vmcnt per wave serialises them, two waves per SIMD cannot cover it, and
// neither a start stagger of the second workgroup (0.5-30 us) nor one burst of patch requests per 32 channels changes the sum.
#ifndef C2_KG
#define C2_KG 1                                    // 16-channel k-groups per staged chunk (one barrier and one burst of patch requests per chunk)
#endif
#ifndef C2_AR
#define C2_AR 3                                    // A ring: (class, tap) positions in flight (3 or 6; 9 positions per k-group)
#endif
#define C2_NU ((2 * C2_KG * 165 + C2_THREADS - 1) / C2_THREADS)   // staging units (8 channels of one patch pixel) per thread and chunk
#define C2_PLANES (2 * C2_KG * CT_NPIX * 16)      // bytes of the hi (or lo) planes of one buffer: 2 octets per k-group
#define C2_PBUF (2 * C2_PLANES)
#define C2_LDS_BYTES (2 * C2_PBUF + 32)            // + a 32-byte dump slot
#ifndef C2_ABL
#define C2_ABL 0   // stand-alone harness only (tools/ubench/mk_ct_bench.sh; results WRONG): 1 no stores, 2 no epilogue, 4 no patch requests, 8 no A requests in the loop, 16 no MFMA, 64 no staging writes
#endif

// position q of a k-group -> (class, tap of the class's packed list, dy, dx), ordered by B fragment so that fragments are released early:
// classes (py, px): 0 = (1,1): taps (dy,dx) = (1,1) (1,0) (0,1) (0,0); 1 = (1,0): (1,0) (0,0); 2 = (0,1): (0,1) (0,0); 3 = (0,0): (0,0)
constexpr int c2_cls(int q) { constexpr int t[9] = {0, 1, 2, 3, 0, 1, 0, 2, 0}; return t[q]; }
constexpr int c2_tap(int q) { constexpr int t[9] = {3, 1, 1, 0, 1, 0, 2, 0, 0}; return t[q]; }
constexpr int c2_dy(int q) { constexpr int t[9] = {0, 0, 0, 0, 1, 1, 0, 0, 1}; return t[q]; }
constexpr int c2_dx(int q) { constexpr int t[9] = {0, 0, 0, 0, 0, 0, 1, 1, 1}; return t[q]; }

// LIST: the workgroup walks entries L0, L0 + G, ... of p.list (p.count[0] of them) instead of every tile of the plane -- the tiles whose output
// something downstream reads (sparse tail, DESIGN.md 4.17); the grid stays what the dense launch takes and workgroups beyond the count leave at once.
// A template parameter: the kernel sits at the register limit and the dense instantiation must stay what it was.
template <bool LIST = false>
__global__ __launch_bounds__(C2_THREADS, 2) void CB_NAME(convt2_kernel)(CtParams p) {
    static_assert((C2_AR == 3 || C2_AR == 6) && (C2_KG == 1 || C2_KG == 2), "ring slot = compile-time function of (k-group parity, position)");
    constexpr int KG = C2_KG, AR = C2_AR, NU = C2_NU;
    const int tid = threadIdx.x, lane = tid & 63, wave = LAMA_WAVE_UNIFORM(tid >> 6);
    const int f = wave & 1, pp = wave >> 1;
    const int khalf = lane >> 5, l31 = lane & 31;
    const int HW = p.H * p.W;
    char* const smem = lama_smem;
    const int L0 = lama_xcd_remap(blockIdx.x, gridDim.x), G = gridDim.x;
    const int ndense = p.B * p.tiles_y * p.tiles_x * p.MG;
    int ntiles = ndense;
    if constexpr (LIST) { const int n = p.count[0]; ntiles = n < ntiles ? (n > 0 ? n : 0) : ntiles; }   // (never more entries than the list holds)
    const int ntl = L0 < ntiles ? (ntiles - L0 + G - 1) / G : 0;     // tiles of this workgroup
    const int ngr = p.C / 16, nch = ngr / KG, nseq = ntl * nch;      // k-groups / staged chunks per tile (Cin % 32 == 0), chunks of this workgroup
    auto tile_of = [&](int tl, int& mg, int& b, int& gy0, int& gx0) {
        int t0 = L0 + tl * G;
        if constexpr (LIST) { t0 = p.list[t0]; t0 = t0 < 0 ? 0 : (t0 >= ndense ? ndense - 1 : t0); }   // (an entry is a tile of this plane whatever the buffer holds)
        mg = t0 % p.MG;
        t0 /= p.MG;
        const int tx = t0 % p.tiles_x;
        t0 /= p.tiles_x;
        gy0 = (t0 % p.tiles_y) * 4;
        gx0 = tx * 32;
        b = t0 / p.tiles_y;
    };
    // staging units of this thread: (channel octet, patch pixel) -> 8 channels of one pixel; 2 KG x 165 units on 256 threads.
    // One packed word per unit (octet << 16 | patch row << 8 | patch column; -1 = no unit): the kernel sits at the register limit
    int uinf[NU];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const int u = tid + i * C2_THREADS;
        uinf[i] = -1;
        if (u < 2 * KG * 165) {
            const int o = u / 165, pq = u - o * 165, ry = pq / 33;
            uinf[i] = (o << 16) | (ry << 8) | (pq - ry * 33);
        }
    }
    float preg[NU][8];
    unsigned rw = 0;
    lama_buf_t xres;
    int vo[NU];
    auto unit_addr = [&](int sq) {                        // sequence position sq = (tile, chunk); past the end: out of range, the loads return 0
        const bool live = sq < nseq;
        const int tl = live ? sq / nch : 0, c = live ? sq - tl * nch : 0;
        int mg, b, gy0, gx0;
        tile_of(tl, mg, b, gy0, gx0);
        xres = LAMA_BUF_RSRC(reinterpret_cast<const char*>(p.x) + (long long)b * p.x_bstride * 4 + (long long)c * 16 * KG * HW * 4,
                             live ? (long long)(p.C - c * 16 * KG) * HW * 4 : 0ll);
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const int iy = gy0 + ((uinf[i] >> 8) & 255), ix = gx0 + (uinf[i] & 255);
            vo[i] = (uinf[i] >= 0 && iy < p.H && ix < p.W) ? ((uinf[i] >> 16) * 8 * HW + iy * p.W + ix) * 4 : 0x7ffffff0;   // beyond the bottom / right edge -> 0
        }
    };
    auto load_part = [&](int e) {                         // channel e of every unit's octet
        if constexpr (C2_ABL & 4) return;
#pragma unroll
        for (int i = 0; i < NU; ++i) preg[i][e] = __builtin_bit_cast(float, LAMA_BUF_LOAD_B32(xres, vo[i], e * HW * 4));
    };
    auto load_units = [&](int sq) {
        unit_addr(sq);
#pragma unroll
        for (int e = 0; e < 8; ++e) load_part(e);
    };
    u32x4 sh, sl;
    auto split_unit = [&](int i) {
        unsigned hh[4], ll[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) cb_split2(preg[i][2 * e], preg[i][2 * e + 1], hh[e], ll[e], rw);
        sh = u32x4{hh[0], hh[1], hh[2], hh[3]};
        sl = u32x4{ll[0], ll[1], ll[2], ll[3]};
    };
    auto store_unit = [&](char* buf, int i) {             // threads without this unit write to the dump slot behind the buffers: no branch in the K loop
        if constexpr (C2_ABL & 64) { LAMA_KEEP_LIVE(sh); LAMA_KEEP_LIVE(sl); return; }
        char* d = uinf[i] >= 0 ? buf + ((uinf[i] >> 16) * CT_NPIX + ((uinf[i] >> 8) & 255) * CT_PWS + (uinf[i] & 255)) * 16 : smem + 2 * C2_PBUF;
        *reinterpret_cast<u32x4*>(d) = sh;
        *reinterpret_cast<u32x4*>(d + (uinf[i] >= 0 ? C2_PLANES : 16)) = sl;
    };
    auto write_units = [&](char* buf) {
#pragma unroll
        for (int i = 0; i < NU; ++i) { split_unit(i); store_unit(buf, i); }
    };
    // A operands: position q of k-group g = packed k-step (g, tap) of class cls at ((g * T + tap) * mft + F) * 2048; one buffer resource per class
    const lama_buf_t wres0 = LAMA_BUF_RSRC(p.w[0], (long long)(p.C / 16) * 4 * p.mft * 2048);
    const lama_buf_t wres1 = LAMA_BUF_RSRC(p.w[1], (long long)(p.C / 16) * 2 * p.mft * 2048);
    const lama_buf_t wres2 = LAMA_BUF_RSRC(p.w[2], (long long)(p.C / 16) * 2 * p.mft * 2048);
    const lama_buf_t wres3 = LAMA_BUF_RSRC(p.w[3], (long long)(p.C / 16) * 1 * p.mft * 2048);
    bf16x8 ah[AR], al[AR];
    auto load_a = [&](auto q_tag, int g, int F, auto slot_tag) {
        constexpr int q = decltype(q_tag)::value, S = decltype(slot_tag)::value;
        constexpr int cls = c2_cls(q), T = cls == 0 ? 4 : (cls == 3 ? 1 : 2);
        const int so = ((g * T + c2_tap(q)) * p.mft + F) * 2048;
#define C2_LOAD_A(wr)                                                                      \
    do {                                                                                   \
        ah[S] = __builtin_bit_cast(bf16x8, LAMA_BUF_LOAD_B128(wr, lane * 16, so));         \
        al[S] = __builtin_bit_cast(bf16x8, LAMA_BUF_LOAD_B128(wr, lane * 16 + 1024, so));  \
    } while (0)
        if constexpr (cls == 0) C2_LOAD_A(wres0);
        else if constexpr (cls == 1) C2_LOAD_A(wres1);
        else if constexpr (cls == 2) C2_LOAD_A(wres2);
        else C2_LOAD_A(wres3);
#undef C2_LOAD_A
    };
    // B fragments: patch row 2 pp + r (r = 0..2), column shift dx, octet 2 kg + khalf of the chunk
    const int boff = (khalf * CT_NPIX + 2 * pp * CT_PWS + l31) * 16;
    bf16x8 bh[3][2], bl[3][2];
    auto read_b = [&](const char* buf, int kg, int r, int dx) {
        const char* bp = buf + boff + (2 * kg * CT_NPIX + r * CT_PWS + dx) * 16;
        bh[r][dx] = *reinterpret_cast<const bf16x8*>(bp);
        bl[r][dx] = *reinterpret_cast<const bf16x8*>(bp + C2_PLANES);
    };

#ifdef C2_STAGGER   // stand-alone harness: the second workgroup of every CU (dispatch order: the upper half of the grid) starts C2_STAGGER x 10 ns late
    if ((int)blockIdx.x >= (int)gridDim.x / 2) {
        const long long t0 = LAMA_CLOCK();
        while (LAMA_CLOCK() - t0 < C2_STAGGER) __builtin_amdgcn_s_sleep(32);
    }
#endif
    if (ntl > 0) {
        int mg, b, gy0, gx0;
        tile_of(0, mg, b, gy0, gx0);
        load_units(0);
        // the first AR positions of A (all in k-group 0)
        const int F0 = mg * 2 + f;
        load_a(CbTag<0>{}, 0, F0, CbTag<0>{}); load_a(CbTag<1>{}, 0, F0, CbTag<1>{}); load_a(CbTag<2>{}, 0, F0, CbTag<2>{});
        if constexpr (AR == 6) { load_a(CbTag<3>{}, 0, F0, CbTag<3 % AR>{}); load_a(CbTag<4>{}, 0, F0, CbTag<4 % AR>{}); load_a(CbTag<5>{}, 0, F0, CbTag<5 % AR>{}); }
        write_units(smem);
        load_units(1);
    }
    __syncthreads();
    int s = 0;                                            // sequence position (tile, chunk) of the K loop
    const int Wo = 2 * p.W;
    const long long plane = (long long)4 * p.H * p.W;
#pragma unroll 1
    for (int tl = 0; tl < ntl; ++tl) {
        int mg, b, gy0, gx0, mgn, bn, gy0n, gx0n;
        tile_of(tl, mg, b, gy0, gx0);
        tile_of(tl + 1 < ntl ? tl + 1 : tl, mgn, bn, gy0n, gx0n);
        const bool last_tile = tl + 1 >= ntl;
        f32x16 acc[4][2];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c][j][r] = 0.0f;
        // One k-group = 9 positions x 6 MFMAs, written in issue order and PINNED (a sched_barrier behind every slot): hipcc left alone groups
        // the MFMAs of one accumulator back to back (dependent issue), drags the next chunk's requests over the barrier and orders an A request
        // behind the patch requests only to wait for it with vmcnt(0).  A position walks hi x hi, hi x lo, lo x hi over its two pixel
        // fragments (an accumulator every second MFMA), releases its ring slot and requests position + AR into it; the B reads (two
        // positions ahead of their first use: at most four of the six fragments live), the staging of the next chunk (one unit per position)
        // and the patch requests of the chunk after it sit between the MFMAs.  An A request issued behind a patch request waits for HBM
        // (vmcnt retires in order): ONE burst of patch requests per chunk, at its end.  U: parity of the k-group (ring slot = (9 U + q) % AR)
#define C2_PIN() __builtin_amdgcn_sched_barrier(0)
        auto pos = [&](int g, auto u_tag, auto q_tag, auto&& x1, auto&& x2, auto&& x3, auto&& x4) {
            constexpr int U = decltype(u_tag)::value, q = decltype(q_tag)::value, SA = (9 * U + q) % AR, cls = c2_cls(q), dy = c2_dy(q), dx = c2_dx(q);
#if C2_ABL & 16
#define C2_MM(a_, b_, j_) do { LAMA_KEEP_LIVE(a_); LAMA_KEEP_LIVE(b_); } while (0)
#else
#define C2_MM(a_, b_, j_) acc[cls][j_] = CB_MFMA(a_, b_, acc[cls][j_], 0, 0, 0)
#endif
            C2_MM(ah[SA], bh[dy][dx], 0); C2_PIN();
            x1(); C2_PIN();
            C2_MM(ah[SA], bh[1 + dy][dx], 1); C2_PIN();
            x2(); C2_PIN();
            C2_MM(ah[SA], bl[dy][dx], 0); C2_PIN();
            x3(); C2_PIN();
            C2_MM(ah[SA], bl[1 + dy][dx], 1); C2_PIN();
            x4(); C2_PIN();
            C2_MM(al[SA], bh[dy][dx], 0); C2_PIN();
            C2_MM(al[SA], bh[1 + dy][dx], 1); C2_PIN();
#undef C2_MM
            // the ring slot is free: position q + AR -- of this k-group, the next one, or (wrapping) the next tile's first k-group and row group
            constexpr int qn = q + AR, qq = qn % 9;
            int gn = g + qn / 9, Fn = mg * 2 + f;
            if (gn >= ngr && !last_tile) { gn -= ngr; Fn = mgn * 2 + f; }      // (past the last tile: gn >= ngr is out of range -> zeros, never multiplied)
            if constexpr (!(C2_ABL & 8)) load_a(CbTag<qq>{}, gn, Fn, CbTag<SA>{});
            C2_PIN();
        };
        auto none = [&]() {};
#if C2_KG == 1
        auto chunk = [&](int g, auto u) {
            const char* cur = smem + (s & 1) * C2_PBUF;
            char* nxt = smem + ((s + 1) & 1) * C2_PBUF;
            C2_PIN();
            read_b(cur, 0, 0, 0); read_b(cur, 0, 1, 0);
            C2_PIN();
            pos(g, u, CbTag<0>{}, [&]() { read_b(cur, 0, 2, 0); }, none, none, none);
            pos(g, u, CbTag<1>{}, [&]() { split_unit(0); }, [&]() { store_unit(nxt, 0); }, none, none);    // sequence position s + 1 (requested during the previous chunk)
            pos(g, u, CbTag<2>{}, none, none, none, none);
            pos(g, u, CbTag<3>{}, [&]() { split_unit(1); }, [&]() { store_unit(nxt, 1); }, none, none);
            pos(g, u, CbTag<4>{}, [&]() { read_b(cur, 0, 0, 1); }, [&]() { read_b(cur, 0, 1, 1); }, none, none);
            pos(g, u, CbTag<5>{}, [&]() { unit_addr(s + 2); }, [&]() { load_part(0); }, [&]() { load_part(1); }, none);   // ... and the patch requests of s + 2
            pos(g, u, CbTag<6>{}, [&]() { read_b(cur, 0, 2, 1); }, [&]() { load_part(2); }, [&]() { load_part(3); }, none);
            pos(g, u, CbTag<7>{}, [&]() { load_part(4); }, [&]() { load_part(5); }, none, none);
            pos(g, u, CbTag<8>{}, [&]() { load_part(6); }, [&]() { load_part(7); }, none, none);
            ++s;
            __syncthreads();
        };
#pragma unroll 1
        for (int g = 0; g < ngr; g += 2) {
            chunk(g, CbTag<0>{});
            chunk(g + 1, CbTag<1>{});
        }
#else
#pragma unroll 1
        for (int g = 0; g < ngr; g += 2) {
            const char* cur = smem + (s & 1) * C2_PBUF;
            char* nxt = smem + ((s + 1) & 1) * C2_PBUF;
            CbTag<0> u0;
            CbTag<1> u1;
            C2_PIN();
            read_b(cur, 0, 0, 0); read_b(cur, 0, 1, 0);
            C2_PIN();
            pos(g, u0, CbTag<0>{}, [&]() { read_b(cur, 0, 2, 0); }, none, none, none);
            pos(g, u0, CbTag<1>{}, [&]() { split_unit(0); }, [&]() { store_unit(nxt, 0); }, none, none);   // sequence position s + 1 (loaded during the previous chunk)
            pos(g, u0, CbTag<2>{}, none, none, none, none);
            pos(g, u0, CbTag<3>{}, [&]() { split_unit(1); }, [&]() { store_unit(nxt, 1); }, none, none);
            pos(g, u0, CbTag<4>{}, [&]() { read_b(cur, 0, 0, 1); }, [&]() { read_b(cur, 0, 1, 1); }, none, none);
            pos(g, u0, CbTag<5>{}, [&]() { split_unit(2); }, [&]() { store_unit(nxt, 2); }, none, none);
            pos(g, u0, CbTag<6>{}, [&]() { read_b(cur, 0, 2, 1); }, none, none, none);
            pos(g, u0, CbTag<7>{}, [&]() { read_b(cur, 1, 0, 0); }, none, none, none);
            pos(g, u0, CbTag<8>{}, [&]() { read_b(cur, 1, 1, 0); }, none, none, none);                     // (rows 0, 1 at shift 0 were last read by positions 3 / 5)
            pos(g + 1, u1, CbTag<0>{}, [&]() { read_b(cur, 1, 2, 0); }, none, none, none);
            pos(g + 1, u1, CbTag<1>{}, none, none, none, none);
            pos(g + 1, u1, CbTag<2>{}, [&]() { unit_addr(s + 2); }, none, none, none);
            pos(g + 1, u1, CbTag<3>{}, none, none, none, none);
            pos(g + 1, u1, CbTag<4>{}, [&]() { read_b(cur, 1, 0, 1); }, [&]() { read_b(cur, 1, 1, 1); }, none, none);
            pos(g + 1, u1, CbTag<5>{}, none, none, none, none);
            // ... and the patch requests of s + 2 in ONE burst at the end of the chunk: the A requests queued behind them belong to the next chunk
            pos(g + 1, u1, CbTag<6>{}, [&]() { read_b(cur, 1, 2, 1); }, [&]() { load_part(0); }, [&]() { load_part(1); }, none);
            pos(g + 1, u1, CbTag<7>{}, [&]() { load_part(2); }, [&]() { load_part(3); }, [&]() { load_part(4); }, none);
            pos(g + 1, u1, CbTag<8>{}, [&]() { load_part(5); }, [&]() { load_part(6); }, [&]() { load_part(7); }, none);
            ++s;
            __syncthreads();
        }
#endif
#undef C2_PIN
        if ((p.abl & 2) || (C2_ABL & 2)) {
#pragma unroll
            for (int c = 0; c < 4; ++c) { LAMA_KEEP_LIVE(acc[c][0]); LAMA_KEEP_LIVE(acc[c][1]); }
            continue;
        }
        // ---- epilogue (wave-local): lane (khalf, l31) holds channels 32 f + (r & 3) + 8 (r >> 2) + 4 khalf of input pixel (2 pp + j, l31) for all
        // four classes = output pixels (2 (gy0 + 2 pp + j) + py, 2 (gx0 + l31) + px): the two px of a (channel, output row) are one 8-byte store
        float* const yb = p.y + (long long)b * p.y_bstride;
        const float floor_ = p.act == LAMA_ACT_RELU ? 0.0f : -__builtin_inff();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mg * 64 + f * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
            const float bias = (p.bias && m < p.M) ? p.bias[m] : 0.0f;
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float o0 = acc[py ? 1 : 3][j][r] + bias, o1 = acc[py ? 0 : 2][j][r] + bias;      // px = 0, px = 1
                    o0 = fmaxf(o0, floor_);                // identity / ReLU without a branch (the host sends every other activation elsewhere)
                    o1 = fmaxf(o1, floor_);
                    if (C2_ABL & 1) { LAMA_KEEP_LIVE(o0); LAMA_KEEP_LIVE(o1); }
                    else if (m < p.M && !(p.abl & 1) && gy0 + 2 * pp + j < p.H && gx0 + l31 < p.W)      // (round 6: ragged last tile row / column)
                        *reinterpret_cast<float2*>(yb + (long long)m * plane + (long long)(2 * (gy0 + 2 * pp + j) + py) * Wo + 2 * (gx0 + l31)) = make_float2(o0, o1);
                }
        }
    }
    cb_range_report(rw, p.range_flag);
}
