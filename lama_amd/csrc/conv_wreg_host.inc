// Host side of the weights-in-registers kernels (conv_wreg_dev.inc): shape test + launch.  Same packed weights, same CbParams /
// CbSeg as the LDS-staged kernel, so the C ABI and lama_conv2d_pack_weight are unchanged; returns LAMA_ERR_UNSUPPORTED for
// shapes it does not take (the caller then falls through to the LDS-staged kernel).

template <int T1, int KSC1, int T2, int KSC2, int WMV, int KG>
int cw_launch_t(hipStream_t st, const CbParams& p, int grid, size_t shmem, int io = CB_IO_F32) {
#if CB_HALF
    // 3x3 on 32-pixel tile rows at two waves per SIMD: the row-rolling fragment reads (one product per MAC leaves the LDS pipe as the limit)
    constexpr bool CAN_ROLL = (T1 == 9 && WMV * KG <= 8);
    const bool roll = CAN_ROLL && p.TWlog == 5;
#define CW_H(hi1, hi2, ho)                                                                                                                       \
    do {                                                                                                                                         \
        if (roll) hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<T1, KSC1, T2, KSC2, WMV, KG, 0, 0, true, hi1, hi2, ho, CAN_ROLL>), dim3(grid),    \
                                     dim3(64 * WMV * KG), shmem, st, p);                                                                        \
        else hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<T1, KSC1, T2, KSC2, WMV, KG, 0, 0, true, hi1, hi2, ho>), dim3(grid),                   \
                                dim3(64 * WMV * KG), shmem, st, p);                                                                             \
    } while (0)
    const int io3 = io & 3;
    const bool x2h = (io & CB_IO_X2H) != 0;
    if (io != CB_IO_F32) {
        if (T2 > 0 && !x2h) return LAMA_ERR_UNSUPPORTED;                 // t (the spectral branch's output) is always fp16 on this path
        if (io3 == CB_IO_F16) CW_H(true, true, true);
        else if constexpr ((T1 == 9 && T2 == 0 && WMV == 4 && KG == 2) || (T1 == 9 && T2 == 1 && WMV == 12 && KG == 1)) {
            // the two bottleneck launches with the fp32 residual stream on one side
            if (io3 == CB_IO_F32_F16) CW_H(false, true, true);
            else if (io3 == CB_IO_F16_F32) CW_H(true, true, false);
            else return LAMA_ERR_UNSUPPORTED;
        } else return LAMA_ERR_UNSUPPORTED;
        LAMA_CHECK_LAUNCH();
        return LAMA_OK;
    }
#undef CW_H
    return LAMA_ERR_UNSUPPORTED;
#else
    if (io != CB_IO_F32) return LAMA_ERR_UNSUPPORTED;
    if constexpr (T1 == 9 && WMV * KG <= 8) {   // 32-pixel tile rows: the row-rolling fragment reads (conv_wreg_dev.inc, ROLL)
        static const int roll = lama_env_int("LAMA_CW_ROLL", 1);   // 0: A/B runs of the profiling tools
        if (p.TWlog == 5 && roll) {
            hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<T1, KSC1, T2, KSC2, WMV, KG, 0, 2, false, false, false, false, true>), dim3(grid),
                               dim3(64 * WMV * KG), shmem, st, p);
            LAMA_CHECK_LAUNCH();
            return LAMA_OK;
        }
    }
    hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<T1, KSC1, T2, KSC2, WMV, KG>), dim3(grid), dim3(64 * WMV * KG), shmem, st, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
#endif
}

// LAMA_CONV_WR=0 disables the variant (same-box A/B runs of the profiling tools); read once
bool cw_enabled() {
    static const bool on = lama_env_int("LAMA_CONV_WR", 1) != 0;
    return on;
}

// The same GEMMs over 64-pixel super-tiles of two interleaved MFMA tiles (gemm1x1_w4_kernel<., SUP = 2>, conv_ws_dev.inc): 8-byte activation
// loads and stores, one K-quarter exchange (one barrier) per 108 MFMAs of a wave, the split of the next chunk and the previous super-tile's
// epilogue in the shadow of the MFMAs; identity / ReLU epilogues.
// fp32 tensors, K = 192 / 384, whole row groups of 96, HW % 2 == 0, 8-byte aligned views, launches of at least one workgroup per CU
// (smaller ones fill the chip better with 32-pixel tiles: the kernel below).  SUP = 4 (16-byte accesses, 128 pixels) compiles from the same
// source but needs 144 + 192 + 96 registers next to the split buffers and spills (84 VGPRs): not instantiated.
// LAMA_GEMM_W4 (profiling build): 0 off, 2 whatever the launch size (emulator / forced-path tests); LAMA_GEMM_W4_SLOTS caps the workgroups
// per row group (tests: several rounds on a few super-tiles).
#define G4_SUP 2
int g4_try_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, int Ho, int Wo, int io) {
#if CB_HALF
    return LAMA_ERR_UNSUPPORTED;
#else
    const int mode = lama_env_int("LAMA_GEMM_W4", 1);   // read per launch (tests switch it per case)
    if (mode == 0 || io != CB_IO_F32) return LAMA_ERR_UNSUPPORTED;
    if (a->transposed || a->stride != 1 || a->pad != 0 || pl.mode != 0 || pl.nseg != 1 || pl.T[0] != 1) return LAMA_ERR_UNSUPPORTED;
    const int C = a->x.C;
    if ((C != 192 && C != 384) || pl.mft % 3 != 0 || pl.rows != pl.mft * 32) return LAMA_ERR_UNSUPPORTED;
    if (a->act != LAMA_ACT_NONE && a->act != LAMA_ACT_RELU) return LAMA_ERR_UNSUPPORTED;   // the pipelined epilogue is branch-free
    const long long HW = (long long)Ho * Wo;
    const bool rs = a->resid.ptr != nullptr;
    if (HW % G4_SUP != 0 || a->x.batch_stride % G4_SUP != 0 || a->y.batch_stride % G4_SUP != 0 || (rs && a->resid.batch_stride % G4_SUP != 0)) return LAMA_ERR_UNSUPPORTED;
    if (((uintptr_t)a->x.ptr | (uintptr_t)a->y.ptr | (uintptr_t)a->resid.ptr) & (4 * G4_SUP - 1)) return LAMA_ERR_UNSUPPORTED;
    // one buffer resource spans the batch: 32-bit byte offsets, the out-of-range marker 0x7ffffff0 must stay past every span
    const long long xspan = ((long long)(a->batch - 1) * a->x.batch_stride + (long long)C * HW) * 4;
    const long long yspan = ((long long)(a->batch - 1) * a->y.batch_stride + (long long)pl.rows * HW) * 4;
    const long long rspan = rs ? ((long long)(a->batch - 1) * a->resid.batch_stride + (long long)pl.rows * HW) * 4 : 0;
    if (xspan >= 0x7ffffff0ll || yspan >= 0x7ffffff0ll || rspan >= 0x7ffffff0ll || (long long)a->batch * HW >= (1ll << 30)) return LAMA_ERR_UNSUPPORTED;
    GwParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const float*)a->x.ptr;
    p.x_bstride = a->x.batch_stride;
    p.HW = (int)HW;
    p.C = C;
    p.w = (const char*)a->w_packed + pl.woff[0];
    p.mft = pl.mft;
    p.bias = a->bias;
    p.resid = (const float*)a->resid.ptr;
    p.resid_bstride = a->resid.batch_stride;
    p.y = (float*)a->y.ptr;
    p.y_bstride = a->y.batch_stride;
    p.M = pl.rows;
    p.B = a->batch;
    p.act = a->act;
    p.range_flag = a->range_flag;
    p.tiles_per_img = 0;
    p.ntiles = (int)lama_ceil_div64((long long)a->batch * HW, 32 * G4_SUP);     // super-tiles over the flat pixel list of the batch
    p.ntypes = pl.mft / 3;
    if (p.ntypes > 256) return LAMA_ERR_UNSUPPORTED;
    if (mode != 2 && (long long)p.ntiles * p.ntypes < 256) return LAMA_ERR_UNSUPPORTED;
    p.nslots = 256 / p.ntypes;                                          // one workgroup per CU, resident from the start
    if (p.nslots > p.ntiles) p.nslots = p.ntiles;
    { const int cap = lama_env_int("LAMA_GEMM_W4_SLOTS", 0); if (cap > 0 && p.nslots > cap) p.nslots = cap; }
    const int grid = p.nslots * p.ntypes;
    if (grid <= 0) return LAMA_OK;
    { static const int abl = lama_env_int("LAMA_GW_ABLATE", 0); p.abl = abl; }   // profiling tools only
    const size_t lds = G4_LDS_BYTES(G4_SUP);
#if defined(LAMA_PROFILING)
    if (CB_F16 && C == 384 && !rs) {   // profiling tools only: per-workgroup timeline, LAMA_GW_TRACE = device address of grid * 16 int64
        static const unsigned long long tr = lama_env_u64("LAMA_GW_TRACE");
        if (tr) {
            p.trace = reinterpret_cast<long long*>(tr);
            hipLaunchKernelGGL((CB_NAME(gemm1x1_w4_kernel)<6, G4_SUP, false, true>), dim3(grid), dim3(G4_THREADS), lds, stream, p);
            LAMA_CHECK_LAUNCH();
            return LAMA_OK;
        }
    }
#endif
#define G4_CASE(nch, rs_) hipLaunchKernelGGL((CB_NAME(gemm1x1_w4_kernel)<nch, G4_SUP, rs_>), dim3(grid), dim3(G4_THREADS), lds, stream, p)
    if (C == 384) { if (rs) G4_CASE(6, true); else G4_CASE(6, false); }
    else { if (rs) G4_CASE(3, true); else G4_CASE(3, false); }
#undef G4_CASE
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
#endif
}

// The spectral GEMM of the FourierUnit with all of K in one wave (gemm1x1_wk_kernel, gemm_wk_dev.inc): one workgroup per CU owns a 64-pixel
// super-tile and all 384 rows, activations staged once through LDS in B-fragment order, A fragments streamed from L2, no exchange; left-over
// super-tiles (264 on 256 CUs) go to the fifth waves.  fp32 tensors, C == 384, M == 384, no residual, identity / ReLU, HW % 2 == 0, 8-byte
// aligned views, launches of one super-tile per CU plus left-overs the fifth waves can take (256 .. 277 super-tiles; 8 x 512^2: 264).
// LAMA_GEMM_WK (profiling build): 0 off, 2 whatever the launch size (emulator / forced-path tests); LAMA_GEMM_WK_SLOTS caps the workgroups
// (tests: several rounds on a few super-tiles); LAMA_GEMM_WK_AUX = 0: left-overs are one more round (A/B runs).
#ifndef GK_DEFAULT_MODE
#define GK_DEFAULT_MODE 1
#endif
int gk_try_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, int Ho, int Wo, int io) {
#if CB_HALF
    return LAMA_ERR_UNSUPPORTED;
#else
    const int mode = lama_env_int("LAMA_GEMM_WK", GK_DEFAULT_MODE);   // read per launch (tests switch it per case)
    if (mode == 0 || io != CB_IO_F32) return LAMA_ERR_UNSUPPORTED;
    if (a->transposed || a->stride != 1 || a->pad != 0 || pl.mode != 0 || pl.nseg != 1 || pl.T[0] != 1) return LAMA_ERR_UNSUPPORTED;
    if (a->x.C != 384 || pl.mft != 12 || pl.rows != 384 || a->resid.ptr != nullptr) return LAMA_ERR_UNSUPPORTED;
    if (a->act != LAMA_ACT_NONE && a->act != LAMA_ACT_RELU) return LAMA_ERR_UNSUPPORTED;
    const long long HW = (long long)Ho * Wo;
    if (HW % 2 != 0 || a->x.batch_stride % 2 != 0 || a->y.batch_stride % 2 != 0) return LAMA_ERR_UNSUPPORTED;
    if (((uintptr_t)a->x.ptr | (uintptr_t)a->y.ptr) & 7) return LAMA_ERR_UNSUPPORTED;
    // one buffer resource spans the batch: 32-bit byte offsets, the out-of-range marker 0x7ffffff0 must stay past every span
    const long long xspan = ((long long)(a->batch - 1) * a->x.batch_stride + 384 * HW) * 4;
    const long long yspan = ((long long)(a->batch - 1) * a->y.batch_stride + 384 * HW) * 4;
    if (xspan >= 0x7ffffff0ll || yspan >= 0x7ffffff0ll || (long long)a->batch * HW >= (1ll << 30)) return LAMA_ERR_UNSUPPORTED;
    GwParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const float*)a->x.ptr;
    p.x_bstride = a->x.batch_stride;
    p.HW = (int)HW;
    p.C = 384;
    p.w = (const char*)a->w_packed + pl.woff[0];
    p.mft = pl.mft;
    p.bias = a->bias;
    p.y = (float*)a->y.ptr;
    p.y_bstride = a->y.batch_stride;
    p.M = pl.rows;
    p.B = a->batch;
    p.act = a->act;
    p.range_flag = a->range_flag;
    p.ntiles = (int)lama_ceil_div64((long long)a->batch * HW, 64);     // super-tiles over the flat pixel list of the batch
    // smaller launches fill the chip better with row groups of 96; from two rounds on the pipelined super-tiles of gemm1x1_w4_kernel win (the
    // rounds of this kernel do not overlap: 4 x 384 x 128 x 65 = 520 super-tiles 98.3 against 93.8 us, profiles/r03_gemm_wk.txt).  A part of a
    // batch that runs beside its siblings (LAMA_CONV_SIBLINGS_*, v109) counts with their super-tiles: together they are the one-per-CU launch.
    const long long ntiles_all = (long long)p.ntiles << LAMA_CONV_SIBLINGS_LOG2(a->flags);
    if (mode != 2 && (ntiles_all < 256 || ntiles_all >= 512)) return LAMA_ERR_UNSUPPORTED;
    int grid = p.ntiles < 256 ? p.ntiles : 256;                        // one workgroup per CU, resident from the start
    { const int cap = lama_env_int("LAMA_GEMM_WK_SLOTS", 0); if (cap > 0 && grid > cap) grid = cap; }
    if (grid <= 0) return LAMA_OK;
    const int rem = p.ntiles % grid;
    p.aux = (rem > 0 && rem * 24 <= 2 * grid && lama_env_int("LAMA_GEMM_WK_AUX", 1) != 0) ? 1 : 0;
    // left-overs too many for the fifth waves would be a whole second round (2 x 17 us where the pipelined w4 kernel needs ntiles / 64 x 3.9 + 4.3):
    // production takes this kernel for one round + fifth waves only (256 .. 277 super-tiles: 8 x 512^2 = 264, 2 x 1024^2 = 260)
    if (mode != 2 && rem > 0 && !p.aux) return LAMA_ERR_UNSUPPORTED;
    if (mode != 2 && p.ntiles < 256 && ntiles_all >= 256 + 22) return LAMA_ERR_UNSUPPORTED;   // (siblings: the whole batch would not have taken this kernel either)
    { static const int abl = lama_env_int("LAMA_GW_ABLATE", 0); p.abl = abl; }   // profiling tools only
#if defined(LAMA_PROFILING)
    if (CB_F16) {   // profiling tools only: per-workgroup timeline, LAMA_GW_TRACE = device address of grid * 16 int64
        static const unsigned long long tr = lama_env_u64("LAMA_GW_TRACE");
        if (tr) {
            p.trace = reinterpret_cast<long long*>(tr);
            hipLaunchKernelGGL((CB_NAME(gemm1x1_wk_kernel)<true>), dim3(grid), dim3(GK_THREADS), GK_LDS_BYTES, stream, p);
            LAMA_CHECK_LAUNCH();
            return LAMA_OK;
        }
    }
#endif
    hipLaunchKernelGGL((CB_NAME(gemm1x1_wk_kernel)<false>), dim3(grid), dim3(GK_THREADS), GK_LDS_BYTES, stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
#endif
}

// Weights-stationary persistent kernel for the pointwise GEMMs (conv_ws_dev.inc): flat 1x1, K = 192 / 384, rows in groups of 96.
// LAMA_GEMM_WS: 0 disables it (A/B runs of the profiling tools), 2 takes it whatever the launch size (emulator tests); read once.
int gw_try_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, int Ho, int Wo, int io) {
    static const int mode = lama_env_int("LAMA_GEMM_WS", 1);
    if (io != CB_IO_F32 && io != CB_IO_F16 && io != CB_IO_F32_F16) return LAMA_ERR_UNSUPPORTED;
    if (mode == 0 || a->transposed || a->stride != 1 || a->pad != 0 || pl.mode != 0 || pl.nseg != 1 || pl.T[0] != 1) return LAMA_ERR_UNSUPPORTED;
    const int C = a->x.C;
    if ((C != 192 && C != 384) || pl.mft % 3 != 0) return LAMA_ERR_UNSUPPORTED;
    const long long HW = (long long)Ho * Wo;
    if ((long long)C * HW >= (1ll << 29) || (long long)pl.mft * 32 * HW >= (1ll << 29)) return LAMA_ERR_UNSUPPORTED;   // 32-bit byte offsets inside one image
    GwParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const float*)a->x.ptr;
    p.x_bstride = a->x.batch_stride;
    p.HW = (int)HW;
    p.C = C;
    p.w = (const char*)a->w_packed + pl.woff[0];
    p.mft = pl.mft;
    p.bias = a->bias;
    p.resid = (const float*)a->resid.ptr;
    p.resid_bstride = a->resid.batch_stride;
    p.y = (float*)a->y.ptr;
    p.y_bstride = a->y.batch_stride;
    p.M = pl.rows;
    p.B = a->batch;
    p.act = a->act;
    p.range_flag = a->range_flag;
    // LAMA_GEMM_WS_NH: 2 = one 8-wave workgroup per CU over 64-pixel tiles, 1 = two 4-wave workgroups per CU over 32-pixel tiles
    static const int NH_env = lama_env_int("LAMA_GEMM_WS_NH", 1) == 2 ? 2 : 1;
    const int NH = io != CB_IO_F32 ? 1 : NH_env;
    p.tiles_per_img = (int)lama_ceil_div64(HW, GW_TILE(NH));
    p.ntiles = p.B * p.tiles_per_img;
    p.ntypes = pl.mft / 3;
    const int wgs = 256 * (3 - NH);   // persistent: every workgroup resident from the start
    if (p.ntypes > wgs) return LAMA_ERR_UNSUPPORTED;
    // even with one tile or less per workgroup slot the stationary-weights kernel beats the per-tile ones (4 x 256^2: 7.6 -> 6.7 ms
    // per batch, 1 x 512^2: 7.5 -> 6.7 ms, profiles/r01b_ab_gemm_ws_small.txt); only tiny launches keep them
    if (mode != 2 && (long long)p.ntiles * p.ntypes < 64) return LAMA_ERR_UNSUPPORTED;
    p.nslots = wgs / p.ntypes;
    if (p.nslots > p.ntiles) p.nslots = p.ntiles;
    const int grid = p.nslots * p.ntypes;
    if (grid <= 0) return LAMA_OK;
    { static const int abl = lama_env_int("LAMA_GW_ABLATE", 0); p.abl = abl; }   // profiling tools only
    { static const int prio = lama_env_int("LAMA_SIDE_PRIO", 1); p.prio = prio; }   // profiling tools: 0 = default wave priority
    const dim3 blk(GW_THREADS(NH));
    const size_t lds = GW_LDS_BYTES(NH);
#if defined(LAMA_PROFILING) && !CB_HALF
    if (CB_F16 && C == 384) {   // profiling tools only: per-workgroup timeline, LAMA_GW_TRACE = device address of grid * 16 int64
        static const unsigned long long tr = lama_env_u64("LAMA_GW_TRACE");
        if (tr) {
            p.trace = reinterpret_cast<long long*>(tr);
            if (NH == 2) hipLaunchKernelGGL((CB_NAME(gemm1x1_ws_kernel)<6, true, 2, true>), dim3(grid), blk, lds, stream, p);
            else hipLaunchKernelGGL((CB_NAME(gemm1x1_ws_kernel)<6, true, 1, true>), dim3(grid), blk, lds, stream, p);
            LAMA_CHECK_LAUNCH();
            return LAMA_OK;
        }
    }
#endif
    const bool rs = p.resid != nullptr;
#if CB_HALF
    if (io == CB_IO_F16) {   // fp16 activations, one product (NH = 1 geometry only)
#define GW_CASE_H(nch, rs_) hipLaunchKernelGGL((CB_NAME(gemm1x1_ws_kernel)<nch, rs_, 1, false, true>), dim3(grid), blk, lds, stream, p)
        if (C == 384) { if (rs) GW_CASE_H(6, true); else GW_CASE_H(6, false); }
        else { if (rs) GW_CASE_H(3, true); else GW_CASE_H(3, false); }
#undef GW_CASE_H
        LAMA_CHECK_LAUNCH();
        return LAMA_OK;
    }
    if (io == CB_IO_F32_F16) {   // SpectralTransform.conv1 reads the fp32 residual stream and writes fp16
        if (C != 384 || rs) return LAMA_ERR_UNSUPPORTED;
        hipLaunchKernelGGL((CB_NAME(gemm1x1_ws_kernel)<6, false, 1, false, true, false, true>), dim3(grid), blk, lds, stream, p);
        LAMA_CHECK_LAUNCH();
        return LAMA_OK;
    }
    return LAMA_ERR_UNSUPPORTED;
#else
    if (io != CB_IO_F32) return LAMA_ERR_UNSUPPORTED;
#define GW_CASE(nch, rs, nh) hipLaunchKernelGGL((CB_NAME(gemm1x1_ws_kernel)<nch, rs, nh>), dim3(grid), blk, lds, stream, p)
    if (NH == 2) {
        if (C == 384) { if (rs) GW_CASE(6, true, 2); else GW_CASE(6, false, 2); }
        else { if (rs) GW_CASE(3, true, 2); else GW_CASE(3, false, 2); }
    } else {
        if (C == 384) { if (rs) GW_CASE(6, true, 1); else GW_CASE(6, false, 1); }
        else { if (rs) GW_CASE(3, true, 1); else GW_CASE(3, false, 1); }
    }
#undef GW_CASE
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
#endif
}

// 3x3 stride 2 (the downsampling convs): two 4-wave workgroups per CU, 16-channel chunks, five staging units per thread
int cw_launch_s2(hipStream_t st, const CbParams& p, int grid, size_t shmem, int io) {
#if CB_HALF
    if (io != CB_IO_F16 && io != CB_IO_F16_F32) return LAMA_ERR_UNSUPPORTED;   // the last downsample writes the fp32 residual stream
    if (io == CB_IO_F16) hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 1, 0, 0, 4, 1, 0, 0, true, true, true, true, false, 5>), dim3(grid), dim3(256), shmem, st, p);
    else hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 1, 0, 0, 4, 1, 0, 0, true, true, true, false, false, 5>), dim3(grid), dim3(256), shmem, st, p);
#else
    if (io & (CB_IO_XS | CB_IO_YS)) {   // LAMA_DT_SPLIT16 on either side: the 4 x 1 geometry only
        if (io & ~(CB_IO_XS | CB_IO_YS)) return LAMA_ERR_UNSUPPORTED;
#define CW_S2_SPLIT(xs, ys) hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 1, 0, 0, 4, 1, 0, 2, false, false, false, false, false, 5, false, xs, ys>), dim3(grid), dim3(256), shmem, st, p)
        if (io == (CB_IO_XS | CB_IO_YS)) CW_S2_SPLIT(true, true);
        else if (io == CB_IO_XS) CW_S2_SPLIT(true, false);
        else CW_S2_SPLIT(false, true);
#undef CW_S2_SPLIT
        LAMA_CHECK_LAUNCH();
        return LAMA_OK;
    }
    if (io != CB_IO_F32) return LAMA_ERR_UNSUPPORTED;
    static const int geo = lama_env_int("LAMA_CW_S2", 1);   // 2 (profiling tools): one 8-wave workgroup per CU, K split between two wave groups
#if defined(LAMA_PROFILING)
    if (CB_F16 && geo != 2) {   // profiling tools only: timing ablations of the patch staging (results wrong; profiles/presplit_outer.txt)
        static const int abl = lama_env_int("LAMA_CW_ABLATE", 0);
#define CW_ABL_S2(v) \
    if (abl == v) { hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 1, 0, 0, 4, 1, v, 2, false, false, false, false, false, 5>), dim3(grid), dim3(256), shmem, st, p); LAMA_CHECK_LAUNCH(); return LAMA_OK; }
        CW_ABL_S2(4) CW_ABL_S2(16) CW_ABL_S2(32)
#undef CW_ABL_S2
    }
#endif
    if (geo == 2) hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 0, 0, 4, 2, 0, 2, false, false, false, false, false, 5>), dim3(grid), dim3(512), shmem, st, p);
    else hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 1, 0, 0, 4, 1, 0, 2, false, false, false, false, false, 5>), dim3(grid), dim3(256), shmem, st, p);
#endif
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// round 6: the shape of a 128-pixel tile of the 3x3 kernels -- 32 x 4, 16 x 8 or 8 x 16 pixels (TWlog 5 / 4 / 3).  Planes that are not multiples of the
// tile leave partly empty tiles, and at one workgroup per CU a launch of 257 workgroups takes as long as one of 512: a 135 x 240 plane (1080 x 1920
// input) is 8 x 34 = 272 tiles of 32 x 4 but 15 x 17 = 255 tiles of 16 x 8 -- one round instead of two for the local AND the global launch of every
// layer (152 -> ~100 us each).  The shape with the fewest rounds of 256 workgroups wins (a part of a batch counts with its siblings), ties keep
// 32 x 4 (the row-rolling fragment reads exist for 32-pixel tile rows only).  Returns the tiles of one image.  LAMA_CW_TWLOG (profiling build): 3 / 4 / 5 force a shape.
static long long cw_pick_tile(int GW, int GH, int batch, unsigned flags, int* twlog_out) {
    int twlog = 5;
    while (twlog > 3 && (1 << (twlog - 1)) >= GW) --twlog;
    if (twlog == 5) {
        long long best_rounds = 0;
        for (int tl = 5; tl >= 3; --tl) {
            const long long nt = ((long long)batch * lama_ceil_div(GW, 1 << tl) * lama_ceil_div(GH, 128 >> tl)) << LAMA_CONV_SIBLINGS_LOG2(flags);
            const long long rounds = (nt + 255) / 256;
            if (tl == 5 || rounds < best_rounds) { best_rounds = rounds; twlog = tl; }
        }
        static const int force = lama_env_int("LAMA_CW_TWLOG", 0);
        if (force >= 3 && force <= 5) twlog = force;
    }
    *twlog_out = twlog;
    return (long long)lama_ceil_div(GW, 1 << twlog) * lama_ceil_div(GH, 128 >> twlog);
}

int cw_try_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, const CbPlan* pl2, int Ho, int Wo, int io) {
    if (!pl2) {
        int rc = gk_try_launch(stream, a, pl, Ho, Wo, io);
        if (rc != LAMA_ERR_UNSUPPORTED) return rc;
        rc = g4_try_launch(stream, a, pl, Ho, Wo, io);
        if (rc != LAMA_ERR_UNSUPPORTED) return rc;
        rc = gw_try_launch(stream, a, pl, Ho, Wo, io);
        if (rc != LAMA_ERR_UNSUPPORTED) return rc;
    }
    if (!cw_enabled() || a->transposed || (a->stride != 1 && a->stride != 2) || pl.mode != 0 || pl.nseg != 1) return LAMA_ERR_UNSUPPORTED;
    const bool s2 = a->stride == 2;   // the three downsampling convs: same kernel, parity-split patch columns, five staging units per thread
    if (s2 && (pl.T[0] != 9 || pl2 || a->pad != 1)) return LAMA_ERR_UNSUPPORTED;
    const bool split_io = (io & (CB_IO_XS | CB_IO_YS)) != 0;   // LAMA_DT_SPLIT16 tensors: the stride-2 launch only, whole octets, no residual
    if (split_io && (!s2 || CB_HALF || a->resid.ptr || a->x.C % 8 != 0 || pl.rows % 8 != 0 || pl.rows != a->y.C)) return LAMA_ERR_UNSUPPORTED;
    if (split_io && ((long long)a->x.C * a->x.H * a->x.W >= (1ll << 29) || (long long)a->y.C * Ho * Wo >= (1ll << 29))) return LAMA_ERR_UNSUPPORTED;   // 32-bit byte offsets
    const int T1 = pl.T[0];
    int twlog3 = 5;
    const long long tiles_img = (T1 == 9 && !s2) ? cw_pick_tile(Wo, Ho, a->batch, a->flags, &twlog3) : lama_ceil_div64((long long)Ho * Wo, 128);   // 128-pixel tiles of one image
    if (!((T1 == 9 && a->x.C % 32 == 0) || (T1 == 1 && a->x.C % 64 == 0))) return LAMA_ERR_UNSUPPORTED;
    if (pl2 && a->x2.C % 64 != 0) return LAMA_ERR_UNSUPPORTED;
    if (pl.rows < 96) return LAMA_ERR_UNSUPPORTED;          // a 128-row tile would be mostly padding
    // workgroup geometry: M-waves x K-groups (conv_wreg_dev.inc)
    int WMV = 4, KG = 2;
#if CB_HALF
    const int s2geo = 1;
#else
    static const int s2geo = lama_env_int("LAMA_CW_S2", 1);
#endif
    if (s2 && (s2geo != 2 || split_io)) KG = 1;
    // stride-1 3x3 without second operand (the local conv), geometry by launch size (workgroups of 128 pixels x 128 rows):
    //   >= 512: two 4-wave workgroups per CU (16-channel chunks) instead of one 8-wave K-split workgroup: the launch is one or more full
    //           rounds either way, but the two workgroups of a CU run out of phase.  Kernel alone 426 -> 413 us at 4 x 1024^2; with the
    //           spectral branch beside it +2.5 % images/s at 16 x 512^2, +5 % at 4 x 1024^2 (profiles/r02_ab_local_conv_geometry_by_size.txt)
    //   LAMA_CONV_COOPERATIVE and 224 ... 320 (one workgroup per CU covers the launch): ONE 4-wave workgroup per CU (one wave per SIMD,
    //           32-channel chunks, a six-deep A ring), 232 of the 512 registers of a SIMD lane instead of 2 x 170: the spectral branch's
    //           GEMM / FFT workgroups of the other stream fit beside it.  96 instead of 90 us alone, +2.7 ... 3.7 % images/s at 8 x 512^2
    //           with the branch overlapped (DESIGN.md 4.12); neutral at 192 workgroups, -9 % at 128 (half of the CUs are free for the
    //           branch anyway and the K-split workgroup finishes a lone tile sooner), hence the lower bound
    //   otherwise: one 8-wave workgroup per 128-pixel tile, K split over two wave groups
    // LAMA_CW_41 (profiling tools, emulator tests): -1 = always the last, 2 = always the first, 3 = the cooperative geometry whatever the
    // flag (up to 320 workgroups), -2 = the flag rule without the >= 512 rule
    const int g41 = lama_env_int("LAMA_CW_41", 0);   // read per launch (profiling build): the emulator tests switch it per case
    bool geo41 = false, coop41 = false;
    if (pl.T[0] == 9 && !pl2 && !s2 && pl.mft % 4 == 0) {
        const long long wgs = (long long)a->batch * tiles_img * (pl.mft / 4);
        const bool f32io = (io == CB_IO_F32) && !CB_HALF;
        if (g41 == 2 || ((g41 == 0 || g41 == 1) && wgs >= 512 && f32io)) { geo41 = true; KG = 1; }
        const bool flagged = (a->flags & LAMA_CONV_COOPERATIVE) && g41 != -1 && wgs >= 224;
        if ((flagged || g41 == 3) && f32io && wgs <= 320) { geo41 = true; coop41 = true; KG = 1; }
    }
    // all 384 rows of the global branch in one 12-wave workgroup per 128-pixel tile (patch staged once, one round on 256 CUs at 8 x 512^2) --
    // when the launch has enough tiles: below LAMA_CW_G12_MIN tiles three 128-row workgroups per tile fill more of the chip (1 x 512^2 =
    // 32 tiles: 5.72 -> 4.36 ms per image, 2 x 512^2: 6.33 -> 5.04 ms per batch; profiles/r03_ab_global_geometry_small_batch.txt).
    // LAMA_CW_G12 (profiling tools): 0 = always three tiles, 2 = always one workgroup.
    static const int g12 = lama_env_int("LAMA_CW_G12", 1);
    static const int g12_min = lama_env_int("LAMA_CW_G12_MIN", 160);
    // (a part of a batch beside its siblings -- LAMA_CONV_SIBLINGS_*, v109 -- counts with their tiles: the parts fill the chip together)
    const long long tiles_g = ((long long)a->batch * tiles_img) << LAMA_CONV_SIBLINGS_LOG2(a->flags);
    if (T1 == 9 && pl2 && pl.mft == 12 && (g12 == 2 || (g12 == 1 && tiles_g >= g12_min))) { WMV = 12; KG = 1; }
    if (T1 == 1 && !pl2) {
        // 1x1: short K, the launch is bound by memory latency and by the patch staging rather than the matrix cores -> ALL rows
        // in one 12-wave workgroup per pixel tile (the patch is loaded and split once, not once per 128-row tile) when the
        // launch still covers a good part of the chip: 384 rows = 12 M-waves, 192 rows = 6 M-waves x 2 K-groups.
        // LAMA_CW_1X1: 0 keeps the 128-row tiles (A/B runs of the profiling tools), 2 takes the full-M workgroups whatever the
        // launch size (emulator tests); read once.
        static const int full_m = lama_env_int("LAMA_CW_1X1", 1);
        const long long tiles128 = (long long)a->batch * lama_ceil_div64((long long)Ho * Wo, 128);
        const bool want = full_m >= 2 || (full_m == 1 && tiles128 >= 96);
        if (full_m == 3 && pl.mft == 12) { WMV = 6; KG = 2; }   // profiling tools: 384 rows as two 192-row K-split workgroups
        else if (want && pl.mft == 12) { WMV = 12; KG = 1; }
        else if (want && pl.mft == 6) { WMV = 6; KG = 2; }
        else if (pl.mft % 4 != 0) return LAMA_ERR_UNSUPPORTED;   // no partly empty 128-row tile
    }
    const int threads = 64 * WMV * KG;
    if ((long long)a->x.C * a->x.H * a->x.W >= (1ll << 31) || (pl2 && (long long)a->x2.C * a->x2.H * a->x2.W >= (1ll << 31)))
        return LAMA_ERR_UNSUPPORTED;
    CbParams p;
    memset(&p, 0, sizeof(p));
    const bool flat = (T1 == 1 && a->pad == 0 && !pl2);
    p.bias = a->bias;
    p.resid = (const float*)a->resid.ptr;
    p.resid_bstride = a->resid.batch_stride;
    p.y = (float*)a->y.ptr;
    p.y_bstride = a->y.batch_stride;
    p.M = pl.rows;
    p.MT = lama_ceil_div(pl.mft, WMV);
    p.B = a->batch;
    p.act = a->act;
    p.range_flag = a->range_flag;
    p.ostep = 1;
    if (flat) { p.Ho = 1; p.Wo = Ho * Wo; p.GH = 1; p.GW = Ho * Wo; }
    else { p.Ho = Ho; p.Wo = Wo; p.GH = Ho; p.GW = Wo; }
    int twlog = flat ? 7 : 5;
    while (twlog > 3 && (1 << (twlog - 1)) >= p.GW) --twlog;
    if (T1 == 9 && !s2) twlog = twlog3;
    const int TW = 1 << twlog, TH = 128 >> twlog;
    p.TWlog = twlog;
    p.tiles_x = lama_ceil_div(p.GW, TW);
    p.tiles_y = lama_ceil_div(p.GH, TH);
    const int KSC1 = T1 == 9 ? (KG == 1 && WMV == 4 && !coop41 ? 1 : 2) : 4;
    cb_fill_seg(&p.s1, a->x, (const char*)a->w_packed + pl.woff[0], pl, 0, a->stride, a->pad_mode, TH, TW, flat);
    p.s1.vpad = a->pad;
    int units = p.s1.PH * p.s1.PW * 2 * KSC1;
    long long pbytes = (long long)2 * (2 * KSC1 * p.s1.npix * 16 + 16);   // hi + lo planes, each followed by a 16-byte dump slot
    if (pl2) {
        cb_fill_seg(&p.s2, a->x2, (const char*)a->w2_packed, *pl2, 0, 1, LAMA_PAD_ZERO, TH, TW, false);
        const int u2 = p.s2.PH * p.s2.PW * 8;
        const long long p2 = (long long)2 * (8 * p.s2.npix * 16 + 16);
        units = u2 > units ? u2 : units;
        pbytes = p2 > pbytes ? p2 : pbytes;
    }
    if (units > (s2 ? 5 : (coop41 ? 4 : 2)) * threads) return LAMA_ERR_UNSUPPORTED;
    p.pbytes = (int)pbytes;
    size_t shmem = 2 * (size_t)pbytes;
    if (KG == 2 && shmem < (size_t)(threads / 64) * 8192) shmem = (size_t)(threads / 64) * 8192;   // K-group exchange: 8 KiB per wave
    if (shmem > 160 * 1024) return LAMA_ERR_UNSUPPORTED;
    const int grid = p.B * p.tiles_x * p.tiles_y * p.MT;
    if (grid <= 0) return LAMA_OK;
#if defined(LAMA_PROFILING) && !CB_HALF
    if (CB_F16 && T1 == 9 && !pl2 && WMV == 4 && !s2) {   // profiling tools only: timing ablations
        static const int abl = lama_env_int("LAMA_CW_ABLATE", 0);
#define CW_ABL(v) \
    if (abl == v && p.TWlog == 5) { hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 0, 0, 4, 2, v, 2, false, false, false, false, true>), dim3(grid), dim3(512), shmem, stream, p); LAMA_CHECK_LAUNCH(); return LAMA_OK; }
        CW_ABL(1) CW_ABL(2) CW_ABL(4) CW_ABL(3) CW_ABL(7) CW_ABL(8) CW_ABL(16) CW_ABL(32) CW_ABL(128) CW_ABL(132) CW_ABL(135)
#undef CW_ABL
        static const int sch = lama_env_int("LAMA_CW_SCHED", 2);
        if (sch == 0) { hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 0, 0, 4, 2, 0, 0>), dim3(grid), dim3(512), shmem, stream, p); LAMA_CHECK_LAUNCH(); return LAMA_OK; }
        if (sch == 1) { hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 0, 0, 4, 2, 0, 1>), dim3(grid), dim3(512), shmem, stream, p); LAMA_CHECK_LAUNCH(); return LAMA_OK; }
    }
    if (CB_F16 && pl2 && WMV == 12 && T1 == 9 && io == CB_IO_F32) {   // profiling tools only: timing ablations of the global-branch launch (results wrong)
        static const int ablg = lama_env_int("LAMA_CW_ABLATE", 0);          // 1 = no weight loads in the loops, 256 = waves F >= 6 stream fragment F - 6
        if (ablg == 1 || ablg == 256) {
            if (a->fuse1_w && pl.rows == 384) {
                p.f1_w = (const char*)a->fuse1_w; p.f1_bias = a->fuse1_bias; p.f1_y = (float*)a->fuse1_y.ptr; p.f1_y_bstride = a->fuse1_y.batch_stride;
                const size_t sh1 = shmem < 144 * 1024 ? 144 * 1024 : shmem;
                if (ablg == 1) hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 1, 4, 12, 1, 1, 2, false, false, false, false, false, 2, true>), dim3(grid), dim3(768), sh1, stream, p);
                else hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 1, 4, 12, 1, 256, 2, false, false, false, false, false, 2, true>), dim3(grid), dim3(768), sh1, stream, p);
            } else if (ablg == 1) hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 1, 4, 12, 1, 1>), dim3(grid), dim3(768), shmem, stream, p);
            else hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 1, 4, 12, 1, 256>), dim3(grid), dim3(768), shmem, stream, p);
            LAMA_CHECK_LAUNCH();
            return LAMA_OK;
        }
    }
    if (CB_F16 && pl2 && WMV == 12) {   // profiling tools only: timeline of the global-branch launch
        static const unsigned long long tr2 = lama_env_u64("LAMA_CW_TRACE");
        if (tr2) {
            p.trace = reinterpret_cast<long long*>(tr2);
            hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 1, 4, 12, 1, 64>), dim3(grid), dim3(768), shmem, stream, p);
            LAMA_CHECK_LAUNCH();
            return LAMA_OK;
        }
    }
    if (CB_F16 && !pl2 && !s2) {   // profiling tools only: per-workgroup timeline, LAMA_CW_TRACE = device address of grid * 32 int64
        static const unsigned long long tr = lama_env_u64("LAMA_CW_TRACE");
        if (tr) {
            p.trace = reinterpret_cast<long long*>(tr);
            if (T1 == 9 && p.TWlog == 5) hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 0, 0, 4, 2, 64, 2, false, false, false, false, true>), dim3(grid), dim3(512), shmem, stream, p);
            else if (T1 == 9) hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 0, 0, 4, 2, 64>), dim3(grid), dim3(512), shmem, stream, p);
            else if (WMV == 12) hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<1, 4, 0, 0, 12, 1, 64>), dim3(grid), dim3(768), shmem, stream, p);
            else if (WMV == 6) hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<1, 4, 0, 0, 6, 2, 64>), dim3(grid), dim3(768), shmem, stream, p);
            else hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<1, 4, 0, 0, 4, 2, 64>), dim3(grid), dim3(512), shmem, stream, p);
            LAMA_CHECK_LAUNCH();
            return LAMA_OK;
        }
    }
#endif
    if (T1 == 9 && s2) return cw_launch_s2(stream, p, grid, shmem, io);
#if !CB_HALF
    if (coop41) {   // one 4-wave workgroup per CU (1 wave per SIMD, 32-channel chunks): the other stream's workgroups co-reside
        if (p.TWlog == 5) hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 0, 0, 4, 1, 0, 2, false, false, false, false, true, 4>), dim3(grid), dim3(256), shmem, stream, p);
        else hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 0, 0, 4, 1, 0, 2, false, false, false, false, false, 4>), dim3(grid), dim3(256), shmem, stream, p);
        LAMA_CHECK_LAUNCH();
        return LAMA_OK;
    }
#endif
    if (geo41) return cw_launch_t<9, 1, 0, 0, 4, 1>(stream, p, grid, shmem, io);
    if (T1 == 9 && !pl2) return cw_launch_t<9, 2, 0, 0, 4, 2>(stream, p, grid, shmem, io);
    if (a->fuse1_w && !(T1 == 9 && pl2 && WMV == 12 && io == CB_IO_F32 && pl.rows == 384)) return LAMA_ERR_UNSUPPORTED;
#if !CB_HALF
    if (a->fuse1_w) {   // the global-branch launch with SpectralTransform.conv1 of the next layer in its epilogue
        p.f1_w = (const char*)a->fuse1_w;
        p.f1_bias = a->fuse1_bias;
        p.f1_y = (float*)a->fuse1_y.ptr;
        p.f1_y_bstride = a->fuse1_y.batch_stride;
        if (shmem < 144 * 1024) shmem = 144 * 1024;   // B operands of the fused GEMM (24 k-steps x 2 pixel fragments x (hi, lo) KiB) + 48 KiB of K-half hand-over
        hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<9, 2, 1, 4, 12, 1, 0, 2, false, false, false, false, false, 2, true>), dim3(grid), dim3(768), shmem, stream, p);
        LAMA_CHECK_LAUNCH();
        return LAMA_OK;
    }
#endif
    if (T1 == 9 && pl2 && WMV == 12) return cw_launch_t<9, 2, 1, 4, 12, 1>(stream, p, grid, shmem, io);
    if (T1 == 9 && pl2) return cw_launch_t<9, 2, 1, 4, 4, 2>(stream, p, grid, shmem, io);
    if (T1 == 1 && !pl2 && WMV == 12) return cw_launch_t<1, 4, 0, 0, 12, 1>(stream, p, grid, shmem, io);
    if (T1 == 1 && !pl2 && WMV == 6) return cw_launch_t<1, 4, 0, 0, 6, 2>(stream, p, grid, shmem, io);
    if (T1 == 1 && !pl2) return cw_launch_t<1, 4, 0, 0, 4, 2>(stream, p, grid, shmem, io);
    return LAMA_ERR_UNSUPPORTED;
}

// ConvTranspose2d(k3, s2, p1, op1) as ONE launch, all four output-parity classes in one wave (convt2_kernel, convt_dev.inc).  LAMA_CT (profiling
// build): 0 = off (A/B runs against the fused LDS-staged launch); read per launch.
// ``tl`` (lama_conv2d_list_fwd): the LIST instantiation over the caller's tile list, same grid; tl->dry: every check, no launch.
int ct_try_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, int Ho, int Wo, int io, const LamaTileList* tl = nullptr) {
#if CB_HALF
    (void)stream; (void)a; (void)pl; (void)Ho; (void)Wo; (void)io; (void)tl;
    return LAMA_ERR_UNSUPPORTED;
#else
    const int mode = lama_env_int("LAMA_CT", 1);
    if (mode == 0 || !a->transposed || pl.nseg != 5 || pl.mode != 0 || io != CB_IO_F32 || a->resid.ptr || a->fuse1_w) return LAMA_ERR_UNSUPPORTED;
    const int C = a->x.C, H = a->x.H, W = a->x.W, M = pl.rows;
    // (round 6: any H, W -- ragged last tiles: the patch requests beyond the plane already read zeros, the stores are predicated)
    if (C % 32 != 0 || M % 64 != 0 || H < 1 || W < 1 || Ho != 2 * H || Wo != 2 * W) return LAMA_ERR_UNSUPPORTED;
    if ((long long)C * H * W * 4 >= (1ll << 31)) return LAMA_ERR_UNSUPPORTED;       // 32-bit byte offsets inside one image
    CtParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const float*)a->x.ptr;
    p.x_bstride = a->x.batch_stride;
    p.C = C; p.H = H; p.W = W;
    for (int c = 0; c < 4; ++c) {
        const int cls = c + 1;                                           // plan classes 1..4: (py, px) = (1,1) (1,0) (0,1) (0,0)
        p.w[c] = (const char*)a->w_packed + pl.woff[cls];
        p.T[c] = pl.T[cls];
        p.py[c] = pl.oy0[cls]; p.px[c] = pl.ox0[cls];
        if (pl.T[cls] != (1 + p.py[c]) * (1 + p.px[c])) return LAMA_ERR_UNSUPPORTED;
        for (int t = 0; t < pl.T[cls]; ++t) p.off[c][t] = pl.dy[cls][t] * CT_PWS + pl.dx[cls][t];
    }
    if (p.T[0] != 4 || p.T[3] != 1 || p.T[1] != 2 || p.T[2] != 2) return LAMA_ERR_UNSUPPORTED;
    // the kernel shares B fragments between the classes by position: the plan must match its compile-time tap table; identity / ReLU epilogues
    bool table_ok = true;
    for (int q = 0; q < 9; ++q) table_ok = table_ok && p.off[c2_cls(q)][c2_tap(q)] == c2_dy(q) * CT_PWS + c2_dx(q);
    for (int c = 0; c < 4; ++c) table_ok = table_ok && p.py[c] == (c < 2 ? 1 : 0) && p.px[c] == ((c == 0 || c == 2) ? 1 : 0);
    if (!table_ok || (a->act != LAMA_ACT_NONE && a->act != LAMA_ACT_RELU)) return LAMA_ERR_UNSUPPORTED;
    p.mft = pl.mft;
    p.bias = a->bias;
    p.y = (float*)a->y.ptr;
    p.y_bstride = a->y.batch_stride;
    p.M = M; p.B = a->batch; p.act = a->act;
    p.tiles_x = lama_ceil_div(W, 32); p.tiles_y = lama_ceil_div(H, 4); p.MG = M / 64;
    p.range_flag = a->range_flag;
    if ((a->y.batch_stride % 4) != 0 || ((uintptr_t)a->y.ptr & 15) != 0) return LAMA_ERR_UNSUPPORTED;   // 16-byte stores
    const long long tiles = (long long)a->batch * p.tiles_x * p.tiles_y * p.MG;
    if (tiles <= 0) return LAMA_OK;
    if (tiles >= (1ll << 30)) return LAMA_ERR_UNSUPPORTED;
    if (tl && tl->dry) return LAMA_OK;
    { static const int abl = lama_env_int("LAMA_CT_ABLATE", 0); p.abl = abl; }      // profiling tools only
    long long grid = tiles < 512 ? tiles : 512;                                      // persistent: two workgroups per CU walk tiles w, w + grid, ...
    { const int cap = lama_env_int("LAMA_CT_GRID", 0); if (cap > 0 && grid > cap) grid = cap; }   // emulator tests: several tiles per workgroup
    if (tl) {
        p.list = tl->list; p.count = tl->count;
        hipLaunchKernelGGL(CB_NAME(convt2_kernel)<true>, dim3((int)grid), dim3(C2_THREADS), C2_LDS_BYTES, stream, p);
    } else
        hipLaunchKernelGGL(CB_NAME(convt2_kernel)<false>, dim3((int)grid), dim3(C2_THREADS), C2_LDS_BYTES, stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
#endif
}

// Stem (7x7, cin <= 4, 33..64 output channels, reflect pad 3): conv_stem_dev.inc.  LAMA_STEM_WS: 0 disables it (A/B runs of the
// profiling tools), 2 takes it whatever the launch size (emulator tests); read once.
int stem_try_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, int Ho, int Wo, int io) {
    if (io != CB_IO_F32 && io != CB_IO_F32_F16 && io != CB_IO_YS) return LAMA_ERR_UNSUPPORTED;
    if (io == CB_IO_YS && pl.rows % 8 != 0) return LAMA_ERR_UNSUPPORTED;   // LAMA_DT_SPLIT16: whole channel octets
    static const int mode = lama_env_int("LAMA_STEM_WS", 1);
    if (mode == 0 || pl.mode != 1 || pl.mft != 2 || a->transposed || a->stride != 1 || a->pad != 3 || a->pad_mode != LAMA_PAD_REFLECT ||
        a->resid.ptr || a->x.H < 4 || a->x.W < 4)
        return LAMA_ERR_UNSUPPORTED;
    const long long HW = (long long)Ho * Wo;
    if ((long long)a->x.C * HW >= (1ll << 29) || 64 * HW >= (1ll << 29)) return LAMA_ERR_UNSUPPORTED;   // 32-bit byte offsets inside one image
    StemParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const float*)a->x.ptr;
    p.x_bstride = a->x.batch_stride;
    p.C = a->x.C; p.H = Ho; p.W = Wo;
    p.w = (const char*)a->w_packed + pl.woff[0];
    p.mft = pl.mft;
    p.bias = a->bias;
    p.y = (float*)a->y.ptr;
    p.y_bstride = a->y.batch_stride;
    p.M = pl.rows;
    p.B = a->batch;
    p.act = a->act;
    p.range_flag = a->range_flag;
    p.tx = lama_ceil_div(Wo, 32);
    const long long ntiles = (long long)a->batch * Ho * p.tx;
    if (mode != 2 && ntiles < 4096) return LAMA_ERR_UNSUPPORTED;   // persistent: 1024 wave pairs want a few dozen output rows each
    // a wave pair walks down a column of 32-pixel segments; columns are cut into ns vertical parts so that there are ~1024 parts
    // (every part pays 6 extra input rows to fill its window)
    const long long cols = (long long)a->batch * p.tx;
    long long ns = cols >= 1024 ? 1 : lama_ceil_div64(1024, cols);
    if (ns > Ho) ns = Ho;
    p.rs = (int)lama_ceil_div64(Ho, ns);
    p.ns = lama_ceil_div(Ho, p.rs);
    if (cols * p.ns >= (1ll << 31)) return LAMA_ERR_UNSUPPORTED;
    p.nseg = (int)(cols * p.ns);
    int grid = 512;                                                  // two 4-wave workgroups per CU
    if ((long long)grid * 2 > p.nseg) grid = (p.nseg + 1) / 2;
#if CB_HALF
    if (io != CB_IO_F32_F16) return LAMA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(CB_NAME(stem7_ws_kernel)<true>, dim3(grid), dim3(256), STEM_LDS_BYTES, stream, p);
#else
    if (io == CB_IO_YS) hipLaunchKernelGGL((CB_NAME(stem7_ws_kernel)<false, true>), dim3(grid), dim3(256), STEM_LDS_BYTES, stream, p);
    else if (io != CB_IO_F32) return LAMA_ERR_UNSUPPORTED;
    else hipLaunchKernelGGL(CB_NAME(stem7_ws_kernel)<false>, dim3(grid), dim3(256), STEM_LDS_BYTES, stream, p);
#endif
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// Head (7x7, 64 input channels, <= 4 output channels, reflect pad 3): conv_head_dev.inc.  LAMA_HEAD_WS: 0 disables it (A/B runs of
// the profiling tools), 2 takes it whatever the launch size (emulator tests); read once.
// ``tl`` (lama_conv2d_list_fwd): the LIST instantiation over the caller's segment list, cut into parts of tl->head_rs rows (the host cannot know
// the count, so the parts are small and the grid is the resident 768); fp32 tensors only; tl->dry: every check, no launch.
int head_try_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, int Ho, int Wo, int io, const LamaTileList* tl = nullptr) {
    if (io != CB_IO_F32 && io != CB_IO_F16_F32) return LAMA_ERR_UNSUPPORTED;
    if (tl && (io != CB_IO_F32 || tl->head_rs < HEAD_R || tl->head_rs % HEAD_R != 0)) return LAMA_ERR_UNSUPPORTED;
    static const int mode = lama_env_int("LAMA_HEAD_WS", 1);
    if (mode == 0 || pl.mode != 2 || pl.mft != 1 || a->x.C != 64 || a->y.C > 4 || a->transposed || a->stride != 1 || a->pad != 3 ||
        a->pad_mode != LAMA_PAD_REFLECT || a->resid.ptr || a->x.H < 4 || a->x.W < 4)
        return LAMA_ERR_UNSUPPORTED;
    const long long HW = (long long)Ho * Wo;
    if (64 * HW >= (1ll << 29)) return LAMA_ERR_UNSUPPORTED;   // 32-bit byte offsets inside one image
    HeadParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const float*)a->x.ptr;
    p.x_bstride = a->x.batch_stride;
    p.C = 64; p.H = Ho; p.W = Wo;
    p.w = (const char*)a->w_packed + pl.woff[0];
    p.bias = a->bias;
    p.y = (float*)a->y.ptr;
    p.y_bstride = a->y.batch_stride;
    p.M = a->y.C;
    p.B = a->batch;
    p.act = a->act;
    p.range_flag = a->range_flag;
    p.tx = lama_ceil_div(Wo, 26);
    const long long cols = (long long)a->batch * p.tx;
    if (mode != 2 && cols * Ho < 8192) return LAMA_ERR_UNSUPPORTED;   // persistent: 768 workgroups want a few dozen rows each
    // a workgroup walks down a column of segments; columns are cut into parts of rs rows (a multiple of HEAD_R: the register ring
    // of the kernel is unrolled by it).  Every part pays 6 + HEAD_D extra input rows and the parts should divide evenly among the
    // resident workgroups.
    const int wgs = 768;
    int best_rs = HEAD_R;
    double best = -1.0;
    for (int rs = HEAD_R; rs <= HEAD_R * lama_ceil_div(Ho, HEAD_R); rs += HEAD_R) {
        const long long nseg = cols * lama_ceil_div(Ho, rs);
        const double per = (double)nseg / wgs;
        const double rounds = per <= 1.0 ? 1.0 : (double)lama_ceil_div64(nseg, wgs);
        const double eff = (per <= 1.0 ? per : per / rounds) * rs / (rs + 6.0 + HEAD_D);
        if (eff > best) { best = eff; best_rs = rs; }
    }
    p.rs = tl ? tl->head_rs : best_rs;
    p.ns = lama_ceil_div(Ho, p.rs);
    if (cols * p.ns >= (1ll << 31)) return LAMA_ERR_UNSUPPORTED;
    p.nseg = (int)(cols * p.ns);
    const int grid = p.nseg < wgs ? p.nseg : wgs;
    if (tl && tl->dry) return LAMA_OK;
#if !CB_HALF
    if (tl) {
        p.list = tl->list; p.count = tl->count;
        hipLaunchKernelGGL((CB_NAME(head7_ws_kernel)<false, true>), dim3(grid), dim3(256), HEAD_LDS_BYTES, stream, p);
        LAMA_CHECK_LAUNCH();
        return LAMA_OK;
    }
#endif
#if CB_HALF
    if (io != CB_IO_F16_F32) return LAMA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(CB_NAME(head7_ws_kernel)<true>, dim3(grid), dim3(256), HEAD_LDS_BYTES, stream, p);
#else
    if (io != CB_IO_F32) return LAMA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(CB_NAME(head7_ws_kernel)<false>, dim3(grid), dim3(256), HEAD_LDS_BYTES, stream, p);
#endif
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}
