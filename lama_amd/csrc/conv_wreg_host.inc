// Host side of the split-precision convolution back end.  cb_route() decides which kernel family serves a launch -- every predicate, threshold and
// knob, no launch, no pointer dereferenced (addresses are looked at for alignment only) -- and one launcher per family fills the parameters and
// picks the instantiation.  A launch is routed ONCE: a launcher never answers LAMA_ERR_UNSUPPORTED (CB_ERR_ROUTE marks a route this file does not
// produce: a bug, never a reason to fall through), and lama_conv2d_route_query reports the same record without launching.
//
// The table, in order of precedence (the first family whose conditions hold takes the launch; nothing -> LAMA_ERR_UNSUPPORTED).  Which rows a
// launch may enter: a work-list launch (lama_conv2d_list_fwd) CT or HEAD only; a launch with a LAMA_DT_SPLIT16 tensor STEM (y only) or WR; a
// launch with a second operand WR or LDS; a launch with fuse1_w WR only (the fused conv1 is never silently dropped); every other all eight.
//   WK   gemm1x1_wk_kernel (gemm_wk_dev.inc): the FourierUnit's spectral GEMM with all of K in one wave.  Flat 1x1, fp32, 384 -> 384, no residual,
//        identity / ReLU, HW % 2 == 0, 8-byte aligned views, buffer spans below 0x7ffffff0 bytes.  256 .. 511 super-tiles of 64 pixels (a part of a
//        batch counts with its siblings) AND left-overs the fifth waves can take (256 .. 277: 8 x 512^2 = 264, 2 x 1024^2 = 260): smaller launches
//        fill the chip better with row groups of 96, from two rounds on the pipelined W4 super-tiles win (4 x 384 x 128 x 65 = 520 super-tiles 98.3
//        against 93.8 us, profiles/r03_gemm_wk.txt); left-overs too many for the fifth waves would be a whole second round (2 x 17 us where W4 needs
//        ntiles / 64 x 3.9 + 4.3).  Knobs: LAMA_GEMM_WK, LAMA_GEMM_WK_SLOTS, LAMA_GEMM_WK_AUX.
//   W4   gemm1x1_w4_kernel<., SUP = 2> (conv_ws_dev.inc): the same GEMMs over 64-pixel super-tiles of two interleaved MFMA tiles: 8-byte loads and
//        stores, one K-quarter exchange per 108 MFMAs of a wave, split and epilogue in the shadow of the MFMAs.  Flat 1x1, fp32, K = 192 / 384,
//        whole row groups of 96, identity / ReLU (the pipelined epilogue is branch-free), HW % 2 == 0, 8-byte aligned views, spans as WK.  From 256
//        super-tile x row-group units on (one workgroup per CU; smaller launches fill the chip better with 32-pixel tiles: WS).  SUP = 4 compiles
//        from the same source but spills (84 VGPRs): not instantiated.  Knobs: LAMA_GEMM_W4, LAMA_GEMM_W4_SLOTS.
//   WS   gemm1x1_ws_kernel (conv_ws_dev.inc): weights-stationary persistent GEMM.  Flat 1x1, K = 192 / 384, rows in groups of 96, one image below
//        2^31 bytes; fp32, or under LAMA_PREC_F16 all fp16 / (K = 384, no residual) fp32 in -> fp16 out.  From 64 tile x row-group units on: even
//        with one tile or less per workgroup slot it beats the per-tile kernels (4 x 256^2: 7.6 -> 6.7 ms per batch, 1 x 512^2: 7.5 -> 6.7 ms,
//        profiles/r01b_ab_gemm_ws_small.txt); only tiny launches keep them.  Knobs: LAMA_GEMM_WS, LAMA_GEMM_WS_NH.
//   WR   conv_wr_kernel (conv_wreg_dev.inc): weights in registers.  3x3 (cin % 32 == 0; stride 1, or stride 2 with pad 1) or 1x1 (cin % 64 == 0), a
//        fused 1x1 second operand (cin2 % 64 == 0) with the stride-1 3x3 only, >= 96 rows, staging units and LDS within the geometry's limits.
//        Workgroup geometry WMV M-waves x KG K-groups (wr_route): the local 3x3 by launch size (LAMA_CW_41), the global branch 12 x 1 from
//        LAMA_CW_G12_MIN = 160 tiles on, the 1x1 full-M from 96 tiles on, the stride-2 4 x 1; tile shape by cw_pick_tile.  LAMA_DT_SPLIT16 tensors:
//        the stride-2 4 x 1 launch only.  fuse1_w: the 12 x 1 launch with 384 rows and fp32 tensors only.  LAMA_PREC_F16: the element-type mixes of
//        cw_io_ok.  Knobs: LAMA_CONV_WR, LAMA_CW_S2, LAMA_CW_41, LAMA_CW_G12, LAMA_CW_G12_MIN, LAMA_CW_1X1, LAMA_CW_TWLOG, LAMA_CW_ROLL.
//   CT   convt2_kernel (convt_dev.inc): ConvTranspose2d(k3, s2, p1, op1) as ONE launch, all four output-parity classes in one wave.  fp32, cin % 32
//        == 0, cout % 64 == 0, any H, W (ragged last tiles), identity / ReLU, no residual, 16-byte aligned y.  Knobs: LAMA_CT, LAMA_CT_GRID.
//   STEM stem7_ws_kernel (conv_stem_dev.inc): 7x7 reflect pad 3, cin <= 4, 33 .. 64 output channels, planes of at least 4 x 4.  From 4096 32-pixel
//        row segments on (persistent: 1024 wave pairs want a few dozen output rows each).  fp32 (y may be LAMA_DT_SPLIT16 with whole channel
//        octets), or fp32 -> fp16 under LAMA_PREC_F16.  Knob: LAMA_STEM_WS.
//   HEAD head7_ws_kernel (conv_head_dev.inc): 7x7 reflect pad 3, 64 input channels, <= 4 output channels.  From 8192 26-column row segments on
//        (persistent: 768 workgroups want a few dozen rows each).  fp32, or fp16 -> fp32 under LAMA_PREC_F16; a work list: fp32, head_rs a multiple
//        of HEAD_R.  Knob: LAMA_HEAD_WS.
//   LDS  conv_kernel (conv_split3.inc): the LDS-staged kernel, everything else it has an instantiation for (lds_has_kernel), at most three staging
//        units per thread and 160 KiB of LDS.  Knob: LAMA_CB_BM.
//
// Knobs (profiling build only: the product's lama_env_int returns the default).  once = static const, read at the first launch that gets there;
// launch = read at every launch (the emulator tests switch them between cases).
//   LAMA_GEMM_WK        launch  0 off, 2 whatever the launch size           LAMA_CONV_WR      once  0 disables WR (A/B runs)
//   LAMA_GEMM_WK_SLOTS  launch  caps the workgroups (several rounds)        LAMA_CW_S2        once  2: stride 2 as one 8-wave K-split workgroup per CU
//   LAMA_GEMM_WK_AUX    launch  0: left-overs are one more round            LAMA_CW_41        launch  (wr_route)
//   LAMA_GEMM_W4        launch  0 off, 2 whatever the launch size           LAMA_CW_G12       once  0 always three 128-row tiles, 2 always 12 x 1
//   LAMA_GEMM_W4_SLOTS  launch  caps the workgroups per row group           LAMA_CW_G12_MIN   once  tiles from which the global branch is 12 x 1
//   LAMA_GEMM_WS        once    0 off, 2 whatever the launch size           LAMA_CW_1X1       once  0 128-row tiles, 2 full-M always, 3 two 6 x 2
//   LAMA_GEMM_WS_NH     once    2: one 8-wave workgroup per CU, 64-px tiles LAMA_CW_TWLOG     once  3 / 4 / 5 force the 3x3 tile shape
//   LAMA_CT             launch  0 off (A/B against the fused LDS launch)    LAMA_CW_ROLL      once  0: no row-rolling fragment reads
//   LAMA_CT_GRID        launch  caps the persistent grid                    LAMA_CB_BM        once  M tile of the LDS-staged transposed convs
//   LAMA_STEM_WS        once    0 off, 2 whatever the launch size           LAMA_HEAD_WS      once  0 off, 2 whatever the launch size
// Launcher-only knobs (ablations with wrong results, tracers, wave priority; they never change the route): LAMA_GW_ABLATE, LAMA_GW_TRACE,
// LAMA_SIDE_PRIO, LAMA_CW_ABLATE, LAMA_CW_SCHED, LAMA_CW_TRACE, LAMA_CT_ABLATE, LAMA_CB_ABLATE; all read once.

#define G4_SUP 2
#ifndef GK_DEFAULT_MODE
#define GK_DEFAULT_MODE 1
#endif

enum CbFamily {   // what lama_conv2d_route_query reports (lama_hip.h)
    CB_FAM_WK = LAMA_CONV_FAMILY_GEMM1X1_WK, CB_FAM_W4 = LAMA_CONV_FAMILY_GEMM1X1_W4, CB_FAM_WS = LAMA_CONV_FAMILY_GEMM1X1_WS,
    CB_FAM_WR = LAMA_CONV_FAMILY_CONV_WR, CB_FAM_CT = LAMA_CONV_FAMILY_CONVT2, CB_FAM_STEM = LAMA_CONV_FAMILY_STEM7,
    CB_FAM_HEAD = LAMA_CONV_FAMILY_HEAD7, CB_FAM_LDS = LAMA_CONV_FAMILY_LDS
};

struct CbRoute {
    int family;                 // CbFamily
    int io;                     // CB_IO_* of the launch
    bool list;                  // CT / HEAD over a work list
    // what selects the instantiation inside the family
    int WMV, KG, KSC1, twlog;   // WR: M-waves x K-groups, 16-channel sub-chunks of a chunk, log2 of the tile width
    bool s2, coop, roll, fuse1; // WR: stride 2, one 4-wave workgroup per CU, row-rolling fragment reads, fused conv1 (split io: io & (XS | YS))
    int NH, nch;                // WS: 32-pixel halves of a tile; WS / W4: 64-channel chunks of K
    bool rs;                    // WS / W4: residual
    int BM, BN, mode, maxu;     // LDS: M tile, pixel tile, folded 7x7 mode, staging units per thread (1 or 3)
    bool trf;                   // LDS: ConvTranspose2d's fused tap list
    // launch numbers the conditions needed anyway
    int grid, ntiles, nslots, aux, seg_rows;
    size_t shmem;
};

// the documented packing of lama_conv2d_route_query's *geometry (lama_hip.h)
int cb_route_geometry(const CbRoute& r) {
    const int xs = (r.io & CB_IO_XS) ? 1 : 0, ys = (r.io & CB_IO_YS) ? 1 : 0;
    switch (r.family) {
        case CB_FAM_WK: return r.aux;
        case CB_FAM_W4: return r.nch << 4 | (int)r.rs << 8;
        case CB_FAM_WS: return r.NH | r.nch << 4 | (int)r.rs << 8;
        case CB_FAM_WR: return LAMA_CONV_GEO_WR(r.WMV, r.KG, r.KSC1, r.twlog, (int)r.s2, (int)r.coop, (int)r.roll, (int)r.fuse1, xs, ys);
        case CB_FAM_CT: case CB_FAM_HEAD: return r.list ? 1 : 0;
        case CB_FAM_STEM: return ys << 21;
        case CB_FAM_LDS: return r.BM | r.BN << 8 | r.mode << 20 | (int)r.trf << 22;
    }
    return 0;
}

// 32-bit-offset guard, one for every family: the bytes from element 0 of a view to the end of its image `batch - 1` (batch 1: one image of C x HW
// four-byte elements) stay below the family's `limit`
static inline bool cb_span_fits(long long bstride, int batch, long long C, long long HW, long long limit) {
    return ((long long)(batch - 1) * bstride + C * HW) * 4 < limit;
}
static inline bool cb_act_linear(const lama_conv2d_args* a) { return a->act == LAMA_ACT_NONE || a->act == LAMA_ACT_RELU; }
// the pointwise GEMMs: a 1x1 convolution over the flat pixel list
static inline bool gw_shape(const lama_conv2d_args* a, const CbPlan& pl) {
    return !a->transposed && a->stride == 1 && a->pad == 0 && pl.mode == 0 && pl.nseg == 1 && pl.T[0] == 1;
}
// WK / W4 address the whole batch through one buffer resource: 32-bit byte offsets, the out-of-range marker 0x7ffffff0 must stay past every span
static bool gw_batch_spans_fit(const lama_conv2d_args* a, const CbPlan& pl, long long HW) {
    return cb_span_fits(a->x.batch_stride, a->batch, a->x.C, HW, 0x7ffffff0ll) && cb_span_fits(a->y.batch_stride, a->batch, pl.rows, HW, 0x7ffffff0ll) &&
           (!a->resid.ptr || cb_span_fits(a->resid.batch_stride, a->batch, pl.rows, HW, 0x7ffffff0ll)) && (long long)a->batch * HW < (1ll << 30);
}

// ------------------------------------------------------------------------------------------------
// the rows of the table: conditions only
// ------------------------------------------------------------------------------------------------
bool wk_route(const lama_conv2d_args* a, const CbPlan& pl, long long HW, int io, CbRoute* r) {
#if CB_HALF
    (void)a; (void)pl; (void)HW; (void)io; (void)r;
    return false;
#else
    const int mode = lama_env_int("LAMA_GEMM_WK", GK_DEFAULT_MODE);
    if (mode == 0 || io != CB_IO_F32 || !gw_shape(a, pl)) return false;
    if (a->x.C != 384 || pl.mft != 12 || pl.rows != 384 || a->resid.ptr != nullptr || !cb_act_linear(a)) return false;
    if (HW % 2 != 0 || a->x.batch_stride % 2 != 0 || a->y.batch_stride % 2 != 0) return false;
    if (((uintptr_t)a->x.ptr | (uintptr_t)a->y.ptr) & 7) return false;
    if (!gw_batch_spans_fit(a, pl, HW)) return false;
    r->ntiles = (int)lama_ceil_div64((long long)a->batch * HW, 64);     // super-tiles over the flat pixel list of the batch
    // a part of a batch that runs beside its siblings (LAMA_CONV_SIBLINGS_*, v109) counts with their super-tiles: together they are the one-per-CU launch
    const long long ntiles_all = (long long)r->ntiles << LAMA_CONV_SIBLINGS_LOG2(a->flags);
    if (mode != 2 && (ntiles_all < 256 || ntiles_all >= 512)) return false;
    r->grid = r->ntiles < 256 ? r->ntiles : 256;                        // one workgroup per CU, resident from the start
    { const int cap = lama_env_int("LAMA_GEMM_WK_SLOTS", 0); if (cap > 0 && r->grid > cap) r->grid = cap; }
    if (r->grid > 0) {
        const int rem = r->ntiles % r->grid;
        r->aux = (rem > 0 && rem * 24 <= 2 * r->grid && lama_env_int("LAMA_GEMM_WK_AUX", 1) != 0) ? 1 : 0;
        if (mode != 2 && rem > 0 && !r->aux) return false;                       // production: one round + fifth waves only
        if (mode != 2 && r->ntiles < 256 && ntiles_all >= 256 + 22) return false;   // (siblings: the whole batch would not have taken this kernel either)
    }
    return true;
#endif
}

bool w4_route(const lama_conv2d_args* a, const CbPlan& pl, long long HW, int io, CbRoute* r) {
#if CB_HALF
    (void)a; (void)pl; (void)HW; (void)io; (void)r;
    return false;
#else
    const int mode = lama_env_int("LAMA_GEMM_W4", 1);
    if (mode == 0 || io != CB_IO_F32 || !gw_shape(a, pl)) return false;
    const int C = a->x.C;
    if ((C != 192 && C != 384) || pl.mft % 3 != 0 || pl.rows != pl.mft * 32 || !cb_act_linear(a)) return false;
    r->rs = a->resid.ptr != nullptr;
    if (HW % G4_SUP != 0 || a->x.batch_stride % G4_SUP != 0 || a->y.batch_stride % G4_SUP != 0 || (r->rs && a->resid.batch_stride % G4_SUP != 0)) return false;
    if (((uintptr_t)a->x.ptr | (uintptr_t)a->y.ptr | (uintptr_t)a->resid.ptr) & (4 * G4_SUP - 1)) return false;
    if (!gw_batch_spans_fit(a, pl, HW)) return false;
    r->nch = C / 64;
    r->ntiles = (int)lama_ceil_div64((long long)a->batch * HW, 32 * G4_SUP);     // super-tiles over the flat pixel list of the batch
    const int ntypes = pl.mft / 3;
    if (ntypes > 256) return false;
    if (mode != 2 && (long long)r->ntiles * ntypes < 256) return false;
    r->nslots = 256 / ntypes;                                          // one workgroup per CU, resident from the start
    if (r->nslots > r->ntiles) r->nslots = r->ntiles;
    { const int cap = lama_env_int("LAMA_GEMM_W4_SLOTS", 0); if (cap > 0 && r->nslots > cap) r->nslots = cap; }
    r->grid = r->nslots * ntypes;
    return true;
#endif
}

bool ws_route(const lama_conv2d_args* a, const CbPlan& pl, long long HW, int io, CbRoute* r) {
    static const int mode = lama_env_int("LAMA_GEMM_WS", 1);
    static const int NH_env = lama_env_int("LAMA_GEMM_WS_NH", 1) == 2 ? 2 : 1;
    const int C = a->x.C;
    if (mode == 0 || !gw_shape(a, pl) || (C != 192 && C != 384) || pl.mft % 3 != 0) return false;
    r->rs = a->resid.ptr != nullptr;
#if CB_HALF   // all fp16, or SpectralTransform.conv1 reading the fp32 residual stream and writing fp16
    if (!(io == CB_IO_F16 || (io == CB_IO_F32_F16 && C == 384 && !r->rs))) return false;
#else
    if (io != CB_IO_F32) return false;
#endif
    if (!cb_span_fits(0, 1, C, HW, 1ll << 31) || !cb_span_fits(0, 1, (long long)pl.mft * 32, HW, 1ll << 31)) return false;   // 32-bit byte offsets inside one image
    r->NH = io != CB_IO_F32 ? 1 : NH_env;   // 2 = one 8-wave workgroup per CU over 64-pixel tiles, 1 = two 4-wave workgroups per CU over 32-pixel tiles
    r->nch = C / 64;
    r->ntiles = a->batch * (int)lama_ceil_div64(HW, GW_TILE(r->NH));
    const int ntypes = pl.mft / 3, wgs = 256 * (3 - r->NH);   // persistent: every workgroup resident from the start
    if (ntypes > wgs) return false;
    if (mode != 2 && (long long)r->ntiles * ntypes < 64) return false;
    r->nslots = wgs / ntypes;
    if (r->nslots > r->ntiles) r->nslots = r->ntiles;
    r->grid = r->nslots * ntypes;
    return true;
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

// the output side every tiled launch shares (WR and LDS): epilogue operands and the flat / transposed / plain output geometry
void cb_params_base(CbParams* p, const lama_conv2d_args* a, const CbPlan& pl, int Ho, int Wo, bool flat) {
    memset(p, 0, sizeof(*p));
    p->bias = a->bias;
    p->resid = (const float*)a->resid.ptr;
    p->resid_bstride = a->resid.batch_stride;
    p->y = (float*)a->y.ptr;
    p->y_bstride = a->y.batch_stride;
    p->M = pl.rows;
    p->B = a->batch;
    p->act = a->act;
    p->range_flag = a->range_flag;
    p->ostep = 1;
    if (flat) { p->Ho = 1; p->Wo = Ho * Wo; p->GH = 1; p->GW = Ho * Wo; }
    else if (a->transposed) { p->Ho = Ho; p->Wo = Wo; p->GH = a->x.H; p->GW = a->x.W; p->ostep = 2; p->oy0 = pl.oy0[0]; p->ox0 = pl.ox0[0]; }
    else { p->Ho = Ho; p->Wo = Wo; p->GH = Ho; p->GW = Wo; }
}

// WR: the whole CbParams of a routed geometry (r: WMV, KSC1, twlog); returns the staging units a thread group has to cover
int wr_fill(CbParams* p, const lama_conv2d_args* a, const CbPlan& pl, const CbPlan* pl2, int Ho, int Wo, const CbRoute& r) {
    const bool flat = (pl.T[0] == 1 && a->pad == 0 && !pl2);
    cb_params_base(p, a, pl, Ho, Wo, flat);
    p->MT = lama_ceil_div(pl.mft, r.WMV);
    const int TW = 1 << r.twlog, TH = 128 >> r.twlog;
    p->TWlog = r.twlog;
    p->tiles_x = lama_ceil_div(p->GW, TW);
    p->tiles_y = lama_ceil_div(p->GH, TH);
    cb_fill_seg(&p->s1, a->x, (const char*)a->w_packed + pl.woff[0], pl, 0, a->stride, a->pad_mode, TH, TW, flat);
    p->s1.vpad = a->pad;
    int units = p->s1.PH * p->s1.PW * 2 * r.KSC1;
    long long pbytes = (long long)2 * (2 * r.KSC1 * p->s1.npix * 16 + 16);   // hi + lo planes, each followed by a 16-byte dump slot
    if (pl2) {
        cb_fill_seg(&p->s2, a->x2, (const char*)a->w2_packed, *pl2, 0, 1, LAMA_PAD_ZERO, TH, TW, false);
        const int u2 = p->s2.PH * p->s2.PW * 8;
        const long long p2 = (long long)2 * (8 * p->s2.npix * 16 + 16);
        units = u2 > units ? u2 : units;
        pbytes = p2 > pbytes ? p2 : pbytes;
    }
    p->pbytes = (int)pbytes;
    if (r.fuse1) {   // SpectralTransform.conv1 of the next layer in the epilogue
        p->f1_w = (const char*)a->fuse1_w;
        p->f1_bias = a->fuse1_bias;
        p->f1_y = (float*)a->fuse1_y.ptr;
        p->f1_y_bstride = a->fuse1_y.batch_stride;
    }
    return units;
}

// the element-type mixes conv_wr_kernel is instantiated for outside the stride-2 / cooperative / fused launches (wr_launch_io)
static bool cw_io_ok(int T1, bool has2, int WMV, int KG, int io) {
#if CB_HALF
    if (has2 && !(io & CB_IO_X2H)) return false;                 // t (the spectral branch's output) is always fp16 on this path
    if ((io & 3) == CB_IO_F16) return true;
    // the two bottleneck launches with the fp32 residual stream on one side
    const bool bottleneck = T1 == 9 && ((!has2 && WMV == 4 && KG == 2) || (has2 && WMV == 12 && KG == 1));
    return bottleneck && ((io & 3) == CB_IO_F32_F16 || (io & 3) == CB_IO_F16_F32);
#else
    (void)T1; (void)has2; (void)WMV; (void)KG;
    return io == CB_IO_F32;
#endif
}

bool wr_route(const lama_conv2d_args* a, const CbPlan& pl, const CbPlan* pl2, int Ho, int Wo, int io, CbRoute* r) {
    static const bool enabled = lama_env_int("LAMA_CONV_WR", 1) != 0;
    if (!enabled || a->transposed || (a->stride != 1 && a->stride != 2) || pl.mode != 0 || pl.nseg != 1) return false;
    const int T1 = pl.T[0];
    const bool s2 = a->stride == 2;   // the three downsampling convs: same kernel, parity-split patch columns, five staging units per thread
    if (s2 && (T1 != 9 || pl2 || a->pad != 1)) return false;
    const bool split_io = (io & (CB_IO_XS | CB_IO_YS)) != 0;   // LAMA_DT_SPLIT16 tensors: the stride-2 launch only, whole octets, no residual
    if (split_io && (!s2 || CB_HALF || (io & ~(CB_IO_XS | CB_IO_YS)) || a->resid.ptr || a->x.C % 8 != 0 || pl.rows % 8 != 0 || pl.rows != a->y.C)) return false;
    if (split_io && !(cb_span_fits(0, 1, a->x.C, (long long)a->x.H * a->x.W, 1ll << 31) && cb_span_fits(0, 1, a->y.C, (long long)Ho * Wo, 1ll << 31))) return false;
    if (!((T1 == 9 && a->x.C % 32 == 0) || (T1 == 1 && a->x.C % 64 == 0)) || (T1 == 1 && pl2)) return false;
    if (pl2 && a->x2.C % 64 != 0) return false;
    if (pl.rows < 96) return false;          // a 128-row tile would be mostly padding
    int twlog3 = 5;
    const long long tiles_img = (T1 == 9 && !s2) ? cw_pick_tile(Wo, Ho, a->batch, a->flags, &twlog3) : lama_ceil_div64((long long)Ho * Wo, 128);   // 128-pixel tiles of one image
    // workgroup geometry: M-waves x K-groups (conv_wreg_dev.inc)
    int WMV = 4, KG = 2;
#if CB_HALF
    const int s2geo = 1;
#else
    static const int s2geo = lama_env_int("LAMA_CW_S2", 1);
#endif
    if (s2 && (s2geo != 2 || split_io)) KG = 1;   // LAMA_DT_SPLIT16 on either side: the 4 x 1 geometry only
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
    const int g41 = lama_env_int("LAMA_CW_41", 0);
    bool coop = false;
    if (T1 == 9 && !pl2 && !s2 && pl.mft % 4 == 0) {
        const long long wgs = (long long)a->batch * tiles_img * (pl.mft / 4);
        const bool f32io = (io == CB_IO_F32) && !CB_HALF;
        if (g41 == 2 || ((g41 == 0 || g41 == 1) && wgs >= 512 && f32io)) KG = 1;
        const bool flagged = (a->flags & LAMA_CONV_COOPERATIVE) && g41 != -1 && wgs >= 224;
        if ((flagged || g41 == 3) && f32io && wgs <= 320) { coop = true; KG = 1; }
    }
    // all 384 rows of the global branch in one 12-wave workgroup per 128-pixel tile (patch staged once, one round on 256 CUs at 8 x 512^2) --
    // when the launch has enough tiles: below LAMA_CW_G12_MIN tiles three 128-row workgroups per tile fill more of the chip (1 x 512^2 =
    // 32 tiles: 5.72 -> 4.36 ms per image, 2 x 512^2: 6.33 -> 5.04 ms per batch; profiles/r03_ab_global_geometry_small_batch.txt).
    static const int g12 = lama_env_int("LAMA_CW_G12", 1);
    static const int g12_min = lama_env_int("LAMA_CW_G12_MIN", 160);
    // (a part of a batch beside its siblings -- LAMA_CONV_SIBLINGS_*, v109 -- counts with their tiles: the parts fill the chip together)
    const long long tiles_g = ((long long)a->batch * tiles_img) << LAMA_CONV_SIBLINGS_LOG2(a->flags);
    if (T1 == 9 && pl2 && pl.mft == 12 && (g12 == 2 || (g12 == 1 && tiles_g >= g12_min))) { WMV = 12; KG = 1; }
    if (T1 == 1) {
        // 1x1: short K, the launch is bound by memory latency and by the patch staging rather than the matrix cores -> ALL rows
        // in one 12-wave workgroup per pixel tile (the patch is loaded and split once, not once per 128-row tile) when the
        // launch still covers a good part of the chip: 384 rows = 12 M-waves, 192 rows = 6 M-waves x 2 K-groups.
        static const int full_m = lama_env_int("LAMA_CW_1X1", 1);
        const long long tiles128 = (long long)a->batch * lama_ceil_div64((long long)Ho * Wo, 128);
        const bool want = full_m >= 2 || (full_m == 1 && tiles128 >= 96);
        if (full_m == 3 && pl.mft == 12) { WMV = 6; KG = 2; }   // profiling tools: 384 rows as two 192-row K-split workgroups
        else if (want && pl.mft == 12) { WMV = 12; KG = 1; }
        else if (want && pl.mft == 6) { WMV = 6; KG = 2; }
        else if (pl.mft % 4 != 0) return false;   // no partly empty 128-row tile
    }
    if (!cb_span_fits(0, 1, a->x.C, (long long)a->x.H * a->x.W, 1ll << 33) || (pl2 && !cb_span_fits(0, 1, a->x2.C, (long long)a->x2.H * a->x2.W, 1ll << 33)))
        return false;   // 32-bit element offsets inside one image
    // the fused conv1 exists in the 12 x 1 launch of the global branch only
    if (a->fuse1_w && !(T1 == 9 && pl2 && WMV == 12 && io == CB_IO_F32 && pl.rows == 384 && !CB_HALF)) return false;
    r->WMV = WMV; r->KG = KG; r->s2 = s2; r->coop = coop; r->fuse1 = a->fuse1_w != nullptr;
    r->KSC1 = T1 == 9 ? (KG == 1 && WMV == 4 && !coop ? 1 : 2) : 4;
    const bool flat = (T1 == 1 && a->pad == 0);
    r->twlog = flat ? 7 : 5;
    while (r->twlog > 3 && (1 << (r->twlog - 1)) >= (flat ? Ho * Wo : Wo)) --r->twlog;
    if (T1 == 9 && !s2) r->twlog = twlog3;
    // element types the geometry is instantiated for
    if (s2) {
#if CB_HALF
        if (io != CB_IO_F16 && io != CB_IO_F16_F32) return false;   // the last downsample writes the fp32 residual stream
#else
        if (!split_io && io != CB_IO_F32) return false;
#endif
    } else if (!coop && !r->fuse1 && !cw_io_ok(T1, pl2 != nullptr, WMV, KG, io)) return false;
    // 3x3 on 32-pixel tile rows at two waves per SIMD or fewer: the row-rolling fragment reads (conv_wreg_dev.inc, ROLL)
#if CB_HALF
    r->roll = !s2 && T1 == 9 && WMV * KG <= 8 && r->twlog == 5;
#else
    static const int roll = lama_env_int("LAMA_CW_ROLL", 1);   // 0: A/B runs of the profiling tools
    r->roll = !s2 && r->twlog == 5 && (coop || (T1 == 9 && WMV * KG <= 8 && roll && !r->fuse1));
#endif
    const int threads = 64 * WMV * KG;
    CbParams p;
    const int units = wr_fill(&p, a, pl, pl2, Ho, Wo, *r);
    if (units > (s2 ? 5 : (coop ? 4 : 2)) * threads) return false;
    r->shmem = 2 * (size_t)p.pbytes;
    if (KG == 2 && r->shmem < (size_t)(threads / 64) * 8192) r->shmem = (size_t)(threads / 64) * 8192;   // K-group exchange: 8 KiB per wave
    if (r->shmem > 160 * 1024) return false;
    if (r->fuse1 && r->shmem < 144 * 1024) r->shmem = 144 * 1024;   // B operands of the fused GEMM (24 k-steps x 2 pixel fragments x (hi, lo) KiB) + 48 KiB of K-half hand-over
    r->grid = p.B * p.tiles_x * p.tiles_y * p.MT;
    return true;
}

#if !CB_HALF
// CT: every field of CtParams; false where the plan's parity classes are not the kernel's
bool ct_fill(CtParams* p, const lama_conv2d_args* a, const CbPlan& pl) {
    memset(p, 0, sizeof(*p));
    p->x = (const float*)a->x.ptr;
    p->x_bstride = a->x.batch_stride;
    p->C = a->x.C; p->H = a->x.H; p->W = a->x.W;
    for (int c = 0; c < 4; ++c) {
        const int cls = c + 1;                                           // plan classes 1..4: (py, px) = (1,1) (1,0) (0,1) (0,0)
        p->w[c] = (const char*)a->w_packed + pl.woff[cls];
        p->T[c] = pl.T[cls];
        p->py[c] = pl.oy0[cls]; p->px[c] = pl.ox0[cls];
        if (pl.T[cls] != (1 + p->py[c]) * (1 + p->px[c])) return false;
        for (int t = 0; t < pl.T[cls]; ++t) p->off[c][t] = pl.dy[cls][t] * CT_PWS + pl.dx[cls][t];
    }
    p->mft = pl.mft;
    p->bias = a->bias;
    p->y = (float*)a->y.ptr;
    p->y_bstride = a->y.batch_stride;
    p->M = pl.rows; p->B = a->batch; p->act = a->act;
    p->tiles_x = lama_ceil_div(p->W, 32); p->tiles_y = lama_ceil_div(p->H, 4); p->MG = pl.rows / 64;
    p->range_flag = a->range_flag;
    return true;
}
#endif

bool ct_route(const lama_conv2d_args* a, const CbPlan& pl, int Ho, int Wo, int io, CbRoute* r) {
#if CB_HALF
    (void)a; (void)pl; (void)Ho; (void)Wo; (void)io; (void)r;
    return false;
#else
    const int mode = lama_env_int("LAMA_CT", 1);
    if (mode == 0 || !a->transposed || pl.nseg != 5 || pl.mode != 0 || io != CB_IO_F32 || a->resid.ptr || a->fuse1_w) return false;
    const int C = a->x.C, H = a->x.H, W = a->x.W, M = pl.rows;
    // (round 6: any H, W -- ragged last tiles: the patch requests beyond the plane already read zeros, the stores are predicated)
    if (C % 32 != 0 || M % 64 != 0 || H < 1 || W < 1 || Ho != 2 * H || Wo != 2 * W) return false;
    if (!cb_span_fits(0, 1, C, (long long)H * W, 1ll << 31)) return false;       // 32-bit byte offsets inside one image
    CtParams p;
    if (!ct_fill(&p, a, pl) || p.T[0] != 4 || p.T[3] != 1 || p.T[1] != 2 || p.T[2] != 2) return false;
    // the kernel shares B fragments between the classes by position: the plan must match its compile-time tap table; identity / ReLU epilogues
    bool table_ok = true;
    for (int q = 0; q < 9; ++q) table_ok = table_ok && p.off[c2_cls(q)][c2_tap(q)] == c2_dy(q) * CT_PWS + c2_dx(q);
    for (int c = 0; c < 4; ++c) table_ok = table_ok && p.py[c] == (c < 2 ? 1 : 0) && p.px[c] == ((c == 0 || c == 2) ? 1 : 0);
    if (!table_ok || !cb_act_linear(a)) return false;
    if ((a->y.batch_stride % 4) != 0 || ((uintptr_t)a->y.ptr & 15) != 0) return false;   // 16-byte stores
    const long long tiles = (long long)a->batch * p.tiles_x * p.tiles_y * p.MG;
    if (tiles >= (1ll << 30)) return false;
    long long grid = tiles < 512 ? tiles : 512;                                      // persistent: two workgroups per CU walk tiles w, w + grid, ...
    { const int cap = lama_env_int("LAMA_CT_GRID", 0); if (cap > 0 && grid > cap) grid = cap; }   // emulator tests: several tiles per workgroup
    r->grid = (int)grid;
    return true;
#endif
}

bool stem_route(const lama_conv2d_args* a, const CbPlan& pl, int Ho, int Wo, int io, CbRoute* r) {
#if CB_HALF   // the stem reads the fp32 network input and writes fp16
    if (io != CB_IO_F32_F16) return false;
#else
    if (io != CB_IO_F32 && !(io == CB_IO_YS && pl.rows % 8 == 0)) return false;   // LAMA_DT_SPLIT16: whole channel octets
#endif
    static const int mode = lama_env_int("LAMA_STEM_WS", 1);
    if (mode == 0 || pl.mode != 1 || pl.mft != 2 || a->transposed || a->stride != 1 || a->pad != 3 || a->pad_mode != LAMA_PAD_REFLECT ||
        a->resid.ptr || a->x.H < 4 || a->x.W < 4)
        return false;
    const long long HW = (long long)Ho * Wo;
    if (!cb_span_fits(0, 1, a->x.C, HW, 1ll << 31) || !cb_span_fits(0, 1, 64, HW, 1ll << 31)) return false;   // 32-bit byte offsets inside one image
    const long long cols = (long long)a->batch * lama_ceil_div(Wo, 32);
    if (mode != 2 && cols * Ho < 4096) return false;   // persistent: 1024 wave pairs want a few dozen output rows each
    // a wave pair walks down a column of 32-pixel segments; columns are cut into ns vertical parts so that there are ~1024 parts
    // (every part pays 6 extra input rows to fill its window)
    long long ns = cols >= 1024 ? 1 : lama_ceil_div64(1024, cols);
    if (ns > Ho) ns = Ho;
    r->seg_rows = (int)lama_ceil_div64(Ho, ns);
    const long long nseg = cols * lama_ceil_div(Ho, r->seg_rows);
    if (nseg >= (1ll << 31)) return false;
    r->ntiles = (int)nseg;
    r->grid = 512;                                                  // two 4-wave workgroups per CU
    if ((long long)r->grid * 2 > nseg) r->grid = (int)((nseg + 1) / 2);
    return true;
}

bool head_route(const lama_conv2d_args* a, const CbPlan& pl, int Ho, int Wo, int io, const LamaTileList* tl, CbRoute* r) {
#if CB_HALF   // the head reads fp16 and writes the fp32 image; no work lists
    if (io != CB_IO_F16_F32 || tl) return false;
#else
    if (io != CB_IO_F32) return false;
#endif
    if (tl && (tl->head_rs < HEAD_R || tl->head_rs % HEAD_R != 0)) return false;
    static const int mode = lama_env_int("LAMA_HEAD_WS", 1);
    if (mode == 0 || pl.mode != 2 || pl.mft != 1 || a->x.C != 64 || a->y.C > 4 || a->transposed || a->stride != 1 || a->pad != 3 ||
        a->pad_mode != LAMA_PAD_REFLECT || a->resid.ptr || a->x.H < 4 || a->x.W < 4)
        return false;
    if (!cb_span_fits(0, 1, 64, (long long)Ho * Wo, 1ll << 31)) return false;   // 32-bit byte offsets inside one image
    const long long cols = (long long)a->batch * lama_ceil_div(Wo, 26);
    if (mode != 2 && cols * Ho < 8192) return false;   // persistent: 768 workgroups want a few dozen rows each
    // a workgroup walks down a column of segments; columns are cut into parts of rs rows (a multiple of HEAD_R: the register ring
    // of the kernel is unrolled by it).  Every part pays 6 + HEAD_D extra input rows and the parts should divide evenly among the
    // resident workgroups.  A work list: parts of the caller's head_rs rows (the host cannot know the count, so the parts are small and the
    // grid is the resident 768)
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
    r->seg_rows = tl ? tl->head_rs : best_rs;
    const long long nseg = cols * lama_ceil_div(Ho, r->seg_rows);
    if (nseg >= (1ll << 31)) return false;
    r->ntiles = (int)nseg;
    r->grid = nseg < wgs ? (int)nseg : wgs;
    return true;
}

// LDS: the whole CbParams of a routed tile (r: BM, BN); returns the staging units a workgroup has to cover
int lds_fill(CbParams* p, const lama_conv2d_args* a, const CbPlan& pl, const CbPlan* pl2, int Ho, int Wo, const CbRoute& r) {
    const bool flat = (pl.T[0] == 1 && !a->transposed && a->stride == 1 && a->pad == 0 && !pl2);
    cb_params_base(p, a, pl, Ho, Wo, flat);
    p->MT = lama_ceil_div(pl.rows, r.BM);
    const int stride = a->transposed ? 1 : a->stride;
    const int pad_mode = a->transposed ? LAMA_PAD_ZERO : a->pad_mode;
    // tile: TW = 32 output pixels of one row per wave (conflict-free B fragments), narrower only for narrow images
    int twlog = flat ? lama_ilog2(r.BN) : 5;
    while (pl.mode != 2 && twlog > 3 && (1 << (twlog - 1)) >= p->GW) --twlog;
    const int TW = 1 << twlog, TH = r.BN >> twlog;
    p->TWlog = twlog;
    p->tiles_x = pl.mode == 2 ? lama_ceil_div(p->GW, 26) : lama_ceil_div(p->GW, TW);
    p->tiles_y = lama_ceil_div(p->GH, TH);
    int units = cb_fill_seg(&p->s1, a->x, (const char*)a->w_packed + pl.woff[0], pl, 0, stride, pad_mode, TH, TW, flat);
    p->s1.vpad = a->pad;
    long long wbytes = (long long)pl.TG[0] * pl.KS[0] * (r.BM / 32) * 2048;
    long long pbytes = (long long)2 * 2 * pl.KS[0] * p->s1.npix * 16;
    int smax = p->s1.nchunk * p->s1.NG;   // a segment with S stages touches min(3, S) weight buffers
    if (pl2) {
        const int TG2 = pl2->TG[0], KS2 = pl2->KS[0];
        const int u2 = cb_fill_seg(&p->s2, a->x2, (const char*)a->w2_packed, *pl2, 0, 1, LAMA_PAD_ZERO, TH, TW, false);
        units = u2 > units ? u2 : units;
        const long long w2 = (long long)TG2 * KS2 * (r.BM / 32) * 2048, p2 = (long long)2 * 2 * KS2 * p->s2.npix * 16;
        wbytes = w2 > wbytes ? w2 : wbytes;
        pbytes = p2 > pbytes ? p2 : pbytes;
        if (p->s2.nchunk * p->s2.NG > smax) smax = p->s2.nchunk * p->s2.NG;
    }
    p->wbytes = (int)wbytes;
    p->pbytes = (int)pbytes;
    p->nwbuf = smax < 3 ? smax : 3;
    return units;
}

// the (taps, M tile, element types) conv_kernel is instantiated for: the conditions of lds_launch's tables
static bool lds_has_kernel(int T1, bool has2, int BM, bool trf, int mode, int io) {
#ifdef CB_DEV_NO_GENERIC   // kernel-development builds (tools/kres.py): skip the LDS-staged instantiations, 10x shorter compile
    return false;
#endif
    if (mode) {   // folded 7x7.  LAMA_PREC_F16: the stem reads the fp32 network input and writes fp16, the head reads fp16 and writes the fp32 image
#if CB_HALF
        return (io == CB_IO_F32_F16 && mode == 1 && BM == 64) || (io == CB_IO_F16_F32 && mode == 2 && BM == 32);
#else
        return io == CB_IO_F32 && ((mode == 2 && BM == 32) || (mode == 1 && (BM == 64 || BM == 128 || BM == 32)));
#endif
    }
    if (trf) {
        if (BM != 128 && BM != 64 && BM != 32) return false;
        return CB_HALF ? (io == CB_IO_F16 || io == CB_IO_F32_F16 || io == CB_IO_F16_F32) : io == CB_IO_F32;
    }
    if (!((T1 == 9) || (!has2 && (T1 == 1 || T1 == 49 || T1 == 2 || T1 == 4)))) return false;
    if (BM != 192 && BM != 128 && BM != 64 && BM != 32) return false;
    // LAMA_PREC_F16: all fp16, fp32 in -> fp16 out, fp16 in -> fp32 out (the residual stream of the resnet blocks is fp32), x2 (= t) always fp16
    return CB_HALF ? ((!has2 || (io & CB_IO_X2H)) && (io & 3) != 0) : io == CB_IO_F32;
}

bool lds_route(const lama_conv2d_args* a, const CbPlan& pl, const CbPlan* pl2, int Ho, int Wo, int io, CbRoute* r) {
    int BM = cb_pick_bm(pl.rows, pl.mode ? 49 : pl.T[0], a->transposed ? 1 : a->stride, a->batch, a->transposed ? a->x.H : Ho,
                        a->transposed ? a->x.W : Wo);
    { static const int bm_env = lama_env_int("LAMA_CB_BM", 0); if (bm_env && a->transposed) BM = bm_env; }   // profiling tools: M tile of the transposed convs
    if (BM < 128 && !a->transposed && a->stride == 2) BM = 128;   // a 256-pixel stride-2 tile does not leave room for two patch buffers
    if (pl.mode == 1) BM = a->y.C > 64 ? 128 : 64;   // 128-pixel tiles: 4 channel octets per pixel have to be staged
    r->BM = BM;
    r->BN = (BM >= 128 || ((a->transposed || pl.mode == 1) && BM == 64)) ? 128 : 256;
    r->mode = pl.mode;
    r->trf = a->transposed != 0;
    if (!cb_span_fits(0, 1, a->x.C, (long long)a->x.H * a->x.W, 1ll << 33) || (pl2 && !cb_span_fits(0, 1, a->x2.C, (long long)a->x2.H * a->x2.W, 1ll << 33)))
        return false;   // 32-bit element offsets inside one image
    if (!lds_has_kernel(pl.T[0], pl2 != nullptr, BM, r->trf, pl.mode, io)) return false;
    CbParams p;
    const int maxu = lama_ceil_div(lds_fill(&p, a, pl, pl2, Ho, Wo, *r), CB_THREADS);
    r->shmem = (size_t)p.nwbuf * p.wbytes + 2 * (size_t)p.pbytes;
    if (maxu > 3 || r->shmem > 160 * 1024) return false;
    r->maxu = (maxu <= 1 && !pl.mode) ? 1 : 3;   // (the folded 7x7 kernels exist with three units only)
    r->grid = p.B * p.tiles_x * p.tiles_y * p.MT;
    return true;
}

// ------------------------------------------------------------------------------------------------
// the table
// ------------------------------------------------------------------------------------------------
int cb_route(const lama_conv2d_args* a, const CbPlan& pl, const CbPlan* pl2, int Ho, int Wo, int io, const LamaTileList* tl, CbRoute* r) {
    memset(r, 0, sizeof(*r));
    const long long HW = (long long)Ho * Wo;
    // entry conditions: the rows a launch may take
    enum { WK = 1 << CB_FAM_WK, W4 = 1 << CB_FAM_W4, WS = 1 << CB_FAM_WS, WR = 1 << CB_FAM_WR, CT = 1 << CB_FAM_CT, STEM = 1 << CB_FAM_STEM,
           HEAD = 1 << CB_FAM_HEAD, LDS = 1 << CB_FAM_LDS };
    unsigned rows;
    if (tl) rows = (pl2 || a->fuse1_w) ? 0 : (a->transposed ? CT : HEAD);     // only the two persistent tail kernels walk a work list
    else if (io & (CB_IO_XS | CB_IO_YS)) rows = (CB_HALF || pl2 || a->transposed) ? 0 : ((io == CB_IO_YS ? STEM : 0) | WR);   // the two dedicated kernels or nothing
    else rows = WR | (pl2 ? 0 : WK | W4 | WS | CT) | ((pl2 || a->fuse1_w) ? 0 : STEM | HEAD) | (a->fuse1_w ? 0 : LDS);
    // (a row that declines leaves nothing behind for the rows after it)
#define CB_ROW(bit, fam, call) if (rows & bit) { memset(r, 0, sizeof(*r)); r->io = io; r->list = tl != nullptr; if (call) { r->family = fam; return LAMA_OK; } }
    CB_ROW(WK, CB_FAM_WK, wk_route(a, pl, HW, io, r))
    CB_ROW(W4, CB_FAM_W4, w4_route(a, pl, HW, io, r))
    CB_ROW(WS, CB_FAM_WS, ws_route(a, pl, HW, io, r))
    CB_ROW(WR, CB_FAM_WR, wr_route(a, pl, pl2, Ho, Wo, io, r))
    CB_ROW(CT, CB_FAM_CT, ct_route(a, pl, Ho, Wo, io, r))
    CB_ROW(STEM, CB_FAM_STEM, stem_route(a, pl, Ho, Wo, io, r))
    CB_ROW(HEAD, CB_FAM_HEAD, head_route(a, pl, Ho, Wo, io, tl, r))
    CB_ROW(LDS, CB_FAM_LDS, lds_route(a, pl, pl2, Ho, Wo, io, r))
#undef CB_ROW
    return LAMA_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------
// one launcher per family: parameter fill + the instantiation tables
// ------------------------------------------------------------------------------------------------
// the operands and sizes the three pointwise GEMMs share
void gw_fill(GwParams* p, const lama_conv2d_args* a, const CbPlan& pl, long long HW, const CbRoute& r) {
    memset(p, 0, sizeof(*p));
    p->x = (const float*)a->x.ptr;
    p->x_bstride = a->x.batch_stride;
    p->HW = (int)HW;
    p->C = a->x.C;
    p->w = (const char*)a->w_packed + pl.woff[0];
    p->mft = pl.mft;
    p->bias = a->bias;
    p->resid = (const float*)a->resid.ptr;
    p->resid_bstride = a->resid.batch_stride;
    p->y = (float*)a->y.ptr;
    p->y_bstride = a->y.batch_stride;
    p->M = pl.rows;
    p->B = a->batch;
    p->act = a->act;
    p->range_flag = a->range_flag;
    p->ntiles = r.ntiles;
    static const int abl = lama_env_int("LAMA_GW_ABLATE", 0);   // profiling tools only
    p->abl = abl;
}
#if defined(LAMA_PROFILING) && !CB_HALF
// profiling tools only: per-workgroup timeline of the f16x3 GEMMs, LAMA_GW_TRACE = device address of grid * 16 int64
static bool gw_trace(GwParams* p) {
    static const unsigned long long tr = lama_env_u64("LAMA_GW_TRACE");
    if (!CB_F16 || !tr) return false;
    p->trace = reinterpret_cast<long long*>(tr);
    return true;
}
#endif

int w4_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, long long HW, const CbRoute& r) {
#if CB_HALF
    (void)stream; (void)a; (void)pl; (void)HW; (void)r;
    return CB_ERR_ROUTE;
#else
    if (r.grid <= 0) return LAMA_OK;
    GwParams p;
    gw_fill(&p, a, pl, HW, r);
    p.ntypes = pl.mft / 3;
    p.nslots = r.nslots;
    const size_t lds = G4_LDS_BYTES(G4_SUP);
#define G4_CASE(nch, ...) hipLaunchKernelGGL((CB_NAME(gemm1x1_w4_kernel)<nch, G4_SUP, __VA_ARGS__>), dim3(r.grid), dim3(G4_THREADS), lds, stream, p)
#if defined(LAMA_PROFILING)
    if (r.nch == 6 && !r.rs && gw_trace(&p)) G4_CASE(6, false, true);
    else
#endif
    if (r.nch == 6) { if (r.rs) G4_CASE(6, true); else G4_CASE(6, false); }
    else { if (r.rs) G4_CASE(3, true); else G4_CASE(3, false); }
#undef G4_CASE
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
#endif
}

int wk_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, long long HW, const CbRoute& r) {
#if CB_HALF
    (void)stream; (void)a; (void)pl; (void)HW; (void)r;
    return CB_ERR_ROUTE;
#else
    if (r.grid <= 0) return LAMA_OK;
    GwParams p;
    gw_fill(&p, a, pl, HW, r);
    p.resid_bstride = 0;   // (no residual on this route)
    p.aux = r.aux;
#if defined(LAMA_PROFILING)
    if (gw_trace(&p)) hipLaunchKernelGGL((CB_NAME(gemm1x1_wk_kernel)<true>), dim3(r.grid), dim3(GK_THREADS), GK_LDS_BYTES, stream, p);
    else
#endif
    hipLaunchKernelGGL((CB_NAME(gemm1x1_wk_kernel)<false>), dim3(r.grid), dim3(GK_THREADS), GK_LDS_BYTES, stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
#endif
}

int ws_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, long long HW, const CbRoute& r) {
    if (r.grid <= 0) return LAMA_OK;
    GwParams p;
    gw_fill(&p, a, pl, HW, r);
    p.tiles_per_img = (int)lama_ceil_div64(HW, GW_TILE(r.NH));
    p.ntypes = pl.mft / 3;
    p.nslots = r.nslots;
    { static const int prio = lama_env_int("LAMA_SIDE_PRIO", 1); p.prio = prio; }   // profiling tools: 0 = default wave priority
    const dim3 blk(GW_THREADS(r.NH));
    const size_t lds = GW_LDS_BYTES(r.NH);
#define GW_CASE(...) hipLaunchKernelGGL((CB_NAME(gemm1x1_ws_kernel)<__VA_ARGS__>), dim3(r.grid), blk, lds, stream, p)
#if CB_HALF
    if (r.io == CB_IO_F16) {   // fp16 activations, one product (NH = 1 geometry only)
        if (r.nch == 6) { if (r.rs) GW_CASE(6, true, 1, false, true); else GW_CASE(6, false, 1, false, true); }
        else { if (r.rs) GW_CASE(3, true, 1, false, true); else GW_CASE(3, false, 1, false, true); }
    } else if (r.io == CB_IO_F32_F16 && r.nch == 6 && !r.rs) GW_CASE(6, false, 1, false, true, false, true);
    else return CB_ERR_ROUTE;
#else
#if defined(LAMA_PROFILING)
    if (r.nch == 6 && gw_trace(&p)) { if (r.NH == 2) GW_CASE(6, true, 2, true); else GW_CASE(6, true, 1, true); }
    else
#endif
    if (r.NH == 2) {
        if (r.nch == 6) { if (r.rs) GW_CASE(6, true, 2); else GW_CASE(6, false, 2); }
        else { if (r.rs) GW_CASE(3, true, 2); else GW_CASE(3, false, 2); }
    } else {
        if (r.nch == 6) { if (r.rs) GW_CASE(6, true, 1); else GW_CASE(6, false, 1); }
        else { if (r.rs) GW_CASE(3, true, 1); else GW_CASE(3, false, 1); }
    }
#endif
#undef GW_CASE
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

// conv_wr_kernel<T1, KSC1, T2, KSC2, WMV, KG, ABL, SCH, HF, HI1, HI2, HO, ROLL, NU, FUSE1, XS, YS>: the geometries (the first six arguments) ...
#define CW_LOCAL_42 9, 2, 0, 0, 4, 2     // local 3x3 (and LAMA_CW_S2 = 2): one 8-wave workgroup per tile, K split over two wave groups
#define CW_LOCAL_41 9, 1, 0, 0, 4, 1     // local 3x3 from 512 workgroups on and stride 2: two 4-wave workgroups per CU, 16-channel chunks
#define CW_LOCAL_COOP 9, 2, 0, 0, 4, 1   // LAMA_CONV_COOPERATIVE: one 4-wave workgroup per CU, 32-channel chunks (NU = 4)
#define CW_GLOBAL_12 9, 2, 1, 4, 12, 1   // global branch (3x3 + fused 1x1), all 384 rows in one 12-wave workgroup
#define CW_GLOBAL_42 9, 2, 1, 4, 4, 2    // global branch, 128-row tiles
#define CW_1X1_12 1, 4, 0, 0, 12, 1      // 1x1, 384 rows per workgroup
#define CW_1X1_62 1, 4, 0, 0, 6, 2       // 1x1, 192 rows per workgroup
#define CW_1X1_42 1, 4, 0, 0, 4, 2       // 1x1, 128-row tiles
// ... and what follows them: fp32 tensors (ABL 0, SCH 2), with the row-rolling reads, with NU staging units per thread
#define CW_F32 0, 2, false, false, false, false, false
#define CW_F32_ROLL 0, 2, false, false, false, false, true
// (the workgroup is 64 x WMV x KG threads of the INSTANTIATION: the profiling overrides launch a geometry of their own)
template <int T1, int KSC1, int T2, int KSC2, int WMV, int KG, auto... REST>
int cw_go(hipStream_t st, const CbParams& p, const CbRoute& r) {
    hipLaunchKernelGGL((CB_NAME(conv_wr_kernel)<T1, KSC1, T2, KSC2, WMV, KG, REST...>), dim3(r.grid), dim3(64 * WMV * KG), r.shmem, st, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}
#define CW_GO(...) return cw_go<__VA_ARGS__>(st, p, r)

// one geometry, by the element types of the launch and the row-rolling reads
template <int T1, int KSC1, int T2, int KSC2, int WMV, int KG>
int wr_launch_io(hipStream_t st, const CbParams& p, const CbRoute& r) {
    constexpr bool CAN_ROLL = (T1 == 9 && WMV * KG <= 8);
    if (r.roll && !CAN_ROLL) return CB_ERR_ROUTE;
#if CB_HALF
    // SCH 0, fp16 weights; hi1 / hi2 / ho: x, x2, y (and resid) are fp16
#define CW_H(hi1, hi2, ho)                                                                  \
    do {                                                                                    \
        if (r.roll) CW_GO(T1, KSC1, T2, KSC2, WMV, KG, 0, 0, true, hi1, hi2, ho, CAN_ROLL); \
        CW_GO(T1, KSC1, T2, KSC2, WMV, KG, 0, 0, true, hi1, hi2, ho);                       \
    } while (0)
    if ((r.io & 3) == CB_IO_F16) CW_H(true, true, true);
    if constexpr ((T1 == 9 && T2 == 0 && WMV == 4 && KG == 2) || (T1 == 9 && T2 == 1 && WMV == 12 && KG == 1)) {
        if ((r.io & 3) == CB_IO_F32_F16) CW_H(false, true, true);
        if ((r.io & 3) == CB_IO_F16_F32) CW_H(true, true, false);
    }
#undef CW_H
    return CB_ERR_ROUTE;
#else
    if constexpr (CAN_ROLL) {
        if (r.roll) CW_GO(T1, KSC1, T2, KSC2, WMV, KG, CW_F32_ROLL);
    }
    CW_GO(T1, KSC1, T2, KSC2, WMV, KG);
#endif
}

// 3x3 stride 2 (the downsampling convs): 16-channel chunks, five staging units per thread
int wr_launch_s2(hipStream_t st, const CbParams& p, const CbRoute& r) {
#if CB_HALF
    if (r.io == CB_IO_F16) CW_GO(CW_LOCAL_41, 0, 0, true, true, true, true, false, 5);
    if (r.io == CB_IO_F16_F32) CW_GO(CW_LOCAL_41, 0, 0, true, true, true, false, false, 5);   // the last downsample writes the fp32 residual stream
#else
    if (r.io == (CB_IO_XS | CB_IO_YS)) CW_GO(CW_LOCAL_41, CW_F32, 5, false, true, true);
    if (r.io == CB_IO_XS) CW_GO(CW_LOCAL_41, CW_F32, 5, false, true, false);
    if (r.io == CB_IO_YS) CW_GO(CW_LOCAL_41, CW_F32, 5, false, false, true);
    if (r.io != CB_IO_F32) return CB_ERR_ROUTE;
#if defined(LAMA_PROFILING)
    // ---- profiling tools only (f16x3): timing ablations of the patch staging (results wrong; profiles/presplit_outer.txt) ----
    if (CB_F16 && r.KG == 1) {
        static const int abl = lama_env_int("LAMA_CW_ABLATE", 0);
#define CW_ABL_S2(v) if (abl == v) CW_GO(CW_LOCAL_41, v, 2, false, false, false, false, false, 5);
        CW_ABL_S2(4) CW_ABL_S2(16) CW_ABL_S2(32)
#undef CW_ABL_S2
    }
    // ---- end of the profiling overrides ----
#endif
    if (r.KG == 2) CW_GO(CW_LOCAL_42, CW_F32, 5);   // LAMA_CW_S2 = 2 (profiling tools): one 8-wave workgroup per CU, K split between two wave groups
    CW_GO(CW_LOCAL_41, CW_F32, 5);
#endif
    return CB_ERR_ROUTE;
}

int wr_launch(hipStream_t st, const lama_conv2d_args* a, const CbPlan& pl, const CbPlan* pl2, int Ho, int Wo, const CbRoute& r) {
    if (r.grid <= 0) return LAMA_OK;
    CbParams p;
    wr_fill(&p, a, pl, pl2, Ho, Wo, r);
    const int T1 = pl.T[0];
#if defined(LAMA_PROFILING) && !CB_HALF
    // ---- profiling tools only (f16x3): timing ablations (results wrong) and timelines override the instantiation ----
    if (CB_F16) {
        static const int abl = lama_env_int("LAMA_CW_ABLATE", 0);
        static const int sch = lama_env_int("LAMA_CW_SCHED", 2);
        static const unsigned long long tr = lama_env_u64("LAMA_CW_TRACE");   // device address of grid * 32 int64
        if (T1 == 9 && !pl2 && r.WMV == 4 && !r.s2) {   // the local conv as the 4 x 2 geometry
#define CW_ABL(v) if (abl == v && p.TWlog == 5) CW_GO(CW_LOCAL_42, v, 2, false, false, false, false, true);
            CW_ABL(1) CW_ABL(2) CW_ABL(4) CW_ABL(3) CW_ABL(7) CW_ABL(8) CW_ABL(16) CW_ABL(32) CW_ABL(128) CW_ABL(132) CW_ABL(135)
#undef CW_ABL
            if (sch == 0) CW_GO(CW_LOCAL_42, 0, 0);
            if (sch == 1) CW_GO(CW_LOCAL_42, 0, 1);
        }
        if (pl2 && r.WMV == 12 && T1 == 9 && r.io == CB_IO_F32 && (abl == 1 || abl == 256)) {   // the global-branch launch: 1 = no weight loads in the loops, 256 = waves F >= 6 stream fragment F - 6
            if (r.fuse1) { if (abl == 1) CW_GO(CW_GLOBAL_12, 1, 2, false, false, false, false, false, 2, true); else CW_GO(CW_GLOBAL_12, 256, 2, false, false, false, false, false, 2, true); }
            if (abl == 1) CW_GO(CW_GLOBAL_12, 1);
            CW_GO(CW_GLOBAL_12, 256);
        }
        if (tr && pl2 && r.WMV == 12) { p.trace = reinterpret_cast<long long*>(tr); CW_GO(CW_GLOBAL_12, 64); }
        if (tr && !pl2 && !r.s2) {
            p.trace = reinterpret_cast<long long*>(tr);
            if (T1 == 9 && p.TWlog == 5) CW_GO(CW_LOCAL_42, 64, 2, false, false, false, false, true);
            if (T1 == 9) CW_GO(CW_LOCAL_42, 64);
            if (r.WMV == 12) CW_GO(CW_1X1_12, 64);
            if (r.WMV == 6) CW_GO(CW_1X1_62, 64);
            CW_GO(CW_1X1_42, 64);
        }
    }
    // ---- end of the profiling overrides ----
#endif
    if (r.s2) return wr_launch_s2(st, p, r);
#if !CB_HALF
    if (r.coop) { if (r.roll) CW_GO(CW_LOCAL_COOP, CW_F32_ROLL, 4); else CW_GO(CW_LOCAL_COOP, CW_F32, 4); }
#endif
    if (T1 == 9 && !pl2) return r.KG == 1 ? wr_launch_io<CW_LOCAL_41>(st, p, r) : wr_launch_io<CW_LOCAL_42>(st, p, r);
#if !CB_HALF
    if (r.fuse1) CW_GO(CW_GLOBAL_12, CW_F32, 2, true);   // the global-branch launch with SpectralTransform.conv1 of the next layer in its epilogue
#endif
    if (T1 == 9) return r.WMV == 12 ? wr_launch_io<CW_GLOBAL_12>(st, p, r) : wr_launch_io<CW_GLOBAL_42>(st, p, r);
    if (r.WMV == 12) return wr_launch_io<CW_1X1_12>(st, p, r);
    if (r.WMV == 6) return wr_launch_io<CW_1X1_62>(st, p, r);
    return wr_launch_io<CW_1X1_42>(st, p, r);
}
#undef CW_GO

int ct_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, const LamaTileList* tl, const CbRoute& r) {
#if CB_HALF
    (void)stream; (void)a; (void)pl; (void)tl; (void)r;
    return CB_ERR_ROUTE;
#else
    if (r.grid <= 0) return LAMA_OK;
    CtParams p;
    ct_fill(&p, a, pl);
    { static const int abl = lama_env_int("LAMA_CT_ABLATE", 0); p.abl = abl; }      // profiling tools only
    if (tl) {   // the LIST instantiation over the caller's tile list, same grid
        p.list = tl->list; p.count = tl->count;
        hipLaunchKernelGGL(CB_NAME(convt2_kernel)<true>, dim3(r.grid), dim3(C2_THREADS), C2_LDS_BYTES, stream, p);
    } else
        hipLaunchKernelGGL(CB_NAME(convt2_kernel)<false>, dim3(r.grid), dim3(C2_THREADS), C2_LDS_BYTES, stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
#endif
}

int stem_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, int Ho, int Wo, const CbRoute& r) {
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
    p.rs = r.seg_rows;
    p.ns = lama_ceil_div(Ho, p.rs);
    p.nseg = r.ntiles;
#if CB_HALF
    hipLaunchKernelGGL(CB_NAME(stem7_ws_kernel)<true>, dim3(r.grid), dim3(256), STEM_LDS_BYTES, stream, p);
#else
    if (r.io == CB_IO_YS) hipLaunchKernelGGL((CB_NAME(stem7_ws_kernel)<false, true>), dim3(r.grid), dim3(256), STEM_LDS_BYTES, stream, p);
    else hipLaunchKernelGGL(CB_NAME(stem7_ws_kernel)<false>, dim3(r.grid), dim3(256), STEM_LDS_BYTES, stream, p);
#endif
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}

int head_launch(hipStream_t stream, const lama_conv2d_args* a, const CbPlan& pl, int Ho, int Wo, const LamaTileList* tl, const CbRoute& r) {
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
    p.rs = r.seg_rows;
    p.ns = lama_ceil_div(Ho, p.rs);
    p.nseg = r.ntiles;
#if CB_HALF
    if (tl) return CB_ERR_ROUTE;
    hipLaunchKernelGGL(CB_NAME(head7_ws_kernel)<true>, dim3(r.grid), dim3(256), HEAD_LDS_BYTES, stream, p);
#else
    if (tl) {   // the LIST instantiation over the caller's segment list
        p.list = tl->list; p.count = tl->count;
        hipLaunchKernelGGL((CB_NAME(head7_ws_kernel)<false, true>), dim3(r.grid), dim3(256), HEAD_LDS_BYTES, stream, p);
    } else
        hipLaunchKernelGGL(CB_NAME(head7_ws_kernel)<false>, dim3(r.grid), dim3(256), HEAD_LDS_BYTES, stream, p);
#endif
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}
