// Multi-dilated 3x3 reflect convolution as ONE implicit GEMM (MultidilatedConv(comb_mode='cat_in') of the lama-dilated generator,
// multidilated_conv.py:36-63,73-98):
//
//   y = act( sum_{j<G} conv3x3(reflect_pad(x[:, j*Cin/G : (j+1)*Cin/G], d_j), w_j, dilation = d_j) + bias ) [+ resid],  d_j = dmin * 2^j
//
// The packed weights are the plain lama_conv2d_pack_weight image of the G weights concatenated along Cin ([Cout, Cin, 3, 3]): K order is
// (16-channel chunk, tap row, tap column), so a chunk belongs to exactly one group and the dilation is a per-chunk constant of the K loop.
//
// Workgroup = 512 threads = 8 waves (2 along M x 4 along N), output tile 128 channels x 128 pixels (TH x TW = 8 x 16, or 16 x 8 for narrow
// planes).  K is walked in stages of one tap row (3 taps) x 16 channels = 3 MFMA k-steps:
//   * weights: the stage image of this M tile (3 taps x 4 fragments x (hi | lo) KiB = 24 KiB) goes L2 -> registers at the start of the stage
//     before, -> LDS at its end; two buffers;
//   * activations: the patch of a chunk is (TH + 2d) x (TW + 2d) pixels x 16 channels with the reflection applied at staging time (computed
//     from the PLANE: at d = 8 on a 9-pixel plane the mirror image lies on the far side of the centre), split into (hi, lo) ONCE per
//     element and stored as [channel octet][pixel][8 halves] planes -- a B fragment of tap (ky, kx) is one 16-byte read at pixel offset
//     (ky * d) * PW + kx * d.  At d = 8 a patch is 768 pixels = 48 KiB (hi + lo): three (pixel, octet) units per thread, one per stage of the
//     chunk before (loaded at the start of the stage, split and written at its end); two buffers;
//   * one barrier per stage.
// LDS: 2 x 24 KiB + 2 x 48 KiB = 144 KiB at d_max = 8.
#define MD_THREADS 512
#define MD_WBYTES (3 * 4 * 2048)
#define MD_MAX_DIL 8

struct MdParams {
    const float* x;
    long long x_bstride;
    int C, H, W;
    const char* w;        // lama_conv2d_pack_weight image: [chunk][tap row][tap column][32-row fragment][hi | lo][lane][8 halves]
    int mft;              // fragments per k-step = Cout / 32
    const float* bias;
    const float* resid;
    long long resid_bstride;
    float* y;
    long long y_bstride;
    int M, MT, B;
    int TWlog, tiles_x, tiles_y;
    int act;
    int gchunks;          // 16-channel chunks per dilation group
    int dmin;
    int pbytes;           // bytes of ONE patch buffer (hi + lo planes at d_max)
    unsigned* range_flag;
};

__global__ __launch_bounds__(MD_THREADS) void CB_NAME(mdconv_kernel)(MdParams p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 2, wn = wave & 3;
    const int khalf = lane >> 5, l31 = lane & 31;
    char* wbuf0 = lama_smem;
    char* pbuf0 = lama_smem + 2 * MD_WBYTES;

    const int L = lama_xcd_remap(blockIdx.x, gridDim.x);
    const int mt = L % p.MT;
    int tile = L / p.MT;
    const int tix = tile % p.tiles_x;
    tile /= p.tiles_x;
    const int tiy = tile % p.tiles_y;
    const int b = tile / p.tiles_y;
    const int TW = 1 << p.TWlog, TH = 128 >> p.TWlog;
    const int gy0 = tiy * TH, gx0 = tix * TW;
    const int HW = p.H * p.W;
    const float* xb = p.x + (long long)b * p.x_bstride;
    const int nchunk = p.C >> 4, S = nchunk * 3;

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    unsigned rw = 0;   // range watch of the f16 split
    float preg[8];
    u32x4 wreg[3];
    auto dil = [&](int ch) { return p.dmin << (ch / p.gchunks); };
    // unit u of chunk ch = (patch pixel, channel octet): request its 8 channels; returns the unit's LDS byte offset (-1: no such unit)
    auto load_unit = [&](int ch, int u) {
        const int d = dil(ch), PW = TW + 2 * d, NPR = (TH + 2 * d) * PW;
        const int idx = u * MD_THREADS + tid;
        if (idx >= 2 * NPR) return -1;
        const int q = idx >= NPR ? 1 : 0, pp = idx - q * NPR;
        const int py = pp / PW, px = pp - py * PW;
        const int iy = cb_src_coord(gy0 - d + py, p.H, LAMA_PAD_REFLECT), ix = cb_src_coord(gx0 - d + px, p.W, LAMA_PAD_REFLECT);
        const float* xc = xb + (long long)(ch * 16 + q * 8) * HW;
        const unsigned so = (unsigned)(iy * p.W + ix);
#pragma unroll
        for (int e = 0; e < 8; ++e) preg[e] = xc[so + (unsigned)(e * HW)];
        return idx * 16;
    };
    auto write_unit = [&](char* pb, int off, int plo) {
        if (off < 0) return;
        unsigned hh[4], ll[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) cb_split2(preg[2 * e], preg[2 * e + 1], hh[e], ll[e], rw);
        *reinterpret_cast<u32x4*>(pb + off) = u32x4{hh[0], hh[1], hh[2], hh[3]};
        *reinterpret_cast<u32x4*>(pb + plo + off) = u32x4{ll[0], ll[1], ll[2], ll[3]};
    };
    // weight stage st of this M tile: k-step kk = round r, fragment mt * 4 + (tid >> 7) (clamped: rows past M are never stored)
    int F = mt * 4 + (tid >> 7);
    F = F < p.mft ? F : p.mft - 1;
    const int witem = F * 128 + (tid & 127);
    auto load_w = [&](int st) {
        const u32x4* g = reinterpret_cast<const u32x4*>(p.w) + (long long)st * 3 * p.mft * 128;
#pragma unroll
        for (int r = 0; r < 3; ++r) wreg[r] = g[r * p.mft * 128 + witem];
    };
    auto write_w = [&](char* wb) {
#pragma unroll
        for (int r = 0; r < 3; ++r) reinterpret_cast<u32x4*>(wb)[r * MD_THREADS + tid] = wreg[r];
    };

    // prologue: weight stage 0 and the patch of chunk 0
    load_w(0);
    write_w(wbuf0);
    {
        const int d0 = dil(0), plo0 = 2 * (TH + 2 * d0) * (TW + 2 * d0) * 16;
#pragma unroll
        for (int u = 0; u < 3; ++u) write_unit(pbuf0, load_unit(0, u), plo0);
    }
    __syncthreads();

    const int n = wn * 32 + l31;
    const int ty = n >> p.TWlog, tx = n & (TW - 1);
    const int aoff = wm * 2 * 2048 + lane * 16;
    for (int ch = 0; ch < nchunk; ++ch) {
        const int d = dil(ch), PW = TW + 2 * d, NPR = (TH + 2 * d) * PW, plo = 2 * NPR * 16;
        const bool nextc = ch + 1 < nchunk;
        const int dn = nextc ? dil(ch + 1) : d, plon = 2 * (TH + 2 * dn) * (TW + 2 * dn) * 16;
        const char* pb = pbuf0 + (ch & 1) * p.pbytes;
        char* pbn = pbuf0 + ((ch + 1) & 1) * p.pbytes;
        const int boff = (khalf * NPR + ty * PW + tx) * 16;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const int st = ch * 3 + g;
            const char* wb = wbuf0 + (st & 1) * MD_WBYTES;
            const bool more = st + 1 < S;
            if (more) load_w(st + 1);
            const int poff = nextc ? load_unit(ch + 1, g) : -1;
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
                const char* bp = pb + boff + (g * d * PW + kk * d) * 16;
                const bf16x8 bh = *reinterpret_cast<const bf16x8*>(bp);
                const bf16x8 bl = *reinterpret_cast<const bf16x8*>(bp + plo);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const char* ap = wb + (kk * 4 + i) * 2048 + aoff;
                    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(ap);
                    const bf16x8 al = *reinterpret_cast<const bf16x8*>(ap + 1024);
                    acc[i] = CB_MFMA(ah, bh, acc[i], 0, 0, 0);
                    acc[i] = CB_MFMA(ah, bl, acc[i], 0, 0, 0);
                    acc[i] = CB_MFMA(al, bh, acc[i], 0, 0, 0);
                }
            }
            if (more) write_w(wbuf0 + ((st + 1) & 1) * MD_WBYTES);
            write_unit(pbn, poff, plon);
            __syncthreads();
        }
    }
    cb_range_report(rw, p.range_flag);

    // epilogue: D[row = (r&3) + 8*(r>>2) + 4*(lane>>5)][col = lane&31]; resid may be y (read before written, by the thread that writes it)
    const int gy = gy0 + ty, gx = gx0 + tx;
    if (gy >= p.H || gx >= p.W) return;
    const long long pix = (long long)gy * p.W + gx;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mt * 128 + (wm * 2 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
            if (m < p.M) {
                float v = acc[i][r];
                if (p.bias) v += p.bias[m];
                if (p.act == LAMA_ACT_RELU) v = fmaxf(v, 0.0f);
                else if (p.act == LAMA_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
                else if (p.act == LAMA_ACT_TANH) v = tanhf(v);
                const long long o = (long long)m * HW + pix;
                if (p.resid) v += p.resid[(long long)b * p.resid_bstride + o];
                p.y[(long long)b * p.y_bstride + o] = v;
            }
        }
    }
}
