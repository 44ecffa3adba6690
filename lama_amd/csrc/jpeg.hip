// The entropy-coded scan of a baseline JPEG, made on the device from the u8 HWC result slots of the predict step (lama_jpeg_scan_u8_fwd).  A JPEG
// encoder owes its decoder a conforming stream, not particular bytes, so the stream is this engine's own -- integer arithmetic only, shaped for a
// GPU, and pinned byte for byte by tests/jpeg_ref.py::scan_ref:
//   colour      Y  = (19595 R + 38470 G +  7471 B + 32768) >> 16          (JFIF YCbCr in 16-bit fixed point, libjpeg's constants; the Y row sums to
//               Cb = ((-11059 R - 21709 G + 32768 B + 32767) >> 16) + 128   65536 and the chroma rows to 0: gray stays gray.  >> is arithmetic (floor);
//               Cr = (( 32768 R - 27439 G -  5329 B + 32767) >> 16) + 128   32767, not 32768, keeps B = 255 / R = 255 at 255)
//   edges       the last column and row repeated out to the MCU grid: 8 x 8 (4:4:4: Y, Cb, Cr) or 16 x 16 (4:2:0: four Y blocks in raster order, Cb, Cr)
//   4:2:0       chroma sample = (a + b + c + d + 2) >> 2 over each 2 x 2 of the full-size Cb / Cr
//   dummies     4:2:0 only: a Y block that lies wholly outside the image (8 bx >= w or 8 by >= h) is not transformed: its DC level is that of the block
//               coded before it (the same MCU's previous Y block), its AC levels are 0 -- a zero DC difference and an EOB, as libjpeg codes them
//   DCT         s = sample - 128;  C[u][x] = round(2^13 a(u) cos((2x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u) = 1/2 (orthonormal: JPEG's own scale):
//                   2896  2896  2896  2896 |  4017  3406  2276   799 |  3784  1567 -1567 -3784 |  3406  -799 -4017 -2276      (x = 0 .. 3 of u = 0 .. 3;
//                   2896 -2896 -2896  2896 |  2276 -4017   799  3406 |  1567 -3784  3784 -1567 |   799 -2276  3406 -4017       u = 4 .. 7 below them)
//               and C[u][7 - x] = (-1)^u C[u][x].  rows: t[y][u] = (sum_x C[u][x] s[y][x] + 2^7) >> 8 (5 fraction bits); columns:
//               c[v][u] = (sum_y C[v][y] t[y][u] + 2^14) >> 15 -- the coefficient times 8 (3 fraction bits: the quantiser rounds once, not twice)
//   quantise    Q = clamp((base scale + 50) / 100, 1, 255) over the Annex K tables, scale = 5000 / q below 50, 200 - 2 q from there;
//               level = sign(c) ((|c| + 4 Q) / (8 Q))
//   coding      zigzag, the DC difference per component, (run, size) symbols with ZRL and EOB, the Annex K.3 - K.6 Huffman codes, MSB first
//   intervals   one MCU row is one restart interval: DC predictors 0, the bits padded with 1s to a byte, FF stuffed as FF 00, RSTm (m = row mod 8)
//               between two intervals, none behind the last.  The scan only: the headers are the host's (lama_amd.jpeg.jpeg_from_scan).
// int32 throughout.  |s| <= 128, so the sums / differences of two samples are within 256 and a row sum within (4017 + 3406 + 2276 + 799) 256 < 2^22;
// |t| <= 4 x 2896 x 256 / 256 + 1 = 11585, two of them within 23170, a column sum within 10498 x 23170 < 2^28.  Against the real DCT of the same
// samples: a table entry is off by at most 0.5 / 2^13, so a row sum by 8 x 128 x 0.5 / 2^13 = 1/16 and t, with its rounding, by 1/16 + 1/64; the
// columns weigh that with sum_y |a cos| <= 2.83 (0.221), add 8 x (0.5 / 2^13) x 362.1 = 0.177 of their own table error (|t| / 32 <= 362.1) and
// 1/16 of rounding: |c / 8 - real| < 0.46 < 0.5.  A level therefore differs from round(real / Q) by at most 1, and only where real / Q is within
// 0.5 / Q of a rounding boundary.  The division is a multiplication: (n m) >> 26 with m = ceil(2^26 / 8Q) is n / 8Q exactly while n (m 8Q - 2^26) < 2^26,
// and n < 9300, m 8Q - 2^26 < 8Q <= 2040.
//
// One 256-thread workgroup per (image, MCU row), both uniform; it walks the row in segments of 192 blocks (64 MCUs of 4:4:4, 32 of 4:2:0: 512 pixels)
// and carries the bit offset, the unfinished byte and the three DC predictors from one to the next.  Per segment: the pixels (12-byte groups of 4
// where the slot allows dword loads and the group is inside the image, single bytes otherwise -- nothing outside h x w is read) become u8 sample
// planes in LDS; a thread per block transforms and quantises in registers and leaves the levels in LDS in zigzag order; a thread per block counts
// its bits; an exclusive scan places it; the bits are ORed into LDS words (atomicOr: order-independent, so the bytes are deterministic); a scan over
// the FF bytes of each thread's run of the segment's whole bytes places the stuffed bytes.
// Launch 1, jpeg_scan_kernel<.., false>: all of that without a store -- the interval's exact byte count to the workspace.  Launch 2,
// jpeg_offsets_kernel: one workgroup per image turns the counts into offsets (markers included) and writes out_bytes: the length, or -(bytes needed)
// where it exceeds out_stride.  Launch 3, jpeg_scan_kernel<.., true>: the same work again (recomputing costs one more read of the pixels; keeping
// the levels would cost a write and a read of twice as many bytes), the bytes to their final positions and the marker behind them.  The workspace is
// 4 bytes per MCU row.  The sizes are device data: an image whose (h, w) does not fit its slot, or an empty one, yields out_bytes = 0 and touches
// nothing else.  No scratch, no global atomics, plain vector stores only.
#include "common.h"

namespace {
constexpr int JPEG_THREADS = 256, JPEG_SEG_BLOCKS = 192, JPEG_SEG_PIXELS = 512, JPEG_BLOCK_MAX_BITS = 1660;      // 1660: 11 + 11 bits of DC, 63 x (16 + 10) of AC
// LDS carve-up (bytes): levels (int16, a 32-word row per block, the words XORed with the block index: bank = word ^ block) | staging words of the
// segment's bits, the sample planes before them | 8Q reciprocals | Q | DC levels | scan words
constexpr unsigned JL_LEV = 0, JL_STG = JL_LEV + JPEG_SEG_BLOCKS * 128, JL_STG_BYTES = (JPEG_SEG_BLOCKS * JPEG_BLOCK_MAX_BITS + 8 + 7) / 8 + 15 & ~15u;
constexpr unsigned JL_QM = JL_STG + JL_STG_BYTES, JL_Q = JL_QM + 512, JL_DC = JL_Q + 128, JL_MISC = JL_DC + JPEG_SEG_BLOCKS * 2, JL_TOTAL = JL_MISC + 64;
static_assert(JL_TOTAL <= 65536, "one workgroup's LDS");

// (length << 16) | code: DC luma, DC chroma by category; AC luma, AC chroma by (run << 4) | size -- T.81 K.3 - K.6 in canonical order
__device__ const unsigned JPEG_DC_CODE[24] = {
    0x20000, 0x30002, 0x30003, 0x30004, 0x30005, 0x30006, 0x4000e, 0x5001e, 0x6003e, 0x7007e, 0x800fe, 0x901fe,
    0x20000, 0x20001, 0x20002, 0x30006, 0x4000e, 0x5001e, 0x6003e, 0x7007e, 0x800fe, 0x901fe, 0xa03fe, 0xb07fe,
};
__device__ const unsigned JPEG_AC_CODE[512] = {
    0x4000a, 0x20000, 0x20001, 0x30004, 0x4000b, 0x5001a, 0x70078, 0x800f8, 0xa03f6, 0x10ff82, 0x10ff83, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x4000c, 0x5001b, 0x70079, 0x901f6, 0xb07f6, 0x10ff84, 0x10ff85, 0x10ff86, 0x10ff87, 0x10ff88, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x5001c, 0x800f9, 0xa03f7, 0xc0ff4, 0x10ff89, 0x10ff8a, 0x10ff8b, 0x10ff8c, 0x10ff8d, 0x10ff8e, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x6003a, 0x901f7, 0xc0ff5, 0x10ff8f, 0x10ff90, 0x10ff91, 0x10ff92, 0x10ff93, 0x10ff94, 0x10ff95, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x6003b, 0xa03f8, 0x10ff96, 0x10ff97, 0x10ff98, 0x10ff99, 0x10ff9a, 0x10ff9b, 0x10ff9c, 0x10ff9d, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x7007a, 0xb07f7, 0x10ff9e, 0x10ff9f, 0x10ffa0, 0x10ffa1, 0x10ffa2, 0x10ffa3, 0x10ffa4, 0x10ffa5, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x7007b, 0xc0ff6, 0x10ffa6, 0x10ffa7, 0x10ffa8, 0x10ffa9, 0x10ffaa, 0x10ffab, 0x10ffac, 0x10ffad, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x800fa, 0xc0ff7, 0x10ffae, 0x10ffaf, 0x10ffb0, 0x10ffb1, 0x10ffb2, 0x10ffb3, 0x10ffb4, 0x10ffb5, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901f8, 0xf7fc0, 0x10ffb6, 0x10ffb7, 0x10ffb8, 0x10ffb9, 0x10ffba, 0x10ffbb, 0x10ffbc, 0x10ffbd, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901f9, 0x10ffbe, 0x10ffbf, 0x10ffc0, 0x10ffc1, 0x10ffc2, 0x10ffc3, 0x10ffc4, 0x10ffc5, 0x10ffc6, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901fa, 0x10ffc7, 0x10ffc8, 0x10ffc9, 0x10ffca, 0x10ffcb, 0x10ffcc, 0x10ffcd, 0x10ffce, 0x10ffcf, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0xa03f9, 0x10ffd0, 0x10ffd1, 0x10ffd2, 0x10ffd3, 0x10ffd4, 0x10ffd5, 0x10ffd6, 0x10ffd7, 0x10ffd8, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0xa03fa, 0x10ffd9, 0x10ffda, 0x10ffdb, 0x10ffdc, 0x10ffdd, 0x10ffde, 0x10ffdf, 0x10ffe0, 0x10ffe1, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0xb07f8, 0x10ffe2, 0x10ffe3, 0x10ffe4, 0x10ffe5, 0x10ffe6, 0x10ffe7, 0x10ffe8, 0x10ffe9, 0x10ffea, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x10ffeb, 0x10ffec, 0x10ffed, 0x10ffee, 0x10ffef, 0x10fff0, 0x10fff1, 0x10fff2, 0x10fff3, 0x10fff4, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0xb07f9, 0x10fff5, 0x10fff6, 0x10fff7, 0x10fff8, 0x10fff9, 0x10fffa, 0x10fffb, 0x10fffc, 0x10fffd, 0x10fffe, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x20000, 0x20001, 0x30004, 0x4000a, 0x50018, 0x50019, 0x60038, 0x70078, 0x901f4, 0xa03f6, 0xc0ff4, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x4000b, 0x60039, 0x800f6, 0x901f5, 0xb07f6, 0xc0ff5, 0x10ff88, 0x10ff89, 0x10ff8a, 0x10ff8b, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x5001a, 0x800f7, 0xa03f7, 0xc0ff6, 0xf7fc2, 0x10ff8c, 0x10ff8d, 0x10ff8e, 0x10ff8f, 0x10ff90, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x5001b, 0x800f8, 0xa03f8, 0xc0ff7, 0x10ff91, 0x10ff92, 0x10ff93, 0x10ff94, 0x10ff95, 0x10ff96, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x6003a, 0x901f6, 0x10ff97, 0x10ff98, 0x10ff99, 0x10ff9a, 0x10ff9b, 0x10ff9c, 0x10ff9d, 0x10ff9e, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x6003b, 0xa03f9, 0x10ff9f, 0x10ffa0, 0x10ffa1, 0x10ffa2, 0x10ffa3, 0x10ffa4, 0x10ffa5, 0x10ffa6, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x70079, 0xb07f7, 0x10ffa7, 0x10ffa8, 0x10ffa9, 0x10ffaa, 0x10ffab, 0x10ffac, 0x10ffad, 0x10ffae, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x7007a, 0xb07f8, 0x10ffaf, 0x10ffb0, 0x10ffb1, 0x10ffb2, 0x10ffb3, 0x10ffb4, 0x10ffb5, 0x10ffb6, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x800f9, 0x10ffb7, 0x10ffb8, 0x10ffb9, 0x10ffba, 0x10ffbb, 0x10ffbc, 0x10ffbd, 0x10ffbe, 0x10ffbf, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901f7, 0x10ffc0, 0x10ffc1, 0x10ffc2, 0x10ffc3, 0x10ffc4, 0x10ffc5, 0x10ffc6, 0x10ffc7, 0x10ffc8, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901f8, 0x10ffc9, 0x10ffca, 0x10ffcb, 0x10ffcc, 0x10ffcd, 0x10ffce, 0x10ffcf, 0x10ffd0, 0x10ffd1, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901f9, 0x10ffd2, 0x10ffd3, 0x10ffd4, 0x10ffd5, 0x10ffd6, 0x10ffd7, 0x10ffd8, 0x10ffd9, 0x10ffda, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901fa, 0x10ffdb, 0x10ffdc, 0x10ffdd, 0x10ffde, 0x10ffdf, 0x10ffe0, 0x10ffe1, 0x10ffe2, 0x10ffe3, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0xb07f9, 0x10ffe4, 0x10ffe5, 0x10ffe6, 0x10ffe7, 0x10ffe8, 0x10ffe9, 0x10ffea, 0x10ffeb, 0x10ffec, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0xe3fe0, 0x10ffed, 0x10ffee, 0x10ffef, 0x10fff0, 0x10fff1, 0x10fff2, 0x10fff3, 0x10fff4, 0x10fff5, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0xa03fa, 0xf7fc3, 0x10fff6, 0x10fff7, 0x10fff8, 0x10fff9, 0x10fffa, 0x10fffb, 0x10fffc, 0x10fffd, 0x10fffe, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
};
__device__ const unsigned char JPEG_QUANT_BASE[128] = {
     16,  11,  10,  16,  24,  40,  51,  61,  12,  12,  14,  19,  26,  58,  60,  55,
     14,  13,  16,  24,  40,  57,  69,  56,  14,  17,  22,  29,  51,  87,  80,  62,
     18,  22,  37,  56,  68, 109, 103,  77,  24,  35,  55,  64,  81, 104, 113,  92,
     49,  64,  78,  87, 103, 121, 120, 101,  72,  92,  95,  98, 112, 100, 103,  99,
     17,  18,  24,  47,  99,  99,  99,  99,  18,  21,  26,  66,  99,  99,  99,  99,
     24,  26,  56,  99,  99,  99,  99,  99,  47,  66,  99,  99,  99,  99,  99,  99,
     99,  99,  99,  99,  99,  99,  99,  99,  99,  99,  99,  99,  99,  99,  99,  99,
     99,  99,  99,  99,  99,  99,  99,  99,  99,  99,  99,  99,  99,  99,  99,  99,
};
__device__ const unsigned char JPEG_ZIGZAG_OF[64] = {
     0,  1,  5,  6, 14, 15, 27, 28,
     2,  4,  7, 13, 16, 26, 29, 42,
     3,  8, 12, 17, 25, 30, 41, 43,
     9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54,
    20, 22, 33, 38, 46, 51, 55, 60,
    21, 34, 37, 47, 50, 56, 59, 61,
    35, 36, 48, 49, 57, 58, 62, 63,
};

struct JpegParams {
    const uint8_t* image;      // [batch][Hs][Ws][3]
    const int32_t* sizes;      // device [batch][2] = (h, w)
    uint8_t* out;              // batch scan slots of out_stride bytes
    int32_t* out_bytes;        // device [batch]
    unsigned* lens;            // workspace [batch][max_rows]: launch 1 the interval's bytes, launch 2 its offset
    unsigned long long out_stride;
    int Hs, Ws, max_rows, quality, aligned;      // aligned: slot pointer and Ws 3 are multiples of 4
};

// inclusive-to-exclusive scan of one value per thread over the 256-thread workgroup; `ws`: 4 LDS words of its own per call site
__device__ __forceinline__ unsigned jpeg_exscan(unsigned v, unsigned* ws, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl(inc, lane >= d ? lane - d : lane);
        if (lane >= d) inc += o;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    unsigned base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned t = ws[k];
        base += k < wave ? t : 0u;
        tot += t;
    }
    total = tot;
    return base + inc - v;
}

// (h, w) of image `img` and its MCU grid; false: an empty slot or sizes that do not fit it
template <int SS> __device__ __forceinline__ bool jpeg_image_geom(const JpegParams& p, int img, int& h, int& w, int& rows, int& mpr) {
    h = p.sizes[2 * img];
    w = p.sizes[2 * img + 1];
    if (h < 1 || w < 1 || h > p.Hs || w > p.Ws) return false;
    constexpr int M = SS ? 16 : 8;
    rows = (h + M - 1) / M;
    mpr = (w + M - 1) / M;
    return true;
}

// one 8-point pass of the DCT: the table's symmetry C[u][7 - x] = (-1)^u C[u][x] halves the products, the integers are the same
__device__ __forceinline__ void jpeg_dct8(const int (&s)[8], int (&o)[8], int round, int shift) {
    const int e0 = s[0] + s[7], e1 = s[1] + s[6], e2 = s[2] + s[5], e3 = s[3] + s[4];
    const int d0 = s[0] - s[7], d1 = s[1] - s[6], d2 = s[2] - s[5], d3 = s[3] - s[4];
    o[0] = (2896 * (e0 + e1 + e2 + e3) + round) >> shift;
    o[4] = (2896 * (e0 - e1 - e2 + e3) + round) >> shift;
    o[2] = (3784 * (e0 - e3) + 1567 * (e1 - e2) + round) >> shift;
    o[6] = (1567 * (e0 - e3) - 3784 * (e1 - e2) + round) >> shift;
    o[1] = (4017 * d0 + 3406 * d1 + 2276 * d2 + 799 * d3 + round) >> shift;
    o[3] = (3406 * d0 - 799 * d1 - 4017 * d2 - 2276 * d3 + round) >> shift;
    o[5] = (2276 * d0 - 4017 * d1 + 799 * d2 + 3406 * d3 + round) >> shift;
    o[7] = (799 * d0 - 2276 * d1 + 3406 * d2 - 4017 * d3 + round) >> shift;
}

// level `zz` (zigzag position) of block b in the swizzled LDS rows
__device__ __forceinline__ unsigned jpeg_lev_at(int b, int zz) { return (unsigned)b * 64u + (((((unsigned)zz >> 1) ^ ((unsigned)b & 31u)) << 1) | ((unsigned)zz & 1u)); }

// MSB-first bits: counted (EMIT false) or ORed into the big-endian staging words from a bit position on
template <bool EMIT> struct JpegSink {
    unsigned* words;
    unsigned wi, fill, bits;
    unsigned long long acc;
    __device__ __forceinline__ JpegSink(unsigned* w, unsigned pos) : words(w), wi(pos >> 5), fill(pos & 31u), bits(0), acc(0) {}
    __device__ __forceinline__ void put(unsigned v, unsigned n) {      // n <= 27
        if (!EMIT) {
            bits += n;
            return;
        }
        acc = (acc << n) | v;
        fill += n;
        if (fill >= 32u) {
            fill -= 32u;
            atomicOr(&words[wi], (unsigned)(acc >> fill));
            ++wi;
            acc &= (1ull << fill) - 1ull;
        }
    }
    __device__ __forceinline__ void flush() {
        if (EMIT && fill) atomicOr(&words[wi], (unsigned)(acc << (32u - fill)));
    }
};

__device__ __forceinline__ void jpeg_size_bits(int v, unsigned& cat, unsigned& bits) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    cat = a ? 32u - (unsigned)__builtin_clz(a) : 0u;
    bits = (unsigned)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
}

// one block: the DC difference, then the AC levels of LDS row b (dummy: none) -- tab 0 luma, 1 chroma
template <bool EMIT> __device__ __forceinline__ void jpeg_code_block(JpegSink<EMIT>& sink, const short* lev, int b, int diff, bool dummy, int tab) {
    unsigned cat, bits;
    jpeg_size_bits(diff, cat, bits);
    unsigned t = JPEG_DC_CODE[tab * 12 + (int)cat];
    sink.put(((t & 0xffffu) << cat) | bits, (t >> 16) + cat);
    const unsigned* ac = JPEG_AC_CODE + tab * 256;
    unsigned run = 0;
    if (dummy) run = 63;
    else
        for (int zz = 1; zz < 64; ++zz) {
            const int v = lev[jpeg_lev_at(b, zz)];
            if (v == 0) {
                ++run;
                continue;
            }
            for (; run >= 16u; run -= 16u) sink.put(ac[0xf0] & 0xffffu, ac[0xf0] >> 16);
            jpeg_size_bits(v, cat, bits);
            t = ac[(run << 4) | cat];
            sink.put(((t & 0xffffu) << cat) | bits, (t >> 16) + cat);
            run = 0;
        }
    if (run) sink.put(ac[0] & 0xffffu, ac[0] >> 16);
}

template <int SS, bool EMIT> __global__ __launch_bounds__(JPEG_THREADS) void jpeg_scan_kernel(JpegParams p) {
    constexpr int M = SS ? 16 : 8, BPM = SS ? 6 : 3, T = JPEG_SEG_BLOCKS / BPM, RV = SS ? 2 : 1;      // MCU side, blocks per MCU, MCUs per segment, rows per load unit
    constexpr unsigned CB_AT = SS ? 8192u : 4096u, CR_AT = SS ? 10240u : 8192u;                        // sample planes: Y rows of 512, then Cb, Cr (rows of 256 for 4:2:0)
    constexpr int CW = SS ? 256 : 512;
    const int tid = threadIdx.x;
    const int img = blockIdx.x / p.max_rows, row = blockIdx.x - img * p.max_rows;
    int h, w, rows, mpr;
    if (!jpeg_image_geom<SS>(p, img, h, w, rows, mpr) || row >= rows) return;
    if (EMIT && p.out_bytes[img] <= 0) return;                             // (launch 2 wrote it: the scan does not fit its slot)
    short* lev = reinterpret_cast<short*>(lama_smem + JL_LEV);
    unsigned* stg = reinterpret_cast<unsigned*>(lama_smem + JL_STG);
    unsigned char* smp = reinterpret_cast<unsigned char*>(lama_smem + JL_STG);
    unsigned* qm = reinterpret_cast<unsigned*>(lama_smem + JL_QM);
    unsigned char* qq = reinterpret_cast<unsigned char*>(lama_smem + JL_Q);
    short* dcv = reinterpret_cast<short*>(lama_smem + JL_DC);
    unsigned* misc = reinterpret_cast<unsigned*>(lama_smem + JL_MISC);      // [0..3] [4..7]: scan words

    if (tid < 128) {                                                        // the two quantisation tables in zigzag order, and the reciprocals of 8Q
        const int scale = p.quality < 50 ? 5000 / p.quality : 200 - 2 * p.quality;
        int q = ((int)JPEG_QUANT_BASE[tid] * scale + 50) / 100;
        q = q < 1 ? 1 : (q > 255 ? 255 : q);
        const int at = (tid & 64) + JPEG_ZIGZAG_OF[tid & 63];
        qq[at] = (unsigned char)q;
        qm[at] = ((1u << 26) + 8u * (unsigned)q - 1u) / (8u * (unsigned)q);
    }
    const uint8_t* base = p.image + (long long)img * p.Hs * p.Ws * 3;
    const long long rstride = (long long)p.Ws * 3;
    const int y0 = row * M;
    uint8_t* out = p.out + (unsigned long long)img * p.out_stride;
    unsigned opos = EMIT ? p.lens[(long long)img * p.max_rows + row] : 0u;     // bytes of the interval so far (launch 3: from its offset on)
    unsigned cb = 0, carry = 0;                                             // the unfinished byte: its bit count and its bits
    int pred0 = 0, pred1 = 0, pred2 = 0;                                    // DC predictors: Y, Cb, Cr
    __syncthreads();

    for (int m0 = 0; m0 < mpr; m0 += T) {
        const int nm = mpr - m0 < T ? mpr - m0 : T, nb = nm * BPM;
        const bool last = m0 + T >= mpr;
        // ---- pixels -> sample planes: units of 4 pixels x RV rows
        const int ux_n = nm * M / 4, x0 = m0 * M;
        for (int u = tid; u < ux_n * 8; u += JPEG_THREADS) {
            const int uy = u / ux_n, ux = u - uy * ux_n, lx = ux * 4, gx = x0 + lx;
            int cbs[2] = {0, 0}, crs[2] = {0, 0};
#pragma unroll
            for (int r = 0; r < RV; ++r) {
                const int ly = uy * RV + r, gy = y0 + ly < h ? y0 + ly : h - 1;
                const uint8_t* rp = base + gy * rstride;
                unsigned R[4], G[4], B[4];
                if (p.aligned && gx + 3 < w) {
                    const unsigned* q = reinterpret_cast<const unsigned*>(rp + gx * 3);
                    const unsigned d0 = q[0], d1 = q[1], d2 = q[2];
                    R[0] = d0 & 255u; G[0] = (d0 >> 8) & 255u; B[0] = (d0 >> 16) & 255u;
                    R[1] = d0 >> 24; G[1] = d1 & 255u; B[1] = (d1 >> 8) & 255u;
                    R[2] = (d1 >> 16) & 255u; G[2] = d1 >> 24; B[2] = d2 & 255u;
                    R[3] = (d2 >> 8) & 255u; G[3] = (d2 >> 16) & 255u; B[3] = d2 >> 24;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int x = gx + i < w ? gx + i : w - 1;
                        R[i] = rp[x * 3]; G[i] = rp[x * 3 + 1]; B[i] = rp[x * 3 + 2];
                    }
                }
                unsigned yp = 0, cbp = 0, crp = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r_ = (int)R[i], g_ = (int)G[i], b_ = (int)B[i];
                    const int yy = (19595 * r_ + 38470 * g_ + 7471 * b_ + 32768) >> 16;
                    const int cbv = ((-11059 * r_ - 21709 * g_ + 32768 * b_ + 32767) >> 16) + 128;
                    const int crv = ((32768 * r_ - 27439 * g_ - 5329 * b_ + 32767) >> 16) + 128;
                    yp |= (unsigned)yy << (8 * i);
                    if (SS) {
                        cbs[i >> 1] += cbv;
                        crs[i >> 1] += crv;
                    } else {
                        cbp |= (unsigned)cbv << (8 * i);
                        crp |= (unsigned)crv << (8 * i);
                    }
                }
                *reinterpret_cast<unsigned*>(smp + ly * 512 + lx) = yp;
                if (!SS) {
                    *reinterpret_cast<unsigned*>(smp + CB_AT + ly * 512 + lx) = cbp;
                    *reinterpret_cast<unsigned*>(smp + CR_AT + ly * 512 + lx) = crp;
                }
            }
            if (SS) {
                *reinterpret_cast<unsigned short*>(smp + CB_AT + uy * 256 + ux * 2) = (unsigned short)(((cbs[0] + 2) >> 2) | (((cbs[1] + 2) >> 2) << 8));
                *reinterpret_cast<unsigned short*>(smp + CR_AT + uy * 256 + ux * 2) = (unsigned short)(((crs[0] + 2) >> 2) | (((crs[1] + 2) >> 2) << 8));
            }
        }
        __syncthreads();

        // ---- a thread per block: where it is, whether it is a dummy
        const int b = tid, mcu = b / BPM, k = b - mcu * BPM;
        const bool luma = SS ? k < 4 : k == 0;
        bool dummy[4] = {false, false, false, false};                       // of the MCU's Y blocks (4:2:0)
        if (SS) {
#pragma unroll
            for (int j = 1; j < 4; ++j) dummy[j] = 8 * (2 * (m0 + mcu) + (j & 1)) >= w || 8 * (2 * row + (j >> 1)) >= h;
        }
        const bool mine_dummy = SS && k < 4 && dummy[k & 3];
        if (b < nb && !mine_dummy) {
            // ---- DCT and quantisation in registers, the levels to LDS in zigzag order
            const unsigned char* sp;
            int stride = 512;
            if (!SS) sp = smp + (k == 0 ? 0u : (k == 1 ? CB_AT : CR_AT)) + mcu * 8;
            else if (k < 4) sp = smp + (k >> 1) * 8 * 512 + (mcu * 2 + (k & 1)) * 8;
            else {
                sp = smp + (k == 4 ? CB_AT : CR_AT) + mcu * 8;
                stride = CW;
            }
            int t[8][8];
#pragma unroll
            for (int y = 0; y < 8; ++y) {
                const unsigned lo = *reinterpret_cast<const unsigned*>(sp + y * stride), hi = *reinterpret_cast<const unsigned*>(sp + y * stride + 4);
                int s[8];
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    s[x] = (int)((lo >> (8 * x)) & 255u) - 128;
                    s[4 + x] = (int)((hi >> (8 * x)) & 255u) - 128;
                }
                jpeg_dct8(s, t[y], 1 << 7, 8);
            }
            const int qo = luma ? 0 : 64;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                int col[8], c[8];
#pragma unroll
                for (int y = 0; y < 8; ++y) col[y] = t[y][u];
                jpeg_dct8(col, c, 1 << 14, 15);
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    const int zz = JPEG_ZIGZAG_OF[v * 8 + u];
                    const unsigned a = (unsigned)(c[v] < 0 ? -c[v] : c[v]) + 4u * qq[qo + zz];
                    const int l = (int)(unsigned)(((unsigned long long)a * qm[qo + zz]) >> 26);
                    const short s16 = (short)(c[v] < 0 ? -l : l);
                    lev[jpeg_lev_at(b, zz)] = s16;
                    if (zz == 0) dcv[b] = s16;
                }
            }
        }
        __syncthreads();

        // ---- the block's DC difference (a dummy takes the DC of the real block before it: difference 0) and its bits
        int diff = 0;
        if (b < nb && !mine_dummy) {
            int pred;
            if (!SS) pred = mcu == 0 ? (k == 0 ? pred0 : (k == 1 ? pred1 : pred2)) : dcv[b - 3];
            else if (k >= 4) pred = mcu == 0 ? (k == 4 ? pred1 : pred2) : dcv[b - 6];
            else if (k == 0) {
                if (mcu == 0) pred = pred0;
                else {                                                      // the previous MCU's last real Y block (its dummies are this MCU's: the same row, the next column
                    int j = 3;                                              //  -- but the column parity differs only at the right edge, where no MCU follows)
                    const bool pd1 = 8 * (2 * (m0 + mcu - 1) + 1) >= w, pdb = 8 * (2 * row + 1) >= h;
                    while (j > 0 && ((j & 1) ? (pd1 || (j >> 1 && pdb)) : pdb)) --j;
                    pred = dcv[b - 6 + j];
                }
            } else {
                int j = k - 1;
                while (j > 0 && dummy[j]) --j;
                pred = dcv[b - k + j];
            }
            diff = (int)dcv[b] - pred;
        }
        unsigned nbits = 0;
        if (b < nb) {
            JpegSink<false> cnt(nullptr, 0);
            jpeg_code_block<false>(cnt, lev, b, diff, mine_dummy, luma ? 0 : 1);
            nbits = cnt.bits;
        }
        unsigned total;
        const unsigned my_bit = jpeg_exscan(nbits, misc, total);
        const unsigned end_bit = cb + total, pad = last ? (8u - (end_bit & 7u)) & 7u : 0u;
        const unsigned n_words = (end_bit + pad + 31u) >> 5;
        // the next segment's predictors: the last MCU's last real Y block, its Cb, its Cr (read before anything overwrites them; uniform)
        {
            const int lb = (nm - 1) * BPM;
            if (!SS) {
                pred0 = dcv[lb];
                pred1 = dcv[lb + 1];
                pred2 = dcv[lb + 2];
            } else {
                int j = 3;
                const bool pd1 = 8 * (2 * (m0 + nm - 1) + 1) >= w, pdb = 8 * (2 * row + 1) >= h;
                while (j > 0 && ((j & 1) ? (pd1 || (j >> 1 && pdb)) : pdb)) --j;
                pred0 = dcv[lb + j];
                pred1 = dcv[lb + 4];
                pred2 = dcv[lb + 5];
            }
        }
        for (unsigned i = tid; i < n_words; i += JPEG_THREADS) stg[i] = 0;      // (the sample planes are done with: every thread is past the scan's barrier)
        __syncthreads();
        if (tid == 0 && cb) atomicOr(&stg[0], carry << (32u - cb));
        if (b < nb) {
            JpegSink<true> sink(stg, cb + my_bit);
            jpeg_code_block<true>(sink, lev, b, diff, mine_dummy, luma ? 0 : 1);
            sink.flush();
        }
        if (tid == JPEG_THREADS - 1 && pad) {
            JpegSink<true> sink(stg, end_bit);
            sink.put((1u << pad) - 1u, pad);
            sink.flush();
        }
        __syncthreads();

        // ---- the segment's whole bytes, FF stuffed: a contiguous run per thread
        const unsigned n_bytes = (end_bit + pad) >> 3;
        const unsigned per = (n_bytes + JPEG_THREADS - 1) / JPEG_THREADS;
        const unsigned i0 = tid * per < n_bytes ? tid * per : n_bytes, i1 = i0 + per < n_bytes ? i0 + per : n_bytes;
        unsigned ff = 0;
        for (unsigned i = i0; i < i1; ++i) ff += ((stg[i >> 2] >> (24u - 8u * (i & 3u))) & 255u) == 255u ? 1u : 0u;
        unsigned ff_total;
        const unsigned ff_before = jpeg_exscan(ff, misc + 4, ff_total);
        if (EMIT) {
            uint8_t* d = out + opos + i0 + ff_before;
            for (unsigned i = i0; i < i1; ++i) {
                const unsigned v = (stg[i >> 2] >> (24u - 8u * (i & 3u))) & 255u;
                *d++ = (uint8_t)v;
                if (v == 255u) *d++ = 0;
            }
        }
        opos += n_bytes + ff_total;
        cb = (end_bit + pad) & 7u;
        carry = cb ? ((stg[n_bytes >> 2] >> (24u - 8u * (n_bytes & 3u))) & 255u) >> (8u - cb) : 0u;
        __syncthreads();
    }
    if (tid == 0) {
        if (!EMIT) p.lens[(long long)img * p.max_rows + row] = opos;
        else if (row < rows - 1) {
            out[opos] = 0xff;
            out[opos + 1] = (uint8_t)(0xd0 + (row & 7));
        }
    }
}

// per image: the intervals' byte counts -> their offsets (2 bytes of marker behind every interval but the last), and out_bytes
template <int SS> __global__ __launch_bounds__(JPEG_THREADS) void jpeg_offsets_kernel(JpegParams p) {
    const int tid = threadIdx.x, img = blockIdx.x;
    int h, w, rows, mpr;
    if (!jpeg_image_geom<SS>(p, img, h, w, rows, mpr)) {
        if (tid == 0) p.out_bytes[img] = 0;
        return;
    }
    unsigned* misc = reinterpret_cast<unsigned*>(lama_smem);
    unsigned* lens = p.lens + (long long)img * p.max_rows;
    unsigned carry = 0;
    for (int t0 = 0; t0 < rows; t0 += JPEG_THREADS) {
        const int j = t0 + tid;
        const unsigned n = j < rows ? lens[j] + (j < rows - 1 ? 2u : 0u) : 0u;
        unsigned tot;
        const unsigned before = jpeg_exscan(n, misc, tot);
        if (j < rows) lens[j] = carry + before;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) p.out_bytes[img] = (unsigned long long)carry <= p.out_stride ? (int32_t)carry : -(int32_t)carry;
}

bool jpeg_grid(int32_t h, int32_t w, int32_t ss, long long& rows, long long& mpr) {
    if ((ss != LAMA_JPEG_444 && ss != LAMA_JPEG_420) || h < 1 || w < 1 || h > 65535 || w > 65535) return false;
    const int M = ss == LAMA_JPEG_420 ? 16 : 8;
    rows = (h + M - 1) / M;
    mpr = (w + M - 1) / M;
    return true;
}
}  // namespace

extern "C" size_t lama_jpeg_scan_bound(int32_t h, int32_t w, int32_t subsampling) {
    long long rows, mpr;
    if (!jpeg_grid(h, w, subsampling, rows, mpr)) return 0;
    // every block at its longest codes, every byte of an interval stuffed, the markers between the intervals
    const long long per = 2 * ((mpr * (subsampling == LAMA_JPEG_420 ? 6 : 3) * JPEG_BLOCK_MAX_BITS + 7) / 8);
    return (size_t)(rows * per + 2 * (rows - 1));
}

static int jpeg_check(int32_t batch, int32_t Hs, int32_t Ws, int32_t subsampling, long long& rows) {
    if (batch <= 0 || Hs <= 0 || Ws <= 0 || (subsampling != LAMA_JPEG_444 && subsampling != LAMA_JPEG_420)) return LAMA_ERR_BAD_ARG;
    long long mpr;
    if (!jpeg_grid(Hs, Ws, subsampling, rows, mpr) || mpr > 65535) return LAMA_ERR_UNSUPPORTED;      // SOF0 and DRI hold 16 bits
    if (lama_jpeg_scan_bound(Hs, Ws, subsampling) > 0x7fffffffull || (long long)batch * rows > 0x3fffffffll) return LAMA_ERR_UNSUPPORTED;      // out_bytes is an int32; one grid dimension
    return LAMA_OK;
}

extern "C" int lama_jpeg_scan_workspace_bytes(int32_t batch, int32_t Hs, int32_t Ws, int32_t subsampling, size_t* bytes) {
    if (!bytes) return LAMA_ERR_BAD_ARG;
    long long rows;
    const int rc = jpeg_check(batch, Hs, Ws, subsampling, rows);
    if (rc != LAMA_OK) return rc;
    *bytes = ((size_t)batch * rows * sizeof(unsigned) + 15) & ~(size_t)15;
    return LAMA_OK;
}

extern "C" int lama_jpeg_scan_u8_fwd(void* stream, const uint8_t* image_hwc, const int32_t* sizes, int32_t Hs, int32_t Ws, int32_t batch, int32_t quality,
                                     int32_t subsampling, uint8_t* out, size_t out_stride, int32_t* out_bytes, void* workspace, size_t workspace_bytes) {
    if (!image_hwc || !sizes || !out || !out_bytes || !workspace || quality < 1 || quality > 100) return LAMA_ERR_BAD_ARG;
    long long rows;
    const int rc = jpeg_check(batch, Hs, Ws, subsampling, rows);
    if (rc != LAMA_OK) return rc;
    if (((unsigned long long)workspace & 15) || ((unsigned long long)sizes & 3) || ((unsigned long long)out_bytes & 3)) return LAMA_ERR_BAD_ARG;
    const size_t n_rows = (size_t)batch * rows;
    if (workspace_bytes < ((n_rows * sizeof(unsigned) + 15) & ~(size_t)15)) return LAMA_ERR_WORKSPACE;
    JpegParams p;
    p.image = image_hwc; p.sizes = sizes; p.out = out; p.out_bytes = out_bytes;
    p.lens = reinterpret_cast<unsigned*>(workspace);
    p.out_stride = out_stride;
    p.Hs = Hs; p.Ws = Ws; p.max_rows = (int)rows; p.quality = quality;
    p.aligned = !(((unsigned long long)image_hwc | (unsigned long long)((long long)Ws * 3)) & 3) ? 1 : 0;
    const dim3 grid((unsigned)n_rows), block(JPEG_THREADS);
    const hipStream_t s = (hipStream_t)stream;
    if (subsampling == LAMA_JPEG_420) hipLaunchKernelGGL((jpeg_scan_kernel<1, false>), grid, block, JL_TOTAL, s, p);
    else hipLaunchKernelGGL((jpeg_scan_kernel<0, false>), grid, block, JL_TOTAL, s, p);
    LAMA_CHECK_LAUNCH();
    if (subsampling == LAMA_JPEG_420) hipLaunchKernelGGL(jpeg_offsets_kernel<1>, dim3((unsigned)batch), block, 16 * sizeof(unsigned), s, p);
    else hipLaunchKernelGGL(jpeg_offsets_kernel<0>, dim3((unsigned)batch), block, 16 * sizeof(unsigned), s, p);
    LAMA_CHECK_LAUNCH();
    if (subsampling == LAMA_JPEG_420) hipLaunchKernelGGL((jpeg_scan_kernel<1, true>), grid, block, JL_TOTAL, s, p);
    else hipLaunchKernelGGL((jpeg_scan_kernel<0, true>), grid, block, JL_TOTAL, s, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}
