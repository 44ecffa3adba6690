// The zlib stream of a PNG's IDAT, made on the device from the u8 HWC result slots of the predict step (lama_png_deflate_u8_fwd).  A PNG encoder
// owes its decoder the pixels, not particular bytes, so the stream is this engine's own -- shaped for a GPU, and pinned byte for byte by
// tests/png_ref.py::deflate_ref:
//   filtered bytes   per row the byte 1 (Sub), then w c bytes x[i] - x[i - c] mod 256 (the first pixel as is); row = 1 + w c
//   chunks           R = max(1, chunk_bytes / row) whole rows, the last one may be shorter; each is coded on its own and ends on a byte boundary
//   one chunk        ONE dynamic-Huffman block of literals (BFINAL 0, BTYPE 10, HLIT 0, HDIST 0 with a distance code of length 0, HCLEN 15 with the
//                    complete 4-bit code-length code: every code length travels as 4 bits, 1106 header bits), symbol 256, then an empty stored block
//                    (000, pad, 00 00 FF FF); or, where that is not shorter than raw + 5 bytes, the stored form 00 LEN ~LEN + raw
//   code lengths     depths of the Huffman tree over the used symbols (256 counts once): two-queue merge over the symbols sorted by (count, symbol), a
//                    leaf before an internal node on ties; deeper than 15: every non-zero count n becomes (n + 1) >> 1 and the tree is built again
//   image            78 01, the chunks, 01 00 00 FF FF, Adler-32 of the filtered bytes (big endian)
// No matches (not even distance 1), no filter but Sub, 8-bit gray / RGB only; the PNG container and its CRC are the host's (predict.png_from_zlib).
//
// Launch 1, png_encode_kernel: one 256-thread workgroup per (image, chunk), both uniform.  The chunk's rows are read from the slot with 16-byte,
// 4-byte or single-byte loads (what Ws c and the slot pointer allow), Sub-filtered four bytes at a time (SWAR) into LDS and counted with LDS
// atomics.  The table: every thread ranks its own symbol among the used ones (257 broadcast reads), ONE lane runs the two-queue merge (the serial
// part: at most 256 merges of two dependent LDS reads each), every thread walks its leaf up to the root for its depth and counts the shorter codes
// for its canonical code.  Every thread then codes a contiguous run of the chunk: the run's bit count (and its share of the chunk's Adler sums), a
// block-wide exclusive scan, the bits ORed into an LDS word buffer (atomicOr: order-independent, so the bytes are deterministic).  The result
// goes to the chunk's slot in the workspace with 16-byte stores, its record (bytes, Adler sums, raw length) beside it.
// Launch 2, png_assemble_kernel: per image one workgroup for every four chunks and one more.  A copy workgroup sums the sizes of the chunks in front
// of its own (their records: 16 bytes each) and copies its four behind them (a wave per chunk; dword stores with a byte alignment shift between the
// 16-byte aligned workspace slot and the byte-granular destination, single bytes at a chunk's two ends).  The last workgroup walks the records in tiles
// of 256 -- the total size, the Adler sums combined in chunk order -- and writes 78 01, the final block, the Adler-32 and out_bytes.  (One workgroup per
// image that also copied took 2.6 ms for 8 x 2048^2: 8 workgroups moving 68 MB.)
// The sizes are device data: an image whose (h, w) does not fit its slot, or an empty one, yields out_bytes = 0 and touches nothing else; nothing is
// read or written outside a slot for any sizes array.  No scratch, no global atomics, plain vector stores only.
#include "common.h"

namespace {
constexpr int PNG_THREADS = 256, PNG_COPY_CHUNKS = 4;      // PNG_COPY_CHUNKS: chunks per copy workgroup of the assembly, a wave each
constexpr int PNG_DEFAULT_CHUNK = 24576, PNG_MIN_CHUNK = 64, PNG_MAX_CHUNK = 32768, PNG_MAX_RAW = 65535;
constexpr int PNG_HEADER_BITS = 17 + 3 * 19 + 4 * 258;      // 1106
constexpr unsigned PNG_ADLER = 65521u;

typedef unsigned png_u32x4 __attribute__((ext_vector_type(4)));

struct PngGeom {
    int max_chunks;      // per image: ceil(Hs / R(Ws)), the most any (h <= Hs, w <= Ws) can have
    int max_raw;         // bytes of the largest chunk any such image can have
    size_t slot;         // workspace bytes per chunk: max_raw + 16 rounded up to 16
};

// (host) the chunk geometry of a slot; row(Ws) <= 65535 is checked by the caller
PngGeom png_geom(int Hs, int Ws, int c, int chunk_bytes) {
    const int row = 1 + Ws * c;
    const int R = chunk_bytes / row > 1 ? chunk_bytes / row : 1;
    PngGeom g;
    g.max_chunks = lama_ceil_div(Hs, R);
    g.max_raw = chunk_bytes > row ? chunk_bytes : row;
    g.slot = ((size_t)g.max_raw + 16 + 15) & ~(size_t)15;
    return g;
}

// LDS carve-up (bytes, every part 16-byte aligned): raw | out words | hist | lens | tab | weight | parent | leafsym | misc
struct PngLds {
    unsigned raw, out, hist, lens, tab, weight, parent, leafsym, misc, total;
};
__host__ __device__ inline PngLds png_lds(int max_raw) {
    PngLds l;
    unsigned o = 0;
    l.raw = o; o += ((unsigned)max_raw + 4 + 15) & ~15u;
    l.out = o; o += ((unsigned)max_raw + 16 + 15) & ~15u;
    l.hist = o; o += 272 * 4;
    l.lens = o; o += 272 * 4;
    l.tab = o; o += 272 * 4;
    l.weight = o; o += 528 * 4;
    l.parent = o; o += 528 * 2;
    l.leafsym = o; o += 272 * 2;
    l.misc = o; o += 64 * 4;
    l.total = o;
    return l;
}

struct PngParams {
    const uint8_t* image;      // [batch][Hs][Ws][c]
    const int32_t* sizes;      // device [batch][2] = (h, w)
    uint8_t* out;              // batch stream slots of out_stride bytes
    int32_t* out_bytes;        // device [batch]
    png_u32x4* recs;           // workspace: [batch][max_chunks] (bytes, s1, s2, raw length)
    uint8_t* slots;            // workspace: [batch][max_chunks] chunk slots of `slot` bytes
    unsigned long long out_stride, slot;
    int Hs, Ws, c, chunk_bytes, max_chunks, max_raw, merge_reps;
};

// inclusive-to-exclusive scan of one value per thread over the 256-thread workgroup; `ws`: 4 LDS words of its own per call site
__device__ __forceinline__ unsigned png_exscan(unsigned v, unsigned* ws, unsigned& total) {
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

// `n` bits of `v` ORed into the LSB-first bit stream at bit `pos`
__device__ __forceinline__ void png_or_bits(unsigned* words, unsigned pos, unsigned v, unsigned n) {
    const unsigned w = pos >> 5, s = pos & 31;
    atomicOr(&words[w], v << s);
    if (s + n > 32) atomicOr(&words[w + 1], v >> (32 - s));
}

__device__ __forceinline__ void png_count4(unsigned* hist, unsigned char* dst, unsigned f, int i, int wc) {
    if (i + 3 < wc && f == (f & 0xffu) * 0x01010101u) {              // four equal bytes (flat regions): one atomic instead of four on one address
        dst[0] = dst[1] = dst[2] = dst[3] = (unsigned char)f;
        atomicAdd(&hist[f & 0xffu], 4u);
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (i + e < wc) {
            const unsigned b = (f >> (8 * e)) & 0xffu;
            dst[e] = (unsigned char)b;
            atomicAdd(&hist[b], 1u);
        }
}

// rows of the chunk -> Sub-filtered bytes in LDS + histogram.  VB: bytes per global load (16 / 4: Ws c and the slot pointer are multiples of it; 1: any)
template <int VB> __device__ __forceinline__ void png_load_rows(const uint8_t* src, long long rstride, int rows, int wc, int c, unsigned char* raw, int row,
                                                                unsigned* hist) {
    const int tid = threadIdx.x;
    if (VB == 1) {
        const int total = rows * row;
        for (int g = tid; g < total; g += PNG_THREADS) {
            const int r = g / row, i = g - r * row - 1;
            unsigned b = 1;                                           // the filter type byte
            if (i >= 0) {
                const uint8_t* p = src + (long long)r * rstride + i;
                b = ((unsigned)p[0] - (i >= c ? (unsigned)p[-c] : 0u)) & 0xffu;
            }
            raw[g] = (unsigned char)b;
            atomicAdd(&hist[b], 1u);
        }
        return;
    }
    const int gpr = (wc + VB - 1) / VB, total = rows * gpr;
    const unsigned sh = 32u - 8u * (unsigned)c;
    for (int g = tid; g < total; g += PNG_THREADS) {
        const int r = g / gpr, k = g - r * gpr;
        const uint8_t* p = src + (long long)r * rstride + (long long)k * VB;
        unsigned d[VB >= 4 ? VB / 4 : 1];
        if constexpr (VB == 16) {
            const png_u32x4 v = *reinterpret_cast<const png_u32x4*>(p);
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = v[j];
        } else {
            d[0] = *reinterpret_cast<const unsigned*>(p);
        }
        unsigned prev = k > 0 ? *reinterpret_cast<const unsigned*>(p - 4) : 0u;      // the pixel to the left of the group's first bytes (none: 0)
        unsigned char* dst = raw + r * row + 1 + k * VB;
        if (k == 0) {
            raw[r * row] = 1;
            atomicAdd(&hist[1], 1u);
        }
#pragma unroll
        for (int j = 0; j < VB / 4; ++j) {
            const unsigned cur = d[j];
            const unsigned left = (unsigned)(((((unsigned long long)cur) << 32) | prev) >> sh);
            const unsigned f = ((cur | 0x80808080u) - (left & 0x7f7f7f7fu)) ^ ((cur ^ ~left) & 0x80808080u);     // bytewise cur - left
            png_count4(hist, dst + 4 * j, f, k * VB + 4 * j, wc);
            prev = cur;
        }
    }
}

// (h, w) of image `img` and its chunk geometry; false: an empty slot or sizes that do not fit it
__device__ __forceinline__ bool png_image_geom(const PngParams& p, int img, int& h, int& w, int& row, int& R, int& nch) {
    h = p.sizes[2 * img];
    w = p.sizes[2 * img + 1];
    if (h < 1 || w < 1 || h > p.Hs || w > p.Ws) return false;
    row = 1 + w * p.c;
    R = p.chunk_bytes / row > 1 ? p.chunk_bytes / row : 1;
    nch = (h + R - 1) / R;
    return true;
}

template <int VB> __global__ __launch_bounds__(PNG_THREADS) void png_encode_kernel(PngParams p) {
    const int tid = threadIdx.x;
    const int img = blockIdx.x / p.max_chunks, chunk = blockIdx.x - img * p.max_chunks;
    int h, w, row, R, nch;
    if (!png_image_geom(p, img, h, w, row, R, nch) || chunk >= nch) return;
    const int y0 = chunk * R, rows = h - y0 < R ? h - y0 : R;
    const int N = rows * row;                                        // <= max_raw: R row <= chunk_bytes, or one row of at most 1 + Ws c bytes
    const int wc = w * p.c;
    const PngLds L = png_lds(p.max_raw);
    unsigned char* raw = reinterpret_cast<unsigned char*>(lama_smem + L.raw);
    unsigned* outw = reinterpret_cast<unsigned*>(lama_smem + L.out);
    unsigned* hist = reinterpret_cast<unsigned*>(lama_smem + L.hist);
    unsigned* lens = reinterpret_cast<unsigned*>(lama_smem + L.lens);
    unsigned* tab = reinterpret_cast<unsigned*>(lama_smem + L.tab);
    unsigned* weight = reinterpret_cast<unsigned*>(lama_smem + L.weight);
    unsigned short* parent = reinterpret_cast<unsigned short*>(lama_smem + L.parent);
    unsigned short* leafsym = reinterpret_cast<unsigned short*>(lama_smem + L.leafsym);
    unsigned* misc = reinterpret_cast<unsigned*>(lama_smem + L.misc);      // [0..3] [4..7] [8..11]: scan / reduction words; [16]: depth flag

    // ---- zero the histogram, the output words and the pad behind the raw bytes
    const int out_words = (N + 16 + 3) >> 2;
    for (int i = tid; i < out_words; i += PNG_THREADS) outw[i] = 0;
    for (int i = tid; i < 272; i += PNG_THREADS) hist[i] = 0;
    if (tid < 4) raw[(N & ~3) + tid] = 0;                                   // the last dword of the raw bytes is read whole
    __syncthreads();

    // ---- the chunk's rows, Sub-filtered, and their histogram
    const long long rstride = (long long)p.Ws * p.c;
    const uint8_t* src = p.image + ((long long)img * p.Hs + y0) * rstride;
    png_load_rows<VB>(src, rstride, rows, wc, p.c, raw, row, hist);
    if (tid == 0) hist[256] = 1;                                            // (nobody else touches it)
    __syncthreads();

    // ---- code lengths: rank, merge, depths; halve the counts and start over while a code is longer than 15 bits
    int n_used;
    for (;;) {
        // every thread: the rank of its symbol (thread 0: of 256 too) among the used ones by (count, symbol)
        const unsigned mine = hist[tid];
        unsigned rank = 0, rank256 = 0, used = 0;
        for (int u = 0; u < 256; ++u) {
            const unsigned cu = hist[u];
            used += cu ? 1u : 0u;
            rank += (cu && (cu < mine || (cu == mine && u < tid))) ? 1u : 0u;
            rank256 += cu == 1u ? 1u : 0u;                                  // 256 has count 1 and the largest index: behind every other count of 1
        }
        n_used = (int)used + 1;
        if (mine) {
            rank += mine > 1u ? 1u : 0u;                                    // symbol 256 (count 1) sorts in front of every larger count
            weight[rank] = mine;
            leafsym[rank] = (unsigned short)tid;
        }
        if (tid == 0) {
            weight[rank256] = 1u;
            leafsym[rank256] = 256;
            misc[16] = 0;
        }
        lens[tid] = 0;
        if (tid < 16) lens[256 + tid] = 0;
        __syncthreads();
        // the serial part: nodes 0 .. n-1 = leaves in sorted order, n .. 2n-2 = internal.  (merge_reps: 1; the profiling build's LAMA_PNG_MERGE_REPS
        // runs the merge that many times -- it is idempotent, so the bytes stay right and the time that is added is the merge's own)
        for (int rep = 0; tid == 0 && rep < p.merge_reps; ++rep) {
            const int n = n_used;
            int li = 0, ii = n;
            unsigned wl = weight[0], wi = 0;
            for (int k = n; k < 2 * n - 1; ++k) {
                unsigned sum = 0;
#pragma unroll
                for (int pick = 0; pick < 2; ++pick) {
                    if (li < n && (ii >= k || wl <= wi)) {
                        sum += wl;
                        parent[li] = (unsigned short)k;
                        ++li;
                        wl = li < n ? weight[li] : 0u;
                    } else {
                        sum += wi;
                        parent[ii] = (unsigned short)k;
                        ++ii;
                        if (ii < k) wi = weight[ii];
                    }
                }
                weight[k] = sum;
                if (ii == k) wi = sum;
            }
        }
        __syncthreads();
        // every thread: the depth of its leaf (thread 0: leaf 256 too), at most 16 steps up
        const int root = 2 * n_used - 2;
        for (int leaf = tid; leaf < n_used; leaf += PNG_THREADS) {
            int k = leaf, d = 0;
            while (k != root && d < 16) {
                k = parent[k];
                ++d;
            }
            if (k != root || d > 15) atomicOr(&misc[16], 1u);
            lens[leafsym[leaf]] = (unsigned)d;
        }
        __syncthreads();
        if (!misc[16]) break;
        if (mine) hist[tid] = (mine + 1u) >> 1;
        __syncthreads();
    }

    // ---- canonical codes (RFC 1951 3.2.2), bit-reversed: code = sum over shorter lengths b of count[b] << (l - b), + the smaller symbols of length l
    for (int s = tid; s < 257; s += PNG_THREADS) {
        const unsigned l = lens[s];
        unsigned code = 0;
        for (int u = 0; u < 257; ++u) {
            const unsigned lu = lens[u];
            if (lu && lu < l) code += 1u << (l - lu);
            if (lu == l && u < s) code += 1u;
        }
        tab[s] = l ? ((__builtin_bitreverse32(code) >> (32u - l)) | (l << 16)) : 0u;
    }
    __syncthreads();

    // ---- every thread: a contiguous run of `per` bytes (a multiple of 4): its bit count and its share of the Adler sums
    const int per = (((N + PNG_THREADS - 1) / PNG_THREADS) + 3) & ~3;
    const int i0 = tid * per;
    const unsigned* raw32 = reinterpret_cast<const unsigned*>(raw);
    unsigned bits = 0, s1 = 0;
    unsigned long long s2 = 0;
    for (int q = 0; q < per; q += 4) {
        const int i = i0 + q;
        if (i >= N) break;
        const unsigned v = raw32[i >> 2];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i + e < N) {
                const unsigned b = (v >> (8 * e)) & 0xffu;
                bits += tab[b] >> 16;
                s1 += b;
                s2 += (unsigned long long)(unsigned)(N - (i + e)) * b;       // Adler's B gains (N - i) b_i over the chunk
            }
    }
    unsigned total_bits, t1, t2;
    const unsigned my_bit = png_exscan(bits, misc, total_bits);
    png_exscan(s1 % PNG_ADLER, misc + 4, t1);
    png_exscan((unsigned)(s2 % PNG_ADLER), misc + 8, t2);
    const unsigned e256 = tab[256];
    const unsigned end_bits = PNG_HEADER_BITS + total_bits + (e256 >> 16) + 3u;
    const unsigned dyn_bytes = ((end_bits + 7u) >> 3) + 4u;
    const bool stored = dyn_bytes >= (unsigned)N + 5u;
    const unsigned nbytes = stored ? (unsigned)N + 5u : dyn_bytes;

    if (stored) {
        unsigned char* o8 = reinterpret_cast<unsigned char*>(outw);
        if (tid == 0) {
            o8[0] = 0;
            o8[1] = (unsigned char)(N & 255);
            o8[2] = (unsigned char)(N >> 8);
            o8[3] = (unsigned char)(~N & 255);
            o8[4] = (unsigned char)((~N >> 8) & 255);
        }
        for (int i = tid; i < N; i += PNG_THREADS) o8[5 + i] = raw[i];
    } else {
        // header: BFINAL 0, BTYPE 10, HLIT 0, HDIST 0, HCLEN 15; 19 x 3 bits (0 for 16 / 17 / 18, then sixteen 4s); 258 x 4 bits of code lengths
        if (tid == 0) atomicOr(&outw[0], 4u | (15u << 13));
        if (tid >= 3 && tid < 19) png_or_bits(outw, 17u + 3u * tid, 4u, 3);
        for (int s = tid; s < 257; s += PNG_THREADS) {
            const unsigned l = lens[s];
            if (l) png_or_bits(outw, 74u + 4u * s, __builtin_bitreverse32(l) >> 28, 4);
        }
        unsigned pos = PNG_HEADER_BITS + my_bit;
        unsigned wi = pos >> 5, fill = pos & 31;
        unsigned long long acc = 0;
        for (int q = 0; q < per; q += 4) {
            const int i = i0 + q;
            if (i >= N) break;
            const unsigned v = raw32[i >> 2];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < N) {
                    const unsigned t = tab[(v >> (8 * e)) & 0xffu];
                    acc |= (unsigned long long)(t & 0xffffu) << fill;
                    fill += t >> 16;
                    if (fill >= 32) {
                        atomicOr(&outw[wi], (unsigned)acc);
                        ++wi;
                        acc >>= 32;
                        fill -= 32;
                    }
                }
        }
        if (fill) atomicOr(&outw[wi], (unsigned)acc);
        if (tid == 0) {
            png_or_bits(outw, PNG_HEADER_BITS + total_bits, e256 & 0xffffu, e256 >> 16);      // symbol 256; the stored block's 000 are zeros already
            const unsigned b = (end_bits + 7u) >> 3;                                          // 00 00 FF FF behind the pad
            atomicOr(&outw[(b + 2) >> 2], 0xffu << (8 * ((b + 2) & 3)));
            atomicOr(&outw[(b + 3) >> 2], 0xffu << (8 * ((b + 3) & 3)));
        }
    }
    __syncthreads();

    // ---- the chunk's bytes to its workspace slot (16-byte aligned both sides; the slot holds raw + 16 bytes at least), and its record
    const long long ci = (long long)img * p.max_chunks + chunk;
    png_u32x4* dst = reinterpret_cast<png_u32x4*>(p.slots + (unsigned long long)ci * p.slot);
    const png_u32x4* so = reinterpret_cast<const png_u32x4*>(outw);
    const int nv = (int)((nbytes + 15u) >> 4);
    for (int i = tid; i < nv; i += PNG_THREADS) dst[i] = so[i];
    if (tid == 0) {
        png_u32x4 rec;
        rec[0] = nbytes;
        rec[1] = t1 % PNG_ADLER;
        rec[2] = t2 % PNG_ADLER;
        rec[3] = (unsigned)N;
        p.recs[ci] = rec;
    }
}

__global__ __launch_bounds__(PNG_THREADS) void png_assemble_kernel(PngParams p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int parts = (p.max_chunks + PNG_COPY_CHUNKS - 1) / PNG_COPY_CHUNKS;
    const int img = blockIdx.x / (parts + 1), part = blockIdx.x - img * (parts + 1);
    int h, w, row, R, nch;
    if (!png_image_geom(p, img, h, w, row, R, nch)) {
        if (part == parts && tid == 0) p.out_bytes[img] = 0;
        return;
    }
    unsigned* misc = reinterpret_cast<unsigned*>(lama_smem);               // the scan words
    uint8_t* out = p.out + (unsigned long long)img * p.out_stride;
    const png_u32x4* recs = p.recs + (long long)img * p.max_chunks;
    if (part < parts) {
        // ---- a copy workgroup: chunks c0 .. c0 + 3, a wave each, behind the bytes of every chunk in front of them
        const int c0 = part * PNG_COPY_CHUNKS;
        if (c0 >= nch) return;
        const unsigned* bytes_of = reinterpret_cast<const unsigned*>(recs);    // word 0 of each 4-word record
        unsigned mine = 0, before;
        for (int j = tid; j < c0; j += PNG_THREADS) mine += bytes_of[4 * j];
        png_exscan(mine, misc, before);
        const int cj = c0 + wave;
        if (cj >= nch) return;
        unsigned off = 2u + before;
        for (int k = c0; k < cj; ++k) off += bytes_of[4 * k];
        const unsigned len = bytes_of[4 * cj];
        uint8_t* d = out + off;
        const uint8_t* s = p.slots + (unsigned long long)((long long)img * p.max_chunks + cj) * p.slot;
        const unsigned head0 = (unsigned)((4u - ((unsigned)(unsigned long long)d & 3u)) & 3u);
        const unsigned head = head0 < len ? head0 : len;                  // single bytes up to the destination's first dword boundary
        if ((unsigned)lane < head) d[lane] = s[lane];
        const unsigned nd = (len - head) >> 2;                            // whole destination dwords
        const unsigned* sw = reinterpret_cast<const unsigned*>(s);
        unsigned* dw = reinterpret_cast<unsigned*>(d + head);
        const unsigned sh = 8u * (head & 3u), w0 = head >> 2;
        for (unsigned q = lane; q < nd; q += 64) {
            const unsigned lo = sw[w0 + q];
            unsigned v = lo;
            if (sh) v = (lo >> sh) | (sw[w0 + q + 1] << (32u - sh));      // (the next source dword is inside the slot: len + 8 <= raw + 16)
            dw[q] = v;
        }
        const unsigned tail0 = head + 4u * nd;
        if (tail0 + (unsigned)lane < len) d[tail0 + lane] = s[tail0 + lane];
        return;
    }
    // ---- the image's last workgroup: the total size, the Adler-32 over the chunks in order, header and trailer
    unsigned off_carry = 2, a_carry = 1, b_sum = 0;                         // bytes in front of the next chunk; Adler A in front of it; Adler B so far (uniform)
    for (int t0 = 0; t0 < nch; t0 += PNG_THREADS) {
        const int j = t0 + tid;
        png_u32x4 rec = {0u, 0u, 0u, 0u};
        if (j < nch) rec = recs[j];
        unsigned tot_bytes, tot_a, tot_b;
        png_exscan(rec[0], misc, tot_bytes);
        const unsigned a_before = (a_carry + png_exscan(rec[1], misc + 4, tot_a)) % PNG_ADLER;
        // B' = B + N A + s2 per chunk, A the value in front of it: N <= 65535, A < 65521, so the product fits 32 bits
        const unsigned term = ((rec[3] * a_before) % PNG_ADLER + rec[2]) % PNG_ADLER;
        png_exscan(term, misc + 8, tot_b);
        off_carry += tot_bytes;
        a_carry = (a_carry + tot_a) % PNG_ADLER;
        b_sum = (b_sum + tot_b) % PNG_ADLER;
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = 0x78;
        out[1] = 0x01;
        uint8_t* e = out + off_carry;
        e[0] = 1; e[1] = 0; e[2] = 0; e[3] = 0xff; e[4] = 0xff;
        e[5] = (uint8_t)(b_sum >> 8); e[6] = (uint8_t)b_sum; e[7] = (uint8_t)(a_carry >> 8); e[8] = (uint8_t)a_carry;
        p.out_bytes[img] = (int32_t)(off_carry + 9u);
    }
}

bool png_args_ok(int32_t channels, int32_t& chunk_bytes) {
    if (chunk_bytes == 0) chunk_bytes = PNG_DEFAULT_CHUNK;
    return (channels == 1 || channels == 3) && chunk_bytes >= PNG_MIN_CHUNK && chunk_bytes <= PNG_MAX_CHUNK;
}
}  // namespace

extern "C" size_t lama_png_deflate_bound(int32_t h, int32_t w, int32_t channels, int32_t chunk_bytes) {
    if (!png_args_ok(channels, chunk_bytes) || h <= 0 || w <= 0) return 0;
    const long long row = 1 + (long long)w * channels;
    const long long R = chunk_bytes / row > 1 ? chunk_bytes / row : 1;
    // every chunk in its stored form (the dynamic form is taken only where it is shorter) + 78 01 + the final block + the Adler-32
    return (size_t)((long long)h * row + 5 * ((h + R - 1) / R) + 11);
}

extern "C" int lama_png_deflate_workspace_bytes(int32_t batch, int32_t Hs, int32_t Ws, int32_t channels, int32_t chunk_bytes, size_t* bytes) {
    if (!bytes || batch <= 0 || Hs <= 0 || Ws <= 0 || !png_args_ok(channels, chunk_bytes)) return LAMA_ERR_BAD_ARG;
    if (1 + (long long)Ws * channels > PNG_MAX_RAW) return LAMA_ERR_UNSUPPORTED;
    const PngGeom g = png_geom(Hs, Ws, channels, chunk_bytes);
    *bytes = (size_t)batch * g.max_chunks * (g.slot + sizeof(png_u32x4));
    return LAMA_OK;
}

extern "C" int lama_png_deflate_u8_fwd(void* stream, const uint8_t* image_hwc, const int32_t* sizes, int32_t Hs, int32_t Ws, int32_t channels, int32_t batch,
                                       int32_t chunk_bytes, uint8_t* out, size_t out_stride, int32_t* out_bytes, void* workspace, size_t workspace_bytes) {
    if (!image_hwc || !sizes || !out || !out_bytes || !workspace || batch <= 0 || Hs <= 0 || Ws <= 0 || !png_args_ok(channels, chunk_bytes))
        return LAMA_ERR_BAD_ARG;
    if (1 + (long long)Ws * channels > PNG_MAX_RAW) return LAMA_ERR_UNSUPPORTED;           // a row is the least a chunk can hold, and LEN has 16 bits
    if (out_stride < lama_png_deflate_bound(Hs, Ws, channels, chunk_bytes)) return LAMA_ERR_BAD_ARG;
    if (((unsigned long long)workspace & 15) || ((unsigned long long)sizes & 3) || ((unsigned long long)out_bytes & 3)) return LAMA_ERR_BAD_ARG;
    const PngGeom g = png_geom(Hs, Ws, channels, chunk_bytes);
    const size_t n_slots = (size_t)batch * g.max_chunks;
    if (n_slots > 0x3fffffffull) return LAMA_ERR_UNSUPPORTED;                               // one grid dimension, in either launch
    if (workspace_bytes < n_slots * (g.slot + sizeof(png_u32x4))) return LAMA_ERR_WORKSPACE;
    PngParams p;
    p.image = image_hwc; p.sizes = sizes; p.out = out; p.out_bytes = out_bytes;
    p.recs = reinterpret_cast<png_u32x4*>(workspace);
    p.slots = reinterpret_cast<uint8_t*>(workspace) + n_slots * sizeof(png_u32x4);
    p.out_stride = out_stride; p.slot = g.slot;
    p.Hs = Hs; p.Ws = Ws; p.c = channels; p.chunk_bytes = chunk_bytes; p.max_chunks = g.max_chunks; p.max_raw = g.max_raw;
    p.merge_reps = lama_env_int("LAMA_PNG_MERGE_REPS", 1) > 1 ? lama_env_int("LAMA_PNG_MERGE_REPS", 1) : 1;
    const size_t lds = png_lds(g.max_raw).total;
    const dim3 grid((unsigned)n_slots), block(PNG_THREADS);
    const unsigned long long align = (unsigned long long)image_hwc | (unsigned long long)((long long)Ws * channels);
    if (!(align & 15)) hipLaunchKernelGGL(png_encode_kernel<16>, grid, block, lds, (hipStream_t)stream, p);
    else if (!(align & 3)) hipLaunchKernelGGL(png_encode_kernel<4>, grid, block, lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(png_encode_kernel<1>, grid, block, lds, (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    const size_t n_asm = (size_t)batch * (lama_ceil_div(g.max_chunks, PNG_COPY_CHUNKS) + 1);
    hipLaunchKernelGGL(png_assemble_kernel, dim3((unsigned)n_asm), block, 16 * sizeof(unsigned), (hipStream_t)stream, p);
    LAMA_CHECK_LAUNCH();
    return LAMA_OK;
}
