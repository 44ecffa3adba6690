/* lama_hip.h -- C ABI of liblama_hip.so: the MI355X (gfx950) kernels behind the LaMa FFC generator.
 *
 * The reference (advimman/lama) has no FFI: its hot path is Python calling PyTorch ops.  This header
 * is the boundary a maintainer binds instead (ctypes stub in INTEGRATION.md).  Each entry point
 * names the reference code whose arithmetic it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = LAMA_ERR_* (bad argument / unsupported shape),
 *     >0 = hipError_t of the failing runtime call.  Nothing throws, exits or synchronises the host.
 *   - all pointers are DEVICE pointers owned by the caller (inputs, outputs, packed weights and
 *     workspace).  The library allocates nothing and keeps no state; every launch is asynchronous on
 *     the given hipStream_t (passed as void*) and is hipGraph-capturable.  The library reads no environment variable
 *     (kernel-selection overrides, ablations and tracers exist only in the -DLAMA_PROFILING build used by tools/).
 *   - activations are fp32 NCHW "views": element (b,c,y,x) of a lama_tensor lives at
 *     ptr[b*batch_stride + (c*H + y)*W + x]; batch_stride lets a view address a channel slice of a
 *     wider buffer (the bottleneck state keeps x_l | x_g in one 512-channel buffer, which makes
 *     ConcatTupleLayer, ffc.py:295-302, free).
 */
#ifndef LAMA_HIP_H
#define LAMA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LAMA_HIP_VERSION 112

#define LAMA_OK 0
#define LAMA_ERR_BAD_ARG (-1)
#define LAMA_ERR_UNSUPPORTED (-2)
#define LAMA_ERR_WORKSPACE (-3)

/* activation applied in a conv epilogue */
#define LAMA_ACT_NONE 0
#define LAMA_ACT_RELU 1
#define LAMA_ACT_SIGMOID 2
#define LAMA_ACT_TANH 3

/* padding mode of a conv */
#define LAMA_PAD_ZERO 0
#define LAMA_PAD_REFLECT 1

/* arithmetic of the MFMA contraction */
#define LAMA_PREC_F32 0    /* v_mfma_f32_32x32x2_f32: exact fp32 (bitwise an fmaf chain)          */
#define LAMA_PREC_BF16X3 1 /* 3-term bf16 split (hi*hi + hi*lo + lo*hi) on v_mfma_f32_32x32x16_bf16: fp32 range  */
#define LAMA_PREC_F16X3 2  /* 3-term fp16 split on v_mfma_f32_32x32x16_f16: 22 mantissa bits, |x| <= 65504     */
#define LAMA_PREC_F16 3    /* BASELINE configs[2] "fp16": fp16 activations in HBM (lama_tensor.dtype = LAMA_DT_F16), fp16 weights (the hi
                            * part of the LAMA_PREC_F16X3 packing), ONE v_mfma_f32_32x32x16_f16 product per MAC, fp32 accumulation,
                            * fp32 epilogue (bias, activation, residual), fp16 store.  x, x2 share one element type, resid and y share
                            * one; fp32 -> fp16 (the stem) and fp16 -> fp32 (the head) are allowed.                                    */

/* element type of an activation tensor in HBM */
#define LAMA_DT_F32 0
#define LAMA_DT_F16 1 /* IEEE half: BASELINE configs[2] "fp16"; every tensor of a call is fp16 except where an entry says otherwise */
/* LAMA_DT_SPLIT16 (no new symbol, no version bump): the (hi, lo) 16-bit parts of the call's precision, stored in the order the MFMA
 * kernels stage them -- fp16 parts under LAMA_PREC_F16X3, bf16 parts under LAMA_PREC_BF16X3: hi = rne16(x), lo = rne16(x - hi), exactly
 * the values the kernels form from an fp32 tensor while they stage it.  FOUR bytes per logical element (batch_stride keeps counting
 * logical elements: a buffer sized for fp32 holds the tensor), C % 8 == 0, and per image
 *     [C / 8][hi | lo][H][W][8 halves]:  part p (0 = hi, 1 = lo) of element (c, y, x) is the 16-bit word at byte
 *     (((c / 8) * 2 + p) * H * W + y * W + x) * 16 + (c % 8) * 2  behind  (char*)ptr + b * batch_stride * 4.
 * The lo part is exactly zero (0x0000) for every element whose hi part is a zero or whose x - hi is zero.
 * Range contract: a CONSUMER of such a tensor does not watch the fp16 range (it never sees the fp32 value) -- whoever WRITES one does:
 * a kernel that stores a hi part >= 0x7c00 in magnitude (inf, or a NaN that came through) under LAMA_PREC_F16X3 ORs 1 into
 * *range_flag in the same launch; it watches what it stores and nothing else.
 * Accepted by lama_conv2d_fwd only, under the two split precisions: as y of the 7x7 stem kernel (cin <= 4, 40 .. 64 output channels,
 * reflect pad 3) and as x and / or y of the 3x3 stride-2 convolutions (pad 1), without resid; x2, resid and fuse1_y never have this
 * type.  Every other combination, and every other entry point, returns LAMA_ERR_UNSUPPORTED with nothing launched. */
#define LAMA_DT_SPLIT16 2

typedef struct lama_tensor {
    void* ptr;            /* device pointer to element (0,0,0,0) of the view; NULL = absent          */
    int64_t batch_stride; /* ELEMENTS between consecutive images                                     */
    int32_t C, H, W;
    int32_t dtype;        /* LAMA_DT_F32 (0), LAMA_DT_F16 or LAMA_DT_SPLIT16 (its own layout, above) */
} lama_tensor;

/* One fused convolution launch:
 *     y = act( conv(x, w) [+ conv1x1(x2, w2)] + bias ) [+ resid]
 * Replaces nn.Conv2d(padding_mode='reflect') + BatchNorm2d(eval) + ReLU (+ residual add) chains:
 *   - FFC.convl2l/convl2g/convg2l 3x3 reflect convs, ffc.py:188-196, 220-223
 *   - FFC_BN_ACT bn_l/bn_g + act, ffc.py:251-255 (BN scale folded into w at pack time, shift = bias)
 *   - SpectralTransform.conv1 / conv2 and FourierUnit.conv_layer 1x1 convs, ffc.py:57-59,128-140
 *   - FFCResnetBlock residual add, ffc.py:288 (resid)
 *   - stem 7x7 / stride-2 downsamples / ConvTranspose2d upsamples / 7x7 head + sigmoid,
 *     ffc.py:315-363 (transposed = 1 means ConvTranspose2d(k3,s2,p1,op1))
 * x2/w2: optional second operand contracted with a 1x1 kernel into the same accumulator
 *        (out_xg = convl2g(x_l) + convg2g.conv2(t), ffc.py:161,223 in one pass).
 */
typedef struct lama_conv2d_args {
    lama_tensor x;
    const void* w_packed; /* from lama_conv2d_pack_weight                                  */
    int32_t kh, kw, stride, pad, pad_mode, transposed;
    lama_tensor x2;
    const void* w2_packed;
    const float* bias; /* [Cout] or NULL                                                 */
    int32_t act;
    lama_tensor resid; /* added after the activation; ptr NULL = none                    */
    lama_tensor y;
    int32_t batch;
    int32_t precision; /* LAMA_PREC_*                                                    */
    /* Range watch of LAMA_PREC_F16X3 (ignored by the other precisions; NULL = off).  The fp16 split represents |x| <= 65504
     * only: a kernel that meets a larger activation (or a NaN) while splitting x / x2 ORs 1 into *range_flag (device
     * uint32, zeroed by the caller); its output is then garbage and the caller re-runs with LAMA_PREC_BF16X3 (fp32 exponent
     * range, 16 mantissa bits) or LAMA_PREC_F32.  The weights are range-checked by the host at pack time instead.
     * Precision of an UNFLAGGED result: per output within c (|x| (*) |w scale|), c = 2^-20 (F16X3: 22 bits of each operand, lo * lo dropped) /
     * 2^-14 (BF16X3), plus fp32 accumulation -- with one floor of the fp16 format: a packed (scale-folded) weight below 2^-3 has an fp16-SUBNORMAL
     * lo part (grid 2^-24), i.e. an absolute error of up to 2^-25 however small it is, so a tap adds up to 2^-25 |x|.  Trained, folded weights are
     * mostly below 2^-3, so this floor is the working precision of F16X3 weights: K taps of O(1) activations give at most K 2^-25 (1.4e-4 at
     * K = 4608, 2e-6 with random signs), inside the 2e-4 every accuracy test holds; it grows linearly with |x| (2e-3 per tap at 65504) and stays a
     * relative 2^-25 of the activation, below fp32's own rounding of it.  Asserted: tests/range_watch_util.py (bar_of). */
    uint32_t* range_flag;
    /* Optional fused second stage (NULL / ptr NULL = off): SpectralTransform.conv1 of the NEXT layer, ffc.py:128-133,145, i.e.
     *     fuse1_y = ReLU( W1 y + fuse1_bias ),  W1 [192, 384] 1x1,
     * computed in the epilogue of the launch that produces the 384-channel x_g state y (the global branch of an FFC layer:
     * 3x3 over x_l + fused 1x1 over x2, Cout = 384, fp32 tensors, LAMA_PREC_F16X3 / BF16X3, planes of at least one 128-pixel
     * tile per CU; anything else returns LAMA_ERR_UNSUPPORTED when fuse1_w is set -- the caller then launches conv1 itself).
     * fuse1_w = lama_conv2d_pack_weight of W1 (BatchNorm scale folded) whose INPUT channels were reordered with
     * lama_fuse1_channel_order (the accumulator layout of the producing kernel); fuse1_y [B,192,H,W] fp32. */
    const void* fuse1_w;
    const float* fuse1_bias;
    lama_tensor fuse1_y;
    /* LAMA_CONV_* bits.  LAMA_CONV_COOPERATIVE: another stream has work for this GPU while this launch runs (the spectral branch of the
     * same FFC layer): kernels that would fill every CU's register file (the local 3x3 conv: two waves per SIMD) take a geometry that
     * leaves room for the other stream's workgroups (one 4-wave workgroup per CU, taken when the launch has 224 ... 320 workgroups) -- a few
     * per cent slower alone, faster together.  Results equal the plain launch up to fp32 summation order. */
    int32_t flags;
} lama_conv2d_args;
#define LAMA_CONV_COOPERATIVE 1
/* (v109) bits 8..10: log2 of the number of SIBLING launches that run at the same time as this one -- the parts of a batch that the host runs as
 * parallel branches of one hipGraph (lama_amd: generator.split_batch).  A launch over 1 / 2^n of the batch then takes the kernel geometry the WHOLE
 * batch would take (one 12-wave workgroup per 128-pixel tile of the global branch, with the optional fused conv1; the all-of-K-in-one-wave spectral
 * GEMM; no split-K in the Winograd conv) instead of the geometry that lets a lone small launch fill the chip: n siblings fill it together.
 * Same results as the unflagged launch up to fp32 summation order -- and bit-identical to the launch over the whole batch. */
#define LAMA_CONV_SIBLINGS_SHIFT 8
#define LAMA_CONV_SIBLINGS_MASK (7 << LAMA_CONV_SIBLINGS_SHIFT)
#define LAMA_CONV_SIBLINGS_LOG2(flags) (((flags) & LAMA_CONV_SIBLINGS_MASK) >> LAMA_CONV_SIBLINGS_SHIFT)
/* (v108, lama_winograd_conv3x3_fwd only) launch the GEMM half only; the caller owes the output transform -- lama_winograd_out_fwd or
 * lama_rfft2_winograd_out_fwd with the SAME arguments and workspace -- before anything reads y */
#define LAMA_CONV_DEFER_OUT 2

/* order[k] = the input channel of conv1 that sits at packed K position k (0 <= k < 384) of lama_conv2d_args.fuse1_w */
void lama_fuse1_channel_order(int32_t* order);

int lama_version(void);
const char* lama_error_string(int code);

/* Packed-weight size in BYTES for a conv with the given geometry. */
int64_t lama_conv2d_packed_weight_bytes(int32_t cout, int32_t cin, int32_t kh, int32_t kw, int32_t stride,
                                        int32_t transposed, int32_t precision);
/* Repack reference-layout weights (Conv2d: [Cout,Cin,kh,kw]; ConvTranspose2d: [Cin,Cout,kh,kw], both
 * as stored in the checkpoint) into the kernel's K-major layout, multiplying
 * output channel o by scale[o] (folded BatchNorm gamma/sqrt(var+eps); NULL = 1). */
int lama_conv2d_pack_weight(void* stream, const float* w, const float* scale, int32_t cout, int32_t cin, int32_t kh,
                            int32_t kw, int32_t stride, int32_t transposed, int32_t precision, void* dst);
int lama_conv2d_fwd(void* stream, const lama_conv2d_args* args);

/* Winograd F(2x2, 3x3) form of a 3x3 / stride 1 / reflect-pad 1 convolution: the SAME function as lama_conv2d_fwd on such a layer
 * (FFC.convl2l + convg2l over the 512-channel bottleneck state -> the 128 local output channels, ffc.py:188-196,220, with the folded
 * BatchNorm + ReLU of FFC_BN_ACT, ffc.py:251-255, and the FFCResnetBlock residual, ffc.py:288), computed with 16 instead of 36
 * multiplies per 2 x 2 output tile and (output, input) channel pair -- the launch is bound by the power the matrix cores draw, so
 * fewer MFMA products is what shortens it.  Split precisions only (LAMA_PREC_F16X3 / BF16X3; the 3-term split is applied to the
 * transformed operands: 1.2e-5 max-abs end to end with every such conv of the generator in this form); fp32 tensors; Cin % 32 == 0,
 * Cout % 128 == 0, H >= 4, W >= 8 (v110: any plane size -- tile rows are cut into overlapping segments of 8 / 16 / 32 column quads and the
 * columns behind W - 1 inside the last quad are reflected in registers; W in {32, 64, 128, 256} with H a multiple of 512 / W keep the exact
 * geometry of v107).  Anything else: LAMA_ERR_UNSUPPORTED (use lama_conv2d_fwd).
 *   lama_winograd_pack_weight: Conv2d weights [Cout, Cin, 3, 3] -> U = G g G^T per channel pair, BatchNorm scale folded, (hi, lo)
 *     split, MFMA A-fragment order; lama_winograd_packed_weight_bytes bytes.
 *   lama_winograd_conv3x3_fwd: args as lama_conv2d_fwd (x, w_packed, bias, act, resid, y, batch, precision, range_flag; kh = kw = 3,
 *     stride = 1, pad = 1, pad_mode = LAMA_PAD_REFLECT, or (v108) LAMA_PAD_ZERO: the dgrad convs of the reverse pass); workspace = lama_winograd_workspace_bytes device bytes (the half-inverted
 *     transform-domain sums between its two launches).  The exact geometries want x, y, resid as 16-byte aligned pointers with batch strides
 *     that are multiples of 4 elements (else LAMA_ERR_UNSUPPORTED); the any-size geometry needs element alignment only.
 *   lama_winograd_supported: 1 when lama_winograd_conv3x3_fwd takes this (cout, cin, H, W, precision) -- every bound of the launch,
 *     including the 32-bit byte offsets inside one image (cin * H * W * 4 < 2^31), which the workspace query alone does not see.
 *   lama_winograd_preferred (v110): 1 when this form is expected to beat lama_conv2d_fwd for (batch, cout, cin, H, W) -- always for the exact
 *     geometries; for the any-size geometry a cost model of whole rounds of workgroups (one per CU) against the direct kernel's: a launch of a
 *     little more than 256 units takes two rounds and loses (1 x 135 x 240), one of a little less wins (1 x 168 x 168: 65 against 92 us).
 *   range_flag (LAMA_PREC_F16X3): NOT the same watch as lama_conv2d_fwd's.  It is kept on the row sums r of the input transform
 *     (|V| <= 2 max|r|) and is raised at 2 max|r| >= 65504, i.e. up to 2x EARLY against a real overflow of a transformed operand, and it
 *     is BLIND TO NaN inputs (fmaxf drops them).  Inside the generator the global-branch launch (lama_conv2d_fwd) reads the same state
 *     buffer in the same layer and raises the flag for NaN / |x| > 65504; a stand-alone caller that needs NaN detection must run its own
 *     check (or lama_conv2d_fwd) on x.
 *   Precision: the split is applied to the TRANSFORMED operands U = G g G^T scale and V = B^T d B, so the rounding error of a result is relative
 *     to |A^T| (sum_c |U| |V|) |A|, not to |x| (*) |w scale| as in lama_conv2d_fwd: one large element reaches up to nine entries of V and meets all
 *     nine taps through U, so an output whose own tap is small carries its neighbours' rounding.  With one or a few large elements among O(1)
 *     data single outputs pass c (|x| (*) |w scale|): F16X3, unflagged, two elements of +-1.6e4 in a tile: up to 1.23x; BF16X3 (16 bits, no watch), one
 *     element of 3e4 / 7e4: up to 2x / 21x -- and stay below 0.25x / 0.1x of c |A^T| (sum |U| |V|) |A|, the bound that holds.  Safe inside the generator:
 *     the error stays a relative 2^-20 / 2^-14 of the LARGE activation of the tile, and the layer's outputs feed a BatchNorm-folded
 *     ReLU of the same scale.  Asserted: tests/range_watch_util.py (check_winograd). */
int64_t lama_winograd_packed_weight_bytes(int32_t cout, int32_t cin, int32_t precision);
int32_t lama_winograd_supported(int32_t cout, int32_t cin, int32_t H, int32_t W, int32_t precision);
int32_t lama_winograd_preferred(int32_t batch, int32_t cout, int32_t cin, int32_t H, int32_t W, int32_t precision);
int lama_winograd_pack_weight(void* stream, const float* w, const float* scale, int32_t cout, int32_t cin, int32_t precision, void* dst);
size_t lama_winograd_workspace_bytes(int32_t batch, int32_t cout, int32_t H, int32_t W);
int lama_winograd_conv3x3_fwd(void* stream, const lama_conv2d_args* args, void* workspace, size_t workspace_bytes);
/* (v108) the second launch of lama_winograd_conv3x3_fwd on its own (after a call with LAMA_CONV_DEFER_OUT), and the same work inside the
 * rfft2 launch of the NEXT FFC layer (ffc.py:86 of layer l + 1 with ffc.py:220,251-255,288 of layer l): both are memory-bound and independent, and
 * the FFT workgroups leave the HBM idle while they transform.  64 x 64 fp32 planes only (LAMA_ERR_UNSUPPORTED otherwise, nothing launched). */
/* lama_fourier_unit_winograd_out_fwd: lama_fourier_unit_fwd whose first launch is lama_rfft2_winograd_out_fwd (or, where that is unsupported,
 * lama_winograd_out_fwd followed by the plain FourierUnit): what the host mirror calls for layer l + 1 when layer l deferred its transform. */
int lama_winograd_out_fwd(void* stream, const lama_conv2d_args* args, void* workspace, size_t workspace_bytes);
int lama_rfft2_winograd_out_fwd(void* stream, const lama_tensor* x, const lama_tensor* spec, int32_t batch, void* workspace, size_t workspace_bytes,
                                const lama_conv2d_args* wino_args, void* wino_workspace, size_t wino_workspace_bytes);
int lama_fourier_unit_winograd_out_fwd(void* stream, const lama_tensor* x, const void* w_packed, const float* bias, const lama_tensor* y,
                                       int32_t batch, int32_t add_input, int32_t precision, void* workspace, size_t workspace_bytes,
                                       uint32_t* range_flag, const lama_conv2d_args* wino_args, void* wino_workspace,
                                       size_t wino_workspace_bytes);

/* (v112) Multi-dilated 3x3 reflect convolution in ONE launch:
 *     y = act( sum_{j < groups} conv3x3(reflect_pad(x[:, j*Cin/groups : (j+1)*Cin/groups], d_j), w_j, dilation = d_j) + bias ) [+ resid],
 *     d_j = min_dilation * 2^j.
 * Replaces MultidilatedConv(comb_mode='cat_in', equal_dim=True), multidilated_conv.py:36-63,73-98 (the G dilated nn.Conv2d over the channel
 * chunks of x and their sum), with the BatchNorm2d(eval) + ReLU behind it and the residual add of MultidilatedResnetBlock, pix2pixhd.py:155-175,
 * in the epilogue -- four separate launches cannot do that: the ReLU would fall between partial sums.
 *   args: read as for lama_conv2d_fwd with kh = kw = 3, stride = 1, pad_mode = LAMA_PAD_REFLECT (pad is implied: d_j per group), no x2, no
 *     fuse1_*, fp32 tensors; anything else returns LAMA_ERR_UNSUPPORTED.  w_packed = lama_conv2d_pack_weight (stride 1) of the group weights
 *     concatenated along Cin to [Cout, Cin, 3, 3]; bias = the sum of the group biases (folded with the BatchNorm).  resid may alias y.
 *   groups in {1, 2, 4}, (Cin / groups) % 16 == 0, Cout % 32 == 0, min_dilation * 2^(groups-1) <= 8 on the split precisions.
 *   Planes with H <= d_max or W <= d_max have no reflect padding (the reference raises there): LAMA_ERR_UNSUPPORTED.
 *   precision: LAMA_PREC_F16X3 / BF16X3 (3-term split on v_mfma_f32_32x32x16_*; range_flag as lama_conv2d_fwd) or LAMA_PREC_F32 (an exact fmaf
 *     chain per output, slow: the path errors are localised with). */
int lama_multidilated_conv3x3_fwd(void* stream, const lama_conv2d_args* args, int32_t groups, int32_t min_dilation);

/* torch.fft.rfftn(x, dim=(-2,-1), norm='ortho') followed by the Re/Im channel interleave
 * (ffc.py:86-89): x [B,C,h,w] -> spec [B,2C,h,w/2+1], channel 2c = Re, 2c+1 = Im. */
int lama_rfft2_fwd(void* stream, const lama_tensor* x, const lama_tensor* spec, int32_t batch, void* workspace,
                   size_t workspace_bytes);
/* de-interleave + torch.fft.irfftn(s=(h,w), dim=(-2,-1), norm='ortho') on a NON-Hermitian spectrum
 * (ffc.py:103-108; complex inverse along h, then c2r along w ignoring Im of bins 0 and w/2), fused
 * with the `x + fu(x)` add of SpectralTransform.forward (ffc.py:161): y = resid + irfft2(spec).
 * resid may be absent.  y [B,C,h,w]. */
int lama_irfft2_fwd(void* stream, const lama_tensor* spec, const lama_tensor* resid, const lama_tensor* y,
                    int32_t batch, void* workspace, size_t workspace_bytes);
/* (v108) the same transforms with the ReLU derivative that follows them in the reverse pass of the FourierUnit (refinement.py:163 through
 * ffc.py:101 and ffc.py:131): out = transform(...) * [mask_y > 0], mask_y laid out like the output (spec for the forward transform, y for the
 * inverse one).  Only where the compile-time two-pass kernels run (fp32 planes of 256 x 256, 16-byte aligned views): LAMA_ERR_UNSUPPORTED
 * otherwise, with nothing launched -- the caller then runs the plain transform + lama_act_bwd. */
int lama_rfft2_masked_fwd(void* stream, const lama_tensor* x, const lama_tensor* spec, const lama_tensor* mask_y, int32_t batch,
                          void* workspace, size_t workspace_bytes);
int lama_irfft2_masked_fwd(void* stream, const lama_tensor* spec, const lama_tensor* resid, const lama_tensor* mask_y, const lama_tensor* y,
                           int32_t batch, void* workspace, size_t workspace_bytes);
/* scratch bytes lama_rfft2_fwd / lama_irfft2_fwd / lama_fourier_unit_fwd need for [B,C,h,w] */
size_t lama_fft_workspace_bytes(int32_t batch, int32_t C, int32_t h, int32_t w);
/* (added to v112 without a version bump: one new symbol, nothing else changes) Which kernels would serve a transform, asked on the host:
 * returns exactly the code lama_rfft2_fwd (inverse == 0: `real` is x, `resid` is ignored) / lama_irfft2_fwd (inverse != 0: `real` is y, `resid` may
 * be NULL) -- or, with mask != NULL, lama_rfft2_masked_fwd / lama_irfft2_masked_fwd -- return for the same views, batch and workspace.  Nothing is
 * launched and no tensor or workspace pointer is dereferenced: only their addresses (alignment) are looked at.  On LAMA_OK *family is the kernel
 * family, 1 .. 6 (1 plane in LDS, power of two; 2 one-launch mixed radix; 3 compile-time 256 x 256 pair; 4 two-pass power of two; 5 two-launch
 * mixed radix; 6 separable DFT), and *kind the kernel inside family 1 (LAMA_FFT_KIND_*), the threads per workgroup (256 / 1024) for family 2, and
 * 0 otherwise.  A plane is served only where BOTH directions have a kernel for it: the two directions of one set of views report the same code and
 * family.  LAMA_ERR_BAD_ARG also for family == NULL or kind == NULL.  lama_rfft2_winograd_out_fwd is not covered. */
#define LAMA_FFT_KIND_WINO64 0  /* one-buffer 64 x 64 with the Winograd output transform (lama_rfft2_winograd_out_fwd only: never reported) */
#define LAMA_FFT_KIND_IP64 1    /* one-buffer 64 x 64 */
#define LAMA_FFT_KIND_IP128 2   /* one-buffer 128 x 128 */
#define LAMA_FFT_KIND_TRACE64 3 /* profiling build only */
#define LAMA_FFT_KIND_SEQ 4     /* profiling build only */
#define LAMA_FFT_KIND_SIZED 5   /* two-buffer, compile-time 32 / 64 / 128 squares */
#define LAMA_FFT_KIND_GENERIC 6 /* two-buffer, any power-of-two plane of 16 .. 128 */
int lama_fft_route_query(const lama_tensor* real, const lama_tensor* resid, const lama_tensor* spec, const lama_tensor* mask, int32_t batch,
                         int32_t inverse, const void* workspace, size_t workspace_bytes, int32_t* family, int32_t* kind);

/* FourierUnit.forward (ffc.py:76-113) in one call: y = [x +] irfft2( relu( W' rfft2(x) + b ) ).
 * w_packed = lama_conv2d_pack_weight(conv_layer.weight [2C,2C,1,1], bn scale); bias = bn shift.
 * workspace >= lama_fourier_unit_workspace_bytes. add_input != 0 fuses SpectralTransform's x + fu(x).
 * range_flag: as in lama_conv2d_args (the spectrum's DC bin grows with sqrt(h*w): the first tensor to leave the fp16 range). */
size_t lama_fourier_unit_workspace_bytes(int32_t batch, int32_t C, int32_t h, int32_t w);
int lama_fourier_unit_fwd(void* stream, const lama_tensor* x, const void* w_packed, const float* bias,
                          const lama_tensor* y, int32_t batch, int32_t add_input, int32_t precision, void* workspace,
                          size_t workspace_bytes, uint32_t* range_flag);
/* (v109) the superset of lama_fourier_unit_fwd and lama_fourier_unit_winograd_out_fwd (wino_args NULL = no deferred output transform) with the
 * LAMA_CONV_* flags of its spectral 1x1 launch (ffc.py:100-101) -- LAMA_CONV_SIBLINGS_* when the FourierUnit runs on a part of the batch beside
 * its siblings. */
int lama_fourier_unit_ex_fwd(void* stream, const lama_tensor* x, const void* w_packed, const float* bias, const lama_tensor* y,
                             int32_t batch, int32_t add_input, int32_t precision, void* workspace, size_t workspace_bytes,
                             uint32_t* range_flag, int32_t flags, const lama_conv2d_args* wino_args, void* wino_workspace,
                             size_t wino_workspace_bytes);

/* masked_img = cat(img*(1-mask), mask), trainers/default.py:59,67-68.  img [B,3,H,W], mask [B,1,H,W] -> out [B,4,H,W] */
int lama_mask_compose_fwd(void* stream, const lama_tensor* image, const lama_tensor* mask, const lama_tensor* out,
                          int32_t batch);
/* inpainted = mask*pred + (1-mask)*img, trainers/default.py:71 */
int lama_blend_fwd(void* stream, const lama_tensor* image, const lama_tensor* mask, const lama_tensor* pred,
                   const lama_tensor* out, int32_t batch);
/* np.clip(x*255, 0, 255).astype(uint8) of the HWC-permuted, cropped result, bin/predict.py:86-92.
 * src [B,3,H,W] fp32 -> dst u8 [B, crop_h, crop_w, 3] (RGB). */
int lama_quantize_u8_hwc_fwd(void* stream, const lama_tensor* src, uint8_t* dst, int32_t batch, int32_t crop_h,
                             int32_t crop_w);

/* (v110) The two ends of the predict step on what is on DISK: u8 HWC image [B][Hp][Wp][3] + u8 mask [B][Hp][Wp] (device pointers), each image's
 * valid h x w region in the top-left corner of its slot, sizes = int32 [B][2] (h, w) on the device (NULL: every image fills its slot; h = 0: an
 * empty slot of a partial batch -> zeros).  The kernels do what the reference's host code does per image:
 *   image.astype('float32') / 255 (evaluation/data.py:12-20: the same IEEE fp32 division), symmetric padding bottom / right up to (Hp, Wp)
 *   (data.py:29-33, np.pad mode='symmetric': row h + i = row h - 1 - i), mask > 0 (bin/predict.py:84; binarize == 0: mask / 255),
 * so a step uploads 4 bytes per pixel instead of 16 and the host neither converts nor pads.
 *   lama_mask_compose_u8_fwd:   out [B,4,Hp,Wp] fp32 = cat(img * (1 - mask), mask)                      (trainers/default.py:59,67-68)
 *   lama_blend_quantize_u8_fwd: dst u8 [B][Hp][Wp][3] = clip((mask * pred + (1 - mask) * img) * 255, 0, 255) truncated   (default.py:71 + bin/predict.py:86-92)
 * Bit-identical to lama_mask_compose_fwd / lama_blend_fwd + lama_quantize_u8_hwc_fwd on the fp32 tensors the host would have built. */
int lama_mask_compose_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* sizes, const lama_tensor* out,
                             int32_t batch, int32_t binarize);
int lama_blend_quantize_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* sizes, const lama_tensor* pred,
                               uint8_t* dst_hwc, int32_t batch, int32_t binarize);

/* (added to v112 without a version bump: one new symbol, nothing else changes) dataset.scale_factor inside the u8 predict step: the loader's whole
 * chain for a batch of DECODED images in one launch, so that a scaled run uploads 4 bytes per SOURCE pixel and the host only decodes.
 *   image_hwc u8 [B][Hs][Ws][3] + mask u8 [B][Hs][Ws] (device pointers): source slots, each image's own h x w pixels in the top-left corner;
 *   src_sizes int32 [B][2] = (h, w) on the device (h = 0: an empty slot of a partial batch -> zeros);
 *   dst_sizes int32 [B][2] = the size cv::resize(dsize=None, fx, fy) gives that image, saturate_cast<int>(size * factor) (round half to even),
 *     computed by the host;  factor = dataset.scale_factor.
 * Per image the kernel does what InpaintingDataset.__getitem__ does on the host:
 *   image.astype('float32') / 255 (evaluation/data.py:12-20: the same IEEE fp32 division as lama_mask_compose_u8_fwd),
 *   scale_image = cv2.resize(fx = fy = factor) with INTER_AREA on the image and INTER_NEAREST on the mask (data.py:42-55,74-77) -- the three
 *     regimes of INTER_AREA (integer shrink: resizeAreaFast's sums of four and its border loop; fractional shrink: computeResizeAreaTab's taps,
 *     x pass then y pass; enlarging: the linear path with area coefficients), tap indices and weights computed in fp64 from the destination
 *     index, 1.0 / factor and the image's own size and rounded to fp32 where OpenCV rounds them,
 *   pad_img_to_modulo's symmetric padding of the SCALED dh x dw result up to (Hp, Wp) = the views' H x W (data.py:29-33; np.pad mode='symmetric'
 *     is periodic: the padding may exceed the scaled side),
 *   mask > 0 (bin/predict.py:84; binarize == 0: the mask stays mask / 255).
 * out_image [B,3,Hp,Wp], out_mask [B,1,Hp,Wp] fp32: what lama_mask_compose_fwd / lama_blend_fwd take.  Bit-identical to lama_amd.predict's
 * host restatement of resize.cpp (scale_image + pad_img_to_modulo): no floating-point contraction anywhere in the kernel.
 * LAMA_ERR_BAD_ARG: a null pointer, factor <= 0 (or not finite), views that are not [.,3,Hp,Wp] / [.,1,Hp,Wp] of one size; LAMA_ERR_UNSUPPORTED:
 * views that are not fp32.  The per-image sizes live on the device, where the host cannot read them without a synchronisation: an image whose
 * source size exceeds its slot or whose destination size exceeds the output view is written as zeros, like an empty slot -- nothing is read or
 * written out of bounds (lama_amd.predict.HostFedStep.put refuses such an image on the host, where the sizes are known). */
int lama_resize_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes, const int32_t* dst_sizes, int32_t Hs,
                       int32_t Ws, double factor, const lama_tensor* out_image, const lama_tensor* out_mask, int32_t batch, int32_t binarize);

/* (added to v112 without a version bump: one new symbol, nothing else changes) The evaluator's loader on what is on DISK: a batch of decoded
 * (ground truth, prediction, mask) triples in one launch, so that scoring uploads 7 bytes per pixel instead of 28 and the host only decodes.
 *   image_hwc, pred_hwc u8 [B][Hs][Ws][3], mask u8 [B][Hs][Ws] (device pointers): slots, each image's own h x w pixels in the top-left corner;
 *   sizes: HOST array int32 [B][2] = (h, w), or NULL: every image fills its slot.  It is read during the call (the checks below need it) and
 *     rides in the kernel's argument block: the launch stays asynchronous and capturable, 64 images per launch (a larger batch is more launches);
 *   pad_mod: dataset_kwargs.pad_out_to_modulo (1 = no padding); out_image, out_pred: [B,3,Hp,Wp] fp32 with Hp = ceil_modulo(h, pad_mod),
 *     Wp = ceil_modulo(w, pad_mod) (evaluation/data.py:23-26) for EVERY image of the call.
 * Per image the kernel does what PrecomputedInpaintingResultsDataset.__getitem__ and InpaintingEvaluator.evaluate do on the host:
 *   out = u8.astype('float32') / 255 of both images (data.py:12-20: the same IEEE fp32 division as lama_mask_compose_u8_fwd), pad_img_to_modulo's
 *   symmetric padding bottom / right (data.py:29-33: row h + i = row h - 1 - i), torch.clamp(image, clamp_lo, clamp_hi) of the ground truth ONLY
 *   and only when clamp != 0 (evaluator.py:87-90: clamp_image_range; the prediction is never clamped).
 *   mask_sum[b] (device int64 [B]) = the exact sum of the u8 mask values over the symmetric-padded Hp x Wp mask plane of image b: integer adds
 *   in a fixed order, no atomics, nothing to zero.  The evaluator needs the mask only as its mean (evaluator.py:58,164), which the host forms as
 *   mask_sum / (255 Hp Wp) in fp64; no float mask plane is written.
 * Bit-identical to the host chain.  Any Hs, Ws, Hp, Wp >= 1 (dword loads where Ws % 4 == 0, float4 stores where Wp % 4 == 0 and the views are
 * 16-byte aligned with batch strides that are multiples of 4; element accesses otherwise).
 * LAMA_ERR_BAD_ARG: a null pointer, batch / Hs / Ws / pad_mod <= 0, views that are not two [.,3,Hp,Wp] of one size, outputs that are not
 *   4-byte aligned or a mask_sum that is not 8-byte aligned, clamp_lo > clamp_hi, an image with h or w outside 1 .. Hs / Ws, an image whose
 *   padded size is not (Hp, Wp) (one padded size per call);
 * LAMA_ERR_UNSUPPORTED: views that are not fp32; an image whose padding exceeds its own extent (Hp > 2 h or Wp > 2 w: np.pad's periodic
 *   mirror, which lama_mask_compose_u8_fwd serves and this entry does not).  Nothing is launched on an error. */
int lama_eval_ingest_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* pred_hwc, const uint8_t* mask, const int32_t* sizes, int32_t Hs,
                            int32_t Ws, int32_t pad_mod, int32_t clamp, float clamp_lo, float clamp_hi, const lama_tensor* out_image,
                            const lama_tensor* out_pred, int64_t* mask_sum, int32_t batch);

/* ---- (added to v112 without a version bump: new symbols only, nothing else changes) the sparse tail of the predict step ------------------------
 * The predict step keeps inpainted = mask * pred + (1 - mask) * image (trainers/default.py:71; bin/predict.py writes nothing else): wherever the mask
 * is 0 the generator's output is multiplied by zero.  The bottleneck sees every pixel through its FFTs; the ConvTranspose2d upsamplings and the 7x7
 * head behind it (ffc.py:348-363) have receptive fields of 1 and 3 pixels, so their persistent kernels can walk only the work units the output needs.
 *
 * lama_tail_lists_build: two launches, no host synchronisation, hipGraph-capturable.  mask = the [batch, 1, H, W] fp32 view of channel 3 of the
 *   generator's input (what lama_mask_compose_fwd / lama_mask_compose_u8_fwd wrote there); a pixel is needed where it is not 0.  Units:
 *     head   segment g = part * (batch * ceil(W / 26)) + b * ceil(W / 26) + column: rows part * head_rs .., 26 columns (head_rs: a multiple of 8);
 *     up[i]  (i = 0 feeds the head, i = 1 feeds up[0], ...; input plane H / 2^(i+1) x W / 2^(i+1), H and W divisible by 2^n_up): tile
 *            t = ((b * ceil(h / 4) + ty) * ceil(w / 32) + tx) * up_mg[i] + mg: 4 x 32 input pixels (8 x 64 output pixels) x 64 output channels.
 *   A head segment is listed iff a needed pixel lies in its rectangle; an up[0] tile iff its output rectangle meets the rectangle of a listed head
 *   segment grown by 3 and clamped to the plane; an up[i] tile iff its output rectangle meets the 5 x 33 input patch (clamped to the plane) of a
 *   listed up[i - 1] tile -- closure at the granularity of what is COMPUTED.  The list variants keep every load inside those rectangles, the lanes
 *   and rows of ragged last segments / parts / tiles that feed no stored pixel included (the head clamps them into its grown rectangle; the
 *   transposed conv reads zeros beyond the plane), so no listed unit reads -- or range-watches -- a pixel that this step did not write.  Every list
 *   is in ascending order (a prefix sum, no atomic append) and bit-identical run to run; *_count is one int32; *_list has room for every unit of its
 *   launch.  workspace: lama_tail_lists_workspace_bytes() bytes (0: bad geometry), 4-byte aligned.
 * lama_conv2d_list_fwd: lama_conv2d_fwd of a ConvTranspose2d(k3,s2,p1,op1) or of the 7x7 reflect head over such a list: the same grid, every
 *   workgroup walks list[0 .. *count) instead of every unit; units that are not listed are NOT written.  Only where the dedicated persistent kernels
 *   run (LAMA_PREC_F16X3 / BF16X3, fp32 tensors, the shapes they take); anything else returns LAMA_ERR_UNSUPPORTED with nothing launched and the caller
 *   runs lama_conv2d_fwd -- a superset.  head_rs: rows per head segment (as given to lama_tail_lists_build; ignored by the transposed conv).
 * lama_conv2d_list_supported: 1 when lama_conv2d_list_fwd takes these arguments (every check, no launch: lama_conv2d_route_query with a list).
 * lama_blend_quantize_u8_fwd does not read pred where the mask is 0. */
typedef struct lama_tail_lists {
    int32_t n_up;    /* ConvTranspose2d launches listed, 0 .. 4 */
    int32_t head_rs; /* rows per head segment, a multiple of 8 */
    int32_t up_mg[4]; /* Cout / 64 of up[i] */
    int32_t* head_list;
    int32_t* head_count;
    int32_t* up_list[4];
    int32_t* up_count[4];
} lama_tail_lists;
size_t lama_tail_lists_workspace_bytes(int32_t batch, int32_t H, int32_t W, const lama_tail_lists* lists);
int lama_tail_lists_build(void* stream, const lama_tensor* mask, int32_t batch, const lama_tail_lists* lists, void* workspace, size_t workspace_bytes);
int lama_conv2d_list_fwd(void* stream, const lama_conv2d_args* args, const int32_t* list, const int32_t* count, int32_t head_rs);
int32_t lama_conv2d_list_supported(const lama_conv2d_args* args, int32_t head_rs);

/* (added to v112 without a version bump: one new symbol, nothing else changes) Which kernel family would serve a convolution, asked on the host:
 * returns exactly the code lama_conv2d_fwd (head_rs < 0) or lama_conv2d_list_fwd with this head_rs (head_rs >= 0) returns for the same arguments,
 * after the same validation.  Nothing is launched and no tensor, weight or list pointer is dereferenced: only the addresses of the views are
 * looked at (alignment).  On LAMA_OK *family is LAMA_CONV_FAMILY_* and *geometry packs what distinguishes the instantiations inside the family:
 *   F32        the exact fmaf-chain path of LAMA_PREC_F32: the M tile (32 / 64 / 128)
 *   GEMM1X1_WK bit 0: left-over super-tiles go to the fifth waves
 *   GEMM1X1_W4 bits 4-7: 64-channel chunks of K (3 / 6); bit 8: residual
 *   GEMM1X1_WS bits 0-3: NH (1: 32-pixel tiles, 2: 64-pixel tiles); bits 4-7: 64-channel chunks of K; bit 8: residual
 *   CONV_WR    bits 0-3: M-waves WMV; 4-7: K-groups KG; 8-11: 16-channel sub-chunks per chunk KSC1; 12-15: log2 of the tile width; bit 16: stride 2;
 *              17: the cooperative one-workgroup-per-CU geometry; 18: row-rolling fragment reads; 19: fused conv1 (fuse1_w); 20 / 21: x / y is
 *              LAMA_DT_SPLIT16 (LAMA_CONV_GEO_WR packs them)
 *   CONVT2, HEAD7  bit 0: over a work list
 *   STEM7      bit 21: y is LAMA_DT_SPLIT16
 *   LDS        bits 0-7: M tile BM; 8-19: pixel tile BN; 20-21: folded 7x7 mode (1 stem, 2 head); bit 22: ConvTranspose2d's fused tap list
 * lama_conv2d_list_supported is this query with a list (1 where it returns LAMA_OK).  LAMA_ERR_BAD_ARG also for family == NULL or geometry == NULL.
 * The Winograd and multi-dilated entries are not covered. */
#define LAMA_CONV_FAMILY_F32 0        /* conv_mfma_f32_kernel (LAMA_PREC_F32) */
#define LAMA_CONV_FAMILY_GEMM1X1_WK 1 /* the spectral GEMM with all of K in one wave */
#define LAMA_CONV_FAMILY_GEMM1X1_W4 2 /* pointwise GEMM over 64-pixel super-tiles */
#define LAMA_CONV_FAMILY_GEMM1X1_WS 3 /* weights-stationary persistent pointwise GEMM */
#define LAMA_CONV_FAMILY_CONV_WR 4    /* weights-in-registers 3x3 / 1x1 */
#define LAMA_CONV_FAMILY_CONVT2 5     /* ConvTranspose2d as one launch */
#define LAMA_CONV_FAMILY_STEM7 6      /* 7x7 stem */
#define LAMA_CONV_FAMILY_HEAD7 7      /* 7x7 head */
#define LAMA_CONV_FAMILY_LDS 8        /* the LDS-staged conv_kernel */
#define LAMA_CONV_GEO_WR(wmv, kg, ksc1, twlog, s2, coop, roll, fuse1, xs, ys) \
    ((wmv) | (kg) << 4 | (ksc1) << 8 | (twlog) << 12 | (s2) << 16 | (coop) << 17 | (roll) << 18 | (fuse1) << 19 | (xs) << 20 | (ys) << 21)
int lama_conv2d_route_query(const lama_conv2d_args* args, int32_t head_rs, int32_t* family, int32_t* geometry);

/* Stand-alone per-channel affine + activation: y = act(x*scale[c] + shift[c]) (scale/shift NULL = identity).
 * Used when a caller runs generator.model layer by layer and hits a bare nn.BatchNorm2d (eval) /
 * nn.ReLU / nn.Sigmoid (ffc.py:352-354,362-363); the fused forward never launches it. */
int lama_affine_act_fwd(void* stream, const lama_tensor* x, const float* scale, const float* shift, int32_t act,
                        const lama_tensor* y, int32_t batch);
/* Stand-alone nn.ReflectionPad2d(pad) (ffc.py:314,360); fused into the 7x7 convs on the normal path. */
int lama_reflect_pad_fwd(void* stream, const lama_tensor* x, int32_t pad, const lama_tensor* y, int32_t batch);

/* ------------------------------------------------------------------------------------------------
 * Feature refinement (saicinpainting/evaluation/refinement.py, `refine=True` of bin/predict.py:75-79): what is
 * not a convolution / FFT.  The dgrad of every conv / FourierUnit of generator.model[first_resblock:] reuses
 * lama_conv2d_fwd / lama_rfft2_fwd / lama_irfft2_fwd with transposed, flipped packed weights (lama_amd/backward.py);
 * autograd (refinement.py:163 loss.backward()) is replaced by that explicit reverse pass.
 * ------------------------------------------------------------------------------------------------ */
/* gout = g * act'(y) with the derivative expressed through the layer OUTPUT y: ReLU -> [y > 0], sigmoid -> y (1 - y),
 * tanh -> 1 - y^2, none -> 1.  Backward of the ReLU / Sigmoid of ffc.py:253-254,354,363 and of FourierUnit's ReLU (ffc.py:101). */
int lama_act_bwd(void* stream, const lama_tensor* g, const lama_tensor* y, int32_t act, const lama_tensor* gout, int32_t batch);
/* out = a + b: gradient joins of the residual / two-branch structure (ffc.py:161,220-223,288) */
int lama_add_fwd(void* stream, const lama_tensor* a, const lama_tensor* b, const lama_tensor* out, int32_t batch);
/* adjoint of nn.ReflectionPad2d(pad) / padding_mode='reflect' (ffc.py:188-196,314,360): gp [B,C,H+2p,W+2p] -> g [B,C,H,W]
 * (+ addend, optional): every padded position is added onto the input pixel it mirrors. */
int lama_reflect_pad_bwd(void* stream, const lama_tensor* gp, const lama_tensor* addend, int32_t pad, const lama_tensor* g,
                         int32_t batch);
/* (v108) the same adjoint fused with what the reverse pass does to its result: s = fold(gp) [+ add1] [+ add2]; g = s (optional, may be
 * add2 itself); gm = s * act'(mask_y) (optional).  add1: the 1x1 path into the same tensor (SpectralTransform.conv1, ffc.py:158), add2: the
 * identity path of the resnet block (ffc.py:288), mask_y: the taped output of the layer upstream (ffc.py:253-254).  Replaces autograd's
 * separate AddBackward / ReluBackward passes of refinement.py:163; at least one of g, gm. */
int lama_reflect_pad_bwd_fused(void* stream, const lama_tensor* gp, const lama_tensor* add1, const lama_tensor* add2, int32_t pad,
                               const lama_tensor* mask_y, int32_t act, const lama_tensor* g, const lama_tensor* gm, int32_t batch,
                               const float* ring);
/* (v108) the data gradient of a reflect-padded 3x3 conv (ffc.py:188-196) WITHOUT its padded plane: the interior H x W of the zero-padded
 * correlation is a zero-pad-1 conv of the output gradient (lama_conv2d_fwd / lama_winograd_conv3x3_fwd with LAMA_PAD_ZERO, pad 1) and the
 * one-pixel frame around it -- rows y = -1, H (x = -1..W), columns x = -1, W (y = 0..H-1) -- is computed here, exact fp32:
 *   ring [batch][cout][2 (W + 2) + 2 H] (top, bottom, left, right; lama_dgrad_ring_bytes),
 *   w_ring [4][cin][3][cout] fp32 = the dgrad weights w'[cout][cin][3][3] (flipped, transposed) as  top: w'[o][c][2][k], bottom: w'[o][c][0][k],
 *   left: w'[o][c][k][2], right: w'[o][c][k][0];  cout % 128 == 0, cin % 64 == 0.
 * lama_reflect_pad_bwd_fused with ring != NULL then takes gp = the interior [B,C,H,W] (pad must be 1). */
size_t lama_dgrad_ring_bytes(int32_t batch, int32_t cout, int32_t H, int32_t W);
int lama_dgrad_ring_fwd(void* stream, const lama_tensor* g, const float* w_ring, int32_t cout, float* ring, int32_t batch);
/* kornia.filters.gaussian_blur2d(x, (5,5), (1.0,1.0)) [border reflect] of the top-left crop [0:y.H, 0:y.W] of x
 * (refinement.py:24,52,149), and its adjoint (gx is zero outside the crop). */
int lama_gauss5_fwd(void* stream, const lama_tensor* x, const lama_tensor* y, int32_t batch);
int lama_gauss5_bwd(void* stream, const lama_tensor* gy, const lama_tensor* gx, int32_t batch);
/* F.interpolate(x, size=(y.H, y.W), mode='bilinear', align_corners=False) (refinement.py:25,53,55,200-201) and its adjoint. */
int lama_bilinear_fwd(void* stream, const lama_tensor* x, const lama_tensor* y, int32_t batch);
int lama_bilinear_bwd(void* stream, const lama_tensor* gy, const lama_tensor* gx, int32_t batch);
/* y = x >= thr ? 1 : 0  (mask[mask >= eps] = 1; mask[mask < eps] = 0: refinement.py:57-62,70-71,300-301) */
int lama_threshold_fwd(void* stream, const lama_tensor* x, float thr, const lama_tensor* y, int32_t batch);
/* kornia.morphology.erosion(x, se) with a flat structuring element se [kh,kw] (device floats, non-zero = member; origin =
 * centre; geodesic border: positions outside the image never lower the minimum), refinement.py:68 with the 15x15 ellipse. */
int lama_erode_fwd(void* stream, const lama_tensor* x, const float* se, int32_t kh, int32_t kw, float max_val, const lama_tensor* y,
                   int32_t batch);
/* Masked L1 terms of refinement.py:75-84 over the elements with mask < thr (select_ge = 0) or mask >= thr (select_ge = 1); a
 * 1-channel mask is broadcast over pred's channels (mask.repeat(1,3,1,1)).
 *   fwd: accum[0] += sum |pred - target|, accum[1] += number of selected elements   (two device doubles, zeroed by the caller)
 *   bwd: g = (accumulate ? g : 0) + scale * sign(pred - target) on the selected elements  (d mean|.| / d pred: scale = 1 / count) */
int lama_l1_masked_fwd(void* stream, const lama_tensor* pred, const lama_tensor* target, const lama_tensor* mask, float thr,
                       int32_t select_ge, double* accum, int32_t batch);
int lama_l1_masked_bwd(void* stream, const lama_tensor* pred, const lama_tensor* target, const lama_tensor* mask, float thr,
                       int32_t select_ge, float scale, int32_t accumulate, const lama_tensor* g, int32_t batch);
/* (v111) the same terms PER IMAGE (refining a batch of images as separate optimisations in one launch chain):
 *   fwd: accum[2 b] += sum |pred - target|, accum[2 b + 1] += count over image b only   (accum: [batch][2] device doubles, zeroed by the caller)
 *   bwd: g_b = (accumulate ? g_b : 0) + s_b * sign(pred - target) on the selected elements of image b, with s_b = (float)(1.0 / n_b) from the
 *        count n_b = accum[2 b + 1] that the fwd left (0 for an empty selection): at batch 1 bit-identical to lama_l1_masked_bwd with
 *        scale = (float)(1.0 / n).  batch <= 65535. */
int lama_l1_masked_per_image_fwd(void* stream, const lama_tensor* pred, const lama_tensor* target, const lama_tensor* mask, float thr,
                                 int32_t select_ge, double* accum, int32_t batch);
int lama_l1_masked_per_image_bwd(void* stream, const lama_tensor* pred, const lama_tensor* target, const lama_tensor* mask, float thr,
                                 int32_t select_ge, const double* accum, int32_t accumulate, const lama_tensor* g, int32_t batch);
/* one torch.optim.Adam step (refinement.py:134,165: betas, eps as given, no weight decay / amsgrad) on a flat fp32 buffer;
 * step = 1, 2, ... */
int lama_adam_step(void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                   float beta2, float eps, int32_t step);

/* ---- quality metrics --------------------------------------------------------------------------
 * SSIM.forward(img1, img2) with size_average=False (saicinpainting/evaluation/losses/ssim.py:18-71): out[i] = mean over (C, H, W)
 * of the SSIM map of image i; depthwise window_size x window_size gaussian window given as its normalised 1-D factor `window1d`
 * (HOST array of window_size floats, ssim.py:36-45), zero padding window_size / 2.  Odd window sizes up to 15.  workspace: device
 * scratch of lama_ssim_workspace_bytes() bytes.  Replaces the five F.conv2d(groups=channel) calls + the elementwise map. */
size_t lama_ssim_workspace_bytes(int32_t batch, int32_t C, int32_t H, int32_t W);
int lama_ssim_fwd(void* stream, const lama_tensor* img1, const lama_tensor* img2, int32_t batch, int32_t window_size,
                  const float* window1d, float* out, void* workspace, size_t workspace_bytes);

/* LPIPS (VGG-16, net-lin; saicinpainting/evaluation/losses/lpips.py) around the backbone's 3x3 convs (lama_conv2d_fwd / lama_winograd_conv3x3_fwd with
 * LAMA_PAD_ZERO).  fp32 tensors only.
 * lama_lpips_scale_fwd: ScalingLayer (lpips.py:603-610) of both inputs into ONE tensor: y[i] = ((2 x0[i] - 1) - shift_c) / scale_c for i < batch,
 *   y[batch + i] = the same of x1[i]; normalize = 0 skips the 2 x - 1 (inputs already in [-1, 1]).  x0, x1: [batch, 3, H, W]; y: [2 batch, 3, H, W];
 *   shift, scale: HOST arrays of 3 floats.  The zero padding of conv1_1 applies to y, so this does not fold into that layer's weights.
 * lama_lpips_layer_fwd: one feature level.  f0, f1: [batch, C, h, w] (the two halves of the backbone's output), w: device [C] (the level's linear head):
 *   acc[b] += (1 / (h w)) sum_pixels sum_c w_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2,   |.| = the channel L2 norm of a pixel
 *   (lpips.py:45-47, 578-586); acc: device [batch] floats that the caller zeroes (or carries from the levels before).  Neither the normalised features nor
 *   the difference reach memory.  pool0 / pool1 (both or neither; NULL or ptr = NULL: off): [batch, C, h / 2, w / 2] = max_pool2d(f, 2, 2) of the two
 *   maps, written by the same launch (floor semantics: an odd last row / column is in the distance, not in the pool).  Any C, h, w >= 1 (h, w >= 2 with
 *   pool).  The sums are formed in a fixed order without atomics: two runs are bit-identical, and f0 == f1 gives exactly 0.  workspace: 8-byte aligned
 *   device scratch of lama_lpips_layer_workspace_bytes() bytes (LAMA_ERR_WORKSPACE otherwise). */
int lama_lpips_scale_fwd(void* stream, const lama_tensor* x0, const lama_tensor* x1, const lama_tensor* y, int32_t batch, int32_t normalize,
                         const float* shift, const float* scale);
size_t lama_lpips_layer_workspace_bytes(int32_t batch, int32_t C, int32_t H, int32_t W);
int lama_lpips_layer_fwd(void* stream, const lama_tensor* f0, const lama_tensor* f1, int32_t batch, const float* w, float* acc,
                         const lama_tensor* pool0, const lama_tensor* pool1, void* workspace, size_t workspace_bytes);

/* ---- (added to v112 without a version bump: new symbols only, nothing else changes) FID: the Inception-v3 feature extractor (saicinpainting/evaluation/losses/fid/inception.py, fid_score.py) -----------------------
 * What torchvision's Inception3 needs beyond lama_conv2d_fwd: rectangular kernels with per-axis zero padding, any channel count, 3x3 max / average
 * pooling, the global average pool and the bilinear resize of the input.  fp32 NCHW views; x and y may be channel slices of wider buffers (an
 * Inception branch stores straight into its block's concatenation buffer: torch.cat is free).
 *
 * lama_conv2d_rect_fwd: y = act( conv2d(x, w, stride, padding=(pad_h, pad_w)) + bias ), zero padding, not transposed, cin = x.C >= 1, cout = y.C >= 1,
 *   kh, kw in 1..7, stride 1 or 2, act LAMA_ACT_NONE / LAMA_ACT_RELU.  y.H = (x.H + 2 pad_h - kh) / stride + 1 (floor), y.W likewise: any other
 *   y view is LAMA_ERR_BAD_ARG; a kernel size or stride outside the ranges is LAMA_ERR_UNSUPPORTED.  Implicit GEMM on v_mfma_f32_32x32x16 with the
 *   3-term split (LAMA_PREC_F16X3 / LAMA_PREC_BF16X3; LAMA_PREC_F32: LAMA_ERR_UNSUPPORTED) and fp32 accumulation; M = cout and N = batch * Ho * Wo
 *   are tiled, K = cin * kh * kw never is split: every output is one k-ordered sum, bit-identical run to run.  range_flag: as in lama_conv2d_args.
 *   w_packed = lama_conv2d_rect_pack_weight(Conv2d weights [cout, cin, kh, kw], scale[o] folded (NULL = 1)); 16-byte aligned,
 *   lama_conv2d_rect_packed_weight_bytes bytes (0: unsupported geometry / precision).  The K tail and the M tail are zero-filled. */
typedef struct lama_conv2d_rect_args {
    lama_tensor x;
    const void* w_packed;
    const float* bias; /* [cout] (the folded BatchNorm shift) or NULL */
    int32_t act;
    lama_tensor y;
    int32_t batch;
    int32_t kh, kw, stride, pad_h, pad_w;
    int32_t precision;
    uint32_t* range_flag;
} lama_conv2d_rect_args;
int64_t lama_conv2d_rect_packed_weight_bytes(int32_t cout, int32_t cin, int32_t kh, int32_t kw, int32_t precision);
int lama_conv2d_rect_pack_weight(void* stream, const float* w, const float* scale, int32_t cout, int32_t cin, int32_t kh, int32_t kw,
                                 int32_t precision, void* dst);
int lama_conv2d_rect_fwd(void* stream, const lama_conv2d_rect_args* args);
/* lama_pool3x3_fwd: 3x3 window, stride 1 or 2, pad 0 or 1, y.H = (x.H + 2 pad - 3) / stride + 1.  LAMA_POOL_MAX = F.max_pool2d (padding never wins);
 * LAMA_POOL_AVG_EXCLUDE_PAD = F.avg_pool2d(count_include_pad=False): the taps inside the plane are added in one fixed order (rows, then columns) in
 * fp32 and divided once by their number. */
#define LAMA_POOL_MAX 0
#define LAMA_POOL_AVG_EXCLUDE_PAD 1
int lama_pool3x3_fwd(void* stream, const lama_tensor* x, const lama_tensor* y, int32_t batch, int32_t mode, int32_t stride, int32_t pad);
/* lama_global_avgpool_fwd: x [batch, C, h, w] -> y [batch, C] (contiguous device floats): the fp64 sum in index order, divided and rounded once. */
int lama_global_avgpool_fwd(void* stream, const lama_tensor* x, float* y, int32_t batch);
/* lama_fid_input_fwd: pred, target [batch, 3, H, W] in [0, 1] -> y [2 batch, 3, y.H, y.W] (pred first): F.interpolate(mode='bilinear',
 * align_corners=False) without antialiasing (the coordinate arithmetic of lama_bilinear_fwd) to y's size (299 x 299 for FID), then 2 x - 1
 * (inception.py:196-203).  resize = 0: 2 x - 1 only, y.H = H, y.W = W. */
int lama_fid_input_fwd(void* stream, const lama_tensor* pred, const lama_tensor* target, const lama_tensor* y, int32_t batch, int32_t resize);

/* ---- (added to v112 without a version bump: new symbols only, nothing else changes) activation ranges: WHERE a tensor leaves the fp16 split's range ----
 * The range watch (lama_conv2d_args.range_flag) is one bit per device.  lama_range_stats_fwd reduces any view to per-channel statistics in one read:
 * for channel c of x [batch, C, H, W] (fp32 or fp16, any batch_stride >= C H W, any element-aligned start, any plane size), over its batch H W elements,
 *   n_nan = NaNs, n_inf = +-inf, n_over = FINITE elements with |e| > limit, abs_max = the largest |e| over the finite elements (+0.0f if none).
 * Elements are classified on their bit patterns (fp16 ones widen exactly): exactly `limit` is not over, the next float is; -0.0 and denormals count as
 * what they are (nothing is flushed).  out: device [x->C], OVERWRITTEN (no zeroing launch).  Two launches (per-piece partials into `workspace`, then one
 * fold per channel), no atomics: bit-identical run to run; asynchronous and hipGraph-capturable.  workspace: lama_range_stats_workspace_bytes() device
 * bytes, 4-byte aligned.
 * LAMA_ERR_BAD_ARG: a null pointer, batch <= 0, an empty view, limit that is not a positive finite number, batch_stride < C H W, a misaligned pointer;
 * LAMA_ERR_WORKSPACE: workspace too small; LAMA_ERR_UNSUPPORTED: an unknown dtype, batch H W >= 2^32 (the counters are 32-bit) or more than 2^31 - 1
 * 32 KiB pieces in all.  Nothing is launched and out is untouched on an error. */
typedef struct lama_range_stats { float abs_max; uint32_t n_nan, n_inf, n_over; } lama_range_stats;   /* 16 bytes, one per channel */
size_t lama_range_stats_workspace_bytes(int32_t batch, int32_t C, int32_t H, int32_t W);
int    lama_range_stats_fwd(void* stream, const lama_tensor* x, int32_t batch, float limit,
                            lama_range_stats* out /* device, [x->C] */, void* workspace, size_t workspace_bytes);
/* The two spectra inside a lama_fourier_unit_fwd workspace for x [batch, C, h, w] of element type dtype, as that call leaves them: spec_in = the
 * interleaved rfft2 of x (the operand the spectral 1x1 splits, ffc.py:86-100), spec_out = relu(bn(conv(spec_in))) (ffc.py:100-101), both
 * [batch, 2C, h, w/2+1].  The library's own statement of the layout (lama_fourier_unit_fwd goes through it); nothing is launched.
 * LAMA_ERR_BAD_ARG / LAMA_ERR_UNSUPPORTED (dtype) / LAMA_ERR_WORKSPACE (smaller than lama_fourier_unit_workspace_bytes). */
int lama_fourier_unit_workspace_views(int32_t batch, int32_t C, int32_t h, int32_t w, int32_t dtype, void* workspace, size_t workspace_bytes,
                                      lama_tensor* spec_in, lama_tensor* spec_out);

/* ---- (added to v112 without a version bump: new symbols only, nothing else changes) the local Fourier unit of SpectralTransform (ffc.py:136-138,148-159) ----
 * With x1 [batch, C, h, h], q = C / 4 and s = h / 2 the reference forms xs_in = cat(split(cat(split(x1[:, :q], s, dim=-2), 1), s, dim=-1), 1), runs a
 * second FourierUnit on it and adds xs.repeat(1, 1, 2, 2) to x1 + fu(x1).  The two data movements around that FourierUnit:
 *   lama_lfu_gather_fwd:   y[b, (2 j + i) q + c, yy, xx] = x[b, c, i s + yy, j s + xx]   c < q; i, j in {0, 1}; yy, xx < s.  x: a [batch, q, h, h] view
 *                          (the first quarter of x1's channels, batch_stride that of x1), y: [batch, 4 q, s, s].  A copy: bit-exact.
 *   lama_lfu_tile_add_fwd: out[b, c, y, x] = a[b, c, y, x] + xs[b, c, y mod s, x mod s].  a, out: [batch, C, h, h], xs: [batch, C, s, s]; out may be a
 *                          itself (in place), xs overlaps neither.  One fp32 add per element; fp16 tensors: the add in fp32, rounded once.
 * Element types LAMA_DT_F32 or LAMA_DT_F16, every tensor of a call the same.  Any batch_stride >= C H W, channel-slice views, any element-aligned start:
 * 16-byte accesses where a row of s elements, the pointers and the batch strides allow, narrower ones (down to one element) where they do not.  One
 * launch each, plain vector loads and stores, no atomics, no workspace: asynchronous and hipGraph-capturable.  Like the reference (which splits BOTH axes
 * by h / 2) only square planes with an even side.
 * LAMA_ERR_BAD_ARG: a null pointer, batch <= 0, an empty view, shapes that do not match the above, batch_stride < C H W, a pointer that is not
 * element-aligned; LAMA_ERR_UNSUPPORTED: H != W or odd H (of x / a), an unknown or mixed dtype, LAMA_DT_SPLIT16, a plane of 2^30 pieces or more.
 * Nothing is launched on an error. */
int lama_lfu_gather_fwd(void* stream, const lama_tensor* x, const lama_tensor* y, int32_t batch);
int lama_lfu_tile_add_fwd(void* stream, const lama_tensor* a, const lama_tensor* xs, const lama_tensor* out, int32_t batch);

/* ---- (added to v112 without a version bump: one new symbol, nothing else changes) paste_back: the result of a dataset.scale_factor step resampled
 * to the SOURCE grid and pasted into the decoded u8 original, in one launch.  THIS OUTPUT HAS NO COUNTERPART IN THE REFERENCE, which writes the
 * scaled image (bin/predict.py:86-94): it is this engine's own definition, pinned byte for byte by tests/paste_back_util.py::paste_back_ref.
 * image_hwc [B][Hs][Ws][3], mask [B][Hs][Ws], out_hwc [B][Hs][Ws][3]: u8 source slots on the device, each image's own h x w pixels in the
 * top-left corner; src_sizes / dst_sizes: device int32 [B][2] = (h, w) / (dh, dw), the arrays lama_resize_u8_fwd takes (h = 0: an empty slot);
 * lowres: fp32 [B,3,Hp,Wp] of which [:dh, :dw] is valid and nothing else is read (any batch_stride >= 3 Hp Wp: channel-slice views work).
 * For image b and source pixel (y, x), y < h, x < w:
 *   v = F.interpolate(lowres[b, :, :dh, :dw], size=(h, w), mode='bilinear', align_corners=False)[:, y, x] -- BILINEAR, the index arithmetic of
 *     lama_bilinear_fwd: sy = (float)dh / (float)h (IEEE fp32), s = max(0, (y + 0.5f) * sy - 0.5f), i0 = min((int)s, dh - 1), i1 = min(i0 + 1, dh - 1),
 *     l = s - i0, the same in x; v = (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11), every operation rounded on its own
 *     (no floating-point contraction anywhere in the kernel);
 *   binarize != 0: mask > 0 -> clip(v * 255, 0, 255) truncated, else the three source bytes;
 *   binarize == 0: m = mask / 255.f, r = m * v + (1 - m) * (u8 / 255.f), byte = clip(r * 255, 0, 255) truncated (= the source byte where m = 0;
 *     lowres is read only where the mask byte is not 0).  A NaN quantises to 0, as in lama_blend_quantize_u8_fwd.
 * Slot bytes outside h x w are written as 0; so is a whole slot that is empty or whose sizes do not fit (h > Hs, w > Ws, dh > Hp, dw > Wp, dh or
 * dw < 1): the sizes are device data, nothing is read or written out of bounds.  7 bytes per source pixel (1 + 3 read, 3 written); dword accesses
 * where Ws % 4 == 0 and the three slot pointers are 4-byte aligned, byte accesses otherwise.  One launch, no workspace, no atomics:
 * asynchronous and hipGraph-capturable.
 * LAMA_ERR_BAD_ARG: a null pointer; batch, Hs or Ws <= 0; a view that is not [., 3, H, W]; batch_stride < 3 H W; a view pointer that is not
 * 4-byte aligned; out_hwc == image_hwc.  LAMA_ERR_UNSUPPORTED: a view that is not fp32; a slot of 2^30 work items (of 4 pixels) or more; a view plane of 2^30 elements or more.
 * Nothing is launched on an error. */
int lama_paste_back_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes, const int32_t* dst_sizes, int32_t Hs,
                           int32_t Ws, const lama_tensor* lowres, uint8_t* out_hwc, int32_t batch, int32_t binarize);

/* ---- (added to v112 without a version bump: new symbols only, nothing else changes) crop_to_mask: the two ends of a u8 predict step whose
 * generator sees only a WINDOW of each source slot.  THIS OUTPUT HAS NO COUNTERPART IN THE REFERENCE (a crop sees less context than the whole
 * image): it is this engine's own definition -- the existing u8 step run on the cropped arrays, pasted by slicing -- pinned bit for bit by
 * tests/crop_util.py against lama_mask_compose_u8_fwd / lama_blend_quantize_u8_fwd on host-cropped slots and against a numpy restatement.
 * image_hwc [B][Hs][Ws][3], mask [B][Hs][Ws], out_hwc [B][Hs][Ws][3]: u8 source slots on the device, each image's own h x w pixels in the
 * top-left corner; src_sizes: device int32 [B][2] = (h, w) (h = 0: an empty slot); rects: device int32 [B][4] = (y0, x0, ch, cw).
 * For image b let C = image[b, y0:y0+ch, x0:x0+cw] and M = mask[b, y0:y0+ch, x0:x0+cw].
 *   lama_crop_compose_u8_fwd: out fp32 [B,4,Hp,Wp] = what lama_mask_compose_u8_fwd writes for a slot batch holding C, M with sizes (ch, cw):
 *     C / 255.f (IEEE fp32 division), np.pad(mode='symmetric') at the bottom / right up to (Hp, Wp) (periodic beyond 2 ch rows), m = mask > 0
 *     (binarize != 0) or M / 255.f, out = cat(C * (1 - m), m).  4 bytes read and 16 written per pixel of the view.
 *   lama_crop_paste_u8_fwd: out_hwc[b, :h, :w] = the source bytes, and inside the window the bytes lama_blend_quantize_u8_fwd gives for
 *     (C, M, pred): clip((m * pred + (1 - m) * C / 255.f) * 255, 0, 255) truncated -- the source byte where the mask byte is 0; pred, fp32
 *     [B,3,Hp,Wp] (any batch_stride >= 3 Hp Wp: channel-slice views work), is read only inside the window where the mask byte is not 0.  A NaN
 *     quantises to 0.  Slot bytes outside h x w are written as 0.  7 bytes per source pixel (1 + 3 read, 3 written).
 * A rect that does not fit -- ch or cw < 1, y0 or x0 < 0, y0 + ch > h, x0 + cw > w, ch > Hp, cw > Wp, h > Hs, w > Ws -- behaves as an empty slot:
 * the compose writes zeros for that image, the paste writes the whole slot as 0.  Sizes and rects are device data: nothing is read or written
 * out of bounds.  Dword accesses to the slots where Ws % 4 == 0 and the slot pointers are 4-byte aligned (the compose: and x0 % 4 == 0), float4
 * stores to a view with Wp % 4 == 0, a 16-byte aligned pointer and batch_stride % 4 == 0; byte / scalar accesses otherwise.  No floating-point
 * contraction in either kernel.  One launch each, no workspace, no atomics: asynchronous and hipGraph-capturable.
 * LAMA_ERR_BAD_ARG: a null pointer; batch, Hs or Ws <= 0; a view that is not [., 4, H, W] (compose) / [., 3, H, W] (paste); batch_stride < C H W;
 * a view pointer that is not 4-byte aligned; out_hwc == image_hwc.  LAMA_ERR_UNSUPPORTED: a view that is not fp32; 2^30 work items (of 4 pixels)
 * or more per image; a view plane of 2^30 elements or more (paste).  Nothing is launched on an error. */
int lama_crop_compose_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes, const int32_t* rects, int32_t Hs,
                             int32_t Ws, const lama_tensor* out, int32_t batch, int32_t binarize);
int lama_crop_paste_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes, const int32_t* rects, int32_t Hs,
                           int32_t Ws, const lama_tensor* pred, uint8_t* out_hwc, int32_t batch, int32_t binarize);

/* ---- (added to v112 without a version bump: new symbols only, nothing else changes) crop_max_side: the two ends of a crop_to_mask step whose
 * window is SHRUNK by a per-image integer k for the generator.  THIS OUTPUT HAS NO COUNTERPART IN THE REFERENCE: it is this engine's own
 * definition, restated in numpy and pinned bit for bit / byte for byte by tests/crop_shrink_util.py (and, where k divides the window, against
 * lama_resize_u8_fwd with factor 1 / k and lama_paste_back_u8_fwd on host-cropped slots).
 * Slots, src_sizes and rects [B][4] = (y0, x0, ch, cw) are those of lama_crop_*_u8_fwd; shrinks: device int32 [B] = k, 1 .. 16.  For image b let
 * C, M be the window, dh = ceil(ch / k), dw = ceil(cw / k).
 *   lama_crop_shrink_compose_u8_fwd: out fp32 [B,4,Hp,Wp] = cat(S * (1 - m), m) after np.pad(mode='symmetric') of the dh x dw planes at the
 *     bottom / right up to (Hp, Wp) (periodic).  S[y, x] is the integer shrink of lama_resize_u8_fwd on C: each byte / 255.f; a whole k x k box
 *     summed in row-major order, four at a time as acc + (((a + b) + c) + d), the remainder one by one, times (float)(1.0 / (k * k)); a box cut
 *     by the window's bottom or right edge is the row-major sum of the pixels inside it / (float)count.  The MASK is the MAX of the box's bytes,
 *     cut boxes included: mu = max, m = mu > 0 (binarize != 0) or mu / 255.f.  This differs from dataset.scale_factor's INTER_NEAREST on
 *     purpose: a one-pixel stroke must not vanish from the generator's mask while the paste still replaces it -- which is also why dh is a
 *     ceiling: every window pixel lies in a box.  The window is read once, 16 bytes are written per pixel of the view.
 *   lama_crop_shrink_paste_u8_fwd: out_hwc[b, :h, :w] = the source bytes, and inside the window, where the mask byte is not 0, the bytes
 *     lama_paste_back_u8_fwd gives for (C, M, lowres[b], (dh, dw)) on window coordinates (y - y0, x - x0), sy = (float)dh / (float)ch: THE
 *     PIXELS UNDER THE MASK ARE A k-FOLD BILINEAR UPSAMPLING OF THE PREDICTION.  lowres, fp32 [B,3,Hp,Wp], is read only inside [:dh, :dw] and
 *     only for such pixels.  Slot bytes outside h x w are written as 0.
 * A rect that does not fit -- the conditions of lama_crop_*_u8_fwd with dh > Hp, dw > Wp in place of ch > Hp, cw > Wp -- or a k outside 1 .. 16
 * behaves as an empty slot in both entries.  Everything is device data: nothing is read or written out of bounds.  Dword accesses to the slots
 * where Ws % 4 == 0 and the slot pointers are 4-byte aligned (any x0), float4 stores to a view as for lama_crop_compose_u8_fwd; byte / scalar
 * accesses otherwise.  No floating-point contraction.  One launch each, no workspace, no atomics, no LDS: asynchronous and hipGraph-capturable.
 * Errors as for lama_crop_*_u8_fwd, and LAMA_ERR_BAD_ARG for a null shrinks.  Nothing is launched on an error. */
int lama_crop_shrink_compose_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes, const int32_t* rects,
                                    const int32_t* shrinks, int32_t Hs, int32_t Ws, const lama_tensor* out, int32_t batch, int32_t binarize);
int lama_crop_shrink_paste_u8_fwd(void* stream, const uint8_t* image_hwc, const uint8_t* mask, const int32_t* src_sizes, const int32_t* rects,
                                  const int32_t* shrinks, int32_t Hs, int32_t Ws, const lama_tensor* lowres, uint8_t* out_hwc, int32_t batch,
                                  int32_t binarize);

/* ---- (added to v112 without a version bump: new symbols only, nothing else changes) the zlib stream of a PNG's IDAT, made on the device from u8
 * HWC slots.  A PNG encoder owes the decoder the pixels, not particular bytes: THE STREAM IS THIS ENGINE'S OWN DEFINITION, pinned byte for byte by
 * tests/png_ref.py::deflate_ref.  image_hwc [batch][Hs][Ws][channels] u8 slots, each image's h x w pixels in the top-left corner; sizes: device int32
 * [batch][2] = (h, w).  Per image:
 *   filtered bytes  per row the byte 1 (filter Sub), then w c bytes x[i] - x[i - c] mod 256 (the first pixel as is): row = 1 + w c bytes
 *   chunks          R = max(1, chunk_bytes / row) whole rows each, the last one may be shorter; chunk_bytes 0 = the default 24576
 *   one chunk       one dynamic-Huffman block (BFINAL 0, BTYPE 10; HLIT 0, HDIST 0 with one distance code of length 0, HCLEN 15 with the lengths 4 for the
 *                   code-length symbols 0..15 and 0 for 16 / 17 / 18: every code length travels as 4 bits) of the chunk's bytes as literals and symbol
 *                   256, then an empty stored block (000, pad to a byte, 00 00 FF FF).  Code lengths: the depths of the Huffman tree over the used
 *                   symbols (256 counts once) by the two-queue merge over the symbols sorted by (count, symbol), a leaf before an internal node on ties;
 *                   deeper than 15, every non-zero count n becomes (n + 1) >> 1 and the tree is built again.  Canonical codes.
 *                   Where that is not shorter than raw + 5 bytes the chunk is stored: 00, LEN, ~LEN (little endian), the raw bytes.
 *   stream          78 01, the chunks in order, 01 00 00 FF FF, Adler-32 of the filtered bytes (big endian)
 * No matches (a flat region costs 1 bit per byte), no filter but Sub, 8-bit gray (channels 1) or RGB (3); the PNG container and its CRC are the
 * caller's (lama_amd.predict.png_from_zlib).  Image j's stream starts at out + j * out_stride and has out_bytes[j] bytes; the bytes behind it are not
 * touched.  An empty slot (h or w < 1) and one whose sizes do not fit (h > Hs, w > Ws) give out_bytes[j] = 0 and touch nothing else: the sizes are device
 * data, nothing is read or written outside a slot.  Two launches (one workgroup per chunk, then one per four chunks and one per image), no global atomics, plain vector stores;
 * asynchronous and hipGraph-capturable.  The same operands give the same bytes.
 * lama_png_deflate_bound: the most bytes one h x w image's stream can take (every chunk stored); 0 for an empty image or refused arguments.
 * lama_png_deflate_workspace_bytes: the workspace (16-byte aligned) of a call with these slots.
 * LAMA_ERR_BAD_ARG: a null pointer; batch, Hs or Ws <= 0; channels not 1 or 3; chunk_bytes neither 0 nor in [64, 32768]; out_stride below
 * lama_png_deflate_bound(Hs, Ws, ...); a workspace that is not 16-byte aligned, sizes / out_bytes that are not 4-byte aligned.  LAMA_ERR_UNSUPPORTED: a row of
 * the slot (1 + Ws channels) beyond 65535 bytes; 2^30 chunks or more.  LAMA_ERR_WORKSPACE: a smaller workspace.  Nothing is launched on an error. */
size_t lama_png_deflate_bound(int32_t h, int32_t w, int32_t channels, int32_t chunk_bytes);
int    lama_png_deflate_workspace_bytes(int32_t batch, int32_t Hs, int32_t Ws, int32_t channels, int32_t chunk_bytes, size_t* bytes);
int    lama_png_deflate_u8_fwd(void* stream, const uint8_t* image_hwc, const int32_t* sizes, int32_t Hs, int32_t Ws, int32_t channels, int32_t batch,
                               int32_t chunk_bytes, uint8_t* out, size_t out_stride, int32_t* out_bytes, void* workspace, size_t workspace_bytes);

/* ---- (added to v112 without a version bump: new symbols only, nothing else changes) the entropy-coded scan of a baseline JPEG, made on the device
 * from u8 HWC RGB slots.  A JPEG encoder owes the decoder a conforming stream, not particular bytes: THE STREAM IS THIS ENGINE'S OWN DEFINITION,
 * integer arithmetic throughout, pinned byte for byte by tests/jpeg_ref.py::scan_ref and stated in full at the head of csrc/jpeg.hip: JFIF YCbCr in
 * 16-bit fixed point, edge replication out to the MCU grid, 4:2:0 chroma as (a + b + c + d + 2) >> 2, a separable integer DCT from a 2^13 table,
 * the Annex K quantisation tables scaled by libjpeg's quality rule, the Annex K Huffman tables, one restart interval per MCU row (RSTm between the
 * intervals, m = row mod 8), FF stuffed as FF 00.  image_hwc [batch][Hs][Ws][3] u8 slots, each image's h x w pixels in the top-left corner; sizes:
 * device int32 [batch][2] = (h, w) -- the arrays lama_png_deflate_u8_fwd takes.  subsampling LAMA_JPEG_444 (MCU 8 x 8: Y, Cb, Cr) or LAMA_JPEG_420
 * (MCU 16 x 16: four Y blocks in raster order, Cb, Cr); quality 1 .. 100.  The scan only: SOI .. SOS and EOI are the caller's
 * (lama_amd.jpeg.jpeg_from_scan; DRI = the MCUs of one row).  Image j's scan starts at out + j * out_stride and has out_bytes[j] bytes; the bytes behind
 * it are not touched.  A scan longer than out_stride gives out_bytes[j] = -(bytes needed) and writes nothing for that image; an empty slot (h or w < 1)
 * and one whose sizes do not fit (h > Hs, w > Ws) give 0 and touch nothing else: the sizes are device data, nothing is read or written outside a slot.
 * Three launches (per MCU row the exact byte count; per image the offsets; per MCU row the bytes), no global atomics, plain vector stores;
 * asynchronous and hipGraph-capturable.  The same operands give the same bytes.
 * lama_jpeg_scan_bound: the most bytes the scan of one h x w image can take (every block at its longest codes, every byte stuffed); 0 for refused arguments.
 * lama_jpeg_scan_workspace_bytes: the workspace (16-byte aligned; 4 bytes per MCU row) of a call with these slots; *bytes is left alone on an error.
 * LAMA_ERR_BAD_ARG: a null pointer; batch, Hs or Ws <= 0; quality outside 1 .. 100; an unknown subsampling; a workspace that is not 16-byte aligned,
 * sizes / out_bytes that are not 4-byte aligned.  LAMA_ERR_UNSUPPORTED: more than 65535 pixels a side or MCUs per row; a slot whose bound is beyond
 * 2^31 - 1 bytes; 2^30 MCU rows or more.  LAMA_ERR_WORKSPACE: a smaller workspace.  Nothing is launched on an error. */
#define LAMA_JPEG_444 0
#define LAMA_JPEG_420 1
size_t lama_jpeg_scan_bound(int32_t h, int32_t w, int32_t subsampling);
int    lama_jpeg_scan_workspace_bytes(int32_t batch, int32_t Hs, int32_t Ws, int32_t subsampling, size_t* bytes);
int    lama_jpeg_scan_u8_fwd(void* stream, const uint8_t* image_hwc, const int32_t* sizes, int32_t Hs, int32_t Ws, int32_t batch, int32_t quality,
                             int32_t subsampling, uint8_t* out, size_t out_stride, int32_t* out_bytes, void* workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* LAMA_HIP_H */
