/*
 * xview_hip.h -- C ABI of libxview_hip.so: the MI355X (gfx950 / CDNA4) kernels behind the
 * two-stream FCN + probabilistic-fusion hot path of ethz-asl/modular_semantic_segmentation.
 *
 * The reference has NO native boundary for this path: every op below is a TensorFlow-1 graph
 * op reached through `sess.run` (xview/models/base_model.py:257-258,288-289,310-311).  Each
 * entry point therefore cites the reference graph call site it replaces; INTEGRATION.md shows
 * the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative XV_E* code for a bad argument, or a
 *     positive hipError_t from the launch; nothing throws, allocates or synchronises
 *   - all pointers are DEVICE pointers owned by the caller; `stream` is a hipStream_t
 *   - activations are bf16 "padded NHWC": a dense [N][H+2][W+2][C] buffer whose 1-pixel border is
 *     zero and is never written by any kernel (3x3 'same' convolutions read it as their zero
 *     padding; custom_layers.py:124-139 `padding='same'`).  `xv_act.data` points at the first
 *     element of the padded buffer.  Network inputs/outputs (images, probabilities, label maps)
 *     are dense unpadded NHWC / NHW tensors in the reference's dtypes (float32 / int64 / int32).
 */
#ifndef XVIEW_HIP_H
#define XVIEW_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "xview_augment.h"   /* xv_augment_plan, the record of xv_augment_batch */

#ifdef __cplusplus
extern "C" {
#endif

#define XV_OK 0
#define XV_EINVAL (-1)      /* bad argument (null pointer, non-positive size, ...)          */
#define XV_ESHAPE (-2)      /* shape not supported by the kernel (see each function)        */
#define XV_EWORKSPACE (-3)  /* workspace too small                                          */

/* padded-NHWC activation: dense [n][h+2][w+2][c], zero border, data -> padded origin.
 * dtype XV_BF16 (every entry point) or XV_FP8 (OCP e4m3fn, one byte per element; xv_conv2d_fwd* only, BASELINE
 * config "fp8 MFMA conv path"): a stored value q stands for q * 2^scale_exp (per-tensor power-of-two scale, 0 for
 * bf16).  Entry points other than the forward convolutions take bf16 maps only and return XV_EINVAL for an XV_FP8
 * descriptor (they would otherwise reinterpret one-byte elements as bf16).                                          */
#define XV_BF16 0
#define XV_FP8 1
typedef struct xv_act {
  void* data;
  int32_t n, h, w, c;
  int32_t dtype;
  int32_t scale_exp;
} xv_act;

/* Library version (major*10000 + minor*100 + patch). */
int xv_version(void);
/* Name of the gfx target the device code was compiled for ("gfx950"). */
const char* xv_arch(void);
/* First 16 hex digits of the sha256 over the sources this binary was compiled from (csrc/Makefile SRC_HASH);
 * the Python loader compares it with the sources next to it and refuses a stale library. */
const char* xv_source_hash(void);

/* ---- weight packing ------------------------------------------------------------------------
 * Conv kernels arrive in the reference npz schema: float32 HWIO [k][k][cin][cout]
 * (base_model.py:361-393 export_weights; tf.layers.conv2d kernel layout).  The MFMA kernels read
 * them as bf16 [tap][cin/64][cout][64 swizzled], 128 B per (tap, cin-chunk, cout) row with
 * 16-byte slot s of row `co` stored at slot s ^ (co & 6) (so a weight tile is a linear copy
 * into bank-conflict-free LDS).  For k = 3 a second image follows in the same buffer for the
 * 32-channel-chunk kernel: bf16 [tap][cin/32][cout][32], 64-byte rows, slot s of row `co` at
 * s ^ ((co >> 1) & 2); and a third for generations 4 / 5 and the fused first pair (16x16x32 MFMA blocks,
 * configurations 26-28): the same [tap][cin/32][row][32] with slot s of row r at s ^ ((r >> 1) & 2) and the rows of
 * every 64-row block permuted (row 16j + 4g + q = channel 16g + 4j + q, so that a lane's 16 accumulator registers of a
 * pixel are 16 consecutive output channels).  xv_packed_weight_bytes is the size of all three.
 * k = 1 or 3, cin % 64 == 0, cout % 64 == 0.                                                       */
size_t xv_packed_weight_bytes(int k, int cin, int cout);
int xv_pack_conv_weights(const float* w_hwio, void* packed, int k, int cin, int cout, void* stream);
/* Forward image and data-gradient image (xv_pack_conv_weights_dgrad) of one layer in a single launch: what a training
 * step does for every conv after the optimizer update.                                                               */
int xv_pack_conv_weights_pair(const float* w_hwio, void* packed, void* packed_dgrad, int k, int cin, int cout,
                              void* stream);

/* fp8 weights (config "fp8 MFMA conv path", vgg16.py:7-51 / custom_layers.py:124-139 call sites): OCP e4m3fn,
 * [tap][cin/128][cout][128] (128-byte rows, slots swizzled like the bf16 image: a weight tile has the same bytes
 * geometry), preceded by a 256-byte header whose first int32 is the per-tensor scale exponent e_w (stored value q
 * stands for q * 2^e_w; the kernel feeds it to the MFMA as a uniform E8M0 block scale).  Values are rounded to
 * nearest-even after the scaling and saturate at +-448.  For k = 3 a second image follows for the generation-4 kernel:
 * [tap][cin/64][row][64], 64-byte rows, slot s of row r at s ^ ((r >> 2) & 3), rows permuted as in the bf16 image;
 * with it cin % 64 == 0 suffices for k = 3 (the first image is left empty unless cin % 128 == 0).  k = 1: cin % 128 == 0.  cout % 64 == 0.                    */
size_t xv_packed_weight_bytes_f8(int k, int cin, int cout);
int xv_pack_conv_weights_f8(const float* w_hwio, void* packed, int k, int cin, int cout, int scale_exp, void* stream);

/* ---- conv2d forward ------------------------------------------------------------------------
 * y = act(conv(x, W) + b): tf.layers.conv2d(padding='same', strides 1) via
 * custom_layers.py:124-139 (call sites simple_fcn.py:39-79).  Implicit GEMM on bf16 MFMA
 * (v_mfma_f32_16x16x32_bf16, fp32 accumulate), input halo tile + weight tile staged in LDS.
 * k = 3 (conv1_2 .. conv5_3) or 1 (score_conv4 / score_conv5, AdapNet's block stages: a flat GEMM over the padded rows
 * from 256 input channels, conv1x1_gemm.hip); cin % 64 == 0, cout % 64 == 0.
 * Inference batch-norm is folded into (W, b) by the host before packing.
 * If pooled != NULL (k = 3 only, h and w even) the 2x2/2 max-pool of y
 * (max_pooling2d, simple_fcn.py:41,44,48,58) is written to `pooled` from the same accumulators;
 * y itself may then be NULL (data == NULL) to skip the full-resolution store.
 * fp8 (the dtype fields select it, no second entry point): x->dtype == XV_FP8 runs the block-scaled
 * v_mfma_scale_f32_16x16x128_f8f6f4 kernel (e4m3 operands, 128-channel chunks, fp32 accumulate; x->scale_exp and the
 * weight header's exponent go in as uniform E8M0 scales, so the accumulators are in real units) and needs weights
 * packed by xv_pack_conv_weights_f8 and cin % 128 == 0; y->dtype / pooled->dtype == XV_FP8 make the epilogue write
 * e4m3 (value * 2^-scale_exp, round-to-nearest-even, saturating at 448) from either kernel.  3x3 convs run on the
 * generation-4 kernel where it is ahead (configurations 24 / 25, conv_f8_dma.hip: v_mfma_scale_f32_32x32x64_f8f6f4 on
 * 64-channel e4m3 chunks, so cin % 64 == 0 suffices for k = 3; v_mfma_f32_32x32x16_bf16 for bf16 maps -- bf16 in / e4m3
 * out included; any map size, partial tiles by clamped DMA offsets and predicated stores): conv2_1 (64 input channels)
 * is an e4m3 convolution there.                                                                                  */
int xv_conv2d_fwd(const xv_act* x, const void* w_packed, const float* bias, const xv_act* y,
                  const xv_act* pooled, int k, int relu, void* stream);

/* The 3x3 conv of a conv -> batch norm block with the batch statistics taken in the conv's own epilogue (generation 4: bf16
 * maps that tile exactly in 16x32 pixels, cout <= 512): y = conv(x, W) + b as xv_conv2d_fwd(relu = 0), and row w of
 * stats_rows ([xv_conv2d_stats_rows()][2 cout] floats) = workgroup w's per-channel sum | sum of squares of the STORED
 * (bf16) outputs; xv_bn_sums_from_rows(stats_rows, xv_conv2d_stats_rows(), 2 cout, sums) adds the rows in a fixed tree and
 * leaves what xv_bn_stats would have.  Returns XV_ESHAPE where that kernel does not apply (use xv_conv2d_fwd + xv_bn_stats). */
int xv_conv2d_stats_rows(void);
int xv_conv2d_fwd_stats(const xv_act* x, const void* w_packed, const float* bias, const xv_act* y, float* stats_rows,
                        size_t stats_bytes, void* stream);
int xv_bn_sums_from_rows(const float* rows, int nrows, int len, double* sums, void* stream);

/* The routed pool of training (generation 4: bf16 maps that tile exactly in 16x32 pixels; XV_ESHAPE elsewhere -- keep the full
 * map and xv_maxpool2x2_bwd there).  Replaces, bit for bit, tf.layers.conv2d(relu) + max_pooling2d forward and
 * Conv2DBackpropInput + MaxPoolGrad + ReluGrad backward (simple_fcn.py:41,44,48 under base_model.py:153-162) without the
 * full-resolution map and without the pooled gradient in memory:
 *   xv_conv2d_fwd_route:      pooled = maxpool2x2(relu(conv3x3(x) + b)); route[n][h/2][w/2][cout] = one byte per pooled value:
 *                             0 = the window's maximum is not positive, else 0x80 >> the first position of the maximum
 *                             (row 0: columns 0, 1; row 1: columns 0, 1 -- MaxPoolGrad's order).
 *   xv_conv2d_bwd_data_route: dx (twice dy's size) = conv3x3(dy, Wd) stored through `route`: every value at the position its
 *                             byte names, zeros at the other three (every interior value of dx is written).
 * xv_conv2d_route_bytes(n, h, w, cout): size of the route buffer of a conv over [n][h][w] maps (0: bad dimensions).      */
size_t xv_conv2d_route_bytes(int n, int h, int w, int cout);
int xv_conv2d_fwd_route(const xv_act* x, const void* w_packed, const float* bias, const xv_act* pooled, void* route,
                        size_t route_bytes, void* stream);
int xv_conv2d_bwd_data_route(const xv_act* dy, const void* w_packed_dgrad, const float* zero_bias, const void* route,
                             size_t route_bytes, const xv_act* dx, void* stream);

/* Residual form for the 1x1 convs that close a ResNet block: y = act(conv1x1(x, W) + b) + residual
 * (block_a / block_b of adapnet.py:38-51,80-100: stage_3 carries its own relu, the block's outer relu is the identity
 * on the sum of two non-negative maps).                                                                               */
int xv_conv2d_fwd_residual(const xv_act* x, const void* w_packed, const float* bias, const xv_act* residual,
                           const xv_act* y, int relu, void* stream);

/* Dense transposed convolution: tf.layers.conv2d_transpose(filters, k, strides=s, padding='same', use_bias=False) with
 * an ARBITRARY kernel (custom_layers.py:71-121 `deconv2d`; the FCN's upscore layers are constants and take the
 * depthwise bilinear kernels below, a trained or imported non-bilinear kernel -- AdapNet trains its deconvs,
 * adapnet.py:156-163 -- takes this path), followed by the optional inference batch norm (scale / shift per channel),
 * the activation and a residual add:  y = act(deconv(x, W) * scale + shift) + residual.
 * k = 2s only ([4,4]/2 and [16,16]/8, every call site of the reference).  w_phases_packed: the kernel re-arranged by
 * the host into a 3x3 conv cin -> s*s*cout (one 2x2-tap sub-conv per output phase; custom_layers.
 * dense_deconv_as_conv3x3) and packed by xv_pack_conv_weights; zero_bias: s*s*cout zeros; workspace: the phase map.  */
size_t xv_deconv_dense_workspace_bytes(int n, int h, int w, int cout, int stride);
int xv_deconv_dense_fwd(const xv_act* x, const void* w_phases_packed, const float* zero_bias, const float* scale,
                        const float* shift, const xv_act* residual, const xv_act* y, int stride, int relu,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Tuning / test entry: the same op with an explicit tile configuration 0 <= cfg < xv_conv2d_num_cfgs()
 * (cfg < 0 = the library's own choice, i.e. xv_conv2d_fwd).  Results are bit-identical across
 * configurations; XV_ESHAPE if the configuration cannot tile this shape.                            */
int xv_conv2d_fwd_cfg(const xv_act* x, const void* w_packed, const float* bias, const xv_act* y,
                      const xv_act* pooled, int k, int relu, int cfg, void* stream);
/* The SAME 3x3 layer of TWO models in one launch: the two experts of a fusion model run identical layer shapes from conv1_2
 * on (basic_fusion_model.py:25-60 builds one fcn() per modality), each with its own maps, weights and bias.  The persistent
 * generation-4 / 5 kernel takes the concatenated tile lists, so the launch makes whole rounds of workgroups where each
 * expert alone leaves its last round half empty (conv4_x at 16 images of 768x384: 2 x 1152 tiles = 9 rounds of 256 CUs
 * against 2 x 5; conv5_x: 3 against 2 x 2).  Arguments per model as xv_conv2d_fwd (k = 3; y descriptors are required, their
 * data may be null with a pooled output); both models give the same set of outputs.  Results are bit-identical to two
 * xv_conv2d_fwd calls.  XV_ESHAPE -- nothing launched -- where the shape does not run on generation 4 / 5 (bf16 maps that
 * tile exactly in 16x32, or in 24x16 / 32x16 without a pooled output): launch the two convs separately then.          */
int xv_conv2d_fwd_pair(const xv_act* xa, const void* wa_packed, const float* bias_a, const xv_act* ya, const xv_act* pooled_a,
                       const xv_act* xb, const void* wb_packed, const float* bias_b, const xv_act* yb, const xv_act* pooled_b,
                       int relu, void* stream);
/* Stream-K tail of the generation-2 3x3 kernel (conv_dma_kernel).  A persistent grid walks (pixel patch, cout tile)
 * tiles round by round; when the last round is incomplete (conv4_x / conv5_x at 16 images: 4.5 / 1.5 rounds; one image:
 * fewer tiles than CUs from conv2 on) its (tile, 32-channel chunk) items are dealt out evenly over ALL workgroups, the
 * partial sums of a split tile meet in fp32 slabs of this workspace and the workgroup that arrives last adds them in
 * a fixed order (bitwise reproducible) and runs the epilogue.  `workspace`: xv_conv2d_streamk_workspace_bytes() bytes,
 * 16-byte aligned, ZERO when first used (the arrival counters; every launch leaves them zero again), owned by ONE
 * stream at a time (two experts on two streams need one each).  NULL = every tile whole (the plain entry points).
 * Same arguments and results otherwise as xv_conv2d_fwd_cfg / xv_conv2d_bwd_data; kernels other than generation 2
 * ignore the workspace.                                                                                               */
size_t xv_conv2d_streamk_workspace_bytes(void);
int xv_conv2d_fwd_ws(const xv_act* x, const void* w_packed, const float* bias, const xv_act* y, const xv_act* pooled,
                     int k, int relu, int cfg, void* workspace, size_t workspace_bytes, void* stream);
/* The forward conv with a workspace for the SPLIT form of the 24x16-tile kernel (round 5, batch-1 latency): where a layer's
 * whole tiles fill less than half the CUs AND its shape sums its input channels in chunk groups (maps that tile in 24x16 and
 * not in 16x32 with >= 256 input channels: conv5_x of a 768x384 input), every (tile, group) is a work item of its own that
 * leaves fp32 accumulators in the workspace, and a second launch adds the groups in order.  The unsplit launch of such a
 * layer adds the same groups in the same order in registers: identical bits at every batch size.
 * xv_conv2d_split_workspace_bytes: bytes this shape needs (0: it is never split; the call below then equals xv_conv2d_fwd_cfg).
 * The workspace belongs to the calling stream until the launch has completed.                                          */
size_t xv_conv2d_split_workspace_bytes(int n, int h, int w, int cin, int cout);
int xv_conv2d_fwd_split(const xv_act* x, const void* w_packed, const float* bias, const xv_act* y, const xv_act* pooled, int k,
                        int relu, int cfg, void* split_workspace, size_t split_workspace_bytes, void* stream);
int xv_conv2d_bwd_data_ws(const xv_act* dy, const void* w_packed_dgrad, const float* zero_bias, const xv_act* relu_ref,
                          const xv_act* addend, const xv_act* dx, int k, void* workspace, size_t workspace_bytes,
                          void* stream);
int xv_conv2d_num_cfgs(void);
/* The tile configuration the library would choose for this shape (what cfg < 0 resolves to), without launching anything:
 * host arithmetic only.  in_dtype / out_dtype: XV_BF16 | XV_FP8; flags: bit 0 = with a pooled output, bit 1 = the
 * data-gradient epilogue (addend / relu mask), bit 2 = with a stream-K workspace.  Returns the configuration index or
 * XV_ESHAPE / XV_EINVAL.                                                                                              */
int xv_conv2d_choose_cfg(int n, int h, int w, int cin, int cout, int k, int in_dtype, int out_dtype, int flags);

/* First layer: conv1_1 = relu(conv3x3(x) + b) on the RAW float32 network input (dense unpadded
 * NHWC, cin = 1..4; simple_fcn.py:39), fp32 weights HWIO [3][3][cin][64], fp32 math, bf16 out.
 * cin = 1 / 3 with w % 16 == 0 runs on the matrix cores with every fp32 operand split exactly into
 * three bf16 terms (fp32 accumulation; rounds like the fp32 FMA chain the other shapes use).        */
int xv_conv2d_first_fwd(const float* x, int n, int h, int w, int cin, const float* w_hwio,
                        const float* bias, const xv_act* y, int relu, void* stream);
/* AdapNet's block_0_1 written straight into the operand of block_0_2 (adapnet.py:126-127): the same values as
 * xv_conv2d_first_fwd + xv_gather_conv7s2, without the 64-channel full-resolution map in between.  cin = 1 or 3, w % 16 == 0,
 * h even; z [N,h/2,w/2,576] bf16, which must hold zeros where the gather has no source pixel (variant 1 of the last operand
 * row / column: neither this kernel nor xv_gather_conv7s2 writes anything else there).                                   */
int xv_conv2d_first_gather7s2_fwd(const float* x, int n, int h, int w, int cin, const float* w_hwio,
                                  const float* bias, const xv_act* z, int relu, void* stream);
/* conv1_1 AND conv1_2 (+ max_pooling2d) of the FCN trunk in one launch (simple_fcn.py:39-41), inference only: conv1_1 is
 * evaluated tile by tile straight into conv1_2's LDS patch buffers, so its 64-channel map never reaches memory.  x / w1_hwio
 * / b1 as xv_conv2d_first_fwd (cin = 1 or 3), w2_packed / b2 as xv_conv2d_fwd (64 -> 64 channels, 3x3); y and / or pooled
 * as xv_conv2d_fwd (either may be NULL or have NULL data).  Bit-identical to the two separate calls.  Maps that tile exactly
 * in 16x32 only: XV_ESHAPE otherwise (run the two kernels).
 * y / pooled may be e4m3 maps (XV_FP8, one scale for both: value * 2^-scale_exp, saturating at +-448): the first e4m3 map of
 * the fp8 graph, the same bytes as xv_conv2d_first_fwd + xv_conv2d_fwd onto e4m3 maps.                                  */
int xv_conv_first_pair_fwd(const float* x, int n, int h, int w, int cin, const float* w1_hwio, const float* b1, int relu1,
                           const void* w2_packed, const float* b2, int relu2, const xv_act* y, const xv_act* pooled,
                           void* stream);


/* 2x2 stride-2 'valid' max pooling (max_pooling2d, simple_fcn.py:41,44,48,58).                  */
int xv_maxpool2x2_fwd(const xv_act* x, const xv_act* y, void* stream);

/* y = relu(bilinear_x2(x)) [+ residual]: deconv2d(k=4, strides 2, 'same', constant bilinear
 * diagonal kernel) + relu, then tf.add_n with score_conv4 (custom_layers.py:8-25,71-121;
 * simple_fcn.py:82-85), computed as the depthwise 2x2-tap interpolation the diagonal kernel
 * collapses to.  residual may be NULL.                                                           */
int xv_upsample2x_relu_add(const xv_act* x, const xv_act* residual, const xv_act* y, void* stream);

/* The same with an inference batch norm between the deconv and its relu (deconv2d(..., batch_normalization=True),
 * custom_layers.py:112-119): y = relu(bilinear_x2(x) * scale[c] + shift[c]) [+ residual]; scale / shift float32 [C]
 * (gamma / sqrt(moving_variance + 1e-3), beta - moving_mean * scale), both NULL = no batch norm.                   */
int xv_upsample2x_affine_relu_add(const xv_act* x, const float* scale, const float* shift, const xv_act* residual,
                                  const xv_act* y, void* stream);

/* The general form: y = act(bilinear_x2(x) * scale[c] + shift[c]) [+ residual], relu = 0 for AdapNet's
 * first_deconvolution_upconv (deconv2d(activation=None, batch_normalization=True) then tf.add with the block-7
 * shortcut, adapnet.py:157-163).                                                                                      */
int xv_upsample2x_affine_act_add(const xv_act* x, const float* scale, const float* shift, const xv_act* residual,
                                 const xv_act* y, int relu, void* stream);

/* tf.layers.dropout(x, rate, training=True) at the MC-dropout sites of encoder / decoder (simple_fcn.py:50-62,71-78,
 * 124-126; enabled only by the uncertainty models, bayesian_fcn.py:74-89): y = x / (1 - rate) where a counter-based
 * random draw per element (a function of `seed` and the element index only) keeps it, else 0.  Not TensorFlow's random
 * stream: masks are reproducible per seed, not comparable with the reference's.                                    */
int xv_dropout(const xv_act* x, const xv_act* y, float rate, uint64_t seed, void* stream);

/* MC-dropout samples of one map (the variance fusion model, variance_mix.py:33-83): y holds num_samples + 1 slots of x's
 * n images, slot-major (y->n == (num_samples + 1) x->n); slot 0 = x, slot t = xv_dropout(x, rate, seed0 + (t-1) stride) bit
 * for bit (the hash takes the index within the slot; the whole padded slot is written).  The in-place form drops slots
 * 1 .. num_samples of y with the same seeds and leaves slot 0 as it is. */
int xv_dropout_samples(const xv_act* x, const xv_act* y, int num_samples, float rate, uint64_t seed0, uint64_t stride,
                       void* stream);
int xv_dropout_samples_inplace(const xv_act* y, int num_samples, float rate, uint64_t seed0, uint64_t stride, void* stream);

/* The same without the plain slot (the MC-dropout Bayesian FCN, bayesian_fcn.py:74-89, computes T samples and no plain
 * pass): y->n == num_samples x->n, slot t = xv_dropout(x, rate, seed0 + t stride) bit for bit, t = 0 .. num_samples-1.  The
 * in-place form drops every slot of y. */
int xv_dropout_samples_only(const xv_act* x, const xv_act* y, int num_samples, float rate, uint64_t seed0, uint64_t stride,
                            void* stream);
int xv_dropout_samples_only_inplace(const xv_act* y, int num_samples, float rate, uint64_t seed0, uint64_t stride,
                                    void* stream);

/* y = concat(a, b) along channels (tf.concat(axis=3) of the two trunks' conv4_3 / conv5_3, fusion_fcn.py:27-28). */
int xv_concat_channels(const xv_act* a, const xv_act* b, const xv_act* y, void* stream);

/* ---- gathers that map AdapNet's strided / dilated convs onto the stride-1 kernels above (adapnet.py:12-173) ----
 * xv_subsample2: y[i][j] = x[2i][2j], the input of a 1x1 stride-2 conv (block_a with strides 2, adapnet.py:39,45).
 * xv_gather_conv7s2: z [N,H/2,W/2,9C] such that the 7x7 stride-2 'same' conv of block_0_2 (adapnet.py:127) equals a 3x3
 *   stride-1 conv of z: group g = 3*rv + cv, variants (parity, shift) = (0,0), (0,1), (1,0) per axis,
 *   z[j][i][g] = x[2(j+sr)+pr][2(i+sc)+pc] (zero outside); the 7x7 tap k = 2(t+s)+p lands on 3x3 tap t.
 * xv_im2col_dilated_pair: z [N,H,W,18C], z[y][x][t] = x[y+ty*d][x+tx*d] with t = 0..8 at rate d1 and 9..17 at rate d2:
 *   the two atrous convs of block_b (adapnet.py:84-88) become one 1x1 conv whose output is their concatenation.     */
int xv_subsample2(const xv_act* x, const xv_act* y, void* stream);
int xv_gather_conv7s2(const xv_act* x, const xv_act* z, void* stream);
int xv_im2col_dilated_pair(const xv_act* x, int dilation1, int dilation2, const xv_act* z, void* stream);
/* The same two atrous convs + concat WITHOUT the 18C operand: an implicit GEMM over nine taps per output half, the taps
 * gathered by the kernel's own loads (adapnet.py:84-88: stage_2_1, stage_2_2, tf.concat).  wpk: the packed [1,1,18C,F] image
 * the materialised form's 1x1 conv takes (rows [0,9C) x columns [0,F/2) = conv 1, rows [9C,18C) x [F/2,F) = conv 2; the two
 * off-diagonal blocks are never read -- except F = 64, where both halves share a tile and all 18 taps are multiplied).  C a
 * multiple of 64, F of 256 or F = 64; y [N,H,W,F]; the same bits as xv_im2col_dilated_pair +
 * xv_conv2d_fwd(ksize 1).  XV_ESHAPE otherwise (callers then take the materialised form).                              */
int xv_conv_dilated_pair_fwd(const xv_act* x, const void* wpk, const float* bias, int dilation1, int dilation2, int relu,
                             const xv_act* y, void* stream);
/* The pair's gradients, also without the operand (training; adapnet.py:84-88 behind base_model.py:153-162).
 * xv_conv_dilated_pair_bwd_data: dx [N,H,W,C] = gradient of the pair's input from dy [N,H,W,F] (both halves): an implicit GEMM
 *   over 18 taps x F/2 channels; wpk_dgrad = the packed forward-format image (xv_pack_conv_weights) of the [1,1,18 F/2,C]
 *   kernel whose row (h * 9 + t) * F/2 + co holds k_h[t][:, co] of conv h; F and C multiples of 128.
 * xv_conv_dilated_pair_bwd_filter_ws: dw1 / dw2 (+=) = HWIO [3][3][C][F/2] gradients of the two kernels; the taps of x gathered
 *   by the kernel's loads, split-K slabs in the workspace (>= ..._workspace_bytes; 0 = shape not taken: C and F multiples of
 *   256) added in a fixed order -- bitwise reproducible.  XV_ESHAPE: callers take the im2col operand + the 1x1 entries.   */
int xv_conv_dilated_pair_bwd_data(const xv_act* dy, const void* wpk_dgrad, const float* zero_bias, int dilation1, int dilation2,
                                  const xv_act* dx, void* stream);
size_t xv_conv_dilated_pair_bwd_filter_workspace_bytes(int n, int h, int w, int c, int f);
int xv_conv_dilated_pair_bwd_filter_ws(const xv_act* x, const xv_act* dy, int dilation1, int dilation2, float* dw1, float* dw2,
                                       void* workspace, size_t workspace_bytes, void* stream);
/* Their transposes for the training graph (each destination element summed by one thread: deterministic), and the
 * residual add y = a + b of a block whose closing conv is followed by a batch norm (adapnet.py:38-51).             */
int xv_subsample2_bwd(const xv_act* dy, const xv_act* dx, void* stream);
int xv_gather_conv7s2_bwd(const xv_act* dz, const xv_act* dx, void* stream);
int xv_im2col_dilated_pair_bwd(const xv_act* dz, int dilation1, int dilation2, const xv_act* dx, void* stream);
int xv_add(const xv_act* a, const xv_act* b, const xv_act* y, void* stream);
/* Phase shuffles of AdapNet's two TRAINABLE transposed convs (adapnet.py:155-163 calls custom_layers.deconv2d:71-121
 * without trainable=False): a k = 2*stride conv2d_transpose is one 3x3 conv onto stride*stride*C phase channels at the
 * input resolution (xv_conv2d_fwd on the kernel custom_layers.dense_deconv_as_conv3x3 arranges) + a depth-to-space
 * shuffle; its filter / data gradients are xv_conv2d_bwd_filter / xv_conv2d_bwd_data of the space-to-depth shuffle of
 * the upstream gradient.  Phase channel (py*stride + px)*C + c <-> output pixel (stride*qy + py, stride*qx + px).
 *   xv_space_to_depth        g [N,s*H,s*W,C] -> out [N,H,W,s*s*C]                         (C % 8 == 0)
 *   xv_space_to_depth_dense  the same from a dense float32 [N,s*H,s*W,num_classes] gradient; out->c = s*s*Cp with
 *                            Cp % 8 == 0, Cp >= num_classes, the padding channels written as zeros
 *   xv_depth_to_space_dense  phase map z [N,H,W,s*s*Cp] -> dense float32 [N,s*H,s*W,num_classes], optional per-class
 *                            scale / shift (the inference batch norm of second_deconvolution_upconv)               */
int xv_space_to_depth(const xv_act* g, int stride, const xv_act* out, void* stream);
int xv_space_to_depth_dense(const float* g, int num_classes, int stride, const xv_act* out, void* stream);
int xv_depth_to_space_dense(const xv_act* z, int stride, int num_classes, const float* scale, const float* shift,
                            float* out, void* stream);
/* The float32 route of AdapNet's trained x8 score deconv (adapnet.py:155-163 computes the class scores in float32): the
 * padded bf16 map as a dense float32 one (exact), the 3x3 conv onto the 64 phases x Cp classes through xv_conv2d_f32 (fp32
 * matrix instruction), and the phases unshuffled from the dense float32 phase map [n][hq][wq][stride*stride*cp]
 * (cp a multiple of 4) [* scale + shift] -- no bf16 rounding between the deconv and the batch norm / softmax.          */
int xv_act_to_dense_f32(const xv_act* x, float* out, void* stream);
int xv_depth_to_space_dense_f32(const float* z, int n, int hq, int wq, int stride, int cp, int num_classes, const float* scale,
                                const float* shift, float* out, void* stream);

/* Decoder head: upscore = relu(bilinear_x8(fused)) (deconv2d k=16 s=8, simple_fcn.py:129-130),
 * score = conv1x1(upscore, Ws) + bs (no activation, simple_fcn.py:131-133), prob = softmax(score),
 * label = argmax(prob, 3) (basic_fusion_model.py:21-22 / simple_fcn.py:223-224), fp32 from the bf16 `fused`
 * features.  `fused` is non-negative by construction (a sum of two relu outputs) and the bilinear
 * weights are positive, so the relu is the identity and the linear x8 deconv and 1x1 conv commute: the
 * 1x1 conv runs at 1/8 resolution into `workspace` and C class scores are interpolated instead of U
 * features; the full-resolution U-channel tensor is never formed.
 * w_score: float32 [U][C] (HWIO of the 1x1 kernel), b_score: float32 [C], C <= 32, U % 8 == 0.
 * Outputs (each may be NULL): score / prob float32 [N][8h][8w][C], label int64 [N][8h][8w].
 * workspace: xv_decoder_head_workspace_bytes(n, h, w, C) bytes, 16-byte aligned (h, w of `fused`).      */
size_t xv_decoder_head_workspace_bytes(int n, int h, int w, int num_classes);
int xv_decoder_head_fwd(const xv_act* fused, const float* w_score, const float* b_score, int num_classes,
                        float* score, float* prob, int64_t* label, void* workspace, size_t workspace_bytes,
                        void* stream);

/* General decoder head for a batch norm with a non-zero shift between the x8 deconv and its relu (the default of
 * decoder() as called by fusion_fcn.py:38; custom_layers.py:112-119): upscore = relu(bilinear_x8(fused) * scale[u] +
 * shift[u]), then score / softmax / argmax as above.  The 1x1 conv no longer commutes with the interpolation, so
 * all U features are interpolated per pixel (16x the FMAs of xv_decoder_head_fwd; no workspace).
 * `label`, where given, is 16-byte aligned (labels leave in 16-byte pairs; XV_EINVAL otherwise), and n, h, w of `fused`
 * are positive (XV_ESHAPE otherwise); nothing is written when either check fails.                                  */
int xv_decoder_head_affine_fwd(const xv_act* fused, const float* scale, const float* shift, const float* w_score,
                               const float* b_score, int num_classes, float* score, float* prob, int64_t* label,
                               void* stream);

/* prob = softmax(score), label = argmax(prob) on a dense float32 [npix][C] score tensor
 * (tf.nn.softmax + tf.argmax, basic_fusion_model.py:21-22); lowest index wins ties.  prob / label
 * may be NULL.                                                                                    */
int xv_softmax_argmax(const float* score, int64_t npix, int num_classes, float* prob, int64_t* label,
                      void* stream);

/* ---- fusion --------------------------------------------------------------------------------
 * Bayes fusion of E experts' label maps (bayes_mix.py:12-58 + tf.argmax at :161):
 *   score[c] = sum_e loglik[e][label_e][c] + logprior[c],  fused = argmax_c score[c]
 * labels: E device pointers (host array of device pointers) to int64 [npix]; loglik: float32
 * [E][C][C] = log(1e-20 + cond_e) computed by the host in fp32; logprior float32 [C].
 * score_out (float32 [npix][C]) may be NULL.  E <= 4, C <= 32.                                     */
int xv_bayes_fuse(const int64_t* const* labels, int num_experts, const float* loglik, const float* logprior,
                  int num_classes, int64_t npix, int64_t* fused, float* score_out, void* stream);

/* Same decision through the C^2 lookup table of bayes_decision_matrix (bayes_mix.py:61-112;
 * experiments/timing.py:87-115): fused = lut[label_a][label_b], lut int64 [C][C].                  */
int xv_bayes_fuse_lut(const int64_t* label_a, const int64_t* label_b, const int64_t* lut, int num_classes,
                      int64_t npix, int64_t* fused, void* stream);

/* Dirichlet fusion of E experts' softmax vectors (dirichlet_mix.py:14-36,96-136):
 *   p_e <- p_e / sum(p_e);  L_e[c] = sum_k am1[e][c][k] * log(1e-20 + p_e[k]) - lognorm[e][c]
 *   fused_score[c] = sum_e L_e[c] + logprior[c];  label = argmax_c
 * am1: float32 [E][C][C] with am1[e][c][k] = sigma*A_e[k][c] - 1; lognorm: float32 [E][C] =
 * sum_k lgamma(sigma*A_e[k][c]) - lgamma(sum_k ...); logprior = log(1e-20 + prior) float32 [C].
 * probs: E device pointers to float32 [npix][C].  score_out may be NULL.  E <= 4, C <= 32.          */
int xv_dirichlet_fuse(const float* const* probs, int num_experts, const float* am1, const float* lognorm,
                      const float* logprior, int num_classes, int64_t npix, int64_t* fused, float* score_out,
                      void* stream);

/* Mean of the experts' probabilities then argmax (average_mix.py:18-21).                         */
int xv_average_fuse(const float* const* probs, int num_experts, int num_classes, int64_t npix,
                    int64_t* fused, void* stream);
/* variance_mix.py:7-15: fused = sum_e probs_e / (1e-20 + var_e) / sum_e 1 / (1e-20 + var_e) per pixel (variances: one float
 * per pixel and expert) -> its argmax (fused, optional) and the fused score itself (fused_score [npix][C], optional); the
 * fusion step of xv_variance_head_fwd, bit for bit. */
int xv_variance_fuse(const float* const* probs, const float* const* variances, int num_experts, int num_classes,
                     int64_t npix, int64_t* fused, float* fused_score, void* stream);

/* bayesian_fcn.py:48-57 (sampling_uncertainty) on materialised samples float [num_samples][npix][C]: mean_prob [npix][C] = the
 * mean over the samples, label = its argmax (lowest index on ties), entropy = H(mean) / ln C, cond_entropy = mean_t H(p_t) /
 * ln C with H(p) = -sum_c p_c ln(clip(p_c, 1e-10, 1)), variance = sum_c population variance over the samples (>= 0; exactly 0
 * for identical samples).  Every output is optional (null skips), at least one is needed; the reduction of
 * xv_mc_uncertainty_head_fwd, bit for bit. */
int xv_sampling_uncertainty(const float* samples, int num_samples, int num_classes, int64_t npix, int64_t* label,
                            float* mean_prob, float* entropy, float* cond_entropy, float* variance, void* stream);

/* ---- training: backward kernels and optimizers ---------------------------------------------------
 * These replace the gradient graph tf.train.{Adam,RMSProp,Adagrad}Optimizer.minimize(self.loss)
 * builds (base_model.py:153-162) over SimpleFCN's training graph (simple_fcn.py:200-214).
 * Activations and activation gradients are bf16 padded NHWC; weight gradients and optimizer
 * state are float32 in the reference's HWIO layout.  Gradient buffers are ACCUMULATED into
 * (callers zero them once per step).                                                               */

/* Packed weights of the data-gradient convolution: Wd[k*k-1-tap][co][ci] = W[tap][ci][co]
 * (xv_packed_weight_bytes(k, cout, cin) bytes).                                                     */
/* All kernels of a model in one launch (the re-pack after every optimizer step): `table_device` = n descriptors in DEVICE
 * memory; packed_dgrad may be NULL per entry.  Shapes as xv_pack_conv_weights / _dgrad (k in {1, 3}, cin, cout % 64 == 0). */
typedef struct xv_pack_desc {
  const float* w_hwio;
  void* packed;
  void* packed_dgrad;
  int32_t k, cin, cout, reserved;
} xv_pack_desc;
int xv_pack_conv_weights_multi(const xv_pack_desc* table_device, int n, void* stream);
/* hipMemsetAsync(p, 0, bytes) on `stream`: the step's own clear of its gradient / loss accumulators (no framework kernel). */
int xv_memset_zero(void* p, size_t bytes, void* stream);
int xv_pack_conv_weights_dgrad(const float* w_hwio, void* packed, int k, int cin, int cout, void* stream);

/* dx = (conv(dy, Wd) + addend) * (relu_ref > 0): Conv2DBackpropInput of tf.layers.conv2d, the AddN
 * where two gradient paths meet (addend, may be NULL) and the ReluGrad of the layer below
 * (relu_ref = that layer's forward output, may be NULL), fused in the forward MFMA kernel.
 * zero_bias: float32 [dx->c] zeros.                                                                */
int xv_conv2d_bwd_data(const xv_act* dy, const void* w_packed_dgrad, const float* zero_bias,
                       const xv_act* relu_ref, const xv_act* addend, const xv_act* dx, int k, void* stream);

/* dW[tap][cin][cout] += sum_pixels x[pix+tap][cin] * dy[pix][cout] (Conv2DBackpropFilter), on MFMA with
 * transposing LDS reads; dbias[cout] += sum_pixels dy (BiasAddGrad; may be NULL).  k = 1 or 3,
 * cin % 64 == 0, cout % 64 == 0.  fp32 atomics: summation order is not fixed run to run.            */
int xv_conv2d_bwd_filter(const xv_act* x, const xv_act* dy, float* dw_hwio, float* dbias, int k, void* stream);
/* Same with a workspace of xv_conv2d_bwd_filter_workspace_bytes(n, h, w, cin, cout, k) bytes: the split-K
 * partial sums go to per-split slabs with plain stores and are added into dw by a second kernel in a fixed
 * order -- bitwise reproducible and faster than the fp32 atomics (~1.3 TB/s) for 3x3 layers with at least four
 * 64x64 channel-block pairs; smaller layers keep the atomics (the slabs would be all reduce and no compute). */
size_t xv_conv2d_bwd_filter_workspace_bytes(int n, int h, int w, int cin, int cout, int k);
int xv_conv2d_bwd_filter_ws(const xv_act* x, const xv_act* dy, float* dw_hwio, float* dbias, int k,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Test / tuning switch for the 3x3 filter-gradient kernel: 1 = register-staged tiles, two 4-wave workgroups
 * per CU; 2 = LDS-DMA double-buffered tiles, one 8-wave workgroup per CU (round 5's default); 3 (default) = the
 * same tiles with four loader waves beside four compute waves that walk the halo rows (three X fragments per
 * row serve all nine taps); 0 = back to the default, 3.  Same sums, equal on integers; the fp32 summation order
 * differs between the variants.                                                                      */
int xv_set_wgrad_variant(int variant);

/* dbias[c] += sum over all pixels of dy[.., c] (BiasAddGrad).                                        */
int xv_bias_grad(const xv_act* dy, float* dbias, void* stream);

/* conv1_1: dW[3][3][cin][64] += sum_pixels x[pix+tap][cin] * dy[pix][:] on the raw float32 input, and
 * dbias[64] += sum_pixels dy (may be NULL).                                                         */
int xv_conv2d_first_bwd_filter(const float* x, int n, int h, int w, int cin, const xv_act* dy, float* dw_hwio,
                               float* dbias, void* stream);
/* The same with per-workgroup partial sums in `workspace` (xv_conv2d_first_bwd_filter_workspace_bytes) and a fixed-order
 * reduce instead of fp32 atomics: bitwise reproducible.  dbias must not be NULL.  NULL workspace = the plain form.       */
size_t xv_conv2d_first_bwd_filter_workspace_bytes(int n, int h, int w, int cin);
int xv_conv2d_first_bwd_filter_ws(const float* x, int n, int h, int w, int cin, const xv_act* dy, float* dw_hwio,
                                  float* dbias, void* workspace, size_t workspace_bytes, void* stream);

/* MaxPoolGrad + ReluGrad: dy = dpooled routed to the first maximum of each 2x2 window, zero where y <= 0. */
int xv_maxpool2x2_bwd(const xv_act* y, const xv_act* dpooled, const xv_act* dy, void* stream);

/* ReluGrad: out = ref > 0 ? g : 0.                                                                 */
int xv_relu_bwd(const xv_act* g, const xv_act* ref, const xv_act* out, void* stream);

/* Gradient of fused = s4 + relu(bilinear_x2(s5)) w.r.t. s5 (through score_conv5's own relu).       */
int xv_upsample2x_bwd(const xv_act* dfused, const xv_act* s5, const xv_act* ds5, void* stream);

/* count += #pixels with 0 <= label < C  (the denominator of utils.py:52).                          */
int xv_count_valid_labels(const int32_t* labels, int num_classes, int64_t npix, int64_t* count, void* stream);

/* S = fused . Ws at 1/8 resolution into a zero-bordered float32 [N][h+2][w+2][CM] buffer, CM = C rounded up
 * to 4: the first half of the decoder head in its commuted form (see xv_decoder_head_fwd).          */
int xv_score_lowres(const xv_act* fused, const float* w_score, int num_classes, float* S, void* stream);

/* Fused head of a two-expert fusion model: both experts' low-resolution class scores (xv_score_lowres of each `fused`
 * map) -> per-pixel x8 bilinear logits + bias -> each expert's softmax / argmax (basic_fusion_model.py:21-22) -> Bayes
 * fusion of the two labels (mode 0; bayes_mix.py:33-58,161: tab = loglik [2][C][C]) or Dirichlet fusion of the two
 * probability vectors (mode 1; dirichlet_mix.py:14-36,96-136: tab = alpha-1 [2][C][C], lognorm [2][C]) -> the fused
 * label map int64 [n][8hi][8wi], and nothing else: no per-pixel intermediate reaches HBM.  Same arithmetic, term for
 * term, as xv_decoder_head_fwd + xv_bayes_fuse / xv_dirichlet_fuse (bit-identical labels).                        */
int xv_fused_head_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n, int hi, int wi,
                      int num_classes, int mode, const float* tab, const float* lognorm, const float* logprior,
                      int64_t* fused_label, void* stream);

/* Grid-scoring form of the Dirichlet fused head (experiments/different_evaluation_parameters.py:10-61 on one pass of the
 * trunks): Sa, Sb, biases, n, hi, wi, num_classes as xv_fused_head_fwd takes them; num_points parameter sets G, each as that
 * function's mode 1 takes one: tab float [G][2][C][C] (alpha-1), lognorm [G][2][C], logprior [G][C].  Every output pixel is
 * fused under all G sets -- the label of point g is the one xv_fused_head_fwd gives with point g's tables, bit for bit -- and
 * cm int64 [G][C][C] (rows = ground truth) counts it as xv_confusion_matrix would against labels int32 [n][8hi][8wi]:
 * accumulated, not cleared; no label map is written.  max_workgroups bounds the grid (0: the kernel's own bound).  XV_EINVAL
 * for a null pointer, num_classes < 2, num_points < 1 or num_points above xv_fused_head_grid_capacity(num_classes).        */
int xv_fused_head_grid_score_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n, int hi,
                                 int wi, int num_classes, int num_points, const float* tab, const float* lognorm,
                                 const float* logprior, const int32_t* labels, int64_t* cm, int max_workgroups, void* stream);

/* Most parameter sets one xv_fused_head_grid_score_fwd launch takes at this class count (its tables and counters share one
 * workgroup's LDS): at least 16 at 12 classes, at least 1 at 32; 0 outside 2..32 classes.  No GPU call.                    */
int xv_fused_head_grid_capacity(int num_classes);

/* Joint label histogram of a two-expert Bayes fusion: both experts' labels as xv_fused_head_fwd's mode 0 takes them
 * (bits of xv_decoder_head_fwd's label) -> hist int64 [C][C][C], hist[label][a][b] += 1 over the pixels with 0 <= label < C
 * (labels int32 [n][8hi][8wi], 16-byte aligned): accumulated, not cleared.  A Bayes-fused label is a function of (a, b)
 * alone, so the histogram gives the confusion matrix of every class prior on the host.  XV_EINVAL for a null pointer,
 * num_classes < 2 or num_classes > 20 (the counters of one workgroup: 32 KB of LDS).                                        */
int xv_fused_head_joint_hist_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n, int hi,
                                 int wi, int num_classes, const int32_t* labels, int64_t* hist, int max_workgroups,
                                 void* stream);

/* The joint histogram per GROUP of images: arguments as xv_fused_head_joint_hist_fwd, group int32 [n] in DEVICE memory, hist
 * int64 [num_groups][C][C][C]: hist[group[i]][label][a][b] += 1 with the experts' labels a, b bit for bit those of the
 * ungrouped call (group g's slice is that call on g's images alone; the sum over the groups is that call on all of them);
 * accumulated, not cleared.  Each workgroup handles one image at a time and flushes once per image; an id outside
 * [0, num_groups) counts nothing.  XV_EINVAL as xv_fused_head_joint_hist_fwd (2..20 classes, labels 16-byte aligned), and for
 * a null or misaligned group / hist or num_groups < 1.                                                                       */
int xv_fused_head_joint_hist_grouped_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n,
                                         int hi, int wi, int num_classes, const int32_t* labels, const int32_t* group,
                                         int num_groups, int64_t* hist, int max_workgroups, void* stream);

/* Fused average head of a two-expert fusion model (average_mix.py:18-21): Sa, Sb, biases, n, hi, wi, num_classes as
 * xv_fused_head_fwd takes them -> per output pixel both experts' softmax (bits of xv_decoder_head_fwd's prob), their sum
 * halved, and its first-maximum argmax -> fused_label int64 [n][8hi][8wi] (16-byte aligned): the labels of two
 * xv_decoder_head_fwd with prob + xv_average_fuse, bit for bit, without the two probability maps.  XV_EINVAL for a null or
 * misaligned pointer, num_classes outside 1..32 or a width 8 wi a thread's pixel group does not divide.                      */
int xv_fused_head_average_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n, int hi,
                              int wi, int num_classes, int64_t* fused_label, void* stream);

/* Fused head of a fusion model with TWO TO FOUR experts: S and bias are host arrays of num_experts device pointers (as
 * xv_bayes_fuse takes `labels`), S[e] float32 [n][hi+2][wi+2][CP] from xv_score_lowres of expert e (16-byte aligned), bias[e]
 * float32 [C]; the pointers travel in the kernel arguments, nothing is staged in device memory.  Per output pixel every
 * expert's softmax / argmax (bits of xv_decoder_head_fwd's prob / label), the experts in ascending order, then
 *   mode 0, Bayes:     tab = loglik float32 [E][C][C], logprior [C]: the label of xv_bayes_fuse on the E label maps;
 *   mode 1, Dirichlet: tab = alpha - 1 float32 [E][C][C], lognorm [E][C], logprior [C]: the label of xv_dirichlet_fuse on
 *                      the E probability maps;
 *   mode 2, mean:      tab, lognorm, logprior ignored (may be NULL): the label of xv_average_fuse on the E probability maps
 * -> fused_label int64 [n][8hi][8wi] (16-byte aligned), bit for bit, without the E label or probability maps.  For two
 * experts the labels are those of xv_fused_head_fwd / xv_fused_head_average_fwd.  XV_EINVAL, with nothing launched and the
 * output untouched, for num_experts outside 2..4, num_classes outside 2..32, an unknown mode, non-positive sizes, or a null
 * or misaligned pointer the mode needs.                                                                                      */
int xv_fused_head_multi_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi, int wi,
                            int num_classes, int mode, const float* tab, const float* lognorm, const float* logprior,
                            int64_t* fused_label, void* stream);

/* Counting form of xv_fused_head_multi_fwd: S, bias, num_experts (2..4), n, hi, wi, num_classes (2..32) and mode as that
 * function takes them; num_points parameter sets G:
 *   mode 0, Bayes:     tab [E][C][C] shared by all points (the log-likelihoods do not depend on the prior), logprior [G][C];
 *   mode 1, Dirichlet: tab [G][E][C][C] (alpha - 1), lognorm [G][E][C], logprior [G][C];
 *   mode 2, mean:      no tables (may be NULL), num_points must be 1.
 * Every output pixel is fused under all G sets -- fused_g is the label xv_fused_head_multi_fwd writes with point g's tables,
 * bit for bit -- and counted against labels int32 [n][8hi][8wi] as xv_confusion_matrix would: cm int64
 * [num_groups][G][C][C] (rows = ground truth), cm[group[i]][g][label][fused_g] += 1 over the pixels with 0 <= label < C.
 * expert_cm (may be NULL) int64 [num_groups][E][C][C]: expert_cm[group[i]][e][label][l_e] += 1 with l_e the label
 * xv_decoder_head_fwd gives expert e.  Both are accumulated, not cleared; no label map is written.  group (may be NULL, then
 * num_groups must be 1) int32 [n] in DEVICE memory as xv_fused_head_joint_hist_grouped_fwd takes it: a workgroup handles one
 * image at a time and flushes once per image, an id outside [0, num_groups) counts nothing, group g's slice is the ungrouped
 * call on g's images alone.  max_workgroups bounds the grid (0: the kernel's own bound).  XV_EINVAL, with nothing launched and
 * the outputs untouched, for num_experts outside 2..4, num_classes outside 2..32, an unknown mode, num_points < 1, above
 * xv_fused_head_multi_count_capacity or not 1 in mode 2, non-positive sizes, max_workgroups < 0, num_groups < 1 (or not 1
 * without group), or a null or misaligned pointer the mode needs.                                                          */
int xv_fused_head_multi_count_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi, int wi,
                                  int num_classes, int mode, int num_points, const float* tab, const float* lognorm,
                                  const float* logprior, const int32_t* labels, const int32_t* group, int num_groups,
                                  int64_t* cm, int64_t* expert_cm, int max_workgroups, void* stream);

/* Most parameter sets one xv_fused_head_multi_count_fwd launch takes (tables and counters share 40 KB of one workgroup's LDS
 * beside the expert counters, which always keep their room): 12 for 12 classes, four experts, Dirichlet; at least 1 up to 32
 * classes and four experts in every mode, within the same 40 KB; 1 in mode 2; 0 outside the supported ranges.  No GPU call. */
int xv_fused_head_multi_count_capacity(int num_classes, int num_experts, int mode);

/* ---- expert-agreement tables (csrc/agreement.hip) --------------------------------------------------------------------------
 * What the confusion matrices above cannot say: where the experts disagree, whom the fusion follows, what it loses and what it
 * rescues.  For E experts (2..4) and C classes (2..32), for every pixel with 0 <= label < C:
 *   mask       bit e is set iff expert e's label equals the ground truth (0 .. 2^E - 1);
 *   unanimous  1 iff all E experts give the same label, else 0;
 *   outcome    0 = the fused label equals the ground truth, 1 = it is wrong and equals at least one expert's label, 2 = it is
 *              wrong and equals no expert's label;
 *   table[group][label][mask][unanimous][outcome] += 1, table int64 [num_groups][C][2^E][2][3], accumulated, not cleared.
 * Cells that cannot occur stay zero (unanimous = 1 with a mask other than 0 or 2^E - 1; mask = 2^E - 1 with unanimous = 0).
 *
 * From the experts' low-resolution scores, in one launch: S, bias, num_experts, n, hi, wi, num_classes and mode as
 * xv_fused_head_multi_count_fwd takes them, with ONE parameter set: mode 0 (Bayes) tab [E][C][C], logprior [C]; mode 1
 * (Dirichlet) tab [E][C][C] (alpha - 1), lognorm [E][C], logprior [C]; mode 2 (mean) no tables (may be NULL).  Per output pixel
 * every expert's label is the one xv_decoder_head_fwd gives it and the fused label the one xv_fused_head_multi_fwd writes,
 * both bit for bit; no label or probability map is written.  labels int32 [n][8hi][8wi].  group (may be NULL, then num_groups
 * must be 1) int32 [n] in DEVICE memory: a workgroup handles one image at a time and flushes once per image with one 64-bit
 * atomic per non-zero cell, an id outside [0, num_groups) counts nothing, group g's slice is the ungrouped call on g's images
 * alone.  max_workgroups bounds the grid (0: the kernel's own bound, two workgroups per CU and never above 512).  XV_EINVAL,
 * with nothing launched and table untouched, for num_experts outside 2..4, num_classes outside 2..32, an unknown mode,
 * non-positive sizes, max_workgroups < 0, num_groups < 1 (or not 1 without group), or a null or misaligned pointer the mode
 * needs (S[e] 16 bytes; table 8; the others their element).                                                                */
int xv_fused_head_multi_agreement_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi, int wi,
                                      int num_classes, int mode, const float* tab, const float* lognorm,
                                      const float* logprior, const int32_t* labels, const int32_t* group, int num_groups,
                                      int64_t* table, int max_workgroups, void* stream);

/* The same table from MATERIALISED maps, for every model the fused heads do not serve: labels int32 [n][ppi] (n images of ppi
 * pixels each), expert_labels a host array of num_experts device pointers to int64 [n][ppi] (as xv_bayes_fuse takes `labels`),
 * fused int64 [n][ppi], group int32 [n] in device memory or NULL.  The same layout, grouping rule, bounds and refusals as
 * above (XV_EINVAL also for n or ppi below 1); the grid is one workgroup per CU and never above 512.  Only comparisons of the
 * map values enter a cell's index, so a map value outside [0, C) is counted as a label no class equals.                     */
int xv_agreement_table(const int32_t* labels, const int64_t* const* expert_labels, int num_experts, const int64_t* fused,
                       const int32_t* group, int n, int64_t ppi, int num_classes, int num_groups, int64_t* table,
                       void* stream);

/* ---- calibration scoring (csrc/calibration.hip) ------------------------------------------------------------------------------
 * Can the confidence of a posterior be believed?  For a pixel with class scores s[k], k < C (2..32), in the log domain -- the
 * fused score xv_bayes_fuse / xv_dirichlet_fuse write to score_out; for the mean ln(1e-20 + mean_e p_e[k]); for one expert its
 * logits -- `win` is the first maximum of s (the label the existing route writes; a temperature never moves it) and, per
 * temperature T > 0,
 *   z = sum_k exp((s[k] - s[win]) / T), conf = 1 / z (IEEE divisions), q = (uint32)(conf 2^24) (truncation, q <= 2^24),
 *   bin = min(q >> (24 - bin_bits), NB - 1) with NB = 1 << bin_bits, correct = (win == label),
 *   nll_pixel = min(ln z - (s[label] - s[win]) / T, -ln 1e-10)                       (the clip of xv_uncertainty_stats).
 * Over the pixels with 0 <= label < C: table int64 [num_groups][num_temperatures][NB][3], table[g][t][bin] += (1, correct, q),
 * and nll double [num_groups][num_temperatures] += nll_pixel; both accumulated, not cleared.  The three columns are integers:
 * groups, ranks and repeated launches add exactly; the mean confidence of a bin is its q sum / count / 2^24.
 *
 * xv_calibration_capacity: temperatures one launch serves with num_tables tables per temperature (1: the fusion alone; 1 + E:
 * the experts' tables beside it) in one workgroup's 160 KB of LDS, of which 20 KB stay with the fusion tables: a cell is 16
 * bytes (the q sum is 64 bits wide), a table 16 NB bytes and 256 bytes of NLL sums, and a launch takes at most 16 temperatures:
 * min(16, 140 KB / (num_tables (16 NB + 256))).  0 for bin_bits outside 4..10 or num_tables outside 1..5.  No GPU call.       */
int xv_calibration_capacity(int bin_bits, int num_tables);

/* The table from a MATERIALISED map: values float32 [n][ppi][C] (n images of ppi pixels each; 4-byte aligned), kind 0 = class
 * scores, kind 1 = probabilities, mapped to ln(1e-20 + p) after `win` is taken as their first maximum; labels int32 [n][ppi];
 * group (may be NULL, then num_groups must be 1) int32 [n] in DEVICE memory; temperatures a HOST array of num_temperatures
 * floats.  A workgroup handles one image at a time and flushes once per image with one 64-bit atomic per non-zero column of a
 * non-empty bin; an id outside [0, num_groups) counts nothing; group g's slice is the ungrouped call on g's images alone; the
 * grid is two workgroups per CU and never above 512.  XV_EINVAL, with nothing launched and the outputs untouched, for bin_bits
 * outside 4..10, num_temperatures < 1 or above xv_calibration_capacity(bin_bits, 1), a temperature that is not finite and
 * positive, num_classes outside 2..32, an unknown kind, n or ppi below 1, num_groups < 1 (or not 1 without group), or a null
 * or misaligned pointer (table and nll 8 bytes; the others their element).                                                    */
int xv_calibration_table(const float* values, int kind, const int32_t* labels, const int32_t* group, int n, int64_t ppi,
                         int num_classes, const float* temperatures, int num_temperatures, int bin_bits, int num_groups,
                         int64_t* table, double* nll, void* stream);

/* The table from the experts' low-resolution scores, in one launch: S, bias, num_experts (2..4), n, hi, wi, num_classes, mode
 * (0 Bayes, 1 Dirichlet, 2 mean), tab, lognorm, logprior, labels, group, num_groups and max_workgroups as
 * xv_fused_head_multi_agreement_fwd takes them, one parameter set.  The fused scores are those of the fusion kernels on the
 * maps xv_decoder_head_fwd writes, `win` the label xv_fused_head_multi_fwd writes.  expert_table int64
 * [num_groups][E][num_temperatures][NB][3] and expert_nll double [num_groups][E][num_temperatures] (both NULL, or both given)
 * take each expert's own table from its interpolated logits at the same temperatures.  No label, score or probability map is
 * written.  XV_EINVAL, with nothing launched and every output untouched, as above (the capacity is that of 1 + E tables with
 * expert_table) and as xv_fused_head_multi_agreement_fwd refuses.                                                             */
int xv_fused_head_multi_calibration_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi, int wi,
                                        int num_classes, int mode, const float* tab, const float* lognorm,
                                        const float* logprior, const int32_t* labels, const int32_t* group, int num_groups,
                                        const float* temperatures, int num_temperatures, int bin_bits, int64_t* table,
                                        double* nll, int64_t* expert_table, double* expert_nll, int max_workgroups,
                                        void* stream);

/* ---- confidence maps (csrc/confidence.hip) -----------------------------------------------------------------------------------
 * The confidence the calibration tables count, handed out per pixel.  For class scores s[k], k < C (2..32), in the log domain
 * and their first maximum `win`, as the calibration section takes them, at ONE temperature T > 0:
 *   d_k = (s[k] - s[win]) / T, e_k = exp(d_k), z = sum_k e_k (ascending k), conf = 1 / z           (the statements of the tables)
 *   entropy = max(0, ln z - (sum_k e_k d_k) / z)   in nats; a term with e_k = 0 adds nothing
 *   margin  = conf - (max_{k != win} e_k) / z      in [0, 1]; 0 where the maximum is tied
 *   label   = conf < threshold ? void_label : win  threshold 0: nothing is void
 * (uint32)(conf 2^24) of a written confidence is exactly the q of xv_calibration_table on the same scores.  Outputs: label_out
 * int64 (8-byte aligned), conf_out, entropy_out, margin_out float32 (4-byte aligned), one entry per pixel; each may be NULL and
 * is then not touched; at least one is given.  A thread takes one pixel; the grid is eight 256-thread workgroups per CU at most.
 *
 * xv_confidence_map, from a MATERIALISED map: values float32 [n][ppi][C] (4-byte aligned), kind 0 = class scores, kind 1 =
 * probabilities, mapped to ln(1e-20 + p) after `win` is taken as their first maximum.  XV_EINVAL, with nothing launched and
 * every output untouched, for a temperature that is not finite and positive, a threshold that is not finite or outside [0, 1],
 * num_classes outside 2..32, an unknown kind, n or ppi below 1, all four outputs NULL, or a null or misaligned pointer.       */
int xv_confidence_map(const float* values, int kind, int n, int64_t ppi, int num_classes, float temperature, float threshold,
                      int64_t void_label, int64_t* label_out, float* conf_out, float* entropy_out, float* margin_out,
                      void* stream);

/* The same maps from the experts' low-resolution scores, in one launch: S, bias, num_experts (2..4), n, hi, wi, num_classes,
 * mode (0 Bayes, 1 Dirichlet, 2 mean), tab, lognorm and logprior as xv_fused_head_multi_calibration_fwd takes them; outputs
 * [n][8 hi][8 wi].  The fused scores are those of the fusion kernels on the maps xv_decoder_head_fwd writes; with threshold 0
 * label_out is the label xv_fused_head_multi_fwd writes, bit for bit.  No probability or score map is written.  XV_EINVAL, with
 * nothing launched and every output untouched, as above (hi or wi below 1 too) and as xv_fused_head_multi_agreement_fwd
 * refuses its experts, mode and tables.                                                                                        */
int xv_fused_head_multi_confidence_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi, int wi,
                                       int num_classes, int mode, const float* tab, const float* lognorm,
                                       const float* logprior, float temperature, float threshold, int64_t void_label,
                                       int64_t* label_out, float* conf_out, float* entropy_out, float* margin_out,
                                       void* stream);

/* ---- uncertainty benchmarks of a posterior (csrc/confidence_stats.hip) ------------------------------------------------------
 * The counting form of the confidence maps: per pixel conf, entropy and margin as above, and three metrics, larger = less
 * certain, each one IEEE float32 operation from a written map value, in this order:
 *   entropy, least_confidence = 1.0f - conf, small_margin = 1.0f - margin.
 * hist uint64 [3][2][octaves << mantissa_bits]: hist[metric][row][bin(value)] += 1, bin as xv_uncertainty_stats bins a metric
 * (values at or below 2^(1 - octaves) share bin 0: with 24 octaves the resolution of 1 - conf in float32).  fixed_row = -1:
 * row = (win != label) over the pixels with 0 <= label < C; fixed_row 0 or 1: that row for every pixel, and labels may be
 * NULL.  With labels (int32, one per pixel), over the valid pixels, nll double [C]: nll[label] += nll_pixel of the calibration
 * section at this temperature, and counts int64 [C]: counts[label] += 1.  Everything is accumulated, nothing cleared, no
 * per-pixel map written.  The grid is two 512-thread workgroups per CU and never above 512; a workgroup counts in 32-bit LDS
 * cells and flushes once, one 64-bit atomic per non-zero cell.
 *
 * xv_confidence_stats, from a MATERIALISED map: values, kind, n, ppi and num_classes as xv_confidence_map takes them.
 * XV_EINVAL, with nothing launched and every table untouched, as xv_confidence_map refuses those and the temperature, for
 * mantissa_bits outside 3..8, octaves outside 8..32, fixed_row outside {-1, 0, 1}, NULL labels with fixed_row = -1, NULL hist,
 * NULL nll or counts with labels, a misaligned pointer (the tables 8 bytes, labels 4), or one table (the histograms and, with
 * labels, 16 C bytes) above 64 KB.                                                                                             */
int xv_confidence_stats(const float* values, int kind, int n, int64_t ppi, int num_classes, float temperature,
                        const int32_t* labels, int mantissa_bits, int octaves, int fixed_row, uint64_t* hist, double* nll,
                        int64_t* counts, void* stream);

/* The same tables from the experts' low-resolution scores, in one launch: S, bias, num_experts (2..4), n, hi, wi, num_classes,
 * mode, tab, lognorm and logprior as xv_fused_head_multi_confidence_fwd takes them, and its fused scores; labels int32
 * [n][8 hi][8 wi].  expert_hist uint64 [E][3][2][bins], expert_nll double [E][C] and expert_counts int64 [E][C] (all NULL, or
 * all given) take every expert's own tables from its interpolated logits, row = (that expert's label != label), as
 * xv_fused_head_multi_calibration_fwd takes expert tables.  XV_EINVAL as above and as xv_fused_head_multi_confidence_fwd
 * refuses its experts, mode and tables, for a partial set of expert outputs, and where the 1 + E tables and the staged fusion
 * tables pass 160 KB.                                                                                                           */
int xv_fused_head_multi_confidence_stats_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi,
                                             int wi, int num_classes, int mode, const float* tab, const float* lognorm,
                                             const float* logprior, float temperature, const int32_t* labels,
                                             int mantissa_bits, int octaves, int fixed_row, uint64_t* hist, double* nll,
                                             int64_t* counts, uint64_t* expert_hist, double* expert_nll,
                                             int64_t* expert_counts, void* stream);

/* ---- label-tuple heads (csrc/tuple_lut.hip)----------------------------------------------------------------------------------
 * For a fusion that sees a pixel only through the tuple of its experts' labels (IBCC: modular_semantic_segmentation_amd/ibcc.py).
 * S, bias, num_experts (2..4), n, hi, wi and num_classes (2..32) as xv_fused_head_multi_fwd takes them.  The tuple index of a
 * pixel is t = ((l_0 C + l_1) C + l_2) ..., expert 0 most significant, T = C^E tuples -- the row-major index of a [C]*E
 * decision array -- where l_e is the label xv_decoder_head_fwd gives expert e for that pixel, bit for bit.
 *
 * xv_tuple_capacity: 1 if the three entry points below serve this pair, else 0; no GPU call.  A pair is served when the T
 * 32-bit counters of the histogram, which stages nothing else, fit the 160 KB of one workgroup's LDS: T <= 40 960 -- every
 * class count for two and three experts, up to 14 classes for four.                                                          */
int xv_tuple_capacity(int num_classes, int num_experts);

/* hist int64 [num_groups][T] (8-byte aligned): hist[group[i]][t] += 1 for EVERY output pixel of image i -- no ground truth
 * enters; accumulated, not cleared.  group (may be NULL, then num_groups must be 1) int32 [n] in DEVICE memory: a workgroup
 * counts one image at a time in its LDS and flushes once per image with one 64-bit atomic per non-zero cell, an id outside
 * [0, num_groups) counts nothing, group g's slice is the ungrouped call on g's images alone.  max_workgroups bounds the grid
 * (0: the kernel's own bound, two workgroups per CU and never above 512).  XV_EINVAL, with nothing launched and hist
 * untouched, for a null or misaligned pointer, num_experts outside 2..4, num_classes outside 2..32, non-positive sizes,
 * max_workgroups < 0, num_groups < 1 (or not 1 without group); XV_ESHAPE where xv_tuple_capacity is 0.                        */
int xv_fused_head_multi_tuple_hist_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi, int wi,
                                       int num_classes, const int32_t* group, int num_groups, int64_t* hist,
                                       int max_workgroups, void* stream);

/* lut uint8 [T] in device memory (4-byte aligned), staged once per workgroup in LDS -> fused_label int64 [n][8hi][8wi]
 * (16-byte aligned) = lut[t]; alignment rules and store shape of xv_fused_head_multi_fwd.  Refusals as above.               */
int xv_fused_head_multi_lut_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi, int wi,
                                int num_classes, const uint8_t* lut, int64_t* fused_label, void* stream);

/* Counting form of xv_fused_head_multi_lut_fwd: labels int32 [n][8hi][8wi], cm int64 [num_groups][C][C] (rows = ground
 * truth), cm[group[i]][label][lut[t]] += 1 over the pixels with 0 <= label < C; accumulated, not cleared; no label map is
 * written.  A table entry outside [0, C) counts nothing.  group, num_groups, max_workgroups and the refusals as
 * xv_fused_head_multi_tuple_hist_fwd.                                                                                       */
int xv_fused_head_multi_lut_count_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi, int wi,
                                      int num_classes, const uint8_t* lut, const int32_t* labels, const int32_t* group,
                                      int num_groups, int64_t* cm, int max_workgroups, void* stream);

/* Counting form of the fused average head: cm int64 [C][C] (rows = ground truth), cm[label][fused] += 1 over the pixels with
 * 0 <= label < C (labels int32 [n][8hi][8wi], 16-byte aligned) as xv_confusion_matrix would count xv_fused_head_average_fwd's
 * labels: accumulated, not cleared; no label map is written.  max_workgroups bounds the grid (0: the kernel's own bound).
 * XV_EINVAL as xv_fused_head_average_fwd, and for max_workgroups < 0.                                                        */
int xv_fused_head_average_count_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n, int hi,
                                    int wi, int num_classes, const int32_t* labels, int64_t* cm, int max_workgroups,
                                    void* stream);

/* Variance head of the MC-dropout fusion model (variance_mix.py:7-15,33-83): Sa / Sb = xv_score_lowres of each expert's
 * (T+1) n-image map (slot 0 plain, slots 1..T dropout samples; T = num_samples) -> per output pixel and expert the softmax of
 * every pass, the variance over the T samples averaged over the classes, and the certainty-weighted fusion of the plain
 * passes' probabilities -> label int64 [n][8hi][8wi].  Optional (null skips): fused_score float [n][8hi][8wi][C], probs
 * float [2][n][8hi][8wi][C] (the plain passes' softmax, bits of xv_decoder_head_fwd's prob), variance float [2][n][8hi][8wi]. */
int xv_variance_head_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n, int hi, int wi,
                         int num_classes, int num_samples, int64_t* label, float* fused_score, float* probs, float* variance,
                         void* stream);

/* Uncertainty head of the MC-dropout Bayesian FCN (bayesian_fcn.py:48-57, custom_layers.py:251-256): S = xv_score_lowres of
 * the T n-image map of one expert, sample-major (images t n .. t n + n-1 are sample t = 0 .. T-1, T = num_samples; no plain
 * slot) -> per output pixel the softmax of every sample (bits of xv_decoder_head_fwd's prob) and from them label int64
 * [n][8hi][8wi] = argmax of the mean and, optional (null skips): mean_prob float [n][8hi][8wi][C], entropy, cond_entropy,
 * variance float [n][8hi][8wi] as xv_sampling_uncertainty defines them.  XV_EINVAL for num_samples < 1, num_classes < 2 or a
 * null label. */
int xv_mc_uncertainty_head_fwd(const float* S, const float* bias, int n, int hi, int wi, int num_classes, int num_samples,
                               int64_t* label, float* mean_prob, float* entropy, float* cond_entropy, float* variance,
                               void* stream);

/* Scoring form of the uncertainty head (uncertainty_model.py; experiments/uncertainty_eval.py:18-52,62-88): S, bias, n, hi, wi,
 * num_classes, num_samples as xv_mc_uncertainty_head_fwd takes them; every interpolated logit is multiplied by inv_temperature
 * before the softmax (custom_layers.py:239-248; 1.0f gives the bits of that head).  The pixel's entropy, cond_entropy and
 * variance are binned as xv_uncertainty_stats bins a metric, into hist uint64 [3][2][octaves << mantissa_bits] in that order,
 * row = (argmax of the mean != label) over the pixels with 0 <= label < C (fixed_row = -1), or row fixed_row (0 or 1) for
 * every pixel; labels int32 [n][8hi][8wi] (may be null with a fixed row) also feed nll double [C], nll[label] -=
 * ln(clip(mean[label], 1e-10, 1)), and counts int64 [C] over the valid pixels.  All three are accumulated, not cleared; no
 * per-pixel map is written.  XV_EINVAL for num_classes < 2, mantissa_bits outside 3..8, octaves outside 8..32, or tables that
 * do not fit a workgroup's LDS (more than 64 KB for one copy). */
int xv_mc_uncertainty_score_fwd(const float* S, const float* bias, int n, int hi, int wi, int num_classes, int num_samples,
                                float inv_temperature, const int32_t* labels, int mantissa_bits, int octaves, int fixed_row,
                                uint64_t* hist, double* nll, int64_t* counts, void* stream);

/* ---- uncertainty-weighted Dirichlet fusion (uncertainty_dirichlet_mix.py) ---------------------------------------------
 * Dropout of the network input, whole pixels at a time (noise_shape [N,H,W,1]): x dense float [n][h][w][cin]; y holds
 * plain + num_samples slots of it, slot-major: slot 0 a copy of x when plain == 1, sample t = 0 .. num_samples-1 with ONE
 * Bernoulli(1 - rate) draw per pixel from (seed0 + t stride, index of the pixel within its slot), shared by the pixel's
 * channels; kept pixels are x * (1 / (1 - rate)) in fp32.  A mask depends on the seed and the pixel alone.  num_samples = 1,
 * plain = 0 is the single pass.  x and y must not overlap; a slot holds fewer than 2^31 - 2^19 elements. */
int xv_dropout_pixels_samples(const float* x, int n, int h, int w, int cin, float* y, int num_samples, int plain, float rate,
                              uint64_t seed0, uint64_t stride, void* stream);

/* Moments pass: Sa / Sb as xv_variance_head_fwd takes them ((T+1) n images each, slot 0 plain, T = num_samples) -> mvar float
 * [2][n][8hi][8wi], per expert the population variance of each class's probability over the T samples averaged over the
 * classes (the bits of xv_variance_head_fwd's variance), and vmax float [2], per expert the largest per-class variance over
 * every pixel, class and image of the call.  vmax is cleared here. */
int xv_uncertainty_moments(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n, int hi, int wi,
                           int num_classes, int num_samples, float* mvar, float* vmax, void* stream);

/* Fusion head: the plain slots of Sa / Sb -> per expert p = softmax (bits of xv_decoder_head_fwd's prob), mix = mvar / vmax
 * (0 where vmax is 0), alpha[j][c] = params[e][j][c] (1 - mix) + mix (1 + delta_jc), ll[c] = sum_j (alpha[j][c] - 1)
 * log(1e-20 + p[j] / sum p) + lgamma(sum_j alpha[j][c]) - sum_j lgamma(alpha[j][c]); score = ll_0 + ll_1 + logprior; label
 * int64 [n][8hi][8wi] = its argmax (lowest index on ties).  params float [2][C][C], logprior float [C].  Optional (null
 * skips): fused_score float [n][8hi][8wi][C], probs float [2][n][8hi][8wi][C], mix float [2][n][8hi][8wi]. */
int xv_uncertainty_dirichlet_head_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n, int hi,
                                      int wi, int num_classes, const float* mvar, const float* vmax, const float* params,
                                      const float* logprior, int64_t* label, float* fused_score, float* probs, float* mix,
                                      void* stream);

/* The same fusion on materialised tensors of TWO experts: probs two device pointers to float [npix][C], mvar float [2][npix],
 * vmax float [2] -> fused int64 [npix] and / or fused_score float [npix][C] (either may be null); the per-pixel step of
 * xv_uncertainty_dirichlet_head_fwd, bit for bit. */
int xv_uncertainty_dirichlet_fuse(const float* const* probs, const float* mvar, const float* vmax, const float* params,
                                  const float* logprior, int num_classes, int64_t npix, int64_t* fused, float* fused_score,
                                  void* stream);

/* One expert's per-class uncertainties float [npix][C] (non-negative) -> mvar float [npix], their mean over the classes, and
 * vmax float [1], their maximum over every pixel and class.  vmax is cleared here. */
int xv_uncertainty_weights(const float* uncertainty, int num_classes, int64_t npix, float* mvar, float* vmax, void* stream);

/* Loss and head backward (simple_fcn.py:212-214, utils.py:43-53) in the same commuted form: recomputes
 * score = bilinear_x8(fused . Ws) + bs, adds -sum(onehot*log_softmax)/(1e-20+count) to *loss, accumulates
 * d(score kernel) [U][C] and d(score bias) [C], and writes dfused = d(loss)/d(fused) (bf16 padded NHWC; the
 * relu masks below `fused` are applied by the callers' next kernels).  valid_count must already hold the
 * batch's count.  workspace: xv_decoder_head_bwd_workspace_bytes(n, h, w, C) bytes, 16-byte aligned (the padded
 * 1/8-resolution scores, the row-weighted column sums of the score gradient -- the dense gradient is never stored --
 * and one slab of score-weight partial sums per 256 low-resolution pixels, reduced in a fixed order).
 * Shapes: U = fused->c a multiple of 8, U <= 256, C <= 32, and with CM = C rounded up to 4 the slab kernel's LDS need
 * (U CM + 256 CM) 4 + 512 U bytes must fit 160 KB (U = 256: C <= 16; C = 32: U <= 200; every U <= 128 fits every C).
 * Anything else returns XV_ESHAPE before the first launch: loss, dw_score, db_score and dfused are untouched.   */
size_t xv_decoder_head_bwd_workspace_bytes(int n, int h, int w, int num_classes);
int xv_decoder_head_bwd(const xv_act* fused, const float* w_score, const float* b_score, const int32_t* labels,
                        const int64_t* valid_count, int num_classes, double* loss, float* dw_score,
                        float* db_score, const xv_act* dfused, void* workspace, size_t workspace_bytes,
                        void* stream);

/* [TF1] optimizers on flat float32 buffers; grad_scale multiplies the gradient first (1/world_size).
 * Adam: m,v updated, p -= lr_t*m/(sqrt(v)+eps) with lr_t = lr*sqrt(1-b2^t)/(1-b1^t) from the host.
 * RMSProp: ms = decay*ms+(1-decay)g^2 (ms initialised to 1), p -= lr*g/sqrt(ms+eps).
 * Adagrad: a += g^2 (a initialised to 0.1), p -= lr*g/sqrt(a).                                      */
int xv_adam_step(float* param, const float* grad, float* m, float* v, int64_t n, float lr_t, float beta1,
                 float beta2, float eps, float grad_scale, void* stream);
int xv_rmsprop_step(float* param, const float* grad, float* ms, int64_t n, float lr, float decay, float eps,
                    float grad_scale, void* stream);
int xv_adagrad_step(float* param, const float* grad, float* accum, int64_t n, float lr, float grad_scale,
                    void* stream);

/* ---- statistics ----------------------------------------------------------------------------
 * Dirichlet sufficient statistics (dirichlet_mix.py:142-163): for every pixel with 0 <= label < C
 *   S[label][k] += log(1e-10 + prob[k]),  counts[label] += 1
 * S: float64 [C][C] (accumulated, not zeroed), counts: int64 [C] (accumulated).  labels int32.     */
int xv_dirichlet_suffstats(const float* prob, const int32_t* labels, int num_classes, int64_t npix,
                           double* S, int64_t* counts, void* stream);

/* Confusion matrix (base_model.py:136-151): cm[label][pred] += 1 for 0 <= label < C (negative
 * labels are the dropped (C+1)-th row); cm int64 [C][C], accumulated, rows = ground truth.         */
int xv_confusion_matrix(const int32_t* labels, const int64_t* pred, int num_classes, int64_t npix,
                        int64_t* cm, void* stream);
/* The same per GROUP of images (experiments/evaluation.py:42-55 scores once per sequence; a bootstrap over images needs a
 * matrix per image): labels int32 / pred int64 [n][ppi] (n images of ppi pixels each), group int32 [n] in DEVICE memory,
 * cm int64 [num_groups][C][C]: cm[group[i]][label][pred] += 1 over the pixels xv_confusion_matrix counts, accumulated, not
 * cleared; summed over the groups it is xv_confusion_matrix of the same maps.  A workgroup counts one image at a time in its
 * LDS and flushes with one atomic per non-zero cell; an image whose id is outside [0, num_groups) counts nothing.  The same
 * class counts as xv_confusion_matrix (XV_ESHAPE beyond 64).  XV_EINVAL for a null pointer, n, ppi or num_groups below 1, or
 * a pointer that is not aligned to its element.                                                                              */
int xv_confusion_matrix_grouped(const int32_t* labels, const int64_t* pred, const int32_t* group, int n, int64_t ppi,
                                int num_classes, int num_groups, int64_t* cm, void* stream);
/* Uncertainty benchmarks on materialised maps (uncertainty_model.py): metric float [npix] (one uncertainty map), pred int64
 * [npix], labels int32 [npix].  hist uint64 [2][bins], bins = octaves << mantissa_bits: hist[row][bin(metric)] += 1 with
 * row = (pred != label) over the pixels with 0 <= label < C (fixed_row = -1), or row fixed_row (0 or 1) for EVERY pixel (pred
 * and labels may then be null).  bin(v) comes from the float's bits: v <= 0 -> 0, NaN -> bins - 1, else
 * (bits(v) >> (23 - mantissa_bits)) - ((128 - octaves) << mantissa_bits) clamped to [0, bins - 1].  mean_prob float [npix][C]
 * (optional; needs labels): nll double [C], nll[label] -= ln(clip(mean_prob[label], 1e-10, 1)), counts int64 [C] += 1, over
 * the valid pixels; null leaves nll / counts untouched.  Everything is accumulated, not cleared.  XV_EINVAL for C < 2,
 * mantissa_bits outside 3..8, octaves outside 8..32, or tables beyond 64 KB of LDS. */
int xv_uncertainty_stats(const float* metric, const int64_t* pred, const int32_t* labels, const float* mean_prob,
                         int num_classes, int64_t npix, int mantissa_bits, int octaves, int fixed_row, uint64_t* hist,
                         double* nll, int64_t* counts, void* stream);
/* Label maps on their way to the host (predict(), base_model.py:279-288): int64 labels in [0, 256) -> one byte per pixel,
 * out[i] = (uint8) labels[i].  The pipelined host boundary sends this image over PCIe (an eighth of the bytes) and widens it
 * to the reference's np.int64 while it fills the result array.  labels 16-byte, out 8-byte aligned.                       */
int xv_narrow_labels(const int64_t* labels, int64_t n, uint8_t* out, void* stream);

/* ---- training-mode batch normalisation -----------------------------------------------------------
 * tf.layers.batch_normalization(training=True) between a conv / deconv and its activation
 * (custom_layers.py:112-119,124-139): per-channel statistics over (N, H, W), normalisation with the biased batch
 * variance, [TF1] epsilon 1e-3 and momentum 0.99 (moving variance fed the unbiased estimate), and its gradient.
 * z: pre-normalisation conv output, y: post-relu output (relu mask of the backward; NULL = no activation).
 * sums: double [2*C] scratch (zeroed inside).  C in {64, 128, 256, 512, ...}: C/8 must divide 256.              */
int xv_bn_stats(const xv_act* z, double* sums, void* stream);
int xv_bn_finalize(const double* sums, int channels, int64_t count, const float* gamma, const float* beta, float eps,
                   float momentum, float* moving_mean, float* moving_var, float* mean, float* invstd, float* scale,
                   float* shift, void* stream);
/* xv_bn_sums_from_rows + xv_bn_finalize, and xv_bn_stats_ws + xv_bn_finalize, with the row sums and the per-channel results
 * in ONE launch (one workgroup per channel; `sums` is left as the two-call form leaves it, bit for bit).  Single-process
 * statistics only: a data-parallel run all-reduces `sums` between the two calls and keeps them.                        */
int xv_bn_finalize_from_rows(const float* rows, int nrows, int channels, int64_t count, const float* gamma, const float* beta,
                             float eps, float momentum, float* moving_mean, float* moving_var, float* mean, float* invstd,
                             float* scale, float* shift, double* sums, void* stream);
int xv_bn_stats_finalize_ws(const xv_act* z, double* sums, void* workspace, size_t workspace_bytes, const float* gamma,
                            const float* beta, float eps, float momentum, float* moving_mean, float* moving_var, float* mean,
                            float* invstd, float* scale, float* shift, void* stream);
int xv_bn_apply(const xv_act* z, const float* scale, const float* shift, int relu, const xv_act* y, void* stream);
/* dz = gamma*invstd*(g - mean(g) - zhat*mean(g*zhat)), g = dy*(y>0); dgamma += sum g*zhat, dbeta += sum g.      */
int xv_bn_bwd(const xv_act* dy, const xv_act* y, const xv_act* z, const float* mean, const float* invstd,
              const float* gamma, double* sums, float* dgamma, float* dbeta, const xv_act* dz, void* stream);
/* The gradient in two steps for data-parallel callers (Sync-BN): xv_bn_bwd_reduce fills `sums` with the LOCAL
 * sum g / sum g*zhat and adds them into dgamma / dbeta; the caller may all-reduce `sums`; xv_bn_bwd_apply then forms
 * dz from `sums` and `count` (the global N*H*W).                                                                    */
int xv_bn_bwd_reduce(const xv_act* dy, const xv_act* y, const xv_act* z, const float* mean, const float* invstd,
                     double* sums, float* dgamma, float* dbeta, void* stream);
int xv_bn_bwd_apply(const xv_act* dy, const xv_act* y, const xv_act* z, const float* mean, const float* invstd,
                    const float* gamma, const double* sums, int64_t count, const xv_act* dz, void* stream);
/* The same two steps for a batch norm FOLLOWED BY A RELU, the mask recomputed from z (z * scale + shift > 0, the forward
 * pass's own expression: scale / shift as xv_bn_finalize left them) instead of read from the activation map: a third / a
 * quarter less HBM traffic.  64 <= C, C divides 2048.                                                                    */
int xv_bn_bwd_reduce_zmask(const xv_act* dy, const xv_act* z, const float* mean, const float* invstd, const float* scale,
                           const float* shift, double* sums, float* dgamma, float* dbeta, void* workspace,
                           size_t workspace_bytes, void* stream);
/* y = relu(z * scale + shift) and pooled = maxpool2x2(y) in one pass; y may be a NULL-data descriptor (only the pooled map is
 * written: the training step recomputes y from z in xv_bn_pool_bwd_*).  64 <= C, C divides 2048; h, w even.               */
int xv_bn_apply_pool(const xv_act* z, const float* scale, const float* shift, const xv_act* y, const xv_act* pooled,
                     void* stream);
/* The batch-norm gradient of a conv -> batch norm -> relu -> 2x2 max-pool block straight from the gradient of the POOLED map:
 * each pass recomputes the window's activations from z, routes the pooled gradient to the first positive maximum
 * (xv_maxpool2x2_bwd's rule on the same values) and reduces / applies -- no routed-gradient map in HBM.  count = n h w of z
 * (x ranks under Sync-BN); workspace as in the _ws forms below (may be NULL).                                            */
int xv_bn_pool_bwd_reduce(const xv_act* dpooled, const xv_act* z, const float* mean, const float* invstd, const float* scale,
                          const float* shift, double* sums, float* dgamma, float* dbeta, void* workspace,
                          size_t workspace_bytes, void* stream);
int xv_bn_pool_bwd_apply(const xv_act* dpooled, const xv_act* z, const float* mean, const float* invstd, const float* scale,
                         const float* shift, const float* gamma, const double* sums, int64_t count, const xv_act* dz,
                         void* stream);
/* Workspace forms of the reductions: with a workspace of xv_bn_workspace_bytes(C) bytes (16-byte aligned, owned by one
 * stream) every workgroup writes its partial sums to its own row and a second kernel adds the rows in a fixed tree --
 * bitwise reproducible statistics and gamma / beta gradients; workspace == NULL: f64 atomics in arrival order (the
 * forms without _ws).                                                                                                   */
size_t xv_bn_workspace_bytes(int channels);
int xv_bn_stats_ws(const xv_act* z, double* sums, void* workspace, size_t workspace_bytes, void* stream);
int xv_bn_bwd_reduce_ws(const xv_act* dy, const xv_act* y, const xv_act* z, const float* mean, const float* invstd,
                        double* sums, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
int xv_bn_dense_stats_ws(const float* z, int64_t rows, int channels, double* sums, void* workspace, size_t workspace_bytes,
                         void* stream);
int xv_bn_dense_bwd_reduce_ws(const float* dy, const float* z, int64_t rows, int channels, const float* mean,
                              const float* invstd, double* sums, float* dgamma, float* dbeta, void* workspace,
                              size_t workspace_bytes, void* stream);
int xv_bn_bwd_apply_zmask(const xv_act* dy, const xv_act* z, const float* mean, const float* invstd, const float* scale,
                          const float* shift, const float* gamma, const double* sums, int64_t count, const xv_act* dz,
                          void* stream);

/* The batch norm BEHIND the x8 deconv without its input in memory: `low` is the deconv's input (padded bf16, 64 .. 2048
 * channels), the normalised map is z = bilinear_x8(low) rounded to bf16 -- exactly what xv_upsample_raw_fwd(low, 8) would
 * store -- recomputed per element in the four passes that would read it back (custom_layers.py:112-119 behind
 * simple_fcn.py:117-119 in training).  Same results, bit for bit, as the entry points without `_ups8` on the stored map.      */
int xv_bn_stats_finalize_ups8_ws(const xv_act* low, double* sums, void* workspace, size_t workspace_bytes, const float* gamma,
                                 const float* beta, float eps, float momentum, float* moving_mean, float* moving_var, float* mean,
                                 float* invstd, float* scale, float* shift, void* stream);
/* (round 6) the statistics pass alone, for data-parallel runs: sums[c] = sum z, sums[C + c] = sum z^2 over the recomputed map;
 * the caller all-reduces `sums` and finalises with xv_bn_finalize on the global pixel count.                                   */
int xv_bn_stats_ups8_ws(const xv_act* low, double* sums, void* workspace, size_t workspace_bytes, void* stream);
int xv_bn_apply_ups8(const xv_act* low, const float* scale, const float* shift, int relu, const xv_act* y, void* stream);
/* ... the forward apply pass FUSED with the dense score conv behind it: y (as xv_bn_apply_ups8 with relu) and score = y . W + b
 * (as xv_score_dense_fwd) in one launch -- 64 units, at most 16 classes; XV_ESHAPE elsewhere.                                  */
int xv_score_dense_fwd_ups8(const xv_act* low, const float* scale, const float* shift, const float* w_score,
                            const float* b_score, int num_classes, const xv_act* y, float* score, void* stream);
int xv_bn_bwd_reduce_zmask_ups8(const xv_act* dy, const xv_act* low, const float* mean, const float* invstd, const float* scale,
                                const float* shift, double* sums, float* dgamma, float* dbeta, void* workspace,
                                size_t workspace_bytes, void* stream);
int xv_bn_bwd_apply_zmask_ups8(const xv_act* dy, const xv_act* low, const float* mean, const float* invstd, const float* scale,
                               const float* shift, const float* gamma, const double* sums, int64_t count, const xv_act* dz,
                               void* stream);
/* The same on a dense float32 [rows][C] tensor, C <= 32 (the batch norm on `score`, simple_fcn.py:131-133).        */
int xv_bn_dense_stats(const float* z, int64_t rows, int channels, double* sums, void* stream);
int xv_bn_dense_apply(const float* z, int64_t rows, int channels, const float* scale, const float* shift, float* y,
                      void* stream);
int xv_bn_dense_bwd(const float* dy, const float* z, int64_t rows, int channels, const float* mean, const float* invstd,
                    const float* gamma, double* sums, float* dgamma, float* dbeta, float* dz, void* stream);
int xv_bn_dense_bwd_reduce(const float* dy, const float* z, int64_t rows, int channels, const float* mean,
                           const float* invstd, double* sums, float* dgamma, float* dbeta, void* stream);
int xv_bn_dense_bwd_apply(const float* dy, const float* z, int64_t rows, int channels, const float* mean,
                          const float* invstd, const float* gamma, const double* sums, int64_t count, float* dz,
                          void* stream);

/* ---- un-commuted training head (batch norm between the x8 deconv and its relu) ---------------------
 * y = bilinear_x{2,8}(x) with no activation (deconv2d with the constant kernel, custom_layers.py:8-25,71-110) and its
 * transpose; score = u . Ws + bs per full-resolution pixel (dense float32 [N*H*W][C]); softmax cross-entropy over the
 * labelled pixels with the loss normalised by *valid_count (models/utils.py:43-53); gradients of the score conv.   */
int xv_upsample_raw_fwd(const xv_act* x, int factor, const xv_act* y, void* stream);
int xv_upsample_raw_bwd(const xv_act* dy, int factor, const xv_act* dx, void* stream);
/* The x8 gradient through per-block sums in a workspace (xv_upsample_raw_bwd_workspace_bytes(n, h, w, c) for the LOW-resolution
 * map [n][h][w][c]): every element of dy is read once instead of from four source pixels' 16x16 footprints.  Same sums in
 * another (fixed) order.  factor 2 or workspace == NULL: xv_upsample_raw_bwd.                                              */
size_t xv_upsample_raw_bwd_workspace_bytes(int n, int h, int w, int c);
int xv_upsample_raw_bwd_ws(const xv_act* dy, int factor, const xv_act* dx, void* workspace, size_t workspace_bytes, void* stream);
int xv_score_dense_fwd(const xv_act* u, const float* w_score, const float* b_score, int num_classes, float* score,
                       void* stream);
int xv_softmax_ce_dense(const float* logits, const int32_t* labels, const int64_t* valid_count, int num_classes,
                        int64_t npix, double* loss, float* dlogits, void* stream);
/* The same with the batch norm's affine on the scores applied inside (logits = scores * scale + shift, the expression of
 * xv_bn_dense_apply; scale == shift == NULL: plain logits): the normalised scores never go to HBM.                      */
int xv_softmax_ce_dense_affine(const float* scores, const float* scale, const float* shift, const int32_t* labels,
                               const int64_t* valid_count, int num_classes, int64_t npix, double* loss, float* dlogits,
                               void* stream);
/* The same with the loss added up in a FIXED order: every workgroup leaves its partial sum in `ws` (at least
 * xv_softmax_ce_dense_workspace_bytes(npix) bytes, 8-byte aligned, owned by the calling stream) and a second one-workgroup
 * launch adds them to *loss -- bit for bit the same loss on every run (the two entries above add the partials with a double
 * atomic in arrival order: equal to ~1e-16 relative).  ws == NULL: the arrival-order form.  scale == shift == NULL: plain
 * logits.                                                                                                               */
size_t xv_softmax_ce_dense_workspace_bytes(int64_t npix);
int xv_softmax_ce_dense_ws(const float* scores, const float* scale, const float* shift, const int32_t* labels,
                           const int64_t* valid_count, int num_classes, int64_t npix, double* loss, float* dlogits, void* ws,
                           size_t ws_bytes, void* stream);
int xv_score_dense_bwd(const xv_act* u, const float* dscore, const float* w_score, int num_classes, float* dw_score,
                       float* db_score, const xv_act* du, void* stream);
/* The same with the filter and bias gradients added in a FIXED order (64 units, at most 16 classes -- the matrix-core form):
 * every workgroup leaves its partial sums in `workspace` (xv_score_dense_bwd_workspace_bytes(n, h, w) bytes, 16-byte aligned),
 * two small launches add them onto dw_score / db_score -- bitwise reproducible from run to run (the entry above adds them by
 * fp32 atomics in arrival order).  workspace == NULL: that form.                                                          */
size_t xv_score_dense_bwd_workspace_bytes(int n, int h, int w);
int xv_score_dense_bwd_ws(const xv_act* u, const float* dscore, const float* w_score, int num_classes, float* dw_score,
                          float* db_score, const xv_act* du, void* workspace, size_t workspace_bytes, void* stream);

/* ---- "exact" mode (conv_dtype='fp32'): the FCN trunk in plain float32 on dense UNPADDED NHWC maps -- the reference
 * graph's own arithmetic type (tf.layers.conv2d / max_pooling2d / conv2d_transpose on float32: simple_fcn.py:39-87,
 * custom_layers.py:71-139), no bf16 storage.  The convs run on the fp32 matrix instruction (v_mfma_f32_32x32x2_f32: bit for
 * bit a k-ordered fmaf chain, at the fp32 vector rate = 1/16 of the bf16 MFMA rate); the mode exists so that label maps
 * EQUAL to the fp32 oracle's on trained weights are a product mode and not only a test (basic_fusion_model.py:21-22).
 *   xv_conv2d_f32             y = [relu](conv_kxk_same(x, w_hwio) + bias), k in {1, 3}, any channel counts and map sizes
 *   xv_conv2d_f32_pool        the same; y and / or the 2x2 max-pooled map (h, w even) written from the accumulators
 *                             (max_pooling2d fused, simple_fcn.py:41-63); y == NULL or pooled == NULL skips that output
 *   xv_conv2d_f32_scalar      round 4's kernel (fp32 FMAs on the vector ALU): the A/B baseline of the bench record
 *   xv_maxpool2x2_f32         2x2 / stride 2
 *   xv_upsample2x_f32         y = relu(bilinear_x2(x)) [+ residual]            (upscore_conv5 + add_score)
 *   xv_score_lowres_f32       S[n][i+1][j+1][k] = fused[n][i][j][:] . Ws[:][k] into the zero-bordered [N][h+2][w+2][CP]
 *                             buffer (CP = num_classes rounded up to 4) that xv_decoder_head_from_scores reads
 *   xv_decoder_head_from_scores  x8 bilinear interpolation of S + bias -> score / prob / label (the second half of
 *                             xv_decoder_head_fwd; also serves the bf16 path's S)                                       */
int xv_conv2d_f32(const float* x, int n, int h, int w, int cin, const float* w_hwio, const float* bias, int k, int cout,
                  int relu, float* y, void* stream);
int xv_conv2d_f32_pool(const float* x, int n, int h, int w, int cin, const float* w_hwio, const float* bias, int k, int cout,
                       int relu, float* y, float* pooled, void* stream);
int xv_conv2d_f32_scalar(const float* x, int n, int h, int w, int cin, const float* w_hwio, const float* bias, int k, int cout,
                         int relu, float* y, void* stream);
int xv_maxpool2x2_f32(const float* x, int n, int h, int w, int c, float* y, void* stream);
int xv_upsample2x_f32(const float* x, int n, int h, int w, int c, const float* residual, float* y, void* stream);
/* ... with the inference batch norm of the deconv between it and its relu: y = relu(bilinear_x2(x) * scale + shift) + residual */
int xv_upsample2x_affine_f32(const float* x, int n, int h, int w, int c, const float* scale, const float* shift,
                             const float* residual, float* y, void* stream);
/* The decoder head without the commutation, in float32 (a batch norm with a shift between the x8 deconv and its relu:
 * custom_layers.py:112-119 under simple_fcn.py:89-135): fused [n][h][w][u] -> score / prob [n][8h][8w][C] float32, label
 * [n][8h][8w] int64 (any of the three may be NULL).  scale / shift: the folded batch norm of `upscore` ([u]).            */
int xv_decoder_head_affine_f32(const float* fused, int n, int h, int w, int u, const float* scale, const float* shift,
                               const float* w_score, const float* b_score, int num_classes, float* score, float* prob,
                               int64_t* label, void* stream);
int xv_score_lowres_f32(const float* fused, int n, int h, int w, int u, const float* w_score, int num_classes, float* S,
                        void* stream);
int xv_decoder_head_from_scores(const float* S, const float* b_score, int n, int hi, int wi, int num_classes, float* score,
                                float* prob, int64_t* label, void* stream);

/* ---- on-device training augmentation (csrc/augment.hip; datasets/device_augmentation.py) ---------------------------------
 * The host chain of datasets/augmentation.py -- scale, rotate + centre crop, shear, crop, flips, contrast / brightness / gamma,
 * label flip / merge -- then crop_multiple and the float cast of DataBaseclass._load_sample, for a batch of N output images in
 * ONE launch, bit for bit what the host computes (float64 in numpy's operation order, no contraction, rint = half to even).
 *   rgb uint8 [M][H][W][3], depth uint16 [M][H][W], labels int32 [M][H][W]   a resident pool of equally sized sources
 *   index int32 [N]       source image of each output image (no gathered copy is made); index_host: the same N values in
 *                         host memory, checked against [0, M) before the launch
 *   plans [N]             one xv_augment_plan record (include/xview_augment.h, xv_augment_plan_bytes() bytes each) per output
 *                         image in device memory; plans_host: the same N records in host memory, checked before the launch
 *   luts uint8 [N][256]   per output image the composed contrast -> brightness -> gamma map (identity: 0..255), made on the
 *                         host by the host's own formulas; the kernel only indexes it with the augmented rgb value
 *   out_rgb float32 [N][S][S][3], out_depth float32 [N][S][S][1], out_labels int32 [N][S][S]: what the trainers take
 * S = the crop size cut down to a multiple of 16.  An output pixel is mapped back through flips and crop to a pixel of the
 * sheared image; that is a bilinear blend (zero outside, rounded to the source integer type) of four pixels of the rotated and
 * centre-cropped image; each of those a blend of four canvas taps of the scaled image; each of those a rounded bilinear blend
 * of four source pixels (rgb) or a floor-index nearest pick (depth, labels).  Rotation and shear resample labels bilinearly
 * too, as the host chain does.  A stage the plan leaves out is skipped.  Nothing intermediate is written to memory.
 * XV_EINVAL, with no launch: a null pointer; M, H, W or N not positive (N at most 65535); S not a positive multiple of 16; an
 * index_host entry outside [0, M); a plans_host record with unknown stage bits, a non-finite matrix, a stage size that
 * contradicts the stages before it, a centre-crop window that leaves its canvas, or a crop window that is smaller than S or
 * leaves its stage's image.  The two host copies must hold what the device buffers hold: the kernel clamps every source read
 * into the selected image, but computes from the device copies.                                                            */
size_t xv_augment_plan_bytes(void);
int xv_augment_batch(const uint8_t* rgb, const uint16_t* depth, const int32_t* labels, int M, int H, int W,
                     const int32_t* index, const int32_t* index_host, const xv_augment_plan* plans,
                     const xv_augment_plan* plans_host, const uint8_t* luts, int N, int S, float* out_rgb, float* out_depth,
                     int32_t* out_labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XVIEW_HIP_H */
