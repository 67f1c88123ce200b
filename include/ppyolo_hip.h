/*
 * ppyolo_hip.h -- C ABI of libppyolo_hip.so: MI355X (gfx950) kernels for the PP-YOLO
 * inference hot path of miemie2013/Pytorch-PPYOLO.
 *
 * The reference has NO FFI on this path (it is a torch.nn.Module tree); the entry points
 * below are what a binding for this path would bind, one per reference operator that the
 * path replaces.  Each declaration cites the reference code it stands in for
 * (file:line inside the reference repo).  The only real FFI in the reference is the
 * optional, CUDA-only `_ext.dcn_v2_forward` (external/DCNv2/src/dcn_v2.h:9-23); the DCN
 * entry points mirror its argument order.
 *
 * Conventions (all functions):
 *   - plain C types only; every pointer is a DEVICE pointer unless named `h_*`;
 *   - activations are fp32 NHWC: element (n,h,w,c) of a tensor with pixel stride `ld`
 *     (in floats, >= C, multiple of 4) lives at  base[((n*H + h)*W + w)*ld + c];
 *     a channel slice of a wider (concat) buffer is expressed as base+offset with the
 *     wide buffer's `ld`;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only
 *     enqueue work, never synchronise, never allocate, keep no state => thread-safe per
 *     stream and capturable into a hipGraph;
 *   - return value: 0 = PPY_OK, negative = error (ppy_error_string()); nothing throws.
 */
#ifndef PPYOLO_HIP_H_
#define PPYOLO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPY_OK 0
#define PPY_ERR_BAD_ARG (-1)      /* shape / alignment / NULL-pointer contract violated   */
#define PPY_ERR_UNSUPPORTED (-2)  /* valid request outside what the kernels implement     */
#define PPY_ERR_WORKSPACE (-3)    /* workspace missing or too small                       */
#define PPY_ERR_LAUNCH (-4)       /* hipLaunch / hipFuncSetAttribute failed               */
#define PPY_ERR_CORRUPT (-5)      /* input data (a JPEG file) damaged or truncated        */

#define PPY_ACT_NONE 0
#define PPY_ACT_RELU 1
#define PPY_ACT_LEAKY 2 /* LeakyReLU(0.1), reference model/custom_layers.py:133 */

int ppy_version(void);
const char *ppy_error_string(int code);
/* Name of the HIP runtime error behind the last PPY_ERR_LAUNCH on the calling thread (diagnostics). */
const char *ppy_last_hip_error(void);
void ppy_note_hip_error(int hip_error);      /* internal: set by the launch paths */

/* ------------------------------------------------------------------------------------
 * Conv2dUnit.forward (reference model/custom_layers.py:243-253): conv(k in {1,3},
 * pad=(k-1)/2) -> eval BatchNorm as per-channel affine -> [+ residual] -> activation.
 * Also covers `x + shortcut; relu` of ConvBlock/IdentityBlock/BasicBlock
 * (model/resnet_vd.py:55-56, :85-86, :265-266) through `residual`, the nearest x2
 * upsample of the head routes (model/head.py:396-397) through `upsample2x`, and the two
 * CoordConv channels (model/custom_layers.py:267-271) through `posbias`.
 *
 * Implicit GEMM on fp32 MFMA (v_mfma_f32_32x32x2_f32):
 *   y[n,ho,wo,k] = act( (sum_{r,s,c} x[n,ho*stride+r-pad,wo*stride+s-pad,c]*w[k,r,s,c]
 *                         + posbias[ho,wo,k]) * scale[k] + shift[k] + residual[n,ho,wo,k] )
 * x: NHWC (ld x_ld), C % 32 == 0.   w: [K][R][S][C] ("KRSC").   scale/shift: [K].
 * residual: NULL or NHWC [N,Ho,Wo,>=K] with ld res_ld.   posbias: NULL or [Ho*Wo][K].
 * y: NHWC ld y_ld; with upsample2x != 0 y is [N,2Ho,2Wo,*] and every result is
 * written to its 2x2 nearest-neighbour block.
 * cfg: tile configuration id, -1 = built-in heuristic; splitk: 0 = heuristic, >=1 forced.
 * ws: scratch for split-K partial sums, ppy_conv2d_workspace_bytes() bytes (may be
 * NULL when that returns 0).
 * w_x3: NULL, or the same weights split into three bf16 planes by
 * ppy_conv2d_split_weights_bf16x3 ([3][K][R][S][C] bf16, 6*K*R*S*C bytes).  With w_x3 the
 * "bf16x3" kernels become selectable (cfg ids >= 31; the heuristic cfg = -1 then prefers
 * them): each fp32 operand is split exactly into 3 bf16 terms and the product is evaluated as
 * the 6 leading partial products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- fp32 in,
 * fp32 out, error vs fp64 at the level of the exact-fp32 fma chain (csrc/conv_x3.hip,
 * profiles/r01_bf16x3_numerics.txt), 6/16 of the fp32-MFMA cost.  Without w_x3 those ids
 * return PPY_ERR_BAD_ARG.
 * w_f16x2 / scale_f16x2: NULL, or the outputs of ppy_conv2d_split_weights_f16x2: the weights times a per-output-
 * channel power of two as two fp16 planes (4*K*R*S*C bytes; opaque layout [2][R*S*C/32][K][32]: the 32-deep reduction chunk is
 * the outer index, so that the 16 weight rows one DMA instruction fetches are one contiguous KB) and `scale` with the inverse of that
 * power folded in.  They make the "f16x2" kernels selectable (cfg ids >= 40; 9 tiles, ids 40-48 with two LDS stages,
 * 49-57 the same tiles with three and 58-66 with four chunks resident / in flight, as far as 160 KB of LDS allow):
 * 2-term fp16 split of both operands,
 * 3 partial products on v_mfma_f32_32x32x16_f16, fp32 accumulation; the activations of an image are scaled on the
 * fly by the power of two that puts that image's maximum into [2^13, 2^14), read from `amax_in`.  Error vs fp64 at the level of
 * the exact-fp32 fma chain (tools/probes/f16x2_probe.hip, profiles/r01_f16x2_numerics.txt).  Needs amax_in, and with a
 * posbias also posbias_f16x2 = posbias[., k] * scale[k] / scale_f16x2[k] (the bias map in the scaled-weight domain),
 * else PPY_ERR_BAD_ARG.
 * amax_in / amax_out: NULL, or N * PPY_AMAX_FLOATS_PER_IMAGE floats each: the running PER-IMAGE max|.| of the input
 * tensor (an upper bound is enough) and the slots into which this launch merges the per-image max|y| of what it stores
 * (atomic max; the owner zeroes the slots before the first producer of a tensor runs).  Image n owns 8 slots, one
 * 64-byte line apart: floats [(n*8 + s)*16], s = 0..7; a consumer takes the maximum over the 8 slots of an image.
 * Per-image scales keep every image's result independent of the rest of the batch.
 */
#define PPY_AMAX_FLOATS_PER_IMAGE 128 /* 8 slots x 16 floats */
int ppy_conv2d_split_weights_bf16x3(const float *w_krsc, long long n_elems, void *out_planes,
                                    void *stream);
int ppy_conv2d_split_weights_f16x2(const float *w_krsc, int K, long long kred, const float *scale,
                                   void *out_planes, float *scale_out, void *stream);
int ppy_conv2d_bn_act_f32(const float *x, int x_ld, const float *w_krsc, const void *w_x3,
                          const void *w_f16x2, const float *scale, const float *scale_f16x2,
                          const float *shift, const float *residual, int res_ld,
                          const float *posbias, const float *posbias_f16x2, float *y, int y_ld, int N,
                          int H, int W, int C, int K, int R, int S, int stride, int pad, int act,
                          int upsample2x, int cfg, int splitk, const float *amax_in, float *amax_out,
                          void *ws, size_t ws_bytes, void *stream);
/* The same launch with PRE-SPLIT tensors on one or both sides ("global pre-split"; f16x2 tile kernels of
 * csrc/conv_x3.hip / conv_ws.hip with an explicit cfg, one split; a pre-split y cannot be combined with upsample2x).  Between a producer convolution and the ONE
 * convolution that consumes its output the tensor can travel as the consumer's finished MFMA operands instead of fp32: per pixel
 * and 32-channel group, 32 fp16 first terms followed by 32 fp16 second terms of value * s_image (RNE; the residual is exact) -- the
 * same 128 bytes, the same pixel stride.  The consumer's main loop then carries no scale / split VALU work.
 *   y_split_scale != NULL: y is WRITTEN in that form (K and y_ld multiples of 32, y 128-byte aligned) and y_split_scale[n]
 *     receives the power of two s_n that puts the STATIC bound  y_bound_mul * max|x_n| + y_bound_add  of |y_n| into [2^13, 2^14)
 *     (caller's duty: y_bound_mul >= max_k |scale_k| * sum_c |w_k,c|, y_bound_add >= max_k |shift_k| (+ |posbias * scale|);
 *     max|x_n| is taken from amax_in, rounded up to a power of two); amax_out still receives max|y|.
 *   x_split_scale != NULL: x holds such operands, written by a launch whose y_split_scale it is (C and x_ld multiples of 32).
 * PPY_ERR_BAD_ARG when the chosen cfg cannot read / write such tensors (never a silent reinterpretation of the bytes).
 *   amax_in2 (round 6; may be NULL): a SECOND block of tracked per-image maxima, for an input whose channels were written by
 *     producers that track into different blocks (the folded projection shortcut's wide buffer [conv2 output | pooled block
 *     input], model/resnet_vd.py:27-33: the pooled part keeps the slots of the tensor it was pooled from, so that tensor's other
 *     readers never see conv2's maximum); the f16x2 kernels scale an image by the larger of the two.  With both split pointers
 *     NULL the call is ppy_conv2d_bn_act_f32 plus this one pointer (cfg -1 and split-K allowed).
 * Reference operator: the same Conv2dUnit.forward (model/custom_layers.py:243-253). */
int ppy_conv2d_bn_act_split_f32(const float *x, int x_ld, const float *w_krsc, const void *w_x3,
                                const void *w_f16x2, const float *scale, const float *scale_f16x2,
                                const float *shift, const float *residual, int res_ld,
                                const float *posbias, const float *posbias_f16x2, float *y, int y_ld, int N,
                                int H, int W, int C, int K, int R, int S, int stride, int pad, int act,
                                int upsample2x, int cfg, int splitk, const float *amax_in, float *amax_out,
                                void *ws, size_t ws_bytes, void *stream, const float *x_split_scale,
                                float *y_split_scale, float y_bound_mul, float y_bound_add, const float *amax_in2);
size_t ppy_conv2d_workspace_bytes(int N, int H, int W, int C, int K, int R, int S, int stride,
                                  int pad, int cfg, int splitk);
int ppy_conv2d_num_configs(void);
/* The cfg ids, family by family in id order (all families compute the same operator; the f16x2 families are bit-identical to
 * each other, the seven k-parity tiles to one another):  exact-fp32 MFMA tiles (csrc/conv_igemm.hip), bf16x3 tiles and f16x2 tiles --
 * plain, with slab reuse (3x3 / stride 1 / pad 1 only), with 96 / 192 rows -- (csrc/conv_x3.hip), the streaming 1x1 kernel
 * (csrc/conv_stream.hip), the patch kernel of the 3x3 stem layers (csrc/conv_patch.hip), the f16x2 tiles with specialised waves --
 * plain, PRE, k-parity -- (csrc/conv_ws.hip), the wave-private tiles for small outputs (csrc/conv_small.hip).  What one id is and
 * can do is answered by ppy_conv2d_config_info, filled in by the family that dispatches the id.
 * An explicit id on a geometry its kernel does not cover returns PPY_ERR_BAD_ARG (never a silent other kernel); the one exception:
 * the scalar epilogue (K % 4 != 0 or unaligned rows) does not exist for the wave tiles of six / eight 32x32 blocks -- such a launch
 * runs on the exact-fp32 fall-back tile. */
enum { PPY_CFG_FP32 = 0, PPY_CFG_BF16X3, PPY_CFG_F16X2, PPY_CFG_F16X2_SLAB, PPY_CFG_F16X2_TALL, PPY_CFG_STREAM, PPY_CFG_PATCH,
       PPY_CFG_WS, PPY_CFG_WS_PRE, PPY_CFG_WS_KPARITY, PPY_CFG_SMALL };                       /* ppy_conv_cfg_info.family */
enum { PPY_CFG_OPERANDS_FP32 = 0,      /* the fp32 weights only */
       PPY_CFG_OPERANDS_BF16X3,        /* + w_x3 */
       PPY_CFG_OPERANDS_F16X2 };       /* + w_f16x2, scale_f16x2, amax_in (posbias_f16x2 beside a posbias) */
enum { PPY_CFG_SPLITK_NONE = 0,        /* splitk == 1 only */
       PPY_CFG_SPLITK_WORKSPACE,       /* partial sums in the workspace (ppy_conv2d_workspace_bytes) + a combine launch */
       PPY_CFG_SPLITK_IN_WORKGROUP };  /* k-parts inside the workgroup: no workspace, no second launch */
typedef struct ppy_conv_cfg_info {
    int family;            /* PPY_CFG_* */
    int local;             /* the id inside the dispatch switch of the family's source file */
    int operands;          /* PPY_CFG_OPERANDS_* */
    int bm, bn, stages;    /* tile rows, columns, LDS stages asked for (0 where the notion does not apply) */
    int splitk_mode;       /* PPY_CFG_SPLITK_* */
    int reads_presplit;    /* takes x_split_scale (ppy_conv2d_bn_act_split_f32) */
    int writes_presplit;   /* takes y_split_scale */
    int bn_stats;          /* its epilogue can write the BatchNorm partials of ppy_conv2d_train_fwd_f32 */
    int stats_twin;        /* bn_stats == 0 and an otherwise identical tile has them: that tile's cfg id; else -1 */
} ppy_conv_cfg_info;
/* PPY_OK, or PPY_ERR_BAD_ARG for cfg outside [0, ppy_conv2d_num_configs()). */
int ppy_conv2d_config_info(int cfg, ppy_conv_cfg_info *out);
/* First cfg id of the streaming 1x1 kernel (csrc/conv_stream.hip; two ids) and of the patch kernel for the 3x3 stem layers
 * with C = 32, K = 32 / 64, stride 1 (csrc/conv_patch.hip; one id) -- both f16x2 only; an explicit id on a geometry the kernel
 * does not cover is PPY_ERR_BAD_ARG. */
int ppy_conv2d_stream_first_config(void);
int ppy_conv2d_patch_first_config(void);
/* First cfg id of the f16x2 tiles with specialised waves (csrc/conv_ws.hip: four waves deliver operands, four multiply; any
 * geometry the f16x2 tiles take, split-K included; bit-identical results). */
int ppy_conv2d_ws_first_config(void);
/* First cfg id of the wave-private tiles for SMALL outputs (round 6, csrc/conv_small.hip; f16x2 only; four ids: 32x32 / 32x64 output
 * tiles per wave, four / eight waves per workgroup) -- batch 1 (the reference's demo loop, demo.py:121-160) and narrow layers.  A wave
 * owns its tile and one k-part of the reduction, operands go from the L2 straight into MFMA fragment registers.  For these ids
 * `splitk` counts k-parts INSIDE the workgroup (rounded down to a power of two <= the workgroup's waves): the parts are added in the LDS
 * in the order 0, 1, 2, ..., no workspace is needed (ppy_conv2d_workspace_bytes = 0), no combine launch follows, pre-split tensors
 * (ppy_conv2d_bn_act_split_f32) are accepted on both sides with splitk > 1 as well; with splitk in {1, 2, 4, 8} results are
 * bit-identical to the f16x2 tiles' split-K of the same count. */
int ppy_conv2d_small_first_config(void);
/* Writes the tile configuration / split the heuristic would pick. */
int ppy_conv2d_pick(int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                    int *cfg_out, int *splitk_out);

/* The HBM-bound 1x1 "expand" convolutions (ResNet-vd BottleNeck conv3 + shortcut + ReLU, reference
 * model/resnet_vd.py:55-91; C64 -> K256 at 152x152 moves 425 MB for 6 GFLOP) as a persistent streaming kernel
 * (csrc/conv_stream.hip): 1x1, stride 1, C == 64 with K % 64 == 0 or C == 128 with K % 128 == 0 (K / 64 resp. K / 128 a power of
 * two <= 16), f16x2 operands (w_f16x2 / scale_f16x2 / amax_in as above),
 * results bit-identical to the f16x2 tiles of ppy_conv2d_bn_act_f32.  The same kernel is selectable there as the cfg ids
 * ppy_conv2d_stream_first_config() + variant (variant 0: two workgroups per CU, 1: one); this entry point adds the second
 * output: pooled (or NULL) = [N][H/2][W/2] rows of ld pooled_ld holding the 2x2 / stride-2 average of y -- the AvgPool2d(2, 2)
 * in front of the vd projection shortcut (reference model/resnet_vd.py:29-33) written from the same epilogue, evaluated
 * (((a + b) + c) + d) * 0.25 exactly as ppy_avgpool2x2_f32 does (H, W even).  PPY_ERR_BAD_ARG for any other geometry:
 * there is no silent fall-back to another kernel. */
int ppy_conv1x1_expand_f32(const float *x, int x_ld, const void *w_f16x2, const float *scale_f16x2, const float *shift,
                           const float *residual, int res_ld, float *y, int y_ld, float *pooled, int pooled_ld, int N, int H,
                           int W, int C, int K, int act, int variant, const float *amax_in, float *amax_out, void *stream);

/* Training forward of a FROZEN 1x1 Conv2dUnit (reference model/custom_layers.py:243-253 with its BatchNorm2d on batch statistics;
 * train.py:259-262 freezes the backbone) on the streaming kernel of ppy_conv1x1_expand_f32 WITHOUT the raw convolution output in memory:
 *   ppy_conv1x1_stats_f32: the first pass of the BatchNorm only -- (n, mean, M2) partials [*bn_slices][K][3] exactly as
 *     ppy_conv2d_train_fwd_f32 writes them (merge with ppy_bn_train_stats_merge_f32); nothing else is stored.
 *   ppy_conv1x1_bn_apply_f32: the convolution again, y = act((conv + bias - mean) * (invstd * gamma) + beta [+ residual]) from its
 *     epilogue, amax_out (or NULL) = tracked per-image max|y| -- value for value ppy_conv2d_train_fwd_f32 + ppy_bn_train_apply_f32.
 * Same geometry rules as ppy_conv1x1_expand_f32 (C = 64 / 128, f16x2 operands, scale_f16x2 from ppy_conv2d_split_weights_f16x2 with
 * scale = 1); mean / invstd / gamma / beta: [K], 16-byte aligned.  Pays the layer's MFMA work twice to save a write and a read of its
 * output: for the HBM-bound stage-2 layers (6 GFLOP for 0.4-0.8 GB) that is a third of the time. */
int ppy_conv1x1_stats_f32(const float *x, int x_ld, const void *w_f16x2, const float *scale_f16x2, const float *bias, int N, int H,
                          int W, int C, int K, int variant, const float *amax_in, float *bn_partials, size_t bn_partials_bytes,
                          int *bn_slices, void *stream);
int ppy_conv1x1_bn_apply_f32(const float *x, int x_ld, const void *w_f16x2, const float *scale_f16x2, const float *bias,
                             const float *mean, const float *invstd, const float *gamma, const float *beta, const float *residual,
                             int res_ld, float *y, int y_ld, int N, int H, int W, int C, int K, int act, int variant,
                             const float *amax_in, float *amax_out, void *stream);

/* The last stem convolution (reference model/resnet_vd.py:110 conv1_3: 3x3, stride 1, pad 1, C = 32 -> K = 64, BatchNorm affine, ReLU)
 * AND the MaxPool2d(kernel_size=3, stride=2, padding=1) that follows it (model/resnet_vd.py:103, 136) in one launch: only the pooled
 * tensor [N][(H-1)/2+1][(W-1)/2+1][pooled_ld] is written; bit-identical to ppy_conv2d_bn_act_f32 on the patch kernel followed by
 * ppy_maxpool3x3s2_f32 (same products in the same order per pixel, exact maxima; padding positions never win, as with -inf padding).
 * f16x2 operands (w_f16x2 / scale_f16x2 from ppy_conv2d_split_weights_f16x2, amax_in the tracked maxima of x); amax_out (or NULL)
 * records max|.| of the pooled tensor per image (= that of the unpooled one: every pixel lies in a window).
 * PPY_ERR_BAD_ARG for any other geometry (C != 32, K != 64): there is no silent fall-back. */
int ppy_conv3x3_maxpool_f32(const float *x, int x_ld, const void *w_f16x2, const float *scale_f16x2, const float *shift,
                            float *pooled, int pooled_ld, int N, int H, int W, int C, int K, int act, const float *amax_in,
                            float *amax_out, void *stream);

/* ------------------------------------------------------------------------------------
 * Backward of the convolution -- training step, SURVEY 8f rank 2 / BASELINE config 5: what torch autograd computes for
 * the F.conv2d inside Conv2dUnit.forward (reference model/custom_layers.py:243-253) when train.py:441 calls
 * all_loss.backward().  Same tensors and layouts as ppy_conv2d_bn_act_f32: x [N,H,W,C] (ld x_ld), w [K][R][S][C],
 * dy = d loss / d conv output [N,Ho,Wo,K] (ld dy_ld; the BN / activation backward is the caller's, upstream of dy).
 *   ppy_conv2d_dgrad_f32: dx[n,h,w,c] = sum_{k,r,s} dy[n,h+pad-r,w+pad-s,k] * w[k,r,s,c]  (written, not accumulated).
 *     stride 1 only (PPY_ERR_UNSUPPORTED otherwise: with the reference's freeze_at = 5 only the head trains and it has
 *     no strided convolution).  Runs the forward implicit-GEMM kernels on the flipped / transposed weights; K need not
 *     be a multiple of 32 (the 258-channel output convolutions are zero-padded in the workspace).  cfg / splitk: tile
 *     configuration of that forward kernel for the geometry (N, Ho, Wo, C' = K rounded up to 32, K' = C), as in
 *     ppy_conv2d_bn_act_f32 (-1 / 0 = heuristic).  amax_dy (or NULL): tracked per-image maxima of dy -> the f16x2 kernels
 *     (cfg then names an f16x2 tile), else bf16x3.
 *   ppy_conv2d_wgrad_f32: dw[k,r,s,c] = sum_{n,ho,wo} dy[n,ho,wo,k] * x[n,ho*stride+r-pad,wo*stride+s-pad,c]
 *     (written, not accumulated; any stride / C / K).  bf16x3 on the 16-bit MFMA (exact fp32 MFMA where alignment rules it
 *     out); with amax_x / amax_dy -- tracked per-image maxima of both operands, as ppy_bn_train_apply_f32 / _bwd_f32 and the
 *     convolution entry point record them -- the f16x2 scheme (one power-of-two scale per operand, 3 products instead of 6).
 *     Pixel slices are combined in a fixed order, so results are run-to-run identical.
 * ws: ppy_conv2d_{dgrad,wgrad}_workspace_bytes() bytes, 256-byte aligned.
 */
/* Training-mode forward of the convolution in front of a BatchNorm2d on batch statistics (reference
 * model/custom_layers.py:243-253): y = conv(x, w) + bias on an f16x2 tile (cfg >= 0: an f16x2 id of csrc/conv_x3.hip or
 * csrc/conv_ws.hip; one split) and, from the same epilogue, the first pass of the BatchNorm: per wave row-tile ("slice") and
 * channel the triple (n, mean, M2) of y in bn_partials[*bn_slices][K][3].  ppy_conv2d_bn_partials_bytes(M, K) bytes always hold
 * the triples AND the scratch ppy_bn_train_stats_merge_f32 needs behind them; that call turns them into mean / invstd / running
 * statistics exactly as ppy_bn_train_stats_f32 does from a pass over y (same Chan merge, slices in order) -- without reading y
 * again.  w_f16x2 / scale_f16x2: ppy_conv2d_split_weights_f16x2 with scale = 1.  PPY_ERR_UNSUPPORTED: cfg names another kernel
 * family (the caller then runs ppy_conv2d_bn_act_f32 + ppy_bn_train_stats_f32). */
size_t ppy_conv2d_bn_partials_bytes(long long M, int K);
int ppy_conv2d_train_fwd_f32(const float *x, int x_ld, const float *w_krsc, const void *w_f16x2, const float *scale_f16x2,
                             const float *bias, float *y, int y_ld, int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                             int cfg, const float *amax_in, float *bn_partials, size_t bn_partials_bytes, int *bn_slices, void *stream);
int ppy_bn_train_stats_merge_f32(float *partials, size_t partials_bytes, int slices, int C, float eps, float momentum, float *mean,
                                 float *invstd, float *running_mean, float *running_var, void *stream);
int ppy_conv2d_dgrad_f32(const float *dy, int dy_ld, const float *w_krsc, float *dx, int dx_ld, int N, int H, int W,
                         int C, int K, int R, int S, int stride, int pad, int cfg, int splitk, const float *amax_dy, void *ws,
                         size_t ws_bytes, void *stream);
size_t ppy_conv2d_dgrad_workspace_bytes(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int cfg,
                                        int splitk);
/* Round 3: the f16x2 operand forms of ALL trainable convolution weights in three launches per step instead of two or three
 * per layer (train.py:442 `optimizer.step()` changes every weight every iteration, so the forward planes and the flipped /
 * transposed planes of the data gradients are rebuilt every step: 47 launches of 7-15 us for the R50vd head).
 *   desc[i]: one weight tensor [K][R][S][C] (C % 32 == 0).  fwd_planes / fwd_scale: exactly what
 *   ppy_conv2d_split_weights_f16x2(w, K, R*S*C, ones, ...) writes.  dgrad_planes / dgrad_scale / dgrad_wt (all three or none):
 *   w'[c][r'][s'][k] = w[k][R-1-r'][S-1-s'][c], K padded with zeros to Kp = K rounded up to 32 -- the planes
 *   [2][R*S*Kp/32][C][32], per-row scales [C] and fp32 copy [C][R][S][Kp] that ppy_conv2d_dgrad_f32 builds in its workspace
 *   (bit-identical).  row0 / blk0: prefix sums over the descriptors of K and of (C / 32) * PPY_PREP_SPLIT.  The table lives in
 *   device memory.  colmax: scratch of blocks_total * 32 floats.
 *   ppy_conv2d_dgrad_prepared_f32 = ppy_conv2d_dgrad_f32 (stride 1, f16x2: amax_dy required) on such buffers; ones / zeros: [C]
 *   constants; workspace as ppy_conv2d_dgrad_workspace_bytes says (the padded copy of a dy with K % 32 != 0, split-K). */
#define PPY_PREP_SPLIT 8
typedef struct PpyWeightPrep {
    const float *w;
    void *fwd_planes;
    float *fwd_scale;
    void *dgrad_planes;
    float *dgrad_scale;
    float *dgrad_wt;
    int K, R, S, C;
    int row0, blk0;
} PpyWeightPrep;
int ppy_train_prepare_weights_f16x2(const PpyWeightPrep *desc_dev, int count, int rows_total, int blocks_total, float *colmax,
                                    size_t colmax_bytes, void *stream);
int ppy_conv2d_dgrad_prepared_f32(const float *dy, int dy_ld, const float *wt, const void *planes, const float *scale_f16x2,
                                  const float *ones, const float *zeros, float *dx, int dx_ld, int N, int H, int W, int C, int K, int R,
                                  int S, int pad, int cfg, int splitk, const float *amax_dy, void *ws, size_t ws_bytes, void *stream);
int ppy_conv2d_wgrad_f32(const float *x, int x_ld, const float *dy, int dy_ld, float *dw_krsc, int N, int H, int W,
                         int C, int K, int R, int S, int stride, int pad, const float *amax_x, const float *amax_dy, void *ws,
                         size_t ws_bytes, void *stream);
size_t ppy_conv2d_wgrad_workspace_bytes(int N, int H, int W, int C, int K, int R, int S, int stride, int pad);

/* ------------------------------------------------------------------------------------
 * Training-step operators around the convolutions (SURVEY 8f rank 2 / BASELINE config 5; csrc/train.hip).  Tensors are
 * fp32 NHWC slices (pointer + pixel stride), P = N*H*W pixels.
 *  ppy_bn_train_stats_f32 / _apply_f32: torch.nn.BatchNorm2d in TRAINING mode (the reference trains with every BatchNorm
 *    on batch statistics: train.py never calls .eval(); model/custom_layers.py:122): per-channel mean and
 *    invstd = 1/sqrt(biased var + eps) of x, running statistics updated in place with `momentum` (unbiased variance), then
 *    y = act((x - mean) * invstd * gamma + beta [+ residual]); amax_out (or NULL): per-image max|y| slots as the convolution
 *    entry point tracks them (zeroed by the caller; pixels_per_image = H*W) -- the operand scale of a following f16x2 kernel.
 *  ppy_bn_train_bwd_f32 (amax_dx or NULL: per-image max|dx| slots, as amax_out above): given dy = d loss / d y: dz = dy * act'(y), dbeta = sum dz, dgamma = sum dz * xhat,
 *    dx = gamma * invstd * (dz - (dbeta + xhat * dgamma) / P).
 *  ppy_act_bwd_f32: dx = dy * act'(y) alone.
 *  ppy_upsample2x_bwd_f32: backward of the nearest x2 upsample of the head routes (model/head.py:396-397): dx = sum of the
 *    2x2 block of dy (accumulate != 0: added to dx).
 *  ppy_spp_bwd_f32: backward of SPP (model/custom_layers.py:281-290): dy is [N,H,W,4C] = (x, pool5, pool9, pool13); every
 *    window's gradient goes to its first maximum in (h, w) scan order, as torch.max_pool2d's does.
 *  ppy_dropblock_mask_f32 / _apply_f32: DropBlock in training mode (custom_layers.py:303-342): seeds = u < gamma (gamma from
 *    the feature HEIGHT, like the reference), mask = 1 - maxpool3x3(seeds), scale = numel / sum(mask); y = x * mask * scale
 *    (the same map serves the backward).  u comes from a counter-based generator keyed by `seed` -- the reference draws from
 *    torch's global generator, so masks are comparable in distribution only; parity tests inject the reference's mask.
 *  ppy_sgd_momentum_f32: torch.optim.SGD(momentum, weight_decay) as built by train.py:271-280:
 *    d = g + wd * p; v = first_step ? d : mu * v + d; p -= lr * v.
 * All reductions run in a fixed order (no float atomics): results are run-to-run identical.
 *  ppy_avgpool2x2_bwd_f32 / ppy_maxpool3x3s2_bwd_f32: backward of the vd shortcut's AvgPool2d(2, 2) (resnet_vd.py:29-33) and of
 *    the stem's MaxPool2d(3, 2, 1) (:103; the gradient of a window goes to its first maximum in scan order, as in torch) --
 *    training with freeze_at < 5.  dx [N,H,W,C] is written whole.
 *  ppy_zero_insert_f32: up[n, i*s, j*s, :] = dy[n, i, j, :] into a zeroed [N,H1,W1,C]: the data gradient of a stride-s
 *    convolution = ppy_conv2d_dgrad_f32 (stride 1) of the zero-inserted gradient with H1 = H + 2*pad - R + 1.
 */
size_t ppy_bn_train_workspace_bytes(int P, int C);
int ppy_avgpool2x2_bwd_f32(const float *dy, int dy_ld, float *dx, int dx_ld, int N, int H, int W, int C, void *stream);
int ppy_maxpool3x3s2_bwd_f32(const float *x, int x_ld, const float *dy, int dy_ld, float *dx, int dx_ld, int N, int H, int W, int C,
                             void *stream);
int ppy_zero_insert_f32(const float *dy, int dy_ld, float *up, int up_ld, int N, int Ho, int Wo, int C, int H1, int W1, int stride,
                        void *stream);
int ppy_bn_train_stats_f32(const float *x, int x_ld, int P, int C, float eps, float momentum, float *mean, float *invstd,
                           float *running_mean, float *running_var, void *ws, size_t ws_bytes, void *stream);
int ppy_bn_train_apply_f32(const float *x, int x_ld, const float *mean, const float *invstd, const float *gamma,
                           const float *beta, const float *residual, int res_ld, float *y, int y_ld, int P, int C, int act,
                           int pixels_per_image, float *amax_out, void *stream);
int ppy_bn_train_bwd_f32(const float *x, int x_ld, const float *y, int y_ld, const float *dy, int dy_ld, const float *mean,
                         const float *invstd, const float *gamma, float *dx, int dx_ld, float *dgamma, float *dbeta, int P, int C,
                         int act, int pixels_per_image, float *amax_dx, void *ws, size_t ws_bytes, void *stream);
int ppy_act_bwd_f32(const float *dy, int dy_ld, const float *y, int y_ld, float *dx, int dx_ld, long long P, int C, int act,
                    void *stream);
int ppy_upsample2x_bwd_f32(const float *dy, int dy_ld, float *dx, int dx_ld, int N, int H, int W, int C, int accumulate,
                           void *stream);
size_t ppy_spp_bwd_workspace_bytes(int N, int H, int W, int C);
int ppy_spp_bwd_f32(const float *x, int x_ld, const float *dy, int dy_ld, float *dx, int dx_ld, int N, int H, int W, int C,
                    void *ws, size_t ws_bytes, void *stream);
size_t ppy_dropblock_workspace_bytes(int N, int H, int W, int C);
int ppy_dropblock_mask_f32(float *mask, float *scale_out, int N, int H, int W, int C, int block_size, float keep_prob,
                           unsigned long long seed, void *ws, size_t ws_bytes, void *stream);
int ppy_dropblock_apply_f32(const float *x, int x_ld, const float *mask, const float *scale, float *y, int y_ld, long long P,
                            int C, void *stream);
int ppy_sgd_momentum_f32(float *param, const float *grad, float *velocity, long long n, float lr, float momentum,
                         float weight_decay, int first_step, void *stream);
/* ExponentialMovingAverage.update of the reference (model/EMA.py:29-44; train.py:443-444), on the device instead of a numpy
 * round trip per step: shadow = decay * shadow + (1 - decay) * param in float32 with separate roundings (numpy's arithmetic);
 * the caller computes decay = min(ema_decay, (1 + t) / (10 + t)) and passes float32(decay), float32(1 - decay). */
int ppy_ema_update_f32(float *shadow, const float *param, long long n, float decay, float one_minus_decay, void *stream);
/* Plumbing of the training graph: dst += src (second gradient of a tensor with two consumers); the nearest x2 upsample
 * forward (model/head.py:396-397; the inference path fuses it into the producing convolution's store, which BatchNorm on
 * batch statistics rules out); per-channel sum over the pixels = gradient of a convolution bias
 * (ws: ppy_bn_train_workspace_bytes(P, C)). */
int ppy_add_inplace_f32(float *dst, int dst_ld, const float *src, int src_ld, long long P, int C, void *stream);
int ppy_upsample2x_f32(const float *x, int x_ld, float *y, int y_ld, int N, int H, int W, int C, void *stream);
int ppy_channel_sum_f32(const float *dy, int dy_ld, int P, int C, float *out, void *ws, size_t ws_bytes, void *stream);

/* YOLOv3Loss of one head level, forward AND backward (csrc/yolo_loss.hip): the reference's
 * YOLOv3Loss._get_fine_grained_loss (model/losses.py:121-253) with IouLoss / IouAwareLoss (model/iou_losses.py:39-246) and
 * the ignore mask (losses.py:296-356), plus the analytic gradient of the SUM of all loss terms with respect to the head
 * output -- what `all_loss.backward()` (train.py:441) hands to the output convolutions.
 * head_out: NHWC [N,S,S,*] raw output of this level, channels [an IoU logits if iou_aware][an x (x, y, w, h, obj, C classes)].
 * target: the reference's Gt2YoloTarget tensor [N, an, 6 + C, S, S] (tx, ty, tw, th, tscale, tobj, classes).
 * gt_box: [N, num_gt, 4] normalised (cx, cy, w, h), zero rows = padding.  h_anchors_px: HOST array, an x (w, h) of this level.
 * dout: NHWC like head_out (channels beyond an*(5+C)(+an) are not written).  loss6: device floats
 * {loss_xy, loss_wh, loss_obj, loss_cls, loss_iou, loss_iou_aware}, each the batch mean as the reference logs it
 * (accumulate != 0: added to what is there, for the sum over levels).  ws: ppy_yolov3_loss_workspace_bytes().
 * iou_loss_square: IouLoss(loss_square=), 1 = (1 - iou^2) * weight (both configurations), 0 = (1 - iou) * weight (iou_losses.py:66-70);
 * IouLoss(ciou_term=True) is not implemented (the reference's own branch stops at `alpha.requires_grad = False`, :131, under autograd).
 * amax_dout (or NULL): zeroed per-image maximum slots that receive max|dout| -- the operand scale of the f16x2 gradient kernels
 * of the output convolution.
 */
size_t ppy_yolov3_loss_workspace_bytes(int N, int S, int an);
int ppy_yolov3_loss_f32(const float *head_out, int out_ld, const float *target, const float *gt_box, int num_gt,
                        const float *h_anchors_px, int an, int num_classes, int N, int S, int downsample, double scale_x_y,
                        double ignore_thresh, double iou_loss_weight, int iou_loss_square, int iou_aware,
                        double iou_aware_loss_weight, float *dout, int dout_ld, float *loss6, int accumulate, float *amax_dout,
                        void *ws, size_t ws_bytes, void *stream);

/* First backbone conv, `stage1_conv1_1` (reference model/resnet_vd.py:100, :133): 3x3
 * stride-2 conv C_in=3 -> K (K % 4 == 0, K <= 64) + BN affine + ReLU, reading the
 * caller's NCHW input directly and writing NHWC (fuses the layout change).
 * x: [N,3,H,W] NCHW contiguous.  w: [K][3][3][3] in the reference's own KCRS order. */
int ppy_stem_conv3x3s2_nchw_f32(const float *x_nchw, const float *w_kcrs, const float *scale,
                                const float *shift, float *y, int y_ld, int N, int H, int W,
                                int K, int act, float *amax_out /* NULL or N * PPY_AMAX_FLOATS_PER_IMAGE floats */, void *stream);

/* The same operator on the bf16 MFMA (round 4): the 27-deep reduction as two k-steps of v_mfma_f32_32x32x16_bf16 on
 * exactly-split operands (3 bf16 terms per fp32 value, 6 partial products, fp32 accumulate -- no scaling, so any input
 * range).  K == 32 only (PPY_ERR_UNSUPPORTED otherwise).  Agrees with the fma chain of the entry above to fp32
 * rounding, not bit for bit; PPYOLO_HIP_MATH=fp32 keeps the entry above. */
int ppy_stem_conv3x3s2_nchw_x3_f32(const float *x_nchw, const float *w_kcrs, const float *scale,
                                   const float *shift, float *y, int y_ld, int N, int H, int W,
                                   int K, int act, float *amax_out, void *stream);

/* Image pre-processing in front of the path, reference Decode.process_image
 * (model/decode_np.py:125-140): BGR->RGB (swap_rb), cv2.resize(fx = S/w, fy = S/h, INTER_CUBIC) on uint8
 * (tools/transform.py:996-1003; OpenCV's 11-bit fixed-point bicubic, A = -0.75, replicated border), then the numpy
 * normalisation (transform.py:895-917) given as lut[c][v] = value of grey level v in OUTPUT channel c, and HWC->CHW
 * (transform.py:1052-1054).  images[i]: device pointer to an h[i] x w[i] x 3 uint8 image with row_stride[i] bytes per
 * row; the arrays images / h / w / row_stride are HOST arrays of length n.  out: device [n][3][S][S] float32. */
int ppy_preprocess_u8_f32(int n, const unsigned char *const *images, const int *h, const int *w,
                          const int *row_stride, int swap_rb, int S, const float *lut /* device [3][256] */,
                          float *out, void *stream);

/* Pillow's resize on the device, bit for bit (csrc/pil_resize.hip): the reference's
 * ResizeImage(use_cv2=False) (tools/transform.py:1016-1024) = Image.fromarray(u8_hwc).resize((ow, oh), filter) for 3-channel
 * uint8 images as Pillow 12.2.0 computes it.  filter is PILLOW's code: 0 NEAREST, 1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX,
 * 5 HAMMING.  Filters 1..5 are two separable passes, horizontal first, through a uint8 intermediate of h rows x ow columns,
 * each clip8((2^21 + sum pixel * k) >> 22) in int32 with k = round(w * 2^22) of the normalised double weights; a pass whose
 * axis keeps its size is skipped; NEAREST is an index map per axis.
 *
 * ppy_pil_resize_plan (HOST only, no GPU call): validates the batch and writes the launch's blob into caller-owned host
 * memory (8-byte aligned, blob_bytes >= ppy_pil_resize_plan_bytes of the same arguments, else PPY_ERR_WORKSPACE): a 64-byte
 * header (the ints magic "PIL1", n, ow, oh, filter, number of tables, tallest image of the horizontal launch, bytes per row of
 * the intermediates; the long longs blob bytes, workspace bytes; the ints descriptor offset, first table offset), n 48-byte
 * descriptors (base, pitch, h, w, byte offset of the horizontal table or -1 when that pass is skipped, byte offset of the
 * vertical table, offset of the intermediate in the workspace) and ONE table per distinct (in, out) axis of the batch, shared
 * between images: the ints in, out, ksize, kind (the filter code; -1: the identity map of an axis that keeps its size), then
 * bounds[out][2] = (first source index, taps), then k[out][ksize].  ksize = 0 marks an index map: bounds[.][0] is the source
 * index.  *ws_bytes (may be NULL) receives the size of the device workspace the launches need (the intermediates).
 * h_images[i].base is a DEVICE pointer (it is only copied into the descriptor): h x w pixels of 3 bytes, `pitch` bytes per row.
 * Limits, refused and never clamped (PPY_ERR_UNSUPPORTED; h_reason, NULL or 96 chars, names the value): an input side
 * outside 1..65535, an output side outside 1..8192, ksize > 1024, a filter outside 0..5.  n outside 1..1024, a null base or a
 * pitch below 3 * w: PPY_ERR_BAD_ARG.  ppy_pil_resize_plan_bytes returns 0 for a batch the planner refuses.
 *
 * The launches (two kernels on `stream`, or one when no image changes its width; no host synchronisation): h_blob is the
 * planner's blob on the HOST, blob its DEVICE copy (blob_bytes each), ws the device workspace.  TRUST BOUNDARY: the host blob is
 * validated and sizes the grids, the kernels read the device copy without further checks.
 *   ppy_pil_resize_u8          out: device uint8 [n][oh][ow][3].
 *   ppy_preprocess_pil_u8_f32  out: device float32 [n][3][oh][ow], 16-byte aligned: channel c of the output is
 *                              lut[c][v] of source channel (swap_rb ? 2 - c : c), as ppy_preprocess_u8_f32 stores it. */
typedef struct ppy_pil_image_t {
    const unsigned char *base;
    long long pitch;                  /* bytes per row */
    int h, w;
} ppy_pil_image_t;
size_t ppy_pil_resize_plan_bytes(int n, const ppy_pil_image_t *h_images, int ow, int oh, int filter);
int ppy_pil_resize_plan(int n, const ppy_pil_image_t *h_images, int ow, int oh, int filter, void *h_blob, size_t blob_bytes,
                        size_t *ws_bytes, char *h_reason);
int ppy_pil_resize_u8(int n, const void *h_blob, const void *blob, size_t blob_bytes, void *ws, size_t ws_bytes,
                      unsigned char *out, void *stream);
int ppy_preprocess_pil_u8_f32(int n, const void *h_blob, const void *blob, size_t blob_bytes, void *ws, size_t ws_bytes,
                              int swap_rb, const float *lut /* device [3][256] */, float *out, void *stream);

/* Crops of detections: Pillow's Image.resize((ow, oh), filter, box=(x0, y0, x1, y1)) with the boxes read ON THE DEVICE
 * (csrc/pil_crop.hip), bit for bit with Pillow 12.2.0.  One call resizes up to cap crops of a batch
 * of n images to one (ow, oh) with one filter in four launches on `stream` (select, plan, horizontal, vertical), without a
 * host synchronisation: every grid is sized from n, K or M, ow, oh and the image sizes.  The box reaches the arithmetic as
 * four float32; per axis scale = (double)(in1 - in0) / out with the subtraction in float32, the taps are clamped to the
 * IMAGE, not to the box (so this is not crop().resize()), the horizontal pass runs on the source rows the vertical taps
 * read, and a pass is skipped iff its axis keeps its size and the box is the whole axis.
 *
 * Rows form (ppy_pil_crop_rows_u8): dets = device float32 [n][K][6] rows (class, score, x0, y0, x1, y1), count = device int32
 * [n], as forward_padded returns them; cap = n * K.  Row r < min(count[i], K) of image i is taken iff all six values are
 * finite, class >= 0, score >= thresh, 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h for the row's own box and for the padded
 * one, and fewer than top_k rows of image i were taken before it.  Padding, in float32 with one rounding per operation:
 * bw = x1 - x0, x0' = max(x0 - pad * bw, 0), x1' = min(x1 + pad * bw, w); y likewise.
 * List form (ppy_pil_crop_list_u8): boxes_in = device float32 [M][4], image = device int32 [M]; cap = M.  An entry is taken
 * iff its image index is in 0..n-1 and its box passes the same test; the list's order is kept.
 * Outputs (device): out uint8 [cap][oh][ow][3], zero past the end; src int32 [cap][2] = (image, row or list index) in
 * image-major, row-ascending order, -1 past the end; total int32 [1]; boxes float32 [cap][4] = the boxes that were resized,
 * 0 past the end.  The order comes from an ordered scan in one workgroup: it does not depend on scheduling.
 *
 * ppy_pil_crop_plan_bytes (HOST only, no GPU call): validates the batch and returns the workspace size in *ws_bytes and the
 * taps reserved per output sample of the x and y axis in ksize_cap[2] (either may be NULL).  form: 0 rows (rows_or_m = K),
 * 1 list (rows_or_m = M; pad and top_k are not read).  With kx = ksize of (largest width -> ow), ky = ksize of (largest
 * height -> oh) (0 for NEAREST), A(v) = v rounded up to 256:
 *   ws_bytes = A(32 cap) + A(4 cap) + A(4 cap ow (2 + kx)) + A(4 cap oh (2 + ky)) + cap A(largest height * A16(3 ow)).
 * Limits, refused and never clamped (PPY_ERR_UNSUPPORTED; h_reason, NULL or 96 chars, names the value): an input side
 * outside 1..65535, an output side outside 1..8192, kx or ky > 1024, a filter outside 0..5, an image with h > 100 * w
 * (Pillow resizes those vertically first), n * K or M outside 1..65536, pad outside [0, 4] or not finite, top_k < 1.
 * n outside 1..1024, a null pointer or a pitch below 3 * w: PPY_ERR_BAD_ARG.  A workspace that is NULL or too small:
 * PPY_ERR_WORKSPACE.
 * TRUST BOUNDARY: h_images (HOST) is validated and sizes the grids and the workspace; the kernels read `images`, its DEVICE
 * copy, and the device rows without further checks beyond keeping every access inside the images and the workspace. */
int ppy_pil_crop_plan_bytes(int n, const ppy_pil_image_t *h_images, int form, int rows_or_m, int ow, int oh, int filter,
                            float pad, int top_k, size_t *ws_bytes, int *ksize_cap, char *h_reason);
int ppy_pil_crop_rows_u8(int n, const ppy_pil_image_t *h_images, const ppy_pil_image_t *images, const float *dets,
                         const int *count, int K, float thresh, float pad, int top_k, int ow, int oh, int filter, void *ws,
                         size_t ws_bytes, unsigned char *out, int *src, int *total, float *boxes, void *stream);
int ppy_pil_crop_list_u8(int n, const ppy_pil_image_t *h_images, const ppy_pil_image_t *images, const float *boxes_in,
                         const int *image, int M, int ow, int oh, int filter, void *ws, size_t ws_bytes, unsigned char *out,
                         int *src, int *total, float *boxes, void *stream);

/* Training batches (ppyolo_hip/augment.py TrainBatchBuilder): the reference's training reader (train.py:36-152) with
 * the transforms of config/ppyolo_2x.py:154-251, planned on the host.  blob: DEVICE copy of the planner's upload (8-byte
 * aligned, blob_bytes long): n per-sample descriptors (augment.hip struct AugSample, 328 bytes each) at offset 0, then
 * the tables, uint8 BGR sources, target offsets / values and boxes they point to by byte offset.  Descriptors whose
 * offsets or extents fall outside the blob are skipped (their output is left as it was).
 * render: every output pixel of every sample = cv2.resize (the sample's interpolation, fx = S / w, fy = S / h) of the
 * pre-resize image, NormalizeImage (uint8 canvas: lut[c][v], device [3][256]; float canvas: mean_std = HOST
 * {mean[3], std[3]} with is_scale), CHW -> out device [n][3][S][S] float32. */
int ppy_augment_render_f32(const void *blob, long long blob_bytes, int n, int S, const float *lut,
                           const double *mean_std, int is_scale, float *out, void *stream);
/* The pre-resize image of sample `index` into out (device [h][w][3] of dtype 0 uint8 / 1 float32 / 2 float64: the
 * sample's canvas dtype); h, w, dtype must match the descriptor, otherwise nothing is written.  For pinning. */
int ppy_augment_canvas(const void *blob, long long blob_bytes, int index, int h, int w, int dtype, void *out,
                       void *stream);
/* The same two calls with sources that lie OUTSIDE the blob (version 102).  A descriptor whose ext0 (ext1) field is 1 names
 * its first (mixup) source by an index into a table of n_src device images instead of a blob offset: src_ptrs[i] points to an
 * src_h[i] x src_w[i] x 3 uint8 image (BGR, pixel stride 3) with 3 * src_w[i] <= src_pitch[i] < 2^31 bytes per row and any
 * alignment -- a decoder's output, or a cropped view of a larger image, read where it lies.  The four arrays are HOST arrays
 * of length n_src (n_src = 0: the calls above); a null pointer, a non-positive extent or a short pitch is PPY_ERR_BAD_ARG.
 * The table reaches the kernels in the launch arguments, 16 entries per launch, consecutive windows sharing one entry: the
 * two external sources of one sample must lie in one window, which adjacent entries (as augment.pack_batch emits them)
 * always do.  A descriptor whose index is >= n_src, whose two indices share no window, or whose h0 / w0 (h1 / w1) differ
 * from the table entry's is skipped like any other invalid descriptor.  In-blob and external sources mix freely. */
int ppy_augment_render_src_f32(const void *blob, long long blob_bytes, int n, int S, const float *lut,
                               const double *mean_std, int is_scale, float *out, int n_src,
                               const unsigned char *const *src_ptrs, const long long *src_pitch, const int *src_h,
                               const int *src_w, void *stream);
int ppy_augment_canvas_src(const void *blob, long long blob_bytes, int index, int h, int w, int dtype, void *out,
                           int n_src, const unsigned char *const *src_ptrs, const long long *src_pitch, const int *src_h,
                           const int *src_w, void *stream);
/* Dense YOLO targets: out (device float32, total elements, 16-byte aligned) is zero-filled, then out[offsets[i]] =
 * values[i] for the n host-computed elements (device arrays, offsets unique; targets.gt2yolo_records). */
int ppy_augment_targets_f32(float *out, long long total, const long long *offsets, const float *values, int n,
                            void *stream);

/* COCO bbox evaluation (ppyolo_hip/cocoeval.py BboxEvaluator): what the reference's eval ends in, tools/cocotools.py:44-98
 * bbox_eval -> cocoapi_eval -> pycocotools COCOeval(cocoGt, cocoDt, 'bbox').evaluate() + accumulate(), bit for bit in
 * float64 (tests/cocoeval_ref.py restates it).  Records are 6 doubles (x, y, w, h, area, score) plus pair[i] = image index *
 * num_cats + category index (-1: not a record); images and categories are indexed in sorted id order.
 * records: forward_padded rows dets [n][keep_k][6] float32 (label, score, xmin, ymin, xmax, ymax) -> the reference writer's
 * record arithmetic (cocotools.py:168-186: w = xmax - xmin + 1 in float32, each bbox entry round(double(v) * 10) / 10,
 * score double(float32)), area = w * h (COCO.loadRes).  Rows at or beyond count[i] (device [n]) and rows whose class maps to
 * no GT category (cls2cat: device [num_classes], class -> category index or -1) get pair -1; img_index: device [n].  A NaN in
 * a record row sets *bad = 1 (device int).  records / pair: device [n * keep_k]. */
int ppy_cocoeval_records_f32(const float *dets, int n, int keep_k, const int *count, const int *img_index,
                             const int *cls2cat, int num_classes, int num_cats, double *records, int *pair, int *bad,
                             void *stream);
/* Workspace of ppy_cocoeval_bbox for these sizes (0 = invalid sizes). */
size_t ppy_cocoeval_workspace_bytes(long long num_records, int num_images, int num_cats, int num_gts, int num_iou_thrs,
                                    int num_areas, int num_max_dets);
/* evaluate() + accumulate() over num_records records.  GTs grouped per pair in annotation-file order: gt_off [P + 1] (P =
 * num_images * num_cats), gt_box [G][4] (x, y, w, h), gt_area [G] (the annotation's `area`), gt_crowd [G], gt_idnz [G]
 * (annotation id != 0: pycocotools reads a match to id 0 as none), gt_cat_off [num_cats + 1] (GTs per category, prefix).
 * iou_row_gts: the largest GT count of a pair (at most 4096 are used): a pair's IoU row with one detection is kept in that
 * much dynamic LDS; pairs with more GTs recompute their IoUs per chain, with the same bits.
 * Params as device doubles from numpy (iou_thrs [T], rec_thrs [R], area_rng [A][2], inclusive bounds), max_dets [M] on the
 * device and h_max_dets the same values on the host (the last one truncates each pair's list); A * T <= 64.  Outputs in
 * COCOeval.eval's layout: precision / scores [T][R][num_cats][A][M], recall [T][num_cats][A][M], -1 where pycocotools
 * leaves -1.  Repeatable bit for bit: sorts on unique keys, no atomics. */
int ppy_cocoeval_bbox(const double *records, const int *pair, long long num_records, int num_images, int num_cats,
                      const int *gt_off, const double *gt_box, const double *gt_area, const int *gt_crowd,
                      const int *gt_idnz, const int *gt_cat_off, int num_gts, int iou_row_gts,
                      const double *iou_thrs, int T,
                      const double *rec_thrs, int R, const double *area_rng, int A, const int *max_dets,
                      const int *h_max_dets, int M, double *precision, double *recall, double *scores, void *workspace,
                      size_t workspace_bytes, void *stream);

/* torch.nn.MaxPool2d(3, 2, 1) of the stem (reference model/resnet_vd.py:103, :136). */
int ppy_maxpool3x3s2_f32(const float *x, int x_ld, float *y, int y_ld, int N, int H, int W,
                         int C, void *stream);
/* torch.nn.AvgPool2d(2, 2, 0) of the vd shortcut (reference model/resnet_vd.py:30, :53). */
int ppy_avgpool2x2_f32(const float *x, int x_ld, float *y, int y_ld, int N, int H, int W, int C,
                       void *stream);
/* SPP (reference model/custom_layers.py:275-290): max-pool 5/9/13, stride 1, "same".
 * x is channel slice [0,C) of the concat buffer; the three pooled maps are written to
 * y5, y9, y13 (normally x+C, x+2C, x+3C of the same buffer), all with ld y_ld. */
int ppy_spp_f32(const float *x, int x_ld, float *y5, float *y9, float *y13, int y_ld, int N,
                int H, int W, int C, void *stream);

/* DCNv2 (reference model/custom_layers.py:551-677; arg order after
 * external/DCNv2/src/dcn_v2.h:9-23: input, weight, bias-like, offset, mask, kernel,
 * stride, pad).  `offset_mask`: NHWC [N,Ho,Wo,27] RAW output of conv_offset (18
 * (y,x)-interleaved offsets then 9 mask logits; sigmoid is applied here).
 * ppy_dcnv2_f32 is ONE kernel: every workgroup gathers the modulated bilinear samples of its
 * output tile into LDS, chunk by chunk, and contracts them on the MFMA with w [K][3][3][C],
 * then BN affine + activation -- there is no "columns" buffer; ws holds split-K partials only
 * (ppy_dcnv2_workspace_bytes; 0 without split-K).  cfg: -1 = heuristic, else
 * math scheme * (ppy_dcnv2_num_configs() / 3) + tile, schemes 0 exact fp32, 1 bf16x3 (needs
 * w_x3), 2 f16x2 (needs w_f16x2, scale_f16x2, amax_in) -- the operands of the convolution entry
 * point above.  ppy_dcnv2_sample_f32 is the stand-alone gather: columns
 * cols[N*Ho*Wo][9*C] in (tap, c) order, the same arithmetic op for op. */
int ppy_dcnv2_sample_f32(const float *x, int x_ld, const float *offset_mask, int om_ld,
                         float *cols, int N, int H, int W, int C, int Ho, int Wo, int stride,
                         int pad, void *stream);
int ppy_dcnv2_f32(const float *x, int x_ld, const float *w_krsc, const void *w_x3, const void *w_f16x2,
                  const float *scale, const float *scale_f16x2, const float *shift,
                  const float *offset_mask, int om_ld, float *y, int y_ld, int N, int H, int W, int C,
                  int K, int stride, int pad, int act, int cfg, int splitk, const float *amax_in,
                  float *amax_out, void *ws, size_t ws_bytes, void *stream);
size_t ppy_dcnv2_workspace_bytes(int N, int H, int W, int C, int K, int stride, int pad, int cfg,
                                 int splitk);
int ppy_dcnv2_num_configs(void);

/* Backward of the deformable convolution (training with freeze_at < 5; arg order after the reference's only real FFI,
 * dcn_v2_backward(input, weight, bias, offset, mask, grad_output, ...) -> [dX, dOffset, dMask, dW, dBias],
 * external/DCNv2/src/dcn_v2.h:41-55; semantics = torch autograd of the pure-PyTorch DCNv2.forward,
 * model/custom_layers.py:551-677).  dy [N,Ho,Wo,K]: gradient of the contraction output (upstream of BN / activation).
 * Written: dx [N,H,W,C] -- the SAMPLING path only, conv_offset's own data gradient is a plain convolution backward of
 * d_offset_mask and the caller's to add --, d_offset_mask [N,Ho,Wo,27] with respect to the RAW conv_offset output (18
 * offsets, 9 mask logits), dw [K][3][3][C].  dx is accumulated with float atomics (data-dependent scatter, as
 * external/DCNv2/src/cuda/dcn_v2_im2col_cuda.cu:197-262 does): not bit-reproducible run to run; d_offset_mask and dw are.
 * ws: ppy_dcnv2_backward_workspace_bytes() bytes, 256-byte aligned (the columns + the inner wgrad / dgrad workspaces). */
int ppy_dcnv2_backward_f32(const float *x, int x_ld, const float *w_krsc, const float *offset_mask, int om_ld,
                           const float *dy, int dy_ld, float *dx, int dx_ld, float *d_offset_mask, int dom_ld,
                           float *dw_krsc, int N, int H, int W, int C, int K, int stride, int pad, void *ws,
                           size_t ws_bytes, void *stream);
size_t ppy_dcnv2_backward_workspace_bytes(int N, int H, int W, int C, int K, int stride, int pad);

/* ------------------------------------------------------------------------------------
 * get_iou_aware_score + yolo_box for ONE head level (reference model/head.py:21-141),
 * fused with the `scores > score_threshold` candidate extraction of matrix_nms
 * (reference model/matrix_nms.py:110-117).
 * head_out: NHWC [N,S,S,A*(5+C) (+A if iou_aware)] with ld head_ld (channel layout as in
 * the reference: [A IoU logits] then A x [tx,ty,tw,th,obj,C classes]).
 * anchors_px: HOST pointer to A (w,h) pairs in pixels.  im_size: [N][2] = (h, w).
 * boxes: [N][M_total][4]; this level writes rows [box_offset, box_offset + S*S*A) in
 * (h, w, anchor) order.  Candidates with score > score_threshold are appended to
 * cand_key/cand_idx ([N][cand_cap]; key = order-preserving uint32 image of the fp32
 * score: bits ^ 0x80000000 for non-negative scores, ~bits for negative ones; idx =
 * box*C + class) with the running count in cand_count[N] (zero it before the first
 * level; it keeps counting past cand_cap, entries beyond cand_cap are dropped, so size
 * cand_cap = M_total*C to make that impossible).  scale_x_y / iou_aware_factor are
 * doubles because the reference derives fp32 constants from Python doubles
 * ((scale_x_y - 1.0) * 0.5, 1 - iou_aware_factor; model/head.py:40, :125).
 * scores_dense: optional [N][M_total][C] (reference layout) or NULL. */
int ppy_yolo_decode_f32(const float *head_out, int head_ld, int N, int S, int A, int num_classes,
                        const float *h_anchors_px, int downsample, double scale_x_y,
                        int iou_aware, double iou_aware_factor, int clip_bbox,
                        const float *im_size, float *boxes, int M_total, int box_offset,
                        float score_threshold, uint32_t *cand_key, uint32_t *cand_idx,
                        int *cand_count, int cand_cap, float *scores_dense, void *stream);

/* The same for ALL head levels of a model in one launch (per-level arrays of length nlevels <= 4; the anchor
 * count A is common to the levels).  No dense-score output.  Candidate order inside an image's list differs
 * from level-by-level calls (the list is an unordered set; matrix_nms orders by (score, index)). */
int ppy_yolo_decode_levels_f32(int nlevels, const float *const *head_out, const int *head_ld, const int *S,
                               const int *downsample, const float *const *h_anchors_px,
                               const int *box_offset, int N, int A, int num_classes, double scale_x_y,
                               int iou_aware, double iou_aware_factor, int clip_bbox, const float *im_size,
                               float *boxes, int M_total, float score_threshold, uint32_t *cand_key,
                               uint32_t *cand_idx, int *cand_count, int cand_cap, void *stream);

/* matrix_nms (reference model/matrix_nms.py:102-151) for a batch, from the candidate
 * lists produced by ppy_yolo_decode_f32 / ppy_nms_candidates_f32.
 * Order (this build's total order where the reference calls the unstable
 * torch.argsort): score descending, ties by ascending candidate index.
 * out_dets [N][keep_top_k][6] = (label, score, x0,y0,x1,y1), rows >= out_count[n] are
 * -1; out_count[n] == 0 <=> the reference returns its [[-1]*6] sentinel.
 * out_keep_idx [N][keep_top_k] = box*C + class of every kept row (-1 padding).
 * Limits: 1 <= nms_top_k <= 1024, 1 <= keep_top_k <= nms_top_k (PPY_ERR_UNSUPPORTED outside, nothing is clamped).
 * The first min(cand_count[n], cand_cap) entries of a list are used, in any order; a cand_cap that is not a multiple
 * of 4 is accepted (tests/test_gpu_matrix_nms.py).
 * ws: ppy_matrix_nms_workspace_bytes(N) bytes of scratch, 16-byte aligned (the sorted top-k boxes and the
 * per-column compensate / decay values travel between the kernels of one call through it; round 4: + 264 KB per image
 * for the compact list of the large-list route).
 * Lists of more than 8192 candidates (only possible when cand_cap > 8192; up to 1.8 M per image when every (box,
 * class) pair passes the threshold) are first cut down chip-wide -- a threshold from 8192 sampled keys, then one
 * streaming pass that moves every entry at or above it to a compact list and counts them -- and the top-k select
 * runs on the compact list iff that list is certain to contain the whole top-k; otherwise it walks the original
 * list.  The result is the same either way (csrc/decode_nms.hip: nms_sample_kernel, nms_collect_kernel). */
size_t ppy_matrix_nms_workspace_bytes(int N);
int ppy_matrix_nms_f32(const float *boxes, int M_total, int num_classes, const uint32_t *cand_key,
                       const uint32_t *cand_idx, const int *cand_count, int cand_cap, int N,
                       float post_threshold, int nms_top_k, int keep_top_k, int use_gaussian,
                       float gaussian_sigma, float *out_dets, int *out_count, int *out_keep_idx,
                       void *ws, size_t ws_bytes, void *stream);
/* Candidate extraction from dense scores [N][M][C] (the reference's own input form,
 * model/matrix_nms.py:110-117), for callers that hold yolo_box outputs. */
int ppy_nms_candidates_f32(const float *scores, int N, int M, int C, float score_threshold,
                           uint32_t *cand_key, uint32_t *cand_idx, int *cand_count, int cand_cap,
                           void *stream);

/* multiclass_nms (PaddleDetection's operator of that name: greedy per-class hard NMS) for a batch, from the same
 * candidate lists as ppy_matrix_nms_f32 (cand_key / cand_idx = box * C + class / cand_count, in any order).
 * Per class != background_label: the candidates by (score descending, box index ascending), the first nms_top_k of
 * them, then a greedy scan that selects a candidate iff iou <= nms_threshold holds against every box already selected
 * in that class (a NaN IoU suppresses).  iou is JaccardOverlap in fp32, one rounding per operation:
 * 0 if the boxes are disjoint, else iw * ih / ((area_a + area_b) - iw * ih) with iw = (min x2 - max x1) + norm,
 * norm = 0 if normalized else 1, area = 0 for an inverted box.  Across classes: the keep_top_k highest scores (ties to
 * the lower class, then the lower box index), emitted in (class ascending, score descending, box ascending) order.
 * Outputs as ppy_matrix_nms_f32 writes them: out_dets [N][keep_top_k][6] = (label, score, x0,y0,x1,y1), rows >=
 * out_count[n] are -1; out_keep_idx [N][keep_top_k] = box * C + class (-1 padding).  The score is the original one.
 * Limits (PPY_ERR_UNSUPPORTED outside, nothing is clamped): 1 <= nms_top_k <= 1024, 1 <= keep_top_k <= 1024,
 * nms_eta == 1 (no adaptive threshold); Paddle's -1 = "no limit" is therefore not accepted.
 * ws: ppy_multiclass_nms_workspace_bytes(N, num_classes, nms_top_k, cand_cap) bytes, 16-byte aligned
 * (= 16-byte-rounded 4 N + 8 N num_classes nms_top_k: the selections of every class before the keep_top_k cut; the
 * candidate list itself is filtered in place, so the bound does not depend on cand_cap).  No host synchronisation:
 * three launches on `stream` (csrc/multiclass_nms.hip), capturable into a graph. */
size_t ppy_multiclass_nms_workspace_bytes(int N, int num_classes, int nms_top_k, int cand_cap);
int ppy_multiclass_nms_f32(const float *boxes, int M_total, int num_classes, const uint32_t *cand_key,
                           const uint32_t *cand_idx, const int *cand_count, int cand_cap, int N,
                           int nms_top_k, int keep_top_k, float nms_threshold, int normalized, float nms_eta,
                           int background_label, float *out_dets, int *out_count, int *out_keep_idx,
                           void *ws, size_t ws_bytes, void *stream);

/* Merge of the rows of a batch of VIEWS (tiled inference: tiles of large images plus the whole image) into one list per
 * image, in the forward_padded row format (csrc/merge_views.hip).
 * dets = device float32 [V][K][6] rows (class, score, x0, y0, x1, y1) in view pixel coordinates, count = device int32 [V]
 * as forward_padded writes them.  The view table [V][3] int32 = (image, ox, oy) is given twice: h_views on the host, where
 * the limits are checked, and views, its device copy, which the kernel reads.  image = -1 marks a padding view, which is
 * ignored; the views of an image may lie anywhere in the table; n = the number of images (image < n).
 *   admission:   row r of view v iff r < min(count[v], K), all six values finite, 0 <= class < 2^24, score >= score_thresh;
 *                the class id is the truncated value
 *   translation: x0, x1 += (float)ox, y0, y1 += (float)oy: one fp32 rounding each, no clipping
 *   order:       per image, score descending as values (-0.0 ties with +0.0), then view ascending, then row ascending
 *   scan:        greedy in that order: a candidate is selected iff metric(candidate, k) <= thresh for every already selected
 *                k (class_agnostic = 0: for every selected k of the same class id); a NaN metric suppresses
 *   metric:      PPY_MERGE_IOU = JaccardOverlap as in ppy_multiclass_nms_f32 with norm = 0; PPY_MERGE_IOS = the same
 *                disjoint rule, iw, ih and inter, then inter / (area_k < area_candidate ? area_k : area_candidate)
 *   output:      the first keep_top_k selections in scan order: out_dets [n][keep_top_k][6] = the original class and score and
 *                the translated box, -1 behind out_count[n]; out_src int32 [n][keep_top_k][2] = (view, row), -1 padding
 * fp32 with one rounding per operation, no fma; no floating-point atomics: two runs give the same bytes.
 * Limits, refused and never clamped (PPY_ERR_UNSUPPORTED; h_reason, NULL or 96 chars, names the value): keep_top_k outside
 * 1..PPY_MERGE_MAX_KEEP, K < 1, an image with more than PPY_MERGE_MAX_ROWS rows ((views of the image) x K), a NaN thresh or
 * score_thresh, an unknown metric.  A null pointer, n outside 1..65535, V < 1, V x K >= 2^31 or a table entry outside
 * -1..n-1: PPY_ERR_BAD_ARG.  ws: ppy_merge_views_workspace_bytes(n, V, K) = 32 n min(V K, PPY_MERGE_MAX_ROWS) bytes (the
 * sorted candidates of every image, 32 bytes each), 16-byte aligned; it carries nothing from one call to the next.
 * No host synchronisation: one launch on `stream`, one workgroup per image, capturable into a graph. */
#define PPY_MERGE_IOU 0
#define PPY_MERGE_IOS 1
#define PPY_MERGE_MAX_ROWS 8192   /* rows of one image: the keys' stage in LDS                          */
#define PPY_MERGE_RANK_MAX 1024   /* admitted rows up to which the counting sort orders; beyond: bitonic */
#define PPY_MERGE_CHUNK 64        /* candidates per step of the greedy scan                              */
#define PPY_MERGE_MAX_KEEP 1024
size_t ppy_merge_views_workspace_bytes(int n, int V, int K);
int ppy_merge_views_f32(const float *dets, const int *count, int V, int K, const int *h_views, const int *views, int n,
                        int metric, float thresh, float score_thresh, int class_agnostic, int keep_top_k,
                        float *out_dets, int *out_count, int *out_src, void *ws, size_t ws_bytes, char *h_reason,
                        void *stream);

/* Weighted boxes fusion of the rows of a batch of VIEWS (test-time augmentation: the whole image at several input sides,
 * plain and mirrored) into one list per image, in the forward_padded row format (csrc/fuse_views.hip).
 * dets, count, V, K, n as for ppy_merge_views_f32.  The view table [V][4] int32 = (image, ox, oy, mirror_w) and the view weights
 * float32 [V] are given twice: h_views / h_view_weight on the host, where the limits are checked, and views / view_weight, their
 * device copies, which the kernel reads.  image = -1 marks a padding view: nothing of it is read or checked.
 *   transform:   mirror_w > 0: the row is mirrored in view coordinates first, nx0 = (float)mirror_w - x1, nx1 = (float)mirror_w
 *                - x0 (w - x, not w - 1 - x: the decode clips boxes to [0, w]); then x += (float)ox, y += (float)oy as
 *                ppy_merge_views_f32 translates
 *   admission:   ppy_merge_views_f32's rule, and score > 0, and a transformed box with x1 > x0 and y1 > y0
 *   weighted score: s = score * view_weight[v]
 *   order:       per image, s descending, then view ascending, then row ascending
 *   clusters:    per (image, class id), rows in that order: the row's IoU (PPY_MERGE_IOU, the row as the candidate) with the
 *                fused box of every cluster of its class; it joins the cluster with the largest IoU STRICTLY above thresh (a tie:
 *                the earliest created; a NaN IoU never matches): S += s, X[k] += s * b[k] (the product rounded, then the sum),
 *                T += 1, fused[k] = X[k] / S.  Otherwise it opens a cluster: S = s, X[k] = s * b[k], T = 1, fused = the row's box
 *                bit for bit
 *   confidence:  wsum = the fp32 sum of view_weight over the image's non-padding views in table order; q = S / (float)T,
 *                m = min((float)T, wsum), conf = (q * m) / wsum  (ensemble_boxes' conf_type = 'avg', one model per view)
 *   output:      an image's clusters by conf descending, then class ascending, then creation order; the first keep_top_k:
 *                out_dets [n][keep_top_k][6] = ((float)class id, conf, fused box), -1 behind out_count[n]; out_src int32
 *                [n][keep_top_k][2] = (view, row) of the cluster's first member; out_members int32 [n][keep_top_k] = T; -1 padding
 * fp32 with one rounding per operation, no fma; no floating-point atomics: two runs give the same bytes.
 * Limits, refused and never clamped (PPY_ERR_UNSUPPORTED; h_reason, NULL or 96 chars, names the value): keep_top_k outside
 * 1..PPY_MERGE_MAX_KEEP, K < 1, an image with more than PPY_MERGE_MAX_ROWS rows, a NaN thresh or score_thresh, a weight that is
 * not finite and positive, mirror_w < 0.  A null pointer, n outside 1..65535, V < 1, V x K >= 2^31 or a table entry outside
 * -1..n-1: PPY_ERR_BAD_ARG.  ws: ppy_fuse_views_workspace_bytes(n, V, K) = 64 n min(V K, PPY_MERGE_MAX_ROWS) bytes (per row
 * the gathered row and a cluster slot, 32 bytes each), 16-byte aligned; it carries nothing from one call to the next.
 * No host synchronisation: one launch on `stream`, one workgroup per image, capturable into a graph. */
size_t ppy_fuse_views_workspace_bytes(int n, int V, int K);
int ppy_fuse_views_f32(const float *dets, const int *count, int V, int K, const int *h_views, const int *views,
                       const float *h_view_weight, const float *view_weight, int n, float thresh, float score_thresh,
                       int keep_top_k, float *out_dets, int *out_count, int *out_src, int *out_members, void *ws,
                       size_t ws_bytes, char *h_reason, void *stream);

/* Tracking across frames: the rows of the current frame of each of n STREAMS are associated with the stream's tracks, whose
 * state lives in a caller-owned device buffer that the call reads and rewrites (csrc/track.hip).
 * ByteTrack-shaped and deterministic.  dets = device float32 [n][K][6] rows (class, score, x0, y0, x1, y1), count = device
 * int32 [n] as forward_padded writes them; count[i] < 0: stream i has no frame in this call, its state is left untouched, its
 * out_count is 0 and its outputs are -1.  h_params is read on the host during the call.
 *   state:       per stream 16 + 112 max_tracks bytes: a header of int32 (frame, ids issued, rows dropped for lack of a slot,
 *                0) and max_tracks slots of 28 words: int32 state (PPY_TRACK_FREE, _NEW, _TRACKED, _LOST), id, class, float32
 *                score, int32 hits, last (the frame of the last match), four filters for cx, cy, a = w / h, h of float32 (x, v,
 *                Ppp, Ppv, Pvv) each, two zero words.  A FREE slot is all zero; an all-zero buffer is a fresh tracker (frame 0,
 *                the first id is 1).  ids are int32 and are never reused.
 *   per call and stream, in this order:
 *   frame:       frame += 1
 *   predict:     every slot that is not FREE: if it is not TRACKED, v_h = 0; with h = x_h before the prediction, q_pos =
 *                (h / 20)^2, q_vel = (h / 160)^2, for the aspect filter q_pos = 1e-4f, q_vel = 1e-10f; per filter, from the old
 *                values: x = x + v, Ppp = ((Ppp + Ppv) + (Ppv + Pvv)) + q_pos, Ppv = Ppv + Pvv, Pvv = Pvv + q_vel
 *   box:         of a slot: w = a * h, hw = w * 0.5, hh = h * 0.5, (cx - hw, cy - hh, cx + hw, cy + hh)
 *   admission:   row r iff r < min(count, K), all six values finite, 0 <= class < 2^24 (the id is the truncated value), x1 > x0,
 *                y1 > y0 and score >= low_thresh; an admitted row is HIGH iff score >= high_thresh, else LOW
 *   association: three stages of one rule: stage 1 the HIGH rows x the TRACKED and LOST slots, IoU > match_thresh[0]; stage 2
 *                the LOW rows x the TRACKED slots stage 1 left, IoU > match_thresh[1]; stage 3 the HIGH rows stage 1 left x
 *                the NEW slots, IoU > match_thresh[2] (states as they were before this call's update).  The rule: of all pairs
 *                above the threshold (class_agnostic = 0: of equal class id), in the order IoU descending, then track id
 *                ascending, then row ascending, a pair is taken iff both its ends are still free.  IoU = PPY_MERGE_IOU's
 *                JaccardOverlap(a = the row's box, b = the slot's predicted box) with norm = 0; a NaN IoU never matches
 *   update:      a matched slot, with z = (x0 + w * 0.5, y0 + h * 0.5, w / h, h) of the row, w = x1 - x0, h = y1 - y0:
 *                r = (x_h / 20)^2 of the predicted x_h, 1e-2f for the aspect; per filter, from the old values: s = Ppp + r,
 *                kp = Ppp / s, kv = Ppv / s, y = z - x, x = x + kp * y, v = v + kv * y, Ppp = Ppp - kp * Ppp, Ppv = Ppv - kp * Ppv,
 *                Pvv = Pvv - kv * Ppv.  The slot takes the row's score and class, hits += 1, last = frame, state = TRACKED
 *   demotion:    an unmatched TRACKED slot becomes LOST, an unmatched NEW slot FREE; then every LOST slot with frame - last >
 *                max_lost becomes FREE; a slot that becomes FREE is zeroed
 *   opening:     the HIGH rows still unmatched with score >= new_thresh, in row order: the lowest FREE slot, id = ++(ids
 *                issued), state NEW (TRACKED when frame == 1), x = z, v = 0, Ppv = 0, Ppp = ((2 * h) / 20)^2 and Pvv =
 *                ((10 * h) / 160)^2 for cx, cy and h, Ppp = 1e-4f and Pvv = 1e-10f for a; the row's score and class, hits = 1,
 *                last = frame.  With no FREE slot the row is skipped and `dropped` counts it
 *   output:      the TRACKED slots matched or opened in this call, by id ascending: out_dets [n][max_tracks][6] = ((float)class,
 *                score, the slot's box after the update), out_ids, out_src (the row that matched or opened it) and out_hits
 *                int32 [n][max_tracks]; -1 behind out_count[i]
 * fp32 with one rounding per operation, no fma; no atomics: two runs give the same bytes, state included.
 * Limits, refused and never clamped (PPY_ERR_UNSUPPORTED; h_reason, NULL or 96 chars, names the value): max_tracks outside
 * 1..PPY_TRACK_MAX_TRACKS, K outside 1..PPY_TRACK_MAX_ROWS, a NaN threshold, max_lost < 0.  A null pointer, n outside 1..65535, a
 * state that is not 16-byte aligned or shorter than ppy_track_state_bytes(n, max_tracks) (0 outside the limits):
 * PPY_ERR_BAD_ARG.  ppy_track_workspace_bytes is 0 and ws may be NULL: between the load and the store of the state everything
 * lives in registers and LDS (32 bytes per slot, 36 per row); the argument stays in the signature for a form that needs scratch.
 * No host synchronisation: one launch on `stream`, one workgroup per stream, capturable into a graph (the frame counter is the
 * kernel's).  Calls on one state must be stream-ordered. */
#define PPY_TRACK_FREE 0
#define PPY_TRACK_NEW 1
#define PPY_TRACK_TRACKED 2
#define PPY_TRACK_LOST 3
#define PPY_TRACK_MAX_TRACKS 1024 /* a thread of the workgroup owns a slot; with 1024 rows 68 KB of the CU's 160 KB of LDS  */
#define PPY_TRACK_MAX_ROWS 1024   /* K: a thread owns a row                                                                 */
typedef struct ppy_track_params_t {
    float high_thresh, low_thresh, new_thresh;
    float match_thresh[3];
    int max_lost, class_agnostic;
} ppy_track_params_t;
size_t ppy_track_state_bytes(int n, int max_tracks);
size_t ppy_track_workspace_bytes(int n, int max_tracks, int K);
int ppy_track_update_f32(const float *dets, const int *count, int n, int K, int max_tracks, const ppy_track_params_t *h_params,
                         void *state, size_t state_bytes, float *out_dets, int *out_count, int *out_ids, int *out_src,
                         int *out_hits, void *ws, size_t ws_bytes, char *h_reason, void *stream);

/* ------------------------------------------------------------------------------------
 * conv2 -> conv3 of an identity bottleneck in ONE launch (round 5; reference model/resnet_vd.py:81-87:
 * relu(bn3(conv3(relu(bn2(conv2(t))))) + x)): conv A = 3x3 / stride 1 / pad 1, CA -> KA, BatchNorm, ReLU; conv B = 1x1, KA -> KB,
 * BatchNorm, + residual, ReLU.  The KA-channel intermediate stays on chip (csrc/conv_b2b.hip).  x_split: conv A's input as its
 * producer stored it pre-split (ppy_conv2d_bn_act_split_f32), xscale its [N] per-image scales, amax_in the tracked max|.| of that
 * tensor.  wA / wB + scaleA / scaleB: outputs of ppy_conv2d_split_weights_f16x2 for the two weight tensors; shiftA / shiftB the
 * folded BatchNorm shifts.  t_mul, t_add: static bound |intermediate| <= t_mul * max|x| + t_add (per-image operand scale of the
 * second contraction).  pool (or NULL) / pool_ld: [N, H/2, W/2, pool_ld] receives AvgPool2d(2, 2) of y as well (the vd shortcut of the
 * next stage, reference model/resnet_vd.py:29-33; H, W even), evaluated (((a + b) + c) + d) * 0.25 as ppy_avgpool2x2_f32.
 * Supported: CA = KA = 64, KB = 256 (stage 2 of ResNet50-vd); else PPY_ERR_UNSUPPORTED.  f16x2 arithmetic as
 * ppy_conv2d_bn_act_f32; agrees with the two-launch form to fp32 rounding. */
int ppy_conv3x3_conv1x1_f32(const float *x_split, int x_ld, const float *xscale, const float *amax_in, const void *wA_f16x2,
                            const float *scaleA_f16x2, const float *shiftA, const void *wB_f16x2, const float *scaleB_f16x2,
                            const float *shiftB, const float *residual, int res_ld, float *y, int y_ld, float *pool, int pool_ld, int N,
                            int H, int W, int CA, int KA, int KB, float t_mul, float t_add, float *amax_out, void *stream);

/* ------------------------------------------------------------------------------------
 * Lanes.  The reference evaluates one batch at a time (model/ppyolo.py:19-22, called from model/decode_np.py:142-150); this
 * path keeps several batches on the device at once, each on its own stream ("lane", ppyolo_hip/runtime.py InFlight).
 * ppy_lane_stream_create makes such a stream: mask_words == 0 -> an ordinary non-blocking stream; else h_cu_mask (HOST memory,
 * mask_words x 32 bits) restricts every kernel launched on it -- directly or as nodes of a hipGraph launched on it -- to the
 * compute units whose bit is set (hipExtStreamCreateWithCUMask).  On MI355X bit i is CU i / 8 of XCD i % 8
 * (tools/probes/cu_mask_probe.hip), so `i % 8 < 4` gives a lane four whole XCDs with their L2s.  An all-zero mask is refused.
 * These two calls are the only ones of the library that create or destroy state; they synchronise nothing. */
int ppy_lane_stream_create(void **stream, const uint32_t *h_cu_mask, int mask_words);
int ppy_lane_stream_destroy(void *stream);

/* ------------------------------------------------------------------------------------
 * Baseline JPEG decoding, bit for bit with libjpeg-turbo's defaults -- JDCT_ISLOW inverse DCT, fancy upsampling, integer YCbCr
 * tables -- i.e. the pixels of cv2.imread(path) / cv2.imdecode(buf, 1) (reference demo.py:41, tools/cocotools.py:105,
 * tools/transform.py:87), delivered as the uint8 HWC BGR device images ppy_preprocess_u8_f32 takes.  DESIGN.md section 10.
 *
 * Accepted: SOF0 / SOF1 (Huffman, 8-bit samples), one interleaved scan, 1 component (grey, replicated to B = G = R) or 3
 * (YCbCr) with chroma 1x1 and luma 1x1, 2x1 or 2x2; 8- and 16-bit quantisation tables; restart intervals; any APPn / COM
 * segments and 0xFF fill bytes.  Everything else that is a valid file -- progressive, arithmetic, lossless, 12-bit, 4
 * components, RGB (Adobe transform 0), other sampling factors, several scans -- returns PPY_ERR_UNSUPPORTED, and a file that
 * is damaged or ends early returns PPY_ERR_CORRUPT (libjpeg would fill the rest with grey and warn); both with a reason
 * string.  No input makes these functions read or write outside the buffers they are given.  Progressive files, several
 * scans and further luma sampling factors are taken on request: the _ex calls below.
 *
 * The seam between host and device is the COEFFICIENT BUFFER: int16, per component [block row][block column][64], block
 * counts those of whole MCUs, quantised values as coded, stored TRANSPOSED inside a block (index column * 8 + row; the
 * quant tables of the descriptor in the same order).  ppy_jpeg_info and ppy_jpeg_entropy_decode are plain host code: no
 * GPU call, no state, safe to call from any number of threads, one call per image.  All pointers of the first five
 * functions are HOST pointers.
 *
 * A batch: for each image ppy_jpeg_info -> coef_bytes; place the images' coefficients in one host buffer at offsets that
 * are multiples of 16 (desc.coef_base, set by the caller BEFORE or after the decode; it is preserved);
 * ppy_jpeg_entropy_decode each (it zeroes its part first); ppy_jpeg_pack_table writes the device descriptor table
 * (ppy_jpeg_table_bytes(n) bytes) for the output pointers into host memory; copy table and coefficients to the device
 * (one copy when they share a pinned buffer); ppy_jpeg_reconstruct_u8 enqueues TWO launches for the whole batch, whatever
 * the number and sizes of the images (inverse DCT into block-padded planes in the workspace; upsample + colour +
 * orientation + store).  out[i]: device uint8 [out_height][row_stride[i] bytes], pixel (y, x) channel c at
 * y * row_stride + 3 * x + c, row_stride >= 3 * out_width, any alignment.  apply_orientation != 0 applies the EXIF
 * orientation (1..8) as cv2.imread does; 0 delivers the stored raster (cv2.IMREAD_IGNORE_ORIENTATION).
 * ws: ppy_jpeg_workspace_bytes(n, descs) bytes (0 = a descriptor is invalid), 16-byte aligned; table and coef 16-byte
 * aligned.  TRUST BOUNDARY: h_descs and apply_orientation are validated on the host (geometry, coefficient ranges against
 * coef_bytes, workspace size) and size the grids; the kernels read the device table, including the output pointers and row
 * strides, WITHOUT further checks.  The table must be the one ppy_jpeg_pack_table wrote from these very descriptors with the
 * same apply_orientation, unmodified; a call that never synchronises cannot verify device memory. */
typedef struct ppy_jpeg_info_t {
    int status;                       /* the return value again */
    int width, height;                /* as stored in the file */
    int out_width, out_height;        /* after the EXIF orientation */
    int orientation;                  /* 1..8; 1 when the file has none */
    int components;                   /* 1 or 3 */
    int h_samp[3], v_samp[3];         /* sampling factors (1 x 1 for a grey file) */
    int blocks_w[3], blocks_h[3];     /* 8x8 blocks per row / column of each component */
    int restart_interval;             /* MCUs, 0 = none */
    long long coef_bytes;             /* size of the image's coefficients */
    char reason[64];                  /* why status != PPY_OK */
    int progressive;                  /* 1 for an SOF2 file (only ever under PPY_JPEG_ACCEPT_PROGRESSIVE) */
} ppy_jpeg_info_t;
typedef struct ppy_jpeg_desc_t {
    int width, height, components, orientation;
    int h_samp[3], v_samp[3];
    int blocks_w[3], blocks_h[3];
    long long coef_offset[3];         /* int16 elements from the start of the image's coefficients */
    long long coef_bytes;
    long long coef_base;              /* CALLER: byte offset of the image's coefficients in the batch buffer, % 16 == 0 */
    unsigned short quant[3][64];      /* per component, stored (transposed) order */
} ppy_jpeg_desc_t;
int ppy_jpeg_info(const unsigned char *h_data, size_t bytes, ppy_jpeg_info_t *h_info);
/* h_reason: NULL or 64 chars. */
int ppy_jpeg_entropy_decode(const unsigned char *h_data, size_t bytes, int16_t *h_coef, size_t coef_bytes,
                            ppy_jpeg_desc_t *h_desc, char *h_reason);
/* The same two calls under an ACCEPT MASK (0 = exactly the calls above, code for code and reason for reason).  Each bit lifts
 * one refusal:
 *   PPY_JPEG_ACCEPT_PROGRESSIVE  SOF2 (progressive, Huffman): DC / AC, first and refinement scans as in libjpeg's jdphuff.c;
 *   PPY_JPEG_ACCEPT_MULTISCAN    SOF0 / SOF1 files whose components come in several scans, in any grouping and order;
 *   PPY_JPEG_ACCEPT_SAMPLING     3 components with chroma 1x1 and luma h x v, h, v in 1..4, h * v <= 8 (4:4:0, 4:1:1, 4:1:0, ...).
 * DHT / DQT / DRI between scans hold for the scans that follow; a component's quantisation table is the one in force when its
 * first scan starts.  A scan of one component is not interleaved: it covers the blocks that hold image samples, and the MCU
 * padding of the coefficient buffer stays zero.  A progressive file must have sent every coefficient of every component down
 * to Al = 0 by EOI, otherwise PPY_ERR_UNSUPPORTED "incomplete progressive scan script" (libjpeg would smooth such a file
 * between blocks); a sequential file must send every component exactly once.  Scan parameters outside T.81, unknown or
 * repeated components, missing tables, data that ends early and a missing EOI are PPY_ERR_CORRUPT; more than 256 scans is
 * PPY_ERR_UNSUPPORTED.  The descriptor, the coefficient buffer and everything after them are unchanged: ppy_jpeg_pack_table
 * and ppy_jpeg_reconstruct_u8 take the further luma factors (a chroma plane at half height and full width goes through
 * libjpeg's vertical triangle filter, every other new ratio is replicated), still two launches per batch.
 * ppy_jpeg_scan_prepare (the device entropy mode) takes no mask and keeps refusing all of these. */
#define PPY_JPEG_ACCEPT_PROGRESSIVE 1u
#define PPY_JPEG_ACCEPT_MULTISCAN 2u
#define PPY_JPEG_ACCEPT_SAMPLING 4u
int ppy_jpeg_info_ex(const unsigned char *h_data, size_t bytes, unsigned accept, ppy_jpeg_info_t *h_info);
int ppy_jpeg_entropy_decode_ex(const unsigned char *h_data, size_t bytes, unsigned accept, int16_t *h_coef, size_t coef_bytes,
                               ppy_jpeg_desc_t *h_desc, char *h_reason);
size_t ppy_jpeg_workspace_bytes(int n, const ppy_jpeg_desc_t *h_descs);
size_t ppy_jpeg_table_bytes(int n);
int ppy_jpeg_pack_table(int n, const ppy_jpeg_desc_t *h_descs, unsigned char *const *h_out, const long long *h_row_stride,
                        int apply_orientation, void *h_table, size_t table_bytes);
int ppy_jpeg_reconstruct_u8(int n, const ppy_jpeg_desc_t *h_descs, int apply_orientation, const void *table, const int16_t *coef,
                            size_t coef_bytes, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Device entropy stage (opt-in): the host keeps one linear pass per file, the GPU decodes the Huffman bits into the same
 * coefficient buffer ppy_jpeg_entropy_decode fills, element for element.  DESIGN.md section 10.
 *
 * ppy_jpeg_scan_prepare (host, stateless, any thread, no GPU call) parses the markers exactly as ppy_jpeg_info does (same
 * refusals and reasons), fills h_desc exactly as ppy_jpeg_entropy_decode does (coef_base is preserved), and writes the SCAN
 * RECORD of the file into h_scan (16-byte aligned, at least ppy_jpeg_scan_bytes(h_data, bytes, NULL) bytes; that bound is
 * 0 for a file ppy_jpeg_info refuses, and *h_segments, when given, receives the number of restart segments it allows for):
 *   ppy_jpeg_scan_t | compact Huffman tables, DC then AC of each component (1424 bytes each: uint16 look[512] = length << 8 |
 *   symbol of the 9-bit lookahead, int32 maxcode[18], int32 valoff[18], uint8 vals[256]) | segment table, 4 x uint32 each:
 *   byte offset into the data, bit length, first MCU, MCU count | the entropy-coded bytes WITHOUT the stuffed 00 after FF,
 *   cut at the restart markers, every segment starting on a 4-byte boundary and zero-padded to the next.
 * The offsets in ppy_jpeg_scan_t are bytes from the start of the record.  Stream rules, those of the host decoder: a segment's
 * data ends at the first FF not followed by 00 or at the end of the file; FF fill bytes may precede a restart marker;
 * restart marker k must be D0 + (k & 7), a wrong or missing one is PPY_ERR_CORRUPT here; whatever follows the last
 * segment's data, a missing EOI included, is accepted.  *h_used receives the record's size.  h_reason: NULL or 64 chars.
 *
 * ppy_jpeg_entropy_plan (host) lays a batch out for one subsequence size: subseq_bytes is a power of two from
 * PPY_JPEG_SUBSEQ_MIN to PPY_JPEG_SUBSEQ_MAX (0 = PPY_JPEG_SUBSEQ_DEFAULT).  h_scan is the host copy of the scan buffer,
 * h_scan_off[i] the byte offset of image i's record in it (% 16 == 0).  It writes the plan (ppy_jpeg_entropy_plan_bytes(n,
 * total segments) bytes, 16-byte aligned: 64 bytes per image, then each image's first-subsequence index per segment) and
 * returns the workspace size of the decode in *h_ws_bytes.
 *
 * ppy_jpeg_entropy_device enqueues a FIXED number of launches on `stream`, whatever the images, with no host
 * synchronisation: zero the coefficients and the status words; decode every subsequence from an assumed state and
 * synchronise the states inside each workgroup; link the workgroups and prefix-sum the slot counts; decode again from the
 * true states, writing non-zero coefficients and DC differences; turn the DC differences into values (segmented scan per
 * component, reset at every restart segment, modulo 2^32 truncated to int16).  plan, scan, coef, status and ws are DEVICE
 * pointers (16-byte aligned; plan and scan are the copies of h_plan and the scan buffer); h_plan sizes the grids.
 * status: 3 * n ints -- [0, n) PPY_OK or PPY_ERR_CORRUPT per image, [n, 2n) a reason id for ppy_jpeg_reason_string, [2n, 3n)
 * how many subsequences' entry states only the cross-workgroup step fixed.  The status class equals the host decoder's on
 * every input; the coefficients of an image with a non-OK status are unspecified (every write stays inside the image's own
 * range).  TRUST BOUNDARY as for ppy_jpeg_reconstruct_u8: plan and scan must be what the two host calls wrote.
 *
 * ppy_jpeg_entropy_twin is the same decoder on the host, lane by lane over host memory, through the same decode step,
 * state comparison and slot-to-address map: same arguments (all pointers HOST pointers, no stream), same outputs.  Slow;
 * it exists so that damaged inputs can be swept without a GPU (tools/jpeg_twin_asan.cpp). */
#define PPY_JPEG_SUBSEQ_MIN 8
#define PPY_JPEG_SUBSEQ_MAX 4096
#define PPY_JPEG_SUBSEQ_DEFAULT 32
typedef struct ppy_jpeg_scan_t {
    int components, mcus_w, mcus_h, restart_interval;
    int h_samp[3], v_samp[3], blocks_w[3];
    int segments, mcus;               /* restart segments; MCUs of the image */
    int reserved;
    long long coef_offset[3];         /* as in ppy_jpeg_desc_t */
    long long coef_elems;
    unsigned int table_offset, segment_offset, data_offset, data_bytes, record_bytes, reserved2;
} ppy_jpeg_scan_t;
size_t ppy_jpeg_scan_bytes(const unsigned char *h_data, size_t bytes, long long *h_segments);
int ppy_jpeg_scan_prepare(const unsigned char *h_data, size_t bytes, void *h_scan, size_t scan_bytes, size_t *h_used,
                          ppy_jpeg_desc_t *h_desc, char *h_reason);
size_t ppy_jpeg_entropy_plan_bytes(int n, long long segments);
int ppy_jpeg_entropy_plan(int n, const ppy_jpeg_desc_t *h_descs, const void *h_scan, size_t scan_bytes, const long long *h_scan_off,
                          int subseq_bytes, void *h_plan, size_t plan_bytes, size_t *h_ws_bytes);
int ppy_jpeg_entropy_device(int n, const void *h_plan, const void *plan, const void *scan, int subseq_bytes, int16_t *coef,
                            size_t coef_bytes, int *status, void *ws, size_t ws_bytes, void *stream);
int ppy_jpeg_entropy_twin(int n, const void *h_plan, const void *plan, const void *scan, int subseq_bytes, int16_t *coef,
                          size_t coef_bytes, int *status, void *ws, size_t ws_bytes);
const char *ppy_jpeg_reason_string(int reason);

/* ------------------------------------------------------------------------------------
 * Baseline JPEG ENCODING, byte for byte with libjpeg-turbo's defaults -- jpeg_set_defaults, jpeg_set_quality(q, TRUE),
 * JDCT_ISLOW forward DCT, the standard (Annex K) Huffman tables without optimize_coding, a JFIF 1.01 header with units 0 and
 * density 1:1 -- i.e. the file cv2.imwrite(path, img, [IMWRITE_JPEG_QUALITY, q]) writes (reference demo.py:50) and Pillow's
 * Image.save(buf, 'JPEG', quality=q, subsampling=s, restart_marker_blocks=r).  DESIGN.md section 10b.
 *
 * Input: uint8 DEVICE images, components = 3 (HWC BGR, pixel stride 3; written as YCbCr with luma sampling h_samp x v_samp =
 * 1x1, 2x1 or 2x2 and chroma 1x1) or components = 1 ([h][w]; written as a one-component file, the sampling is ignored);
 * pixel (y, x) channel c at src + y * row_stride + components * x + c, row_stride >= components * width, any alignment.
 * width and height 1..65535.  quality 1..100, restart_interval 0..65535 MCUs.
 *
 * The seam between the stages is the COEFFICIENT BUFFER of the decoder above (int16, per component [block row][block
 * column][64], whole-MCU block counts, stored transposed), so what stage 1 writes ppy_jpeg_reconstruct_u8 can read and what
 * ppy_jpeg_entropy_decode writes stage 2 can code.
 *
 * A batch: fill src, row_stride, width, height, components of every descriptor; ppy_jpeg_enc_layout validates them, fills
 * the rest (geometry; coef_base, ws_base = the image's byte offsets in the batch buffers; scan_capacity) and the four buffer
 * sizes; ppy_jpeg_enc_pack_table writes the device table (sizes.table_bytes) into host memory; copy it to the device;
 *   stage 1  ppy_jpeg_enc_coefficients: ONE launch for the whole batch, whatever the number and sizes of the images:
 *            colour conversion, edge replication, downsampling, forward DCT, quantisation, dummy blocks; integer only;
 *   stage 2  ppy_jpeg_enc_scan_device: EIGHT launches, no host synchronisation: bits per block | segmented prefix sum per
 *            image and the restart segments' byte offsets | zero the unstuffed stream | write the bits (OR into zeroed words:
 *            order-independent, so run-to-run identical) with each segment's 1-bit tail fill | 0xFF count per 64-byte
 *            chunk | prefix sum per image, length per image | offsets of the images in `out` | stuffed write with RSTn.
 *            out receives the images' entropy-coded bytes back to back (image i at the sum of the lengths before it, no
 *            header, no EOI), lengths[i] their sizes.  Every byte of ws it reads it has written in the same call.
 * CAPACITY: one block codes to at most 22 + 63 * 26 = 1660 bits (DC: 11-bit code + 11; AC: 16-bit code + 10), < 208 bytes,
 * every byte may be stuffed, and every restart segment adds at most one stuffed fill byte and a 2-byte marker:
 *   ppy_jpeg_enc_scan_capacity(blocks, segments) = 416 * blocks + 4 * segments.
 * out_bytes below the sum of the images' capacities is refused on the host (PPY_ERR_WORKSPACE), never overrun.  The device
 * stage keeps 32-bit positions: an image whose capacity is above 2^29 is PPY_ERR_UNSUPPORTED in ppy_jpeg_enc_scan_device
 * (the host twin takes it).
 * ppy_jpeg_enc_scan_host is the host twin of stage 2 for ONE image: plain C++, stateless, no GPU call, any thread; the same
 * bytes from the same coefficients (h_coef = the image's own coefficients, desc.coef_bytes of them; coef_base is not read).
 * ppy_jpeg_enc_header writes SOI .. SOS for one image (ppy_jpeg_enc_header_bytes of them); the file is header | scan | FF D9.
 * ppy_jpeg_enc_quant: the two quantiser tables of a quality, 64 entries each in natural (row-major) order.
 * TRUST BOUNDARY as for the decoder: parameters and descriptors are validated on the host and size the grids; the kernels
 * read the device table, source pointers and row strides included, WITHOUT further checks.  The table must be the one
 * ppy_jpeg_enc_pack_table wrote from these very descriptors.  Bad arguments return PPY_ERR_BAD_ARG, a sampling outside the
 * three PPY_ERR_UNSUPPORTED; h_reason (NULL or 64 chars) says why. */
typedef struct ppy_jpeg_enc_params_t {
    int quality;                      /* 1..100 */
    int h_samp, v_samp;               /* luma sampling factors: 1x1 (4:4:4), 2x1 (4:2:2), 2x2 (4:2:0) */
    int restart_interval;             /* MCUs, 0 = none */
} ppy_jpeg_enc_params_t;
typedef struct ppy_jpeg_enc_desc_t {
    const unsigned char *src;         /* CALLER: device image */
    long long row_stride;             /* CALLER: bytes */
    int width, height, components;    /* CALLER */
    int restart_interval;
    int h_samp[3], v_samp[3];
    int blocks_w[3], blocks_h[3];     /* 8x8 blocks per row / column of each component, whole MCUs */
    int real_w[3], real_h[3];         /* of which hold samples: ceil(component size / 8); the others are dummy blocks */
    int mcus_w, mcus_h;
    long long blocks, segments;       /* blocks of the image; restart segments (1 without restarts) */
    long long coef_offset[3];         /* int16 elements from the start of the image's coefficients */
    long long coef_bytes, coef_base;  /* size, and byte offset in the batch coefficient buffer (% 16 == 0) */
    long long scan_capacity;          /* ppy_jpeg_enc_scan_capacity(blocks, segments) */
    long long ws_bytes, ws_base;      /* stage 2 workspace of the image and its byte offset (% 16 == 0) */
} ppy_jpeg_enc_desc_t;
typedef struct ppy_jpeg_enc_sizes_t {
    size_t table_bytes, coef_bytes, ws_bytes, out_bytes;
} ppy_jpeg_enc_sizes_t;
int ppy_jpeg_enc_quant(int quality, unsigned short *h_luma, unsigned short *h_chroma);
size_t ppy_jpeg_enc_header_bytes(int components, int restart_interval);
int ppy_jpeg_enc_header(const ppy_jpeg_enc_params_t *h_params, int width, int height, int components, unsigned char *h_out,
                        size_t capacity, size_t *h_used, char *h_reason);
size_t ppy_jpeg_enc_scan_capacity(long long blocks, long long segments);
int ppy_jpeg_enc_layout(const ppy_jpeg_enc_params_t *h_params, int n, ppy_jpeg_enc_desc_t *h_descs, ppy_jpeg_enc_sizes_t *h_sizes,
                        char *h_reason);
int ppy_jpeg_enc_pack_table(const ppy_jpeg_enc_params_t *h_params, int n, const ppy_jpeg_enc_desc_t *h_descs, void *h_table,
                            size_t table_bytes);
int ppy_jpeg_enc_coefficients(int n, const ppy_jpeg_enc_desc_t *h_descs, const void *table, int16_t *coef, size_t coef_bytes,
                              void *stream);
int ppy_jpeg_enc_scan_device(int n, const ppy_jpeg_enc_desc_t *h_descs, const void *table, const int16_t *coef, size_t coef_bytes,
                             unsigned char *out, size_t out_bytes, unsigned long long *lengths, void *ws, size_t ws_bytes,
                             void *stream);
int ppy_jpeg_enc_scan_host(const ppy_jpeg_enc_desc_t *h_desc, const int16_t *h_coef, size_t coef_bytes, unsigned char *h_out,
                           size_t capacity, size_t *h_len, char *h_reason);

/* ------------------------------------------------------------------------------------
 * Drawing detections: the reference's Decode.draw (model/decode_np.py:98-123) on device images, in place, ONE launch per
 * batch, no host synchronisation, no workspace, no atomics; bit for bit what a sequential painter of the rules below gives,
 * whatever the scheduling (every pixel is stored by the last row that covers it, and by nobody else).  The rows, their
 * order, the rounding, the colours, the label string and the placement are the reference's; the GLYPHS are Pillow's built-in
 * bitmap font (6 x 11 cells), not OpenCV's Hershey font -- cv2.putText is not pinned.  DESIGN.md section 10c.
 *
 * Image i: h x w pixels of 3 bytes, pixel (y, x) at base + y * pitch + 3 * x, pitch >= 3 * w, any alignment (a decoder's
 * output, or a crop of a larger image, drawn where it lies).  h, w in 1..65535.  The colour triple of a class is stored in
 * memory order (on a BGR image, as cv2 does with the reference's tuples).
 * dets: device [n][K][6] float32 rows (class, score, x0, y0, x1, y1), count: device [n] int32 -- what forward_padded returns.
 *   DRAWN  rows r < min(count[i], K) with score >= draw_thresh, 0 <= class < num_classes, 0 <= score <= 1 and all six values
 *          finite; every other row is skipped.  Rows are drawn in row order, a later row over an earlier one; per row the
 *          outline, then the label background, then the text.
 *   CORNERS left = max(0, floor(x0 + 0.5)), top = max(0, floor(y0 + 0.5)), right = min(w, floor(x1 + 0.5)), bottom =
 *          min(h, floor(y1 + 0.5)); sum and floor in float32, clamped to +-2^30 before the conversion.
 *   OUTLINE the four edges of the rectangle (left, top) .. (right, bottom), corners inclusive and in either order, one pixel
 *          thick, class colour, clipped (right == w and bottom == h lie outside).  A flat box is one row, a thin one one column.
 *   LABEL  name + ": " + d.dd with the digits of rint(float64(score) * 100), ties to even (= '%.2f').  tw = 6 * length,
 *          th = 11.  Background: filled rectangle (left, top) .. (left + tw, top - th - 3), inclusive, class colour, clipped.
 *          Text: black, its cell grid's top left corner at (left, top - th - 2), clipped.
 *   FONT   font: device [95][16] bytes, characters 32..126 (any other is drawn as '?'): gx0 + 1, gy0, gx1 + 1, gy1, 0, then
 *          the 11 rows of the band, bit c + 1 = column c of the cell, -1 <= c < 6 (ppyolo_hip/label_font.py device_table).
 *          Glyph i of the string owns [6 i + gx0, 6 i + gx1) x [gy0, gy1); glyphs are pasted in string order, a pixel takes
 *          the bit of the LAST glyph whose rectangle contains it.  A set bit is black, a clear bit leaves the background.
 * colors: device [num_classes][3] bytes.  names: device [num_classes][64] character codes, name_len: device [num_classes]
 * int32; h_name_len: the same lengths on the HOST.  h_images: HOST array of the n descriptors, images: its DEVICE copy.
 * TRUST BOUNDARY: the host arrays are validated and size the grid; the kernel reads the device copies without further
 * checks, except that every store is clipped to the descriptor's h x w and a class outside [0, num_classes) reads no table.
 * K outside 1..1024, num_classes < 1 or a name longer than 64 characters is PPY_ERR_UNSUPPORTED; a null pointer, n outside
 * 1..65535, an extent outside 1..65535 or a short pitch PPY_ERR_BAD_ARG. */
typedef struct ppy_draw_image_t {
    unsigned char *base;
    long long pitch;                  /* bytes per row */
    int h, w;
} ppy_draw_image_t;
int ppy_draw_detections_u8(int n, const ppy_draw_image_t *h_images, const ppy_draw_image_t *images, const float *dets,
                           const int *count, int K, float draw_thresh, const unsigned char *colors, int num_classes,
                           const unsigned char *names, const int *name_len, const int *h_name_len, const unsigned char *font,
                           void *stream);

/* ------------------------------------------------------------------------------------
 * GroupNorm and Mish of Conv2dUnit (reference model/custom_layers.py:37-43, :118-135; csrc/norm_act.hip).  Both work on the
 * NHWC view (ptr, ld, N, H, W, C) every op takes: ld >= C, C and ld multiples of 4, pointers 16-byte aligned.
 *
 * ppy_group_norm_f32: torch.nn.GroupNorm(groups, C) of the RAW convolution output x -- statistics per (image, group) over
 * H * W * C / groups elements, biased variance, eps inside the square root -- then `* gamma + beta`, [+ residual], act
 * (PPY_ACT_NONE / _RELU / _LEAKY / _MISH): the residual is added after the affine and before the activation, the block-level
 * relu(x + shortcut).  y may be a channel slice of a wider buffer; upsample2x != 0: y is the [N, 2H, 2W, C] destination and every
 * pixel is stored to its 2 x 2 nearest-neighbour positions.  Three launches on `stream`, no host synchronisation, no
 * floating-point atomics: sums of d = x - k and d * d per (image, pixel chunk, group) in double, k the group's own first element,
 * combined in a fixed order, so the result is bit-identical from run to run and safe when a group's mean is large against its
 * spread (no E[x^2] - E[x]^2 of the raw values; the mean stays a double up to `x - mean`).  ws: PPY_GN_WS_BYTES(N, groups) bytes, 8-byte aligned, owned by the call until the stream has run it.
 * C % groups != 0 or a short workspace: PPY_ERR_BAD_ARG / PPY_ERR_WORKSPACE; C > 2048: PPY_ERR_UNSUPPORTED.
 *
 * ppy_mish_f32: x * tanh(softplus(x)) in place, softplus with torch's threshold (x > 20: x), evaluated as
 * x * n / (n + 2) with n = e^x (e^x + 2), which has no cancellation. */
#define PPY_ACT_MISH 3 /* norm_act.hip only: the convolution entry points reject it */
#define PPY_GN_MAX_CHUNKS 128
#define PPY_GN_WS_BYTES(N, groups) ((size_t)(N) * (size_t)(groups) * (PPY_GN_MAX_CHUNKS * 16 + 16))
int ppy_group_norm_f32(const float *x, int x_ld, const float *gamma, const float *beta, int groups, float eps, int act,
                       const float *residual, int res_ld, float *y, int y_ld, int upsample2x, int N, int H, int W, int C,
                       void *ws, size_t ws_bytes, void *stream);
int ppy_mish_f32(float *x, int x_ld, int N, int H, int W, int C, void *stream);

/* ------------------------------------------------------------------------------------
 * GroupNorm, AffineChannel and Mish in the TRAINING step (csrc/norm_act.hip, csrc/norm_act_train.hip).  Views
 * and alignment as above; every reduction is a double sum combined in a fixed order (no floating-point atomics, bit-identical from
 * run to run), no call synchronises with the host, every workspace is the caller's.
 *
 * ppy_group_norm_train_f32: ppy_group_norm_f32 (the same three launches, the same values bit for bit, no upsampled store) that
 * also leaves the statistics in the caller's mean [N * groups] (double) and rstd [N * groups] (float), which the caller keeps
 * until the backward has run.  ws: PPY_GN_WS_BYTES(N, groups).
 *
 * ppy_group_norm_bwd_f32: given the raw x, those statistics and dy = d loss / d y:  z = gamma * xhat + beta [+ residual] is
 * recomputed from x (never taken from y: Mish is not invertible), dz = dy * act'(z) -- relu / leaky by the sign of z, the forward's
 * own pattern; Mish: n / (n + 2) + z * 4 e (e + 1) / (n + 2)^2 with e = exp(z), n = e (e + 2), evaluated in double; z > 20: 1 --
 *   dbeta_c = sum dz, dgamma_c = sum dz * xhat over images and pixels;   per (image, group), m = H * W * C / groups:
 *   A = sum gamma_c * dz, B = sum gamma_c * dz * xhat;   dx = rstd * (gamma_c * dz - A / m - xhat * B / m).
 * dx is written; dgamma / dbeta are written (not accumulated) when param_grads != 0 and left untouched otherwise (frozen norm);
 * dz (or NULL) receives dz, the gradient of the residual branch.  ws: ppy_group_norm_bwd_workspace_bytes, 8-byte aligned.
 * C % groups != 0, a NULL or misaligned pointer: PPY_ERR_BAD_ARG; a short workspace: PPY_ERR_WORKSPACE; C > 2048: PPY_ERR_UNSUPPORTED.
 *
 * ppy_affine_act_f32: y = act(x * weight_c + bias_c [+ residual]), act any of the four -- the forward of a TRAINABLE AffineChannel
 * unit behind its raw convolution (a frozen one is folded into the convolution's epilogue).
 * ppy_affine_bwd_f32: z recomputed as above; dz = dy * act'(z), dweight_c = sum dz * x, dbias_c = sum dz, dx = dz * weight_c; the
 * same param_grads / dz rules (ws is needed with param_grads only).  This is NOT ppy_bn_train_bwd_f32 with mean 0 and invstd 1,
 * which subtracts batch means.
 *
 * ppy_mish_bwd_f32: dx = dy * mish'(x * scale_c + shift_c) (scale / shift NULL: 1 / 0): behind a bn + mish or af + mish unit, the
 * pre-activation recomputed from the raw convolution output and the norm's per-channel scale and shift.  dx may alias dy. */
int ppy_group_norm_train_f32(const float *x, int x_ld, const float *gamma, const float *beta, int groups, float eps, int act,
                             const float *residual, int res_ld, float *y, int y_ld, int N, int H, int W, int C, double *mean,
                             float *rstd, void *ws, size_t ws_bytes, void *stream);
size_t ppy_group_norm_bwd_workspace_bytes(int N, int H, int W, int C, int groups);
int ppy_group_norm_bwd_f32(const float *x, int x_ld, const double *mean, const float *rstd, const float *gamma, const float *beta,
                           int groups, int act, const float *residual, int res_ld, const float *dy, int dy_ld, float *dx, int dx_ld,
                           float *dz, int dz_ld, float *dgamma, float *dbeta, int param_grads, int N, int H, int W, int C, void *ws,
                           size_t ws_bytes, void *stream);
int ppy_affine_act_f32(const float *x, int x_ld, const float *weight, const float *bias, int act, const float *residual, int res_ld,
                       float *y, int y_ld, int N, int H, int W, int C, void *stream);
size_t ppy_affine_bwd_workspace_bytes(int N, int H, int W, int C);
int ppy_affine_bwd_f32(const float *x, int x_ld, const float *weight, const float *bias, int act, const float *residual, int res_ld,
                       const float *dy, int dy_ld, float *dx, int dx_ld, float *dz, int dz_ld, float *dweight, float *dbias,
                       int param_grads, int N, int H, int W, int C, void *ws, size_t ws_bytes, void *stream);
int ppy_mish_bwd_f32(const float *x, int x_ld, const float *scale, const float *shift, const float *dy, int dy_ld, float *dx, int dx_ld,
                     int N, int H, int W, int C, void *stream);

/* ------------------------------------------------------------------------------------
 * PNG reconstruction: inflated scanline streams -> the uint8 HWC BGR device images cv2.imread(path) gives for a PNG file
 * (reference demo.py:41, tools/cocotools.py:105, tools/transform.py:87; pinned to Pillow / libpng).
 * The library links no zlib: the caller walks the chunks (signature, CRCs, IHDR, PLTE), inflates the concatenated IDAT data
 * and hands in, per image, the SCANLINE STREAM -- for the single image or for each non-empty Adam7 pass in turn, rows of
 * 1 filter-type byte + ceil(cols * channels * depth / 8) bytes -- and a descriptor.  ppyolo_hip/png.py is that caller in Python.
 *
 * Accepted: colour types 0, 2, 3, 4, 6 at every bit depth the PNG specification pairs them with; interlace 0 or 1.  Grey is
 * replicated to B = G = R (depth 1 / 2 / 4 scaled by 255 / 85 / 17), a palette index is looked up in `palette` (an index at or
 * past palette_entries gives black), an alpha channel is dropped, a 16-bit sample gives its high byte.
 *
 * A batch: place the streams in one buffer at offsets that are multiples of 16 (desc.scan_offset), each followed by padding up
 * to the next multiple of 16; ppy_png_pack_table writes the device descriptor table (ppy_png_table_bytes(n) bytes, palettes
 * included) for the output pointers into host memory; copy table and streams to the device (one copy when they share a pinned
 * buffer); ppy_png_reconstruct_u8 enqueues ONE launch for the whole batch, one workgroup per (image, Adam7 pass), and never
 * synchronises.  out[i]: device uint8 [height][row_stride[i] bytes], pixel (y, x) channel c at y * row_stride + 3 * x + c,
 * row_stride >= 3 * width, any alignment.  ws: ppy_png_workspace_bytes(n, descs) bytes (0 = a descriptor is invalid), 16-byte
 * aligned (the last row of each band of 1024 rows is handed to the next band through it); table and scan 16-byte aligned.
 * A filter-type byte above 4 is the caller's to refuse; the kernel reads such a row as filter 0.
 * TRUST BOUNDARY as for ppy_jpeg_reconstruct_u8: h_descs are validated on the host (geometry, scan_bytes against the
 * expected length, stream ranges against the buffer, workspace size) and size the launch; the kernel reads the device table,
 * output pointers and row strides included, WITHOUT further checks.  The table must be the one ppy_png_pack_table wrote from
 * these very descriptors, unmodified. */
typedef struct ppy_png_desc_t {
    int width, height;                /* 1..65535 */
    int bit_depth, colour_type;       /* as in IHDR */
    int interlace;                    /* 0, or 1 = Adam7 */
    int palette_entries;              /* 0..256; colour type 3 needs at least 1 */
    long long scan_offset;            /* CALLER: byte offset of the image's stream in the scan buffer, % 16 == 0 */
    long long scan_bytes;             /* its length: the sum over non-empty passes of rows * (1 + row bytes), exactly */
    unsigned char palette[768];       /* PLTE: R, G, B per entry */
} ppy_png_desc_t;
size_t ppy_png_table_bytes(int n);
int ppy_png_pack_table(int n, const ppy_png_desc_t *h_descs, unsigned char *const *h_out, const long long *h_row_stride, void *h_table,
                       size_t table_bytes);
size_t ppy_png_workspace_bytes(int n, const ppy_png_desc_t *h_descs);
int ppy_png_reconstruct_u8(int n, const ppy_png_desc_t *h_descs, const void *table, const void *scan, size_t scan_bytes, void *ws,
                           size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PPYOLO_HIP_H_ */
