/*
 * vosdet.h -- C ABI of the MI355X (gfx950) per-frame Mask R-CNN hot path.
 *
 * Library: vosdetectron_amd/libvosdet.so (built by __graft_entry__.build()).
 * Plain C: raw device pointers, sizes and an explicit stream (a hipStream_t
 * passed as void*, NULL = the null stream).  No torch types.  Every call is
 * asynchronous on `stream`, performs no allocation, no host<->device copy and
 * no synchronisation (graph-capturable), and returns a status code instead of
 * the reference's fprintf + exit(-1) (roi_align_kernel.cu:135-139).
 *
 * Each entry point cites the reference interface it replaces.  Numerics follow
 * the reference functions cited in the kernel sources; see DESIGN.md.
 */
#ifndef VOSDET_H_
#define VOSDET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VD_MAX_LEVELS 5

enum {
    VD_OK = 0,
    VD_ERR_ARG = 1,       /* bad argument (e.g. rois row width != 5) */
    VD_ERR_SHAPE = 2,     /* shape outside what the kernel supports */
    VD_ERR_LAUNCH = 3,    /* kernel launch failed */
    VD_ERR_WORKSPACE = 4  /* workspace too small */
};

enum { VD_LAYOUT_NCHW = 0, VD_LAYOUT_NHWC = 1 };

/* Per-frame failure codes written in place of a device count (never a valid
 * count; downstream kernels treat a negative count as an empty frame and keep it):
 *   VD_COUNT_SELECT_FAILED   the proposal top-k could not bracket pre_nms_topN
 *   VD_COUNT_PREV_BOXES      NMS_SMALL_BOX_IOU: the previous frame kept more
 *                            than one box of a class (vos_test.py:848 asserts) */
#define VD_COUNT_SELECT_FAILED (-1)
#define VD_COUNT_PREV_BOXES (-2)

int vd_version(void);
const char *vd_status_string(int status);

/* ---------------------------------------------------------------------------
 * RoIAlign (Caffe2-exact).  Replaces
 *   int roi_align_forward_cuda(int aligned_height, int aligned_width,
 *       float spatial_scale, int sampling_ratio, THCudaTensor *features,
 *       THCudaTensor *rois, THCudaTensor *output)
 *   lib/modeling/roi_xfrom/roi_align/src/roi_align_cuda.h:1-2, .c:7-40.
 * features: B x C x H x W fp32 NCHW contiguous; rois: num_rois x roi_cols fp32
 * [batch, x1, y1, x2, y2] in input-image coordinates; output: num_rois x C x
 * aligned_height x aligned_width (written entirely).  roi_cols != 5 ->
 * VD_ERR_ARG (the reference silently returns 0 with the output untouched).
 * ------------------------------------------------------------------------- */
int vd_roi_align_forward(int aligned_height, int aligned_width, float spatial_scale,
                         int sampling_ratio, const float *features, int B, int C, int H, int W,
                         const float *rois, int num_rois, int roi_cols, float *output,
                         void *stream);

/* Replaces roi_align_backward_cuda (roi_align_cuda.h:4-5, .c:42-76).
 * bottom_grad (B x C x H x W) must be zero-filled by the caller (as the
 * reference's RoIAlignFunction.backward does, functions/roi_align.py:40-45);
 * contributions are accumulated with fp32 atomics. */
int vd_roi_align_backward(int aligned_height, int aligned_width, float spatial_scale,
                          int sampling_ratio, const float *top_grad, int B, int C, int H, int W,
                          const float *rois, int num_rois, int roi_cols, float *bottom_grad,
                          void *stream);

/* Multi-level FPN RoIAlign: the whole per-level loop + cat + unshuffle of
 * Generalized_RCNN.roi_feature_transform (lib/modeling/model_builder.py:252-303)
 * in one launch.  Level l of the pyramid is levels[l]; roi r is pooled from
 * levels[roi_level[r]] (roi_level == NULL -> level 0) and written to output
 * row r, i.e. already in the order the reference restores with
 * `_idx_restore_int32`.  layout: VD_LAYOUT_NHWC (B x H x W x C, the product
 * layout; C % 4 == 0) or VD_LAYOUT_NCHW.  roi_order (optional): a permutation
 * that only changes the order in which RoIs are scheduled (L2 locality), never
 * the output placement.  output_layout: VD_LAYOUT_NCHW -> num_rois x C x ah x aw
 * (the reference's layout), VD_LAYOUT_NHWC -> num_rois x ah x aw x C (NHWC
 * input, ah == aw in {7, 14}; what channels_last heads consume). */
typedef struct {
    const float *data;
    int H;
    int W;
    float spatial_scale;
} VdFeatLevel;

int vd_roi_align_fpn_forward(const VdFeatLevel *levels, int num_levels, int B, int C, int layout,
                             const float *rois, const int32_t *roi_level,
                             const int32_t *roi_order, int num_rois, int aligned_height,
                             int aligned_width, int sampling_ratio, int output_layout,
                             float *output, void *stream);

/* Tile-binned, LDS-staged multi-level RoIAlign: the same operation as
 * vd_roi_align_fpn_forward(layout = output_layout = VD_LAYOUT_NHWC,
 * aligned_height = aligned_width = aligned_size) -- the per-level loop + cat +
 * unshuffle of roi_feature_transform (lib/modeling/model_builder.py:252-303)
 * over the Caffe2 RoIAlign of lib/modeling/roi_xfrom/roi_align/src/
 * roi_align_kernel.cu:65-121 -- computed in the reference's per-sample
 * arithmetic (bit-identical to it).  Serves sampling_ratio 2, C % 32 == 0,
 * B <= 64, aligned_size <= 64; returns VD_ERR_SHAPE otherwise (callers then use
 * vd_roi_align_fpn_forward).  workspace: >= vd_roi_align_fpn_tiled_workspace_size()
 * bytes of device memory, stream-ordered (no host sync, graph-capturable). */
size_t vd_roi_align_fpn_tiled_workspace_size(const VdFeatLevel *levels, int num_levels, int B,
                                             int C, int num_rois, int aligned_size);
int vd_roi_align_fpn_tiled_forward(const VdFeatLevel *levels, int num_levels, int B, int C,
                                   const float *rois, const int32_t *roi_level, int num_rois,
                                   int aligned_size, int sampling_ratio, float *output,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* jwyang RoIAlign (legacy, lib/model/roi_align).  Replaces
 * roi_align_forward_cuda(int aligned_height, int aligned_width, float
 * spatial_scale, THCudaTensor *features, THCudaTensor *rois, THCudaTensor
 * *output)  lib/model/roi_align/src/roi_align_cuda.c. */
int vd_roi_align_legacy_forward(int aligned_height, int aligned_width, float spatial_scale,
                                const float *features, int B, int C, int H, int W,
                                const float *rois, int num_rois, float *output, void *stream);

/* RoIPool.  Replaces roi_pooling_forward_cuda(int pooled_height, int
 * pooled_width, float spatial_scale, THCudaTensor *features, THCudaTensor
 * *rois, THCudaTensor *output, THCudaIntTensor *argmax)
 * lib/model/roi_pooling/src/roi_pooling_cuda.c:7.  argmax may be NULL. */
int vd_roi_pool_forward(int pooled_height, int pooled_width, float spatial_scale,
                        const float *features, int B, int C, int H, int W, const float *rois,
                        int num_rois, float *output, int32_t *argmax, void *stream);
/* Replaces roi_pooling_backward_cuda (roi_pooling_cuda.c): scatter top_grad
 * into the zero-filled bottom_grad at argmax (fp32 atomics). */
int vd_roi_pool_backward(const float *top_grad, const int32_t *argmax, int64_t num_outputs,
                         float *bottom_grad, void *stream);

/* RoICrop bilinear sampler.  Replaces BilinearSamplerBHWD_updateOutput_cuda(
 * THCudaTensor *inputImages, THCudaTensor *grids, THCudaTensor *output)
 * lib/model/roi_crop/src/roi_crop_cuda.c:15.  input B x C x H x W, grid
 * R x GH x GW x 2 in (y, x) order in [-1, 1]; output R x C x GH x GW must be
 * zero-filled by the caller (samples with every tap outside keep the zero). */
int vd_roi_crop_forward(const float *input, int B, int C, int H, int W, const float *grid_yx,
                        int num_rois, int GH, int GW, float *output, void *stream);

/* 1x1 convolution on channels_last tensors as a GEMM with the conv epilogue
 * fused (hipBLASLt): D[M][N] = act(A[M][K] . W[N][K]^T + bias[N] (+ R[M][N])),
 * row-major fp32, act = ReLU when relu != 0.  With bias = the folded frozen-BN
 * shift and R = the block input, this is the whole tail of the reference's
 * bottleneck_transformation (lib/modeling/ResNet.py:246-294: conv3 ->
 * AffineChannel2d -> + residual -> ReLU) in one kernel.  residual may be NULL.
 * workspace: >= vd_gemm_workspace_size() bytes, stream-ordered.  Not a
 * replacement for a reference custom op (those convs run in PyTorch there);
 * it removes the separate epilogue pass over the conv output. */
size_t vd_gemm_workspace_size(void);
/* The key under which this process applies pinned GEMM plans (VOSDET_GEMM_PLANS):
 * "<arch> hipblaslt-<version>-<git revision> cu<CUs>" of the current device; a
 * plans file's "# key ..." line must equal it for the pins below it to apply. */
int vd_gemm_plans_key(char *buf, int n);
/* The GEMM plans this process has made, one line per shape:
 * "M N K relu has_res own|blas workspace_bytes".  A plan with workspace_bytes > 0
 * keeps inter-workgroup state (split-K partials, stream-K fix-up flags) in the
 * caller's workspace, so two launches that may run concurrently (two captured
 * steps replayed on two streams) must be given different workspaces.
 * VD_ERR_WORKSPACE when n bytes cannot hold the list. */
int vd_gemm_plan_list(char *buf, int n);
int vd_gemm_bias_act(const float *A, int M, int K, const float *W, int N, const float *bias,
                     const float *residual, int relu, float *D, void *workspace,
                     size_t workspace_bytes, void *stream);

/* The same GEMM (D[M][N] = act(A[M][K] . W[N][K]^T + bias[N] (+ R[M][N])), fp32
 * in and out) on the bf16 matrix cores at fp32 accuracy: every operand is split
 * into three bf16 pieces carrying its 24-bit significand and the six largest piece
 * products are accumulated in fp32 (csrc/gemm_split3.hip; error measured against
 * fp64 beside torch's fp32 GEMM in tests/test_gemm_split3_gpu.py).  Wp is the
 * weight in split form, vd_gemm_split3_weight_size(N, K) bytes, made once per
 * model by vd_gemm_split3_weight.  K a multiple of 32, N of 64 (VD_ERR_SHAPE
 * otherwise); residual may be NULL.  A2 / K2 > 0 (a multiple of 16): the last K2 of the K
 * input channels come from a second [M][K2] operand (A is then [M][K - K2]): a stage's
 * first block, conv3 of h and the stride-1 downsample of x as ONE GEMM (ResNet.py:246-294
 * with basic_bn_shortcut :195-205).  up_h, up_w > 0 (both even): residual is the
 * top-down map of an FPN level, images x up_h/2 x up_w/2 x N, added at the nearest-2x
 * row of each of the M = images x up_h x up_w pixels after the bias -- the FPN
 * top-down lateral step (FPN.py:292-300) in one launch.  sub_h, sub_w > 0: A is an
 * images x sub_h x sub_w NHWC map read at stride 2 (M = images x ceil(sub_h/2) x
 * ceil(sub_w/2)): a stage's stride-2 1x1 convs (ResNet.py:246-294 with STRIDE_1X1, and
 * the downsample shortcut) without the subsampled copy.  cfg 0 picks the tile shape
 * (1: 256 pixels x 256 channels, 2: 256 x 128, 3: 256 x 64, 4: 128 x 128, 5: 256 x 256 in
 * eight waves per workgroup;
 * VD_ERR_SHAPE when N does not divide by the tile's channels).  a_bias (K - K2 floats,
 * or NULL): A's channels enter as relu(A + a_bias[k]) -- the bias + ReLU of the layer
 * that produced A, applied in fp32 before the split (bit-identical to a separate
 * pass; ResNeXt's grouped conv2 runs on MIOpen without them).  Replaces the same
 * fp32 convolutions / Linear layers as vd_gemm_bias_act (ResNet.py:246-294
 * bottleneck 1x1s, fast_rcnn_heads.py fc6 / fc7, mask_rcnn_heads.py upconv5). */
size_t vd_gemm_split3_weight_size(int N, int K);
int vd_gemm_split3_weight(const float *W, int N, int K, void *Wp, void *stream);
int vd_gemm_split3_bias_act(const float *A, int M, int K, const float *A2, int K2,
                            const float *a_bias, const void *Wp, int N, const float *bias,
                            const float *residual, int up_h, int up_w, int sub_h, int sub_w,
                            int relu, float *D, int cfg, void *stream);

/* The mask head's tail in one split-bf16 GEMM launch: the 2x2 / 2 transposed conv
 * upconv5 + ReLU (mask_rcnn_heads.py:62-68) and the class-selected 1x1 mask logits +
 * sigmoid (mask_rcnn_outputs, mask_rcnn_heads.py:20-35, at each RoI's class as
 * segm_results reads them, test.py:801-855): X = the RoI maps, M = RoIs x P x P
 * NHWC rows of K = 256 channels; Wp = vd_gemm_split3_weight of the upconv weight as
 * [(i, j, co) = 1024][K]; bias [1024] = the upconv bias per (i, j); cls_w [classes][256],
 * cls_b [classes]; roi_ch [RoIs] the class channel of each RoI; masks [RoIs][2P][2P]
 * = sigmoid(sum_co relu(upconv)[2y+i][2x+j][co] * cls_w[ch][co] + cls_b[ch]).  The
 * M x 1024 upconv output never reaches HBM. */
int vd_mask_head_upconv_logits(const float *X, int M, int K, const void *Wp, const float *bias,
                               const float *cls_w, const float *cls_b, const int32_t *roi_ch,
                               int P, float *masks, void *stream);

/* vd_gemm_split3_bias_act's GEMM with three fp16 products per fp32 product instead of
 * six bf16 ones (csrc/gemm_split3.hip, SCH = 1; the error-corrected fp16 scheme of Ootomo
 * & Yokota with one common scale): with S = 2^11, A is split into a0 = fp16(a) and a1 =
 * fp16(S (a - a0)) as it is loaded, the weight row n is scaled by the power of two r_n
 * that brings its largest magnitude into [1, 2) and kept as Wm = fp16(S r_n w), Wr =
 * fp16(S r_n w - Wm), W0 = fp16(r_n w); acc += a0 Wr + a1 W0 + a0 Wm on
 * v_mfma_f32_32x32x16_f16, then acc / (S r_n) (exact), bias, residual, ReLU as above.
 * Wp: vd_gemm_h2_weight_size(N, K) bytes (the three images, N * K * 6, then N floats
 * 1 / (S r_n)), made once per weight by vd_gemm_h2_weight.  Same arguments, shapes,
 * cfg 0-5 and status codes as vd_gemm_split3_bias_act.
 * Input contract: the result is at fp32's error level (tests/test_gemm_h2_gpu.py: against
 * fp64 beside torch's fp32 GEMM) for activations whose largest magnitude lies in
 * [2^-10, 65504].  An activation above 65504 makes a0 infinite and its output row
 * non-finite, never a finite wrong value; below 2^-10 the per-element floor of 2^-36
 * (fp16's subnormal spacing under the scale S) shows against the result.  Weights of any
 * finite fp32 magnitude are covered by the row scale (a row of fp32 subnormals only is
 * scaled as if its largest magnitude were 2^-126).  vd_mask_head_upconv_logits_h2 is
 * vd_mask_head_upconv_logits on this scheme (Wp from vd_gemm_h2_weight). */
size_t vd_gemm_h2_weight_size(int N, int K);
int vd_gemm_h2_weight(const float *W, int N, int K, void *Wp, void *stream);
int vd_gemm_h2_bias_act(const float *A, int M, int K, const float *A2, int K2,
                        const float *a_bias, const void *Wp, int N, const float *bias,
                        const float *residual, int up_h, int up_w, int sub_h, int sub_w,
                        int relu, float *D, int cfg, void *stream);
int vd_mask_head_upconv_logits_h2(const float *X, int M, int K, const void *Wp,
                                  const float *bias, const float *cls_w, const float *cls_b,
                                  const int32_t *roi_ch, int P, float *masks, void *stream);

/* 3x3 stride-1 pad-1 convolution of a channels_last (NHWC) fp32 tensor with
 * the bias (+ ReLU) epilogue fused, one hand-written MFMA implicit-GEMM kernel:
 * Y[n][y][x][co] = act(sum_{ky,kx,ci} X[n][y+ky-1][x+kx-1][ci] W2[co][ky][kx][ci]
 * + bias[co]), out-of-image taps zero.  W2 is the PyTorch weight [Cout][Cin][3][3]
 * permuted to [Cout][3][3][Cin].  bias may be NULL.  The FPN posthoc convs
 * (lib/modeling/FPN.py:227-258), the RPN conv (FPN.py:376-422) and the mask head
 * convs (mask_rcnn_heads.py:178-188) run in PyTorch in the reference.
 * Requires Cin % 64 == 0 and Cout % 128 == 0 or Cout == 64 (VD_ERR_SHAPE otherwise). */
int vd_conv3x3_bias_act(const float *X, int N, int H, int W, int C, const float *W2, int Cout,
                        const float *bias, int relu, float *Y, void *stream);

/* The same convolution by Winograd F(2x2, 3x3) on the MFMA pipes (2.25x fewer
 * multiplies; the transforms add, subtract and halve): U from
 * vd_conv3x3_wino_weight (16 x Cout x Cin fp32 in an opaque chunk-blocked order,
 * once per model) replaces W2.  Both require Cin % 8 == 0 and Cout % 64 == 0
 * (VD_ERR_SHAPE otherwise).  Results agree with the direct form within fp32
 * rounding (not bit for bit). */
int vd_conv3x3_wino_weight(const float *w, int Cout, int Cin, float *U, void *stream);
int vd_conv3x3_wino_bias_act(const float *X, int N, int H, int W, int C, const float *U,
                             int Cout, const float *bias, int relu, float *Y, void *stream);

/* The same convolution by Winograd F(4x4, 3x3) (round 5; 4x fewer multiplies than
 * the direct form, 1.78x fewer than F(2x2); transforms scale by up to 8, so a few
 * times F(2x2)'s rounding error): U from vd_conv3x3_wino4_weight (36 x Cout x Cin
 * fp32, opaque fragment order).  Cin % 8 == 0, Cin <= 4096, Cout % 64 == 0
 * (VD_ERR_SHAPE otherwise).  Replaces the same PyTorch convolutions as above. */
int vd_conv3x3_wino4_weight(const float *w, int Cout, int Cin, float *U, void *stream);
int vd_conv3x3_wino4_bias_act(const float *X, int N, int H, int W, int C, const float *U,
                              int Cout, const float *bias, int relu, float *Y, void *stream);
/* The same over N small maps (H, W <= 15: the mask head's 14 x 14 RoI features,
 * mask_rcnn_heads.py:178-188), two maps per 16 x 32 output block -- eight in 8 x 8
 * cells when H, W <= 7 (C4's res5 head on 7 x 7 RoI maps, ResNet.py:17-155) -- each
 * padded by its own zeros: bit-identical to vd_conv3x3_wino4_bias_act, which gives
 * every map a block of its own.  VD_ERR_SHAPE for larger maps. */
int vd_conv3x3_wino4_mosaic_bias_act(const float *X, int N, int H, int W, int C, const float *U,
                                     int Cout, const float *bias, int relu, float *Y,
                                     void *stream);
/* The same over N maps stacked at a pitch of H + 1 rows and W + 1 columns, both rounded
 * up to 4 (each map padded by its own zeros, every 4 x 4 tile inside one map), g maps
 * per stack row, so the output blocks run on through the stack: for sizes that leave
 * most of a map's last block row or column empty (50 x 84 res4 / P4, 25 x 42 res5).
 * g and the block shape come from the block plan (below).  Bit-identical to
 * vd_conv3x3_wino4_bias_act; VD_ERR_SHAPE when N H W C >= 2^31. */
int vd_conv3x3_wino4_rows_bias_act(const float *X, int N, int H, int W, int C, const float *U,
                                   int Cout, const float *bias, int relu, float *Y,
                                   void *stream);
/* The block plan of vd_conv3x3_wino4_bias_act (mode 0) and of the stacked entries
 * (mode 1: vd_conv3x3_wino4_rows_bias_act, vd_conv3x3_wino4_grouped_bias_act with rows)
 * on a device of n_cu compute units.  A workgroup computes a whole output block, so a
 * launch's time follows its block count: the plan picks the block shape (wide 16 x 32
 * or tall 32 x 16 pixels) and, in mode 1, the maps per stack row g that need the fewest
 * rounds of workgroups, then the fewest blocks; ties keep wide, g = 1.  Every plan gives
 * the same bits.  out = {shape (0 wide, 1 tall), g, spatial blocks, rounds}.  Needs no
 * GPU.  VOSDET_WINO4_PLAN (read at every call and every launch): "0" wide, g = 1;
 * "tall,<g>" / "wide,<g>" forced (g clamped to 1..min(N, 64); 1 in mode 0); unset
 * automatic; anything else VD_ERR_ARG. */
int vd_conv3x3_wino4_plan(int N, int H, int W, int C, int Cout, int mode, int n_cu,
                          int out[4]);
/* A grouped 3x3 convolution (ResNeXt's conv2, ResNet.py:246-294 with groups > 1; C
 * in = out channels, C / groups dividing 64) by the same F(4x4) kernel: every 64-channel
 * output block reads only the 64 input channels of its groups.  U =
 * vd_conv3x3_wino4_weight of the block-diagonal expansion of the [C][C / groups][3][3]
 * weight to [C][64][3][3] (zeros between groups; Cin = 64).  rows != 0: the N maps as
 * the row stack of vd_conv3x3_wino4_rows_bias_act.  VD_ERR_SHAPE for other shapes. */
int vd_conv3x3_wino4_grouped_bias_act(const float *X, int N, int H, int W, int C,
                                      const float *U, int groups, const float *bias, int relu,
                                      float *Y, int rows, void *stream);
/* A 3x3 convolution with dilation 2 and padding 2 (the VOS mask head, MRCNN.DILATION = 2,
 * mask_rcnn_heads.py:178-188) of N maps of H x W (H, W even) by the same F(4x4) kernel:
 * it is the plain pad-1 conv of the 4 N polyphase sub-maps of H/2 x W/2 (output (2i +
 * a, 2j + b) reads only parity-(a, b) inputs at sub-map distance 1), which the kernel
 * reads and writes in place in the full maps.  layout: the sub-maps one per block (0),
 * as pairs / octets (1, H/2, W/2 <= 15) or as the shared-separator grid (2).  U from
 * vd_conv3x3_wino4_weight of the same weight. */
int vd_conv3x3_wino4_dilated2_bias_act(const float *X, int N, int H, int W, int C,
                                       const float *U, int Cout, const float *bias, int relu,
                                       float *Y, int layout, void *stream);
/* The same over N maps laid out as a 2-D grid at a pitch of (H + 1) x (W + 1) -- one
 * zero row / column shared between neighbours, g maps per grid row chosen for the
 * fewest 16 x 32 output blocks (round 6; the mask head's 14 x 14 RoI maps: 32 per
 * 480-column row, 87 % of each block real output against 77 % for map pairs).  Tiles
 * straddle maps, so the result equals vd_conv3x3_wino4_bias_act's within Winograd
 * rounding, not bitwise; each output is still its own map's zero-padded convolution.
 * VD_ERR_SHAPE when N H W C >= 2^31 or H, W > 255. */
int vd_conv3x3_wino4_grid_bias_act(const float *X, int N, int H, int W, int C, const float *U,
                                   int Cout, const float *bias, int relu, float *Y,
                                   void *stream);

/* The Winograd convolution of R images of seg_h x W pixels stored back to back
 * (R x seg_h x W x C, i.e. one H = R * seg_h image), each padded by its own zeros:
 * the mask head's RoI maps run as one mosaic, so the 8 x 16-pixel blocks are not
 * split at every 14-row map.  seg_h even, H % seg_h == 0; bit-identical to
 * vd_conv3x3_wino_bias_act on the R images. */
int vd_conv3x3_wino_seg_bias_act(const float *X, int H, int W, int C, const float *U, int Cout,
                                 const float *bias, int relu, int seg_h, float *Y, void *stream);

/* The Winograd convolution of R maps of H x W pixels (R x H x W x C, each padded by
 * its own zeros) run as one 2-D mosaic: g maps side by side per mosaic row, g the
 * least count with g * W a multiple of 16, so neither the 8-row nor the 16-column
 * side of a pixel block is split at a map edge (the mask head's 14 x 14 RoI maps:
 * 8 per row, 112 columns).  An odd H or W gets one phantom row / column per map
 * (reads 0, never stored).  Output in the input's R x H x W layout; bit-identical to
 * vd_conv3x3_wino_bias_act on the R maps. */
int vd_conv3x3_wino_mosaic_bias_act(const float *X, int R, int H, int W, int C, const float *U,
                                    int Cout, const float *bias, int relu, float *Y, void *stream);

/* Two 1x1 convolutions of two channels_last inputs summed, with the epilogue:
 * D[M][N] = act(A1[M][K1] . W[:, :K1]^T + A2[M][K2] . W[:, K1:]^T + bias[N]),
 * W = [W1 | W2] as N x (K1 + K2) row-major.  With A1 = the bottleneck's conv2
 * output, A2 = the block input, W = [W3 | Wdownsample] and bias = b3 + bd, this
 * is a ResNet stage's first block tail (ResNet.py:246-294 with the stride-1
 * basic_bn_shortcut, :195-205) without the downsample tensor's HBM round trip.
 * One hand-written MFMA kernel (K1 = K2 = 64, N = 256: res2 of the R-50/R-101
 * FPN bodies); other shapes return VD_ERR_SHAPE (callers use vd_gemm_bias_act
 * with the downsample output as the residual). */
int vd_gemm_dual_bias_act(const float *A1, int K1, const float *A2, int K2, int M, const float *W,
                          int N, const float *bias, int relu, float *D, void *stream);

/* The FPN top-down lateral step in one MFMA GEMM with the nearest-2x add fused
 * (replaces lib/modeling/FPN.py:292-300 topdown_lateral_module.forward, which runs
 * in PyTorch in the reference: lat = conv_lateral(lateral); td = F.upsample(top,
 * scale_factor=2, mode='nearest'); return lat + td):
 *   D[p][co] = (A[p] . W[co] + bias[co]) + top[up(p)][co]
 * A: M x K NHWC rows of the lateral (M = images x H x W), top: images x H/2 x W/2 x N
 * (NULL: no top-down term), D: M x N.  H, W even.  Wf from vd_fpn_lateral_weight
 * (W [N][K] row-major -> an opaque fragment order, K x N fp32, once per model).
 * N == 256 and K in {256, 512, 1024}; VD_ERR_SHAPE otherwise. */
int vd_fpn_lateral_weight(const float *W, int N, int K, float *Wf, void *stream);
int vd_fpn_lateral_topdown(const float *A, int64_t M, int K, const float *Wf, int N,
                           const float *bias, const float *top, int H, int W, float *D,
                           void *stream);

/* ---------------------------------------------------------------------------
 * NMS with the semantics of the NMS the reference executes,
 * utils.boxes.nms -> cython_nms.nms (lib/utils/boxes.py:329-333,
 * lib/utils/cython_nms.pyx:37-87): dets n x det_stride fp32 [x1,y1,x2,y2,score,..],
 * processing order score-descending (ties: higher index first), suppression
 * when IoU (+1 convention) >= thresh, kept indices written ascending to
 * keep_out (int64), their count to *num_out (device int32).  n <= 8192.
 * Stands in for the reference's unused GPU path nms_cuda(THCudaIntTensor
 * *keep_out, THCudaTensor *boxes, THCudaIntTensor *num_out, float thresh)
 * (lib/model/nms/src/nms_cuda.c:8-19) WITH THE CYTHON SEMANTICS above: it is
 * not a drop-in for nms_cuda's own rule, which suppresses on IoU > thresh
 * (strict) over pre-sorted input (lib/model/nms/src/nms_cuda_kernel.cu:78). */
size_t vd_nms_workspace_size(int n);
int vd_nms(const float *dets, int n, int det_stride, float thresh, int64_t *keep_out,
           int32_t *num_out, void *workspace, size_t workspace_bytes, void *stream);

/* The VOS fork's mask-IoU NMS, lib_vos/tools/vos_test.py:985-1029
 * nms_with_mask_iou (applied at :113-118 when TEST.NMS_WITH_MASK_IOU > 0) on one
 * frame's n detections (n <= 1024) in cls_boxes (class-major) order:
 * planes n x im_h x im_w uint8 (the pasted, thresholded segms, nonzero = set),
 * dets n x det_stride fp32 (score at column 4), classes n int32.  Score order
 * (np.argsort(-s), ties by index), position j discarded by an earlier kept i
 * when inter / (|m_i| + 1e-6) or inter / (|m_j| + 1e-6) > iou_th (float64), then
 * at most max_per_class (TEST.NUM_DET_PER_CLASS_POST) per class.  Writes the
 * kept detection indices in the reference's output order (class ascending, then
 * score order) to keep_out and their count to *num_out (device int32).
 * workspace: >= vd_mask_iou_nms_workspace_size(n, im_h, im_w) bytes. */
size_t vd_mask_iou_nms_workspace_size(int n, int im_h, int im_w);
int vd_mask_iou_nms(const uint8_t *planes, int n, int im_h, int im_w, const float *dets,
                    int det_stride, const int32_t *classes, double iou_th, int max_per_class,
                    int64_t *keep_out, int32_t *num_out, void *workspace, size_t workspace_bytes,
                    void *stream);

/* TEST.NMS_SMALL_BOX_IOU of the fork's box_results_with_nms_and_limit
 * (lib_vos/tools/vos_test.py:845-860), in place on the device detections of F
 * frames (dets [F][det_cap][5], classes, counts, class-major as vd_box_detections
 * writes them): for each class whose previous-frame result (prev_* of the same
 * row, [F][prev_cap]) holds one box with score >= score_thresh, the class's
 * boxes with IoU (bb_intersection_over_union, float32) < iou_thresh are dropped;
 * order kept.  A previous result with several boxes of one class (the reference
 * asserts for every class, vos_test.py:846-848) sets the frame's count to
 * VD_COUNT_PREV_BOXES.  det_cap <= 1024. */
int vd_detections_prev_box_filter(float *dets, int32_t *classes, int32_t *counts, int F,
                                  int det_cap, const float *prev_dets,
                                  const int32_t *prev_classes, const int32_t *prev_counts,
                                  int prev_cap, float iou_thresh, float score_thresh,
                                  void *stream);

/* FPN level of each RoI: utils/fpn.py:11-28 map_rois_to_fpn_levels
 * (floor(lvl0 + log2(sqrt(area)/s0 + 1e-6)) clipped to [k_min, k_max]).
 * rois: R x roi_stride, the box at columns [col0, col0+4). */
int vd_map_rois_to_fpn_levels(const float *rois, int roi_stride, int col0, int R, int k_min,
                              int k_max, float canonical_scale, float canonical_level,
                              int32_t *lvl_out, void *stream);

/* The mask-head batch of im_detect_mask for all frames of a step, sized
 * without a host read of the detection counts (lib/core/test.py:366-402:
 * _get_rois_blob :877-906 -- box * im_scale as a float64 product stored as
 * float32 -- and _add_multilevel_rois_for_test :909-927).  Detection j of
 * frame f (j < counts[f], vd_box_detections' outputs) is global row
 * prefix(counts)[f] + j, frame-major; rows [row0, row0 + rows) are written:
 * rois_out [rows][5] = (f, x1, y1, x2, y2), lvl_out = FPN level - k_min,
 * cls_out = its class.  Output rows past the total are padding (zero box,
 * level 0, class 1).  total_out[0] = sum(counts) (may exceed row0 + rows: the
 * caller runs a second batch from row0 = rows for those).  im_scale: F doubles. */
int vd_mask_rois(const float *dets, const int32_t *classes, const int32_t *counts,
                 int num_images, int det_cap, const double *im_scale, int row0, int rows,
                 int k_min, int k_max, float canonical_scale, float canonical_level,
                 float *rois_out, int32_t *lvl_out, int32_t *cls_out, int32_t *total_out,
                 void *stream);

/* ---------------------------------------------------------------------------
 * RPN proposals for all FPN levels and images in one launch: per (image,
 * level) GenerateProposalsOp.forward / proposals_for_one_image
 * (lib/modeling/generate_proposals.py:20-168): top pre_nms_topN by score,
 * anchor shift + bbox_transform (boxes.py:156-205), clip to im_info
 * (boxes.py:138-153), _filter_boxes (:171-182), NMS, keep[:post_nms_topN].
 * cls_prob: N x A x H x W, bbox_pred: N x 4A x H x W (conv outputs, NCHW),
 * anchors: A x 4 float64 (generate_anchors.py), im_info: N x 3 device fp32.
 * Outputs per (image i, level l), slot base (i*num_levels + l)*post_nms_topN:
 * rois_out [.][5] = (i, x1, y1, x2, y2), probs_out [.], counts_out[i*L+l].
 * pre_nms_topN <= 2048 per level. */
typedef struct {
    const float *cls_prob;
    const float *bbox_pred;
    const double *anchors;
    int A;
    int H;
    int W;
    float spatial_scale;
} VdRpnLevel;

size_t vd_generate_proposals_workspace_size(const VdRpnLevel *levels, int num_levels,
                                            int num_images, int pre_nms_topN);
int vd_generate_proposals(const VdRpnLevel *levels, int num_levels, int num_images,
                          const float *im_info, int pre_nms_topN, int post_nms_topN,
                          float nms_thresh, float min_size, float *rois_out, float *probs_out,
                          int32_t *counts_out, void *workspace, size_t workspace_bytes,
                          void *stream);

/* collect() + distribute() of CollectAndDistributeFpnRpnProposalsOp at
 * inference (lib/modeling/collect_and_distribute_fpn_rpn_proposals.py:91-138),
 * per image: concatenate the per-level proposals (level-major), keep the top
 * post_nms_topN by score (ties: lower concatenation index first), and give
 * each kept RoI its FPN level (utils/fpn.py:11-28).  Inputs are the outputs of
 * vd_generate_proposals (level_cap = its post_nms_topN).  Outputs per image i:
 * rois_out[i*post_nms_topN + r][5], lvl_out[.] (level index k - k_min),
 * count_out[i]. */
int vd_collect_distribute(const float *level_rois, const float *level_probs,
                          const int32_t *level_counts, int num_levels, int level_cap,
                          int num_images, int post_nms_topN, int k_min, int k_max,
                          float *rois_out, int32_t *lvl_out, int32_t *count_out, void *stream);

/* Box-head post-processing for each image: im_detect_bbox's decode + clip
 * (lib/core/test.py:157-184; bbox_transform with BBOX_REG_WEIGHTS, clip to the
 * original image) followed by box_results_with_nms_and_limit (test.py:733-797;
 * fork fix lib_vos/tools/vos_test.py:748-865): per class j >= 1 score >=
 * score_thresh, NMS, then the top dets_per_im over all classes (score >= the
 * dets_per_im-th largest).  rois: num_images x R_cap x 5 (first roi_count[i]
 * valid), cls_prob: . x R_cap x K, bbox_pred: . x R_cap x 4K, im_scale[i],
 * im_hw[i] = original (height, width) as int32.  Outputs per image i (det_cap
 * slots): dets_out[.][5] = (x1, y1, x2, y2, score) ordered by class then
 * proposal index (np.vstack order), det_cls_out[.] class id,
 * det_count_out[i]. */
size_t vd_box_detections_workspace_size(int R_cap, int num_images, int num_classes);
int vd_box_detections(const float *rois, const float *cls_prob, const float *bbox_pred,
                      const int32_t *roi_count, int R_cap, int num_images, int num_classes,
                      const float *im_scale, const int32_t *im_hw, float score_thresh,
                      float nms_thresh, int dets_per_im, const float *bbox_reg_weights,
                      int det_cap, float *dets_out, int32_t *det_cls_out,
                      int32_t *det_count_out, void *workspace, size_t workspace_bytes,
                      void *stream);

/* vd_box_detections with the inference options of box_results_with_nms_and_limit
 * (lib/core/test.py:756-776):
 *  soft_nms_method  -1 = the NMS above; 0 hard / 1 linear / 2 gaussian =
 *                   TEST.SOFT_NMS (utils/boxes.py:336-355 -> cython_nms.soft_nms,
 *                   cython_nms.pyx:98-203; overlap threshold nms_thresh, sigma,
 *                   min score 0.0001 at test.py:760): the class's rows in soft-NMS
 *                   output order with decayed scores;
 *  bbox_vote_method -1 = off; 0 ID / 1 AVG / 2 IOU_AVG / 3 QUASI_SUM =
 *                   TEST.BBOX_VOTE.SCORING_METHOD (utils/boxes.py:277-333, voters:
 *                   bbox_overlaps >= bbox_vote_thresh among the class's candidates;
 *                   QUASI_SUM's beta = bbox_vote_beta).  GENERALIZED_AVG at beta 1
 *                   is AVG; TEMP_AVG is not offered.
 * Bit-exact to the compiled reference in this container (tests/golden/soft_nms.npz). */
int vd_box_detections_ex(const float *rois, const float *cls_prob, const float *bbox_pred,
                         const int32_t *roi_count, int R_cap, int num_images, int num_classes,
                         const float *im_scale, const int32_t *im_hw, float score_thresh,
                         float nms_thresh, int dets_per_im, const float *bbox_reg_weights,
                         int soft_nms_method, float soft_nms_sigma, float soft_nms_min_score,
                         int bbox_vote_method, float bbox_vote_thresh, float bbox_vote_beta,
                         int det_cap, float *dets_out, int32_t *det_cls_out,
                         int32_t *det_count_out, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ResNet stem in one pass (basic_bn_stem, lib/modeling/ResNet.py:224-230, with
 * the AffineChannel folded into the bias): MaxPool 3x3/2 pad 1 (ReLU (conv1 7x7/2
 * pad 3 (x) + bias)), conv1 3 -> 64 channels on the MFMA pipes; the conv output
 * stays in LDS.  x: N x H x W x 3 fp32 (NHWC, the channels_last blob); y: N x Ho x
 * Wo x 64 (Ho = ((H - 1) / 2) / 2 + 1 ...).  vd_stem_weight_pack reorders the
 * PyTorch weight [64][3][7][7] into vd_stem_weight_size() bytes once. */
size_t vd_stem_weight_size(void);
int vd_stem_weight_pack(const float *w, float *packed, void *stream);
int vd_stem_conv_pool(const float *x, int N, int H, int W, const float *packed, const float *bias,
                      float *y, void *stream);

/* The same stem with conv1 on the bf16 matrix cores at fp32 accuracy (round 6; the
 * three-piece bf16 split of gemm_split3, six piece products per fp32 product, fp32
 * accumulate): vd_stem_split_weight_pack splits the PyTorch weight [64][3][7][7] into
 * vd_stem_split_weight_size() bytes once; vd_stem_split_conv_pool takes that image and
 * is otherwise vd_stem_conv_pool. */
size_t vd_stem_split_weight_size(void);
int vd_stem_split_weight_pack(const float *w, void *packed, void *stream);
int vd_stem_split_conv_pool(const float *x, int N, int H, int W, const void *packed,
                            const float *bias, float *y, void *stream);

/* utils.boxes.soft_nms (lib/utils/boxes.py:336-355 -> cython_nms.soft_nms,
 * cython_nms.pyx:98-203) on the device: dets n x dets_stride (>= 5) float32
 * [x1, y1, x2, y2, score]; method 0 hard / 1 linear / 2 gaussian.  Writes the
 * count_out[0] = N surviving rows (dets_out N x 5, decayed scores, in the
 * reference's output order) and their input indices (keep_out).  n <= 4096;
 * one wavefront (the reference loop is sequential in its selections). */
int vd_soft_nms(const float *dets, int n, int dets_stride, float sigma, float overlap_thresh,
                float score_thresh, int method, float *dets_out, int64_t *keep_out,
                int32_t *count_out, void *stream);

/* utils.boxes.box_voting (lib/utils/boxes.py:277-333): every top row becomes
 * the score-weighted average of the rows of all_dets whose bbox_overlaps
 * (cython_bbox.pyx, float32) with it is >= thresh, in numpy's summation order;
 * scoring_method 0 ID / 1 AVG / 2 IOU_AVG / 3 QUASI_SUM (beta).  out: n_top x 5.
 * n_all <= 4096. */
int vd_box_voting(const float *top_dets, int n_top, int top_stride, const float *all_dets,
                  int n_all, int all_stride, float thresh, int scoring_method, float beta,
                  float *out, void *stream);

/* Frame preparation, lib/utils/blob.py:37-114 at identity scale (im_scale 1): u8 BGR frames
 * (F x H x W x 3) -> fp32 blob minus PIXEL_MEANS, zero-padded to Hp x Wp
 * (multiples of FPN.COARSEST_STRIDE).  lut[3*256] = float32(u - mean_c) for
 * every byte value (numpy's float64 subtraction, then the float32 store).
 * nhwc = 0 -> F x 3 x Hp x Wp, 1 -> F x Hp x Wp x 3. */
int vd_image_to_blob(const uint8_t *frames, int F, int H, int W, const float *lut, int Hp,
                     int Wp, int nhwc, float *blob, void *stream);

/* Frame preparation at any scale: prep_im_for_blob (lib/utils/blob.py:117-139,
 * driven by get_image_blob :37-60 and tools/infer_simple.py:142-149) --
 * float32(BGR) - PIXEL_MEANS, cv2.resize(fx = fy = im_scale, INTER_LINEAR) to
 * Hr x Wr (= rint(H * im_scale), rint(W * im_scale), cv::resize's dsize) --
 * then zero-padded to Hp x Wp like vd_image_to_blob.  The resize restates
 * OpenCV's scalar float INTER_LINEAR path (scale = 1 / im_scale in double,
 * coefficient tables, horizontal then vertical pass, see misc.hip); cv2 is not
 * importable in the build container, so this step's parity against an executed
 * cv2 is unpinned (it is pinned against the numpy restatement and known answers). */
int vd_image_resize_to_blob(const uint8_t *frames, int F, int H, int W, const float *lut,
                            double im_scale, int Hr, int Wr, int Hp, int Wp, int nhwc,
                            float *blob, void *stream);

/* The blob of an aspect-ratio view of the test-time augmentation (lib/core/test.py:
 * 330-363, 509-526, 684-702) in one launch:
 *   im_ar = cv2.resize(im, dsize=(War, H)), War = int(round(ar * W))
 *           (lib/utils/image.py:27-32: u8 -> u8 INTER_LINEAR of the width alone),
 *   the network sees im_ar[:, ::-1] when hflip != 0,
 *   then vd_image_resize_to_blob's steps on that H x War image at im_scale
 *   (Hr x Wr = rint(H * im_scale), rint(War * im_scale); the 2 x 2 area path at
 *   im_scale == 0.5), zero-padded to Hp x Wp.
 * im_ar is never written: each of its pixels that the float resize taps is made
 * from two horizontally adjacent bytes of the frame by OpenCV's 8-bit fixed-point
 * path (scale = 1 / ((double)War / W); fx = (float)((dx + 0.5) * scale - 0.5), sx =
 * floor(fx), fx -= sx, clamped as the float path clamps; a0 = rint((1.f - fx) * 2048),
 * a1 = rint(fx * 2048), each rounded half to even on its own; D = S[sx] * a0 +
 * S[sx + 1] * a1 in int32; out = (uint8)(((D >> 9) + 2) >> 2), the vertical pass with
 * coefficients (2048, 0)).  The flip is applied to im_ar, after the 8-bit resize, as
 * the reference does: pass the unflipped frames.  Every blob element is written; all
 * source indices are clamped to the frame.  cv2 is not importable in the build
 * container, so parity of the 8-bit step against an executed cv2 is unpinned, as the
 * float step's is (both are pinned against the numpy restatement and known answers). */
int vd_image_aspect_resize_to_blob(const uint8_t *frames, int F, int H, int W, int War, int hflip,
                                   const float *lut, double im_scale, int Hr, int Wr, int Hp,
                                   int Wp, int nhwc, float *blob, void *stream);

/* Frames of different sizes in one launch: im_list_to_blob (lib/utils/blob.py:
 * 86-114) over per-frame prep_im_for_blob results, as tools/infer_simple.py and
 * test_net.py meet them.  Frame f is geom[f].H x geom[f].W x 3 u8 BGR starting
 * at byte geom[f].offset of `packed` (any offset, no alignment assumed).  It is
 * prepared exactly as the two entries above prepare it -- LUT copy when
 * inv_scale == 1, the 2 x 2 area path when inv_scale == 2, INTER_LINEAR
 * otherwise -- into the top-left Hr x Wr of slice f of the F x 3 x Hp x Wp
 * (nhwc: F x Hp x Wp x 3) blob; everything else in the slice is written as
 * zero, so every blob element is written.
 *
 * geom is a DEVICE array of F rows and no frame size is a launch argument: a
 * captured launch (hipGraph) replays with whatever the buffers hold at replay.
 * inv_scale = 1.0 / im_scale computed on the host in double (cv::resize's
 * scale); Hr, Wr = rint(H * im_scale), rint(W * im_scale).  The caller keeps
 * Hr <= Hp, Wr <= Wp and offset + H*W*3 inside `packed`; on the device a row's
 * extent is clamped to the blob, so a bad row cannot write outside it. */
typedef struct VdFrameGeom {
    int64_t offset;   /* bytes into packed */
    int32_t H, W;     /* the frame */
    int32_t Hr, Wr;   /* the resized frame */
    double inv_scale; /* 1 / im_scale */
} VdFrameGeom;
int vd_image_resize_to_blob_ragged(const uint8_t *packed, const VdFrameGeom *geom, int F,
                                   const float *lut, int Hp, int Wp, int nhwc, float *blob,
                                   void *stream);

/* Convolution epilogue, in place on x (N x C x H x W logical, physical NHWC when
 * nhwc = 1):  x = act((x + bias[c]) + r),  r = 0 (residual_mode 0), residual
 * (+ residual_bias[c]) of the same shape (mode 1), or residual nearest-2x
 * upsampled from (H/2, W/2) (+ residual_bias[c]) (mode 2: the FPN top-down add,
 * lib/modeling/FPN.py:293-299).  act = ReLU if relu.  One pass instead of the
 * bias / residual / ReLU passes after a bias-free convolution (the frozen
 * AffineChannel2d of ResNet.py:276-294 folded into conv weight + bias).
 * bias / residual_bias may be NULL; N*C*H*W < 2^31. */
int vd_bias_act(float *x, const float *bias, const float *residual, const float *residual_bias,
                int N, int C, int H, int W, int nhwc, int residual_mode, int relu, void *stream);

/* B x C x H x W -> B x H x W x C (pyramid relayout for the NHWC RoIAlign). */
int vd_nchw_to_nhwc(const float *in, int B, int C, int H, int W, float *out, void *stream);


/* ===========================================================================
 * VOS temporal path (lib_vos): FlowAlign, GroupNorm epilogues, ConvGRU gates.
 * ======================================================================== */

/* FlowAlign.  Replaces
 *   int flow_align_forward_cuda(THCudaTensor *bottom, THCudaTensor *flow,
 *                               THCudaTensor *top)
 *   lib_vos/vos_model/flow_align/src/flow_align_cuda.c:7-23 (kernel
 *   flow_align_cuda_kernel.cu:15-55).
 * features: B x C x H x W (layout VD_LAYOUT_NCHW, the reference's) or
 * B x H x W x C (VD_LAYOUT_NHWC, C % 4 == 0); flow: B x 2 x H x W fp32 (x, y
 * displacement in level pixels, already downsampled by the module's
 * conv_flow_downsample, or produced from the raw flow by vd_flow_to_levels);
 * output: same layout/shape as features, written
 * entirely (0 where the displaced position leaves [0, H-1) x [0, W-1)). */
int vd_flow_align_forward(const float *features, const float *flow, int B, int C, int H, int W,
                          int layout, float *output, void *stream);

/* Optical flow as read from the .flo file -> the level flows FlowAlign reads.
 * Replaces
 *   flo_to_blob (lib/utils/blob.py:63-75): prep_im_for_blob's cv2.resize(fx =
 *     fy = im_scale, INTER_LINEAR) of the flow, `flo[0] * flo_scale` (a float32
 *     array times a Python list: numpy multiplies in float64, the blob
 *     assignment rounds once to float32), zero padding to FPN.COARSEST_STRIDE,
 *     NCHW transpose;
 *   FlowAlign.conv_flow_downsample (lib_vos/vos_model/flow_align/modules/
 *     flow_align.py:12-25) of all five modules: a 2 -> 2 conv, kernel = stride
 *     = k, diagonal weight (1/k)^3.
 * raw_flow: F x H x W x 2 fp32 (u then v per pixel).  Hr, Wr = rint(H *
 * im_scale), rint(W * im_scale); Hp, Wp the padded blob, both multiples of 64
 * (VD_ERR_SHAPE otherwise).
 *   blob(f,c,y,x)  = float(double(R(f,y,x,c)) * im_scale) for y < Hr, x < Wr, else 0
 *   out_k(f,c,Y,X) = (1/k)^3 * sum of blob over the k x k block
 * R is vd_image_resize_to_blob's resize on float input: identity at im_scale
 * 1, the 2 x 2 area path at exactly 0.5, else the scalar float INTER_LINEAR
 * (bit-exact against the numpy restatement; vs an executed cv2: unpinned).
 * The block sums are added in a fixed tree (4 x 4 per thread, then 2 x 2 of
 * the finer level; flow_prep.hip), so a value depends on its block alone.
 * out_k: F x 2 x Hp/k x Wp/k, any may be NULL; blob: F x 2 x Hp x Wp (16-byte
 * aligned) or NULL = never written.  One launch, no workspace, no atomics. */
int vd_flow_to_levels(const float *raw_flow, int F, int H, int W, double im_scale, int Hr, int Wr,
                      int Hp, int Wp, float *out4, float *out8, float *out16, float *out32,
                      float *out64, float *blob, void *stream);

/* The delta-flow head of Generalized_VOS_RCNN (MODEL.USE_DELTA_FLOW,
 * lib_vos/vos_modeling/vos_model_builder.py:95-104, 314-326), step 1: for every
 * level l, frame b and pixel
 *   new   = tanh(sum over the 3 x 3 taps and C channels of w * x)   (zero padding)
 *   delta = valid[b] ? new - feat : 0     (one IEEE subtraction of the stored value)
 *   feat  = new
 * in one launch for all levels.  features: B x C x H x W (VD_LAYOUT_NCHW) or
 * B x H x W x C (VD_LAYOUT_NHWC), 16-byte aligned; weight: the Conv2d weight
 * [2][C][3][3] repacked to [18][C], row (ky * 3 + kx) * 2 + o, 16-byte aligned;
 * feat (the state, updated in place: the thread that writes an element is the
 * one that read it) and delta: B x 2 x H x W.  valid: B int32 on the device.
 * `levels` is a host array read at the call (its contents travel as kernel
 * arguments); the launch reads no host value that changes between steps, so a
 * captured step replays.  C % 64 == 0 and C <= 512 (VD_ERR_SHAPE otherwise);
 * any H, W >= 1.  The sum is float32 fused multiply-adds in a fixed order
 * (delta_flow.hip); tanh is the device tanhf. */
typedef struct {
    const float *features;
    int H;
    int W;
    const float *weight;
    float *feat;
    float *delta;
} VdDeltaFlowLevel;

int vd_delta_flow_features(const VdDeltaFlowLevel *levels, int num_levels, int B, int C,
                           int layout, const int32_t *valid, void *stream);

/* Step 2: the five deltas (strides 64, 32, 16, 8, 4; d_k is B x 2 x Hp/k x Wp/k)
 * -> the five FlowAlign level flows and, optionally, the blob-resolution flow:
 *   data_flow(y, x) = sum over k = 64, 32, 16, 8, 4 in that order of
 *                     bilinear_up(d_k)(y, x) * k      (align_corners False: source
 *                     max((dst + 0.5) / k - 0.5, 0), upper tap clamped)
 *   out_k(Y, X)     = (1/k)^3 * sum of data_flow over the k x k block
 * i.e. F.interpolate + division by the scale + the modules' conv_flow_downsample.
 * The block sums are added in a fixed tree, so a value depends on its block
 * alone.  Hp, Wp multiples of 64 (VD_ERR_SHAPE otherwise).  out_k may be NULL;
 * blob: B x 2 x Hp x Wp (16-byte aligned) or NULL = never written.  One launch,
 * no workspace, no atomics. */
int vd_delta_flow_to_levels(const float *d64, const float *d32, const float *d16, const float *d8,
                            const float *d4, int B, int Hp, int Wp, float *out64, float *out32,
                            float *out16, float *out8, float *out4, float *blob, void *stream);

/* Replaces flow_align_backward_cuda (flow_align_cuda.c:25-44, kernel :57-117).
 * NCHW only.  features_grad (B x C x H x W) and flow_grad (B x 2 x H x W) must
 * be zero-filled by the caller (functions/flow_align.py:36-39); contributions
 * are accumulated with fp32 atomics. */
int vd_flow_align_backward(const float *top_grad, const float *features, const float *flow,
                           int B, int C, int H, int W, float *features_grad, float *flow_grad,
                           void *stream);

/* GroupNorm + fused epilogue.  Replaces the nn.GroupNorm (+ residual add,
 * + ReLU) module sequences of the GN ResNet / FPN / heads (ResNet.py:208-345,
 * FPN.py:96-120,268-274, fast_rcnn_heads.py:228-290,
 * mask_rcnn_heads.py:191-255) with one statistics pass and one apply pass:
 *   out = act(GN(x [+ x2]; gamma, beta) + r),  r per residual_mode:
 *     0: none; 1: residual (same shape); 2: residual nearest-2x upsampled
 *     (B x H/2 x W/2); 3: GN(residual; res_gamma, res_beta) (its own
 *     statistics, the basic_gn_shortcut branch).
 * act: VD_ACT_*.  G groups over C channels (C % G == 0; NHWC needs
 * (C / G) % 4 == 0).  Statistics in double, normalisation in fp32.
 * workspace: vd_group_norm_workspace_size(B, G) bytes (x2 for residual_mode 3).
 * out may alias x (in place) but not residual. */
enum { VD_ACT_NONE = 0, VD_ACT_RELU = 1, VD_ACT_SIGMOID = 2, VD_ACT_TANH = 3 };
enum { VD_GN_ACT = 0, VD_GN_GRU_Z = 1, VD_GN_GRU_R = 2, VD_GN_GRU_H = 3 };

size_t vd_group_norm_workspace_size(int B, int G);

int vd_group_norm_act(const float *x, const float *x2, int B, int C, int H, int W, int G,
                      float eps, const float *gamma, const float *beta, const float *residual,
                      int residual_mode, const float *res_gamma, const float *res_beta, int act,
                      int layout, float *out, void *workspace, size_t ws_bytes, void *stream);

/* ConvGRU gates (lib_vos/vos_nn/convgrucell.py:73-92, use_GN branch):
 *   z  = sigmoid(GN_z(Wz_h(h) + Wz_x(x)))
 *   hr = h * sigmoid(GN_r(Wr_h(h) + Wr_x(x)))
 * zh/zx/rh/rx are the convolution outputs (B x C x H x W in `layout`); h the
 * hidden state.  h == NULL means the zero state (first frame of a sequence, or
 * the static model's fresh state): zh/rh/hr are then unused (the h-side
 * convolutions of a zero state are exactly zero) and only z is produced.
 * workspace: 2 * vd_group_norm_workspace_size(B, G). */
int vd_convgru_gates(const float *zh, const float *zx, const float *rh, const float *rx,
                     const float *h, int B, int C, int H, int W, int G, float eps,
                     const float *gamma_z, const float *beta_z, const float *gamma_r,
                     const float *beta_r, int layout, float *z, float *hr, void *workspace,
                     size_t ws_bytes, void *stream);

/* ConvGRU update + VOS top-down fusion (convgrucell.py:88-91;
 * vos_model_builder.py:335-345):
 *   hn  = (1 - z) * h + z * tanh(GN_h(Wh_h(h * r) + Wh_x(x)))   (h == NULL: z * tanh(..))
 *   out = finer ? hn / 2 + bilinear_0.5x(finer) / 2 : hn
 * hh may be NULL with h (zero state).  finer: the already-fused next-finer level
 * (B x C x 2H x 2W in `layout`), or NULL for the finest level. */
int vd_convgru_update(const float *hh, const float *hx, const float *z, const float *h,
                      const float *finer, int B, int C, int H, int W, int G, float eps,
                      const float *gamma_h, const float *beta_h, int layout, float *out,
                      void *workspace, size_t ws_bytes, void *stream);

/* The fork's steps after the detections limit in box_results_with_nms_and_limit
 * (lib_vos/tools/vos_test.py:805-833), in place on vd_box_detections' outputs:
 * nms_cross_class > 0 -> one NMS (cython semantics) over all classes'
 * detections, survivors regrouped by class in row order (TEST.NMS_CROSS_CLASS);
 * num_det_per_class_pre > 0 -> per class the top-k by score, rows reordered by
 * score (TEST.NUM_DET_PER_CLASS_PRE; ties by row order).  Both off -> no-op.
 * det_cap <= 512. */
int vd_detections_postfilter(float *dets, int32_t *classes, int32_t *counts, int num_images,
                             int det_cap, float nms_cross_class, int num_det_per_class_pre,
                             void *stream);

/* vd_bias_relu_maxpool: the stem tail of basic_bn_stem (lib/modeling/ResNet.py:
 * 224-230) after a bias-free conv1: out = MaxPool2d(3, 2, 1)(relu(x + bias[c])),
 * x N x H x W x C (NHWC), out N x Ho x Wo x C with Ho = (H - 1) / 2 + 1,
 * Wo = (W - 1) / 2 + 1.  Bit-identical to vd_bias_act followed by the max-pool.
 * C % 4 == 0. */
int vd_bias_relu_maxpool(const float *x, const float *bias, int N, int C, int H, int W,
                         float *out, void *stream);

/* vd_rpn_head: the FPN RPN head of one level after its shared 3x3 conv
 * (lib/modeling/FPN.py:376-422, test branch): x = the conv's raw output WITHOUT
 * its bias, N x H x W x C (NHWC, contiguous); conv_bias [C]; w [5A][C] = the
 * cls_score (A rows) then bbox_pred (4A rows) 1x1 weights, b [5A] their biases.
 * Writes cls_prob N x A x H x W = sigmoid(w_cls . relu(x + conv_bias) + b_cls)
 * and bbox_pred N x 4A x H x W (NCHW), the layouts vd_generate_proposals reads.
 * C % 64 == 0, 5A <= 16 (else VD_ERR_SHAPE). */
int vd_rpn_head(const float *x, const float *conv_bias, const float *w, const float *b, int N,
                int H, int W, int C, int A, float *cls_prob, float *bbox_pred, void *stream);

/* ---------------------------------------------------------------------------
 * segm_results (lib/core/test.py:801-855; fork lib_vos/tools/vos_test.py:867-921)
 * on the device, SURVEY.md section 8f row 3.
 *
 * vd_paste_masks: masks M x R x R fp32 (each detection's class-selected mask
 * probabilities, i.e. masks[mask_ind, j]), boxes M x box_stride fp32
 * (x1, y1, x2, y2 in image coordinates, the cls_boxes rows) -> out M x im_h x
 * im_w u8 (row-major, every byte written): box_utils.expand_boxes by
 * (R+2)/R (boxes.py:242-258) + astype(int32), cv2.resize(padded_mask, (w, h))
 * INTER_LINEAR (OpenCV's scalar float path, restated), `> thresh`
 * (MRCNN.THRESH_BINARIZE), pasted into the clipped box.  R <= 62.
 *
 * vd_mask_rle: pycocotools mask.encode counts of each M x H x W u8 plane in
 * column-major (Fortran) order: counts[m][0..n) with n = ncounts[m], the
 * first run counting zeros.  If a plane needs more than `cap` runs,
 * ncounts[m] = -n and its counts are not written (call again with cap >= n).
 * The run lengths -> ASCII string step (rleToString) is vd_rle_strings.
 * ------------------------------------------------------------------------- */
int vd_paste_masks(const float *masks, int M, int R, const float *boxes, int box_stride,
                   int im_h, int im_w, float thresh, uint8_t *out, void *stream);
int vd_mask_rle(const uint8_t *masks, int M, int H, int W, uint32_t *counts, int cap,
                int32_t *ncounts, void *stream);

/* vd_segm_rle: vd_paste_masks followed by vd_mask_rle in one launch, without
 * the M x im_h x im_w planes: each detection's pasted values are evaluated in
 * its clipped box only (everything outside is 0) and turned into the same
 * counts / ncounts (retry contract as vd_mask_rle).  im_w <= 8192.
 *
 * vd_rle_strings: pycocotools rleToString (maskApi.c) of each detection's
 * counts[m][0..ncounts[m]).  chars == NULL: lens[m] = the string's length
 * (0 for ncounts[m] <= 0).  chars != NULL: lens must hold those lengths
 * (sum < 2^31); detection m's ASCII string is written at
 * chars[lens[0] + ... + lens[m-1]], unterminated.  Replaces the host-side
 * mask_util.encode(...)['counts'].decode('ascii') of segm_results
 * (lib/core/test.py:844-847). */
int vd_segm_rle(const float *masks, int M, int R, const float *boxes, int box_stride,
                int im_h, int im_w, float thresh, uint32_t *counts, int cap, int32_t *ncounts,
                void *stream);
int vd_rle_strings(const uint32_t *counts, const int32_t *ncounts, int M, int cap,
                   int32_t *lens, uint8_t *chars, void *stream);

/* vd_segm_rle for detections of frames of different sizes: det_hw is a DEVICE
 * array [M][2] = (im_h, im_w) of each detection's own frame, replacing the two
 * scalar arguments; the kernel body, counts, ncounts and the retry contract
 * are vd_segm_rle's.  A row with im_h < 1, im_w < 1 or im_w > 8192 gets
 * ncounts[m] = 0 and no counts (a valid plane has at least one run). */
int vd_segm_rle_ragged(const float *masks, int M, int R, const float *boxes, int box_stride,
                       const int32_t *det_hw, float thresh, uint32_t *counts, int cap,
                       int32_t *ncounts, void *stream);

/* ---------------------------------------------------------------------------
 * viz_mask_result (lib/utils/vis.py:119-157, called per frame from
 * lib_vos/tools/train_davis_online.py:596-600) on the device: the object-ID
 * image of every frame of a step, without the per-detection planes.
 *
 * vd_label_maps: masks rows of R x R fp32 (class-selected probabilities) in
 * (frame, detection) order -- the row of detection (f, i) is
 * sum(clamp(counts[0..f), 0, cap)) + i, formed on the device (no host read, so
 * the call is valid on counts that are still being computed on the stream and
 * can be graph-captured); masks must hold sum(clamp(counts, 0, cap)) rows.
 * dets F x cap x 5 fp32 (x1, y1, x2, y2, score), classes F x cap int32, counts
 * F int32 (device), valid F x cap u8 or NULL (rows a post-filter kept).  A count
 * outside [0, cap] is clamped; nothing outside the buffers is read or written
 * whatever counts holds.
 *
 * Detection i of frame f is painted iff i < counts[f], (valid == NULL or
 * valid[f][i] != 0) and !(score < score_thresh), compared in float32: that is
 * how NumPy >= 2 evaluates `np.float32 < python float` (NEP 50), i.e. the
 * reference's `score < thresh` with the threshold rounded to float32 first.
 * label[f][y][x] = the written id of the painted detection with the highest
 * score whose pasted, binarised mask (vd_paste_masks' value at bin_thresh, bit
 * for bit) covers (x, y), 0 where none does: the reference's painting in
 * ascending score order.  Among equal scores the higher row index is painted
 * later and wins (the reference's np.argsort is not stable; this is the
 * project's rule).  gt[f][y][x] = label[f][y][x] where the winner's
 * score > gt_thresh (float32), else 0: rtv_gt at rvt_cls_threshold = gt_thresh.
 * The written id of class c is lut[c] (c in [0, lut_n)), or c itself (c in
 * [0, 255]) when lut is NULL; any other class writes 0.  label and gt are
 * F x im_h x im_w u8, every byte written; gt may be NULL.
 *
 * R in 1..62, im_h, im_w >= 1, 1 <= cap <= 1024, F <= 65535, im_h <= 2097120
 * (VD_ERR_SHAPE otherwise); workspace_bytes >= vd_label_maps_workspace_size(F,
 * cap) (VD_ERR_WORKSPACE; the size is 0 for an F or cap the kernel refuses),
 * 16-byte aligned; NULL masks / dets / classes / counts / label / workspace or a
 * lut with lut_n < 1 give VD_ERR_ARG.  Nothing is launched on an error.
 * ------------------------------------------------------------------------- */
size_t vd_label_maps_workspace_size(int F, int cap);
int vd_label_maps(const float *masks, int R, const float *dets, const int32_t *classes,
                  const int32_t *counts, const uint8_t *valid, int F, int cap, int im_h, int im_w,
                  float bin_thresh, float score_thresh, float gt_thresh, const uint8_t *lut,
                  int lut_n, uint8_t *label, uint8_t *gt, void *workspace,
                  size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * The DAVIS annotation file of every frame of a step: the last step of
 * viz_mask_result (lib/utils/vis.py:152-155; img_saver is davis_saver ->
 * io.imwrite_indexed, imdb/vos/davis_db.py:45-47), an 8-bit indexed PNG of the
 * label map, formed on the device.
 *
 * vd_label_pngs: labels F x H x W u8 (vd_label_maps' label or gt), palette 256 x 3
 * u8 RGB (device), out F x cap u8, lengths F int32.  out[f][0 .. lengths[f]) is a
 * complete PNG file: signature; IHDR (W, H, bit depth 8, colour type 3, no
 * interlace); PLTE with 256 entries; one IDAT holding a zlib stream (header 78 01);
 * IEND.  Every chunk CRC-32 and the Adler-32 are computed on the device.  The
 * decoded pixels equal labels[f], the decoded palette equals palette.  Bytes of
 * out[f] past lengths[f] hold no defined value.  No host read, no device
 * allocation: the call can be graph-captured.  The bytes depend on the inputs
 * alone, not on what out or workspace held, and are the same in every run.
 *
 * Deflate form: filter type 0 on every row; rows in strips of 8; a strip is one
 * fixed-Huffman block of literals and distance-1 matches of 3..258 bytes (runs
 * within a row), and every strip but the last (BFINAL) is followed by an empty
 * stored block, so that it ends on a byte boundary.
 *
 * vd_label_png_bound(H, W): the per-frame capacity no input can exceed, host only:
 *     843                           signature 8, IHDR 25, PLTE 780, IDAT length and
 *                                   type 8, zlib header 2, Adler-32 4, IDAT CRC 4,
 *                                   IEND 12
 *   + sum over strips of r rows of  floor((9 r (W + 1) + 20) / 8) + 4
 * A strip is at most: 3 bits of block header, 9 bits (the longest literal) for each
 * of its r (W + 1) filtered bytes -- a match costs at most 8 + 5 + 5 bits for at
 * least 3 bytes, never more than the literals it replaces --, 7 bits of end of
 * block, 3 bits of stored-block header, up to 7 bits of padding, 4 bytes LEN / NLEN.
 * 0 for a size the kernel does not serve.  cap below the bound is refused
 * (VD_ERR_ARG) before any launch, so there is no overflow at run time; the strips
 * are first written at their worst-case offsets inside out[f] and then joined.
 *
 * 1 <= W <= 4095, 1 <= H <= 16384, F <= 65535 (VD_ERR_SHAPE otherwise);
 * workspace_bytes >= vd_label_pngs_workspace(F, H, W) (VD_ERR_WORKSPACE; 16 bytes
 * per strip; 0 for a shape the kernel refuses), 16-byte aligned, any contents; NULL
 * labels / palette / out / lengths / workspace or cap < bound give VD_ERR_ARG.
 * Nothing is launched on an error.  F == 0 returns VD_OK.
 * ------------------------------------------------------------------------- */
size_t vd_label_png_bound(int H, int W);
size_t vd_label_pngs_workspace(int F, int H, int W);
int vd_label_pngs(const uint8_t *labels, int F, int H, int W, const uint8_t *palette,
                  uint8_t *out, size_t cap, int32_t *lengths, void *workspace,
                  size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * The objects of a label map: what the reference's host loops over np.unique(gt) make
 * of an H x W object-ID map, for every frame of a step in one call.
 * DAVIS_imdb.get_gt / get_bboxes (imdb/vos/davis_db.py:180-204) with the box form of
 * lib_vos/tools/get_cls_mapper.py:129-136 (the boxes the heads then run on through
 * box_proposals), and DAVIS_imdb.add_gt_annotations_to_entry (davis_db.py:407-517,
 * called from lib_vos/tools/train_davis_online.py:429 on the last_gt that
 * viz_mask_result returned).
 *
 * vd_label_objects: labels F x H x W u8 (device; vd_label_maps' gt or label, or a
 * DAVIS annotation).  Per frame, in this order:
 *   values    the distinct values of the map.  remap255 == 1 applies get_gt's rule
 *             first: if 255 occurs, its pixels take the value len(vals) - 1, vals
 *             counting every distinct value of the raw map (0 and 255 included); if
 *             that value occurs already the two objects merge, as in the reference.
 *             The objects are the non-zero values in ascending order (np.unique).
 *   ids       F x obj_cap u8        the object's value
 *   rects     F x obj_cap x 4 i32   cv2.boundingRect (x, y, w, h) = (xmin, ymin,
 *                                   xmax - xmin + 1, ymax - ymin + 1)
 *   areas     F x obj_cap i32       the pixel count
 *   boxes     F x obj_cap x 4 fp32, counts F i32: the box_proposals layout
 *             vd_rois_from_boxes takes.
 *             expand < 0, the "rect" form: (x, y, x + w, y + h); every object kept.
 *             expand >= 0, the "entry" form (the reference uses 0.05), in float64:
 *             e = sqrt(w * h) * expand (the correctly rounded square root); x -= e / 2,
 *             y -= e / 2, w += e, h += e (_expand_box); x2 = x + max(0, w - 1), y2
 *             likewise (xywh_to_xyxy); every coordinate clipped to [0, W - 1] /
 *             [0, H - 1] (clip_xyxy_to_image); an object is kept iff area > 0 and
 *             x2 > x1 and y2 > y1.  The kept rows are compacted in order, ids / rects /
 *             areas / RLE rows with them; the store rounds to float32 once
 *             (entry['boxes'] is float32).  Nothing is fused (-ffp-contract=off).
 *   counts[f] the number of kept objects; 0 for a frame without one.  More than
 *             obj_cap: counts[f] = VD_COUNT_SELECT_FAILED and nothing else is written
 *             for that frame (vd_rois_from_boxes' convention).
 *   rle_cap > 0: rle_counts F x obj_cap x rle_cap u32, rle_n F x obj_cap i32: the
 *             pycocotools mask.encode counts of (map == value) after the remap,
 *             column-major, the first run counting zeros; rle_n the number of runs.
 *             An object with more than rle_cap runs gets rle_n = -n and no counts
 *             (vd_mask_rle's retry contract).  rle_cap == 0: no RLE, both may be NULL.
 * Rows past counts[f] are not written in any output.
 *
 * No host read, no device allocation, nothing sized by a device value: the call can
 * be graph-captured.  The outputs depend on the inputs alone (the statistics are
 * merged with integer min / max / add atomics, which commute), whatever the workspace
 * held.  Workspace: vd_label_objects_workspace_size(F, H, W, obj_cap) =
 * F * (5136 + 32 * obj_cap) bytes (a 256 x 5 int32 table, the slot count, one 32-byte
 * slot per object), 16-byte aligned; 0 for a shape the kernels refuse (F == 0 included:
 * there is nothing to carve).  The caller's rle_counts is F * obj_cap * rle_cap * 4 bytes
 * -- at obj_cap 255 and rle_cap 4 W + 2 that is 348 MB for 64 maps of 800 x 1333, five
 * times the maps: size obj_cap to the objects expected.  The RLE pass launches obj_cap x F
 * workgroups, of which those past a frame's count return at once.
 *
 * 1 <= obj_cap <= 255, F <= 65535, H >= 1, 1 <= W <= 8192 (the RLE pass keeps one
 * int per column in LDS), H * W < 2^31 (VD_ERR_SHAPE otherwise); a workspace below the
 * size gives VD_ERR_WORKSPACE; NULL labels / ids / rects / areas / boxes / counts /
 * workspace, NULL rle_counts / rle_n with rle_cap > 0, rle_cap < 0, remap255 outside
 * {0, 1}, a NaN expand or F < 0 give VD_ERR_ARG.  Nothing is launched on an error.
 * F == 0 returns VD_OK.
 * ------------------------------------------------------------------------- */
size_t vd_label_objects_workspace_size(int F, int H, int W, int obj_cap);
int vd_label_objects(const uint8_t *labels, int F, int H, int W, int remap255, double expand,
                     int obj_cap, int rle_cap, uint8_t *ids, int32_t *rects, int32_t *areas,
                     float *boxes, int32_t *counts, uint32_t *rle_counts, int32_t *rle_n,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * nms_with_mask_iou (lib_vos/tools/vos_test.py:985-1029) for every frame of a
 * step in one call, without the H x W planes and without a host read.
 *
 * vd_mask_iou_nms_frames: masks / dets / classes / counts as vd_label_maps takes
 * them -- masks `rows` rows of R x R fp32 in (frame, detection) order, the row of
 * detection (f, i) being sum(clamp(counts[0..f), 0, cap)) + i, formed on the
 * device; dets F x cap x 5 fp32, classes F x cap int32, counts F int32 (device).
 * A count above cap is clamped, and the counts are cut to the rows masks holds:
 * frame f takes the detections whose row is below `rows`.  Nothing outside the
 * buffers is read or written whatever counts holds.
 *
 * Per frame the result is, bit for bit, vd_paste_masks (at bin_thresh) followed
 * by vd_mask_iou_nms (iou_th, max_per_class) on the frame's detections: score
 * order is np.argsort(-score) read stably (equal scores: the lower row first); a
 * later position j is discarded by an earlier kept i when inter / (|m_i| + 1e-6)
 * or inter / (|m_j| + 1e-6), in float64, is > iou_th; the kept rows are counted
 * per class in score order and a class keeps its first max_per_class (0 keeps
 * nothing); the output order is class ascending, then score order.
 *   keep         F x cap int32: keep[f][0 .. keep_counts[f]) the kept rows i of
 *                frame f in output order; entries past the count are untouched
 *   keep_counts  F int32
 *   valid        F x cap u8 or NULL: 1 on kept rows, 0 on the other rows below the
 *                (cut) count, untouched past it
 *   prev_dets (F x prev_cap x 5), prev_classes (F x prev_cap), prev_counts (F):
 *                all three or none (VD_ERR_ARG otherwise); prev_cap >= cap.  The
 *                kept dets / classes rows in keep order and their number: the
 *                frame's final result as the next frame's previous result
 *                (vd_detections_prev_box_filter).  Rows past the count untouched.
 * A frame whose count is negative (a failure code of an upstream kernel) keeps
 * that code in keep_counts[f], gets prev_counts[f] = 0 and no other write:
 * propagate, never hide.
 *
 * Workspace: vd_mask_iou_nms_frames_workspace_size(F, cap, rows, im_h, im_w) bytes
 * (0 for a shape the kernels refuse), 16-byte aligned, any contents:
 *   rows * im_h * ceil(im_w / 64) * 8   the packed masks, 64 pixels per word on
 *                                       the frame's 64-column grid
 * + F * cap * cap * 4                   the pair intersections
 * + rows * 20 + F * 8                   boxes, areas, first rows and cut counts
 * each term rounded up to 256 bytes.  No term grows with rows * im_h * im_w bytes.
 *
 * R in 1..62, 1 <= cap <= 1024, 1 <= F <= 65535, im_h, im_w >= 1 with
 * im_h * im_w < 2^31, prev_cap >= cap (VD_ERR_SHAPE otherwise); a workspace below
 * the size gives VD_ERR_WORKSPACE; NULL masks / dets / classes / counts / keep /
 * keep_counts / workspace, rows < 0 or one or two of the prev_* pointers give
 * VD_ERR_ARG.  Nothing is launched on an error.  F == 0 returns VD_OK.
 * ------------------------------------------------------------------------- */
size_t vd_mask_iou_nms_frames_workspace_size(int F, int cap, int rows, int im_h, int im_w);
int vd_mask_iou_nms_frames(const float *masks, int rows, int R, const float *dets,
                           const int32_t *classes, const int32_t *counts, int F, int cap,
                           int im_h, int im_w, float bin_thresh, double iou_th, int max_per_class,
                           int32_t *keep, int32_t *keep_counts, uint8_t *valid, float *prev_dets,
                           int32_t *prev_classes, int32_t *prev_counts, int prev_cap,
                           void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * im_detect_bbox on caller-given boxes (MODEL.FASTER_RCNN False; lib/core/test.py
 * :128-190, lib_vos/tools/vos_test.py:137-205), the part before the heads, for every
 * frame of a step in one call: _get_rois_blob (test.py:877-906) and the DEDUP_BOXES
 * hash with np.unique (test.py:132-139).
 *
 * vd_rois_from_boxes: boxes F x cap x 4 fp32 in image coordinates, counts F int32
 * (device), im_scale F float64 (get_target_scale's scalar per frame), dedup
 * cfg.DEDUP_BOXES as float32.  Per frame f with n = counts[f] rows:
 *   RoI of row r   (f, float32(float64(box) * im_scale[f])): column 0 is the frame
 *   hash           np.round(roi * dedup) in float32 (half to even), then the float64
 *                  dot with (1, 1e3, 1e6, 1e9, 1e12); exact for blobs < 16000 pixels
 *   np.unique      the distinct hashes ascending; index = the first row of each,
 *                  inv_index = the position of each row's hash.  Two boxes that round
 *                  to one hash are merged onto the first, as the reference merges them
 *   rois      F x cap x 5 fp32   rois[f][u] = the RoI of row index[f][u], u < ucounts[f]
 *   ucounts   F int32            the number of distinct hashes
 *   index     F x cap int32      u < ucounts[f]
 *   inv_index F x cap int32      r < counts[f]
 * Rows past ucounts[f] in rois / index and past counts[f] in inv_index are not
 * written.  dedup == 0 is the identity: index = inv_index = 0 .. n - 1, the RoIs in
 * input order, ucounts = counts.  counts[f] == 0 writes ucounts[f] = 0 and nothing
 * else; counts[f] > cap writes ucounts[f] = VD_COUNT_SELECT_FAILED and nothing else;
 * a negative count (an upstream failure code) is copied to ucounts[f].
 *
 * No allocation, host copy or synchronisation: the call can be captured.  The keys
 * are sorted in LDS, so vd_rois_from_boxes_workspace(F, cap) is 0 and workspace may
 * be NULL; the pair is kept so that a larger capacity need not change the interface.
 * 1 <= cap <= 4096 and F >= 1 (VD_ERR_SHAPE otherwise); a NULL pointer, F < 0 or a
 * dedup that is negative or NaN give VD_ERR_ARG.  F == 0 returns VD_OK.
 *
 * vd_gather_rows: test.py:186-189 (scores[inv_index], pred_boxes[inv_index]) moved in
 * front of the decode, which is a function of the row alone.  For r < counts[f], with
 * u = inv_index[f][r]: scores_out[f][r] = scores[f][u] (F x cap x K), deltas_out[f][r] =
 * deltas[f][u] (F x cap x D), and rows_out[f][r] = (f, boxes[f][index[f][u]]), the
 * caller's own box of the representative (boxes[index], test.py:139): the reference
 * decodes from it, not from RoI / im_scale, so vd_box_detections takes rows_out as its
 * rois with an im_scale of 1.  Rows past counts[f] are not written.  counts_out[f] =
 * counts[f], or ucounts[f] when that is negative (the frame failed; nothing else is
 * written for it): the roi_count vd_box_detections takes.  An inv_index entry outside
 * [0, ucounts[f]) or an index entry outside [0, counts[f]) leaves its row unwritten.
 * F <= 65535, cap <= 4096, K, D >= 1 (VD_ERR_SHAPE otherwise).
 * ------------------------------------------------------------------------- */
size_t vd_rois_from_boxes_workspace(int F, int cap);
int vd_rois_from_boxes(const float *boxes, const int32_t *counts, const double *im_scale,
                       float dedup, int F, int cap, float *rois, int32_t *ucounts, int32_t *index,
                       int32_t *inv_index, void *workspace, size_t workspace_bytes, void *stream);
int vd_gather_rows(const float *boxes, const float *scores, const float *deltas,
                   const int32_t *index, const int32_t *inv_index, const int32_t *counts,
                   const int32_t *ucounts, int F, int cap, int K, int D, float *rows_out,
                   float *scores_out, float *deltas_out, int32_t *counts_out, void *stream);

/* ---------------------------------------------------------------------------
 * keypoint_results' heatmap decode (lib/utils/keypoints.py:103-157
 * heatmaps_to_keypoints with scores_to_probs :214-222; called from
 * lib/core/test.py:858-874) on the device.
 *
 * vd_heatmaps_to_keypoints: maps R x K x M x M fp32 logits (M <= 64, K <= 32),
 * boxes R rows of box_stride fp32 (x1, y1, x2, y2 in image coordinates first;
 * box_stride >= 4, so a detection array is read in place), min_size =
 * KRCNN.INFERENCE_MIN_SIZE -> out R x 4 x K fp32, rows (x, y, logit, prob): the
 * reference's xy_preds.  Per RoI: w = max(x2 - x1, 1), Wm = int(ceil(w)) raised
 * to min_size when min_size > 0 (h, Hm likewise; Wm, Hm <= 8192); each map is
 * resized to Hm x Wm by cv2.resize INTER_CUBIC on float32 (restated, rows first:
 * csrc/keypoints.hip) without being written anywhere; per keypoint the first
 * row-major argmax (xi, yi) gives x = (xi + 0.5) * (w / Wm) + x1 in float64 with
 * the float32 quotient, y likewise, logit = the value there and
 * prob = 1 / sum(exp(v - max)) over the resized map.  x, y and logit are
 * bit-identical for equal inputs; prob carries expf's last-place error.
 * R == 0 launches nothing. */
int vd_heatmaps_to_keypoints(const float *maps, int R, int K, int M, const float *boxes,
                             int box_stride, int min_size, float *out, void *stream);

/* ---------------------------------------------------------------------------
 * im_detect_keypoints_aug's combination of the views' heatmaps (lib/core/test.py:
 * 567-651, combine_heatmaps_size_dep :705-730, flip_heatmaps lib/utils/keypoints.py:
 * 90-100) fused into the decode above: one launch, the combined map is made while a
 * workgroup loads its (RoI, keypoint) map and everything after is
 * vd_heatmaps_to_keypoints' code.
 *
 * view_maps: HOST array of V device pointers (1 <= V <= 32), each R x K x M x M fp32
 * logits as the network returned them for that view, in heatmaps_ts order (the
 * identity view first).  Bit v of hflip_mask: view v saw the flipped image, so it is
 * read as flip_heatmaps inverts it -- channel flip_perm[k] (HOST, K entries in [0, K):
 * the left/right swap), column M - 1 - x.  Bits of ds_mask / us_mask: the view's scale
 * is below / above TEST.SCALE; they are disjoint and bit 0 is clear in both (the
 * identity view is never dropped).  heur: VD_KPS_AUG_HM_AVG (np.mean over the views:
 * the float32 sum in view order divided by float(T)) or VD_KPS_AUG_HM_MAX (the running
 * maximum; NaN logits are unsupported).  area_th < 0: every view counts for every row.
 * area_th >= 0 (KPS_AUG.SCALE_SIZE_DEP with KPS_AUG.AREA_TH): per row
 * area = (x2 - x1 + 1) * (y2 - y1 + 1) in float32, each operation rounded; area <
 * area_th drops the ds views, area >= area_th the us views, and T is the number of
 * views left for that row.  boxes, box_stride, min_size, out: as above (the unflipped
 * detection boxes).  combined_out: NULL, or R x K x M x M receiving the combined maps
 * (each written by exactly one workgroup).  The pointers, masks and permutation are
 * copied into the kernel's arguments, so a captured graph replays the launch.
 * Returns VD_ERR_ARG (nothing launched, out untouched) for V outside 1..32, a mask
 * bit at or above V, ds / us bit 0 set, ds & us != 0, a permutation entry outside
 * [0, K), an unknown heur, a NaN area_th or a NULL view.  R == 0 launches nothing. */
#define VD_KPS_AUG_HM_AVG 0
#define VD_KPS_AUG_HM_MAX 1
#define VD_KPS_AUG_MAX_VIEWS 32
int vd_heatmaps_to_keypoints_aug(const float *const *view_maps, int V, uint32_t hflip_mask,
                                 uint32_t ds_mask, uint32_t us_mask, const int32_t *flip_perm,
                                 int heur, float area_th, int R, int K, int M,
                                 const float *boxes, int box_stride, int min_size,
                                 float *combined_out, float *out, void *stream);

/* ---------------------------------------------------------------------------
 * keypoint_results' OKS NMS (lib/utils/keypoints.py:225-266 nms_oks /
 * compute_oks, applied per frame at lib/core/test.py:864-870 as a Python loop over
 * numpy arrays on the host) on the device, for all F frames of a step in two
 * stream-ordered launches with no host read.
 *
 * vd_nms_oks_frames: keyps [keyps_rows, 4, K] fp32 rows (x, y, logit, prob),
 * frame-major as vd_heatmaps_to_keypoints writes them: frame f's rows start at the
 * exclusive prefix sum of the non-negative counts; dets [F, D, 5], classes [F, D],
 * counts [F] as vd_box_detections leaves them; K must be 17 (the reference's sigma
 * table; VD_ERR_ARG otherwise) and D <= 512 (VD_ERR_SHAPE otherwise).  Per frame:
 *   score[i] = mean of the 17 logits in float32 (numpy's pairwise order);
 *   processing order = descending score, the HIGHER index first among equal
 *     scores (numpy's order for n <= 16; for larger n the reference's tie order
 *     is unspecified and this is the library's).  NaN logits are unsupported;
 *   a kept row i drops every later row j with compute_oks(i, j) > thresh, where
 *     only i's box area enters (csrc/oks_nms.hip restates the arithmetic).
 * Outputs (the inputs are not modified): keep [F, D] int32 frame-local indices in
 * kept order (-1 past the count), counts_out [F], dets_out [F, D, 5] and
 * classes_out [F, D] the kept rows in kept order (zeros past the count), keyps_out
 * [keyps_rows, 4, K] the kept rows compacted frame-major -- a frame's first row is
 * the exclusive prefix sum of counts_out -- zeros past the total; scores_out
 * [F, D] fp32 (may be NULL) the scores by input index.  A negative count is a
 * per-frame failure code: it is copied to counts_out and the frame is empty.  Rows
 * past keyps_rows are never read: a frame whose rows extend past the buffer is cut
 * to the rows present (callers that can overflow run again on the full set).
 * F == 0 launches nothing.
 *
 * vd_compute_oks: compute_oks of one source row (src_keypoints [4, K], src_roi
 * [4] = x1, y1, x2, y2) against N destination rows dst_keypoints [N, 4, K] ->
 * out [N] float64.  As in the reference the destination boxes and the
 * visibility / prob row are not read. */
int vd_nms_oks_frames(const float *keyps, int64_t keyps_rows, int K, const float *dets,
                      const int32_t *classes, const int32_t *counts, int F, int D, double thresh,
                      int32_t *keep, int32_t *counts_out, float *dets_out, int32_t *classes_out,
                      float *keyps_out, float *scores_out, void *stream);
int vd_compute_oks(const float *src_keypoints, const float *src_roi, const float *dst_keypoints,
                   int N, int K, double *out, void *stream);

/* ---------------------------------------------------------------------------
 * Test-time augmentation (TEST.BBOX_AUG / TEST.MASK_AUG) with the UNION box
 * heuristics: im_detect_bbox_aug (lib/core/test.py:193-311; flip_boxes,
 * lib/utils/boxes.py:261-266) followed by box_results_with_nms_and_limit on the
 * np.vstack of the views' scores and boxes, and im_detect_mask_aug's combination
 * (test.py:405-476).  Stream-ordered, no allocation, no host read.
 *
 * The union's per-class candidate lists live in the workspace (cand_cap rows per
 * (image, class), cand_cap <= 16384, VD_ERR_SHAPE beyond):
 *   vd_box_union_workspace_size = 2 * al(20 S c) + al(4 S c) + al(S c) + 2 * al(4 S)
 *   + al(4 F) bytes with S = num_images * num_classes, c = cand_cap, F = num_images and
 *   al() rounding up to 256: about 45 bytes per (image, class, row), no quadratic term.
 *
 * vd_box_union_add_view: once per box view, in np.vstack order (test.py:218-261:
 * the flipped view, the scales, the identity view last); first != 0 on the first
 * view of a step empties the lists.  rois / cls_prob / bbox_pred / roi_count are the
 * view's, as for vd_box_detections; im_scale[i] the view's scale, im_hw[i] the
 * original frame.  Per (image, class j >= 1) the rows with cls_prob >= score_thresh
 * are decoded and clipped as vd_box_detections does, a flipped view's (hflip != 0)
 * then mapped back with flip_boxes in float32 (x1' = (W - x2) - 1, x2' = (W - x1) -
 * 1), and appended in row order behind the earlier views' rows.  A list that would
 * exceed cand_cap, or a negative roi_count, fails the image.
 *
 * vd_box_union_add_view_ar: the same for an aspect-ratio view (test.py:330-363).
 * im_hw[i] = (H, War), the view's im_ar: the clip and the flip-back use it.  After
 * them x1' = fl32(x1 * x_inv), x2' = fl32(x2 * x_inv): aspect_ratio(boxes, 1.0 / ar)
 * (lib/utils/boxes.py:269-274), x_inv = float32(1.0 / ar) with the division in double
 * (numpy multiplies a float32 array by a Python float in float32).  x_inv must be
 * positive and finite.
 *
 * vd_box_union_detections: per (image, class) the list sorted by (score
 * descending, higher vstack index first), greedy NMS at any length without an
 * n x n mask, TEST.SOFT_NMS / TEST.BBOX_VOTE as vd_box_detections_ex (voters: all
 * of the class's candidates; soft-NMS needs cand_cap <= 4096, VD_ERR_SHAPE beyond),
 * then the detections limit: dets_out / det_cls_out / det_count_out as
 * vd_box_detections writes them, rows ordered by class then vstack index.  A failed
 * image gets count -1.  cand_count_out (may be NULL): [num_images][num_classes]
 * int32, the lengths of the lists. */
size_t vd_box_union_workspace_size(int cand_cap, int num_images, int num_classes);
int vd_box_union_add_view(const float *rois, const float *cls_prob, const float *bbox_pred,
                          const int32_t *roi_count, int R_cap, int num_images, int num_classes,
                          const float *im_scale, const int32_t *im_hw, int hflip, int first,
                          float score_thresh, const float *bbox_reg_weights, int cand_cap,
                          void *workspace, size_t workspace_bytes, void *stream);
int vd_box_union_add_view_ar(const float *rois, const float *cls_prob, const float *bbox_pred,
                             const int32_t *roi_count, int R_cap, int num_images, int num_classes,
                             const float *im_scale, const int32_t *im_hw, int hflip, float x_inv,
                             int first, float score_thresh, const float *bbox_reg_weights,
                             int cand_cap, void *workspace, size_t workspace_bytes, void *stream);
int vd_box_union_detections(int cand_cap, int num_images, int num_classes, float nms_thresh,
                            int dets_per_im, int soft_nms_method, float soft_nms_sigma,
                            float soft_nms_min_score, int bbox_vote_method,
                            float bbox_vote_thresh, float bbox_vote_beta, int det_cap,
                            float *dets_out, int32_t *det_cls_out, int32_t *det_count_out,
                            int32_t *cand_count_out, void *workspace, size_t workspace_bytes,
                            void *stream);

/* TEST.MASK_AUG.HEUR (test.py:459-474).  vd_mask_aug_accumulate folds one view's
 * class-selected masks [M, R, R] (sigmoid outputs) into acc [M, R, R], once per
 * mask view in masks_ts order (the identity view first; first != 0 there); a
 * flipped view (hflip != 0) is read with its last axis reversed (test.py:491).
 *   SOFT_AVG   acc += y (float32, view order)        finish: acc / float(T)
 *   SOFT_MAX   acc = max(acc, y)                     finish: nothing
 *   LOGIT_AVG  acc += -1 * log((1 - y) / max(y, 1e-20))
 *                                                    finish: 1 / (1 + exp(-acc / T))
 * SOFT_AVG and SOFT_MAX equal numpy's np.mean / np.amax bit for bit; LOGIT_AVG
 * differs by the device's logf / expf rounding. */
#define VD_MASK_AUG_SOFT_AVG 0
#define VD_MASK_AUG_SOFT_MAX 1
#define VD_MASK_AUG_LOGIT_AVG 2
int vd_mask_aug_accumulate(float *acc, const float *masks, int M, int R, int hflip, int heur,
                           int first, void *stream);
int vd_mask_aug_finish(float *acc, int M, int R, int T, int heur, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VOSDET_H_ */
