/*
 * rotmvgaze.h - C ABI of librotmvgaze_hip.so, the MI355X (gfx950) compute library behind the
 * Rot-MVGaze hot path (FeatRotationSymm forward / loss / backward).
 *
 * The reference has NO native layer and no FFI: every FLOP is a stock PyTorch ATen op
 * (SURVEY.md §2).  Each entry point below therefore replaces the ATen op(s) that the cited
 * reference lines dispatch; INTEGRATION.md shows the ctypes stub that binds them and how the
 * drop-in nn.Module calls them.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless named host_*;
 *   - activations are NHWC, images ordered [group][n][h][w][c]; a "group" is one view's batch:
 *     BatchNorm statistics are reduced per group because the reference runs the backbone once
 *     per view (rot_mv.py:196-197).  Storage is fp32 by default; the *_split entry points read
 *     their operands in "sp" (every fp32 value as two fp16 pieces and a per-tensor power-of-two
 *     scale: 8-channel chunks, the two pieces of a chunk adjacent, 4 bytes per element - section
 *     "split operands") and the
 *     *_bf16 entry points keep activations and activation gradients in bf16 (config C5);
 *   - conv weights are KRSC fp32 ([cout][r][s][cin]) = the physical layout of a PyTorch
 *     [O,I,H,W] tensor in torch.channels_last; linear weights are [out][in] (PyTorch native);
 *   - the caller owns every buffer, including workspaces; the library never allocates device
 *     memory and never synchronises (except mvg_prof_collect).  Kernel sequences that want
 *     scratch of their own (stream-K pieces, two-level statistics) take it from the workspace
 *     the caller registered for the stream with mvg_set_scratch, and run their scratch-free
 *     form when there is none;
 *   - every launch goes to the caller's hipStream_t (passed as void*; NULL = default stream);
 *   - return 0 on success, non-zero on error; mvg_last_error() gives the message. No exceptions
 *     cross the boundary.
 */
#ifndef ROTMVGAZE_H
#define ROTMVGAZE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVG_ABI_VERSION 13

/* ---------------------------------------------------------------- library */
int mvg_abi_version(void);
const char *mvg_last_error(void);
/* number of CUs of the current device (used by the host to size split-K). */
int mvg_device_cus(void);
/* Register (ptr != NULL) or drop (ptr == NULL) the caller-owned workspace that launches on `stream` of the
 * current device may use as scratch; 16-byte aligned, valid until replaced or dropped.  Uses are ordered by the
 * stream, so one workspace per stream suffices.  mvg_scratch_bytes(): a size that covers every entry point on
 * the current device.  Without a workspace (or with a smaller one) the affected launches run their
 * scratch-free forms: correct, a few percent slower on the stem / fusion-block GEMMs. */
int mvg_set_scratch(void *ptr, size_t bytes, void *stream);
size_t mvg_scratch_bytes(void);
/* A HIP stream of the device's LOWEST priority (hipStreamNonBlocking) for work that should only fill
 * what the caller's stream leaves idle - the backward-weight kernels, which are off the critical
 * path of backward.  NULL on failure.  The stream lives until process exit. */
void *mvg_stream_create_low_priority(void);
/* Data-parallel runs: leave n CUs out of the stream-K grids / wgrad and split-K plans so that the
 * RCCL kernels of the gradient all-reduce (side stream) find room next to the persistent conv
 * kernels instead of pushing part of their grid into a second round.  0 = use every CU. */
int mvg_set_reserved_cus(int n);

/* ---------------------------------------------------------------- profiling (bench.py)
 * When enabled, every launch is bracketed by hipEvents on its own stream; mvg_prof_collect
 * synchronises those events and returns, per kernel family, launches, summed milliseconds,
 * algorithmic FLOPs and algorithmic bytes since mvg_prof_reset. */
enum {
  MVG_K_CONV_FPROP = 0, MVG_K_CONV_DGRAD = 1, MVG_K_CONV_WGRAD = 2, MVG_K_WGRAD_REDUCE = 3,
  MVG_K_BN_FINALIZE = 4, MVG_K_BN_APPLY = 5, MVG_K_BN_BWD_REDUCE = 6, MVG_K_BN_BWD_APPLY = 7,
  MVG_K_POOL = 8, MVG_K_LAYOUT = 9, MVG_K_LINEAR_FPROP = 10, MVG_K_LINEAR_DGRAD = 11,
  MVG_K_LINEAR_WGRAD = 12, MVG_K_ROTCAT = 13, MVG_K_COLSUM = 14, MVG_K_LOSS = 15,
  MVG_K_GEOMETRY = 16, MVG_K_ELEMENTWISE = 17, MVG_K_FAMILIES = 18
};
typedef struct {
  int64_t launches;
  double ms;
  double flops;
  double bytes;
} mvg_prof_entry;
int mvg_prof_enable(int on);
int mvg_prof_reset(void);
int mvg_prof_collect(mvg_prof_entry *host_out /* [MVG_K_FAMILIES] */);
const char *mvg_prof_family_name(int family);

/* ---------------------------------------------------------------- convolution
 * Replaces nn.Conv2d(bias=False) forward/backward: resnet.py:31-47 (conv3x3/conv1x1), :184
 * (7x7 stem) as used by BasicBlock.forward :80-96 and Bottleneck.forward :128-148, and - with
 * h = w = r = s = 1 - nn.Linear inside Mlp (backbones/blocks.py:41-47,57-60). */
typedef struct {
  int32_t groups;      /* view groups; total images = groups * n */
  int32_t n;           /* images per group */
  int32_t h, w;        /* input spatial size */
  int32_t cin, cout;   /* cin % 4 == 0, cout % 4 == 0 (the stem's 3 channels are padded to 4) */
  int32_t r, s;        /* filter size */
  int32_t stride, pad;
  int32_t ho, wo;      /* output spatial size */
} mvg_conv_desc;

/* y[g][n][ho][wo][cout] = conv(x[g][n][h][w][cin], wgt[cout][r][s][cin]).
 * Epilogue (all optional, NULL = off):
 *   bias[cout]   added to every row, then relu != 0 clamps at 0            (Linear [+ReLU]);
 *   stats        per-(group, 32|64-row partial, channel) {sum, centred sum of squares} of y,
 *                the input of mvg_bn_finalize; needs mvg_conv_stats_partials() * cout * 2 floats
 *                per group.                                                  (conv -> BatchNorm) */
int mvg_conv_fprop(const mvg_conv_desc *d, const float *x, const float *wgt, float *y,
                   const float *bias, int relu, float *stats, void *stream);
/* Inference (model.eval(), trainer.py:164-199): BatchNorm uses its running statistics, so it folds
 * into the conv epilogue: out = [relu]( conv(x, wgt) * scale[cout] + shift[cout] [+ residual] ) in one
 * launch (scale/shift from mvg_bn_eval_affine) - no separate normalisation pass, no raw conv output. */
int mvg_conv_fprop_affine(const mvg_conv_desc *d, const float *x, const float *wgt, float *out,
                          const float *scale, const float *shift, const float *residual, int relu,
                          void *stream);
/* number of row-partials per group that mvg_conv_fprop writes into `stats`, and the rows per
 * partial (out_rows_per_partial, may be NULL). */
int mvg_conv_stats_partials(const mvg_conv_desc *d, int32_t *out_rows_per_partial);

/* dx[g][n][h][w][cin] = conv_transpose(dy[g][n][ho][wo][cout], wgt).  Epilogue (optional):
 *   mask   (same shape as dx): result multiplied by (mask > 0)   (ReLU backward of the producer);
 *   addend (same shape as dx, may alias dx): added after masking (residual / fan-in accumulation). */
int mvg_conv_dgrad(const mvg_conv_desc *d, const float *dy, const float *wgt, float *dx,
                   const float *mask, const float *addend, void *stream);

/* dw[cout][r][s][cin] (+)= sum over all groups/images/pixels of dy (x) x.  Split over the pixel
 * axis into `splits` slabs in `workspace` (splits * cout*r*s*cin floats, ignored when
 * splits == 1) that a second kernel sums in a fixed order (bitwise reproducible).
 * accumulate != 0 adds to the existing dw. */
int mvg_conv_wgrad(const mvg_conv_desc *d, const float *x, const float *dy, float *dw,
                   float *workspace, int splits, int accumulate, void *stream);
/* a split count that fills the device for this shape (host helper, no launch). */
int mvg_conv_wgrad_splits(const mvg_conv_desc *d);
/* Host-only plan queries of the fp32-MFMA kernels (tests guard with them which form a shape runs): answered by the
 * code the launches plan with, for the CUs the planners may use now (mvg_set_reserved_cus); nothing is launched and
 * no device is needed (then: 256 CUs, one workgroup per CU where the occupancy query fails).  -1 (and a message)
 * for a descriptor the launch would reject.
 * mvg_conv_plan_query: `kind` names the launch - MVG_PLAN_FPROP (mvg_conv_fprop without stats, mvg_conv_fprop_affine,
 * mvg_linear_fprop), MVG_PLAN_FPROP_STATS (mvg_conv_fprop with stats: never split-K), MVG_PLAN_DGRAD (mvg_conv_dgrad,
 * mvg_linear_dgrad), MVG_PLAN_FUSER_FPROP (mvg_fuser_fprop with the descriptor {1, rows, 1, 1, cf + 3 nvec, fout, 1, 1,
 * 1, 0, 1, 1}); ws_floats is the split-K workspace the launch would be given (0: none).  out may be NULL. */
enum { MVG_PLAN_FPROP = 0, MVG_PLAN_FPROP_STATS = 1, MVG_PLAN_DGRAD = 2, MVG_PLAN_FUSER_FPROP = 3 };
typedef struct {
  int32_t bm, bn, bk;      /* tile and K-step depth of the kernel instantiation */
  int32_t fasta;           /* 1: the uniform-tap operand loader */
  int32_t ncls;            /* classes in the launch (backward-data at stride 2: up to 4; those without taps are dropped) */
  int32_t cls_tiles[4];    /* per class, in launch order: tiles, */
  int32_t cls_kt[4];       /* ... and K-steps per tile */
  int32_t streamk_grid;    /* persistent workgroups of the stream-K form; 0: one tile (times splitk) per workgroup */
  int32_t splitk;          /* K splits into the caller's workspace (1: none) */
  int64_t scratch_floats;  /* registered scratch the stream-K form needs (0 when streamk_grid == 0); with less
                            * registered for the stream the launch takes the plain form */
} mvg_conv_plan;
int mvg_conv_plan_query(const mvg_conv_desc *d, int kind, size_t ws_floats, mvg_conv_plan *out);
/* the tile (bm rows of cout x bn columns of r*s*cin) mvg_conv_wgrad runs `d` on, and whether its loader steps the
 * pixel coordinates incrementally; every out-pointer may be NULL. */
int mvg_conv_wgrad_tile(const mvg_conv_desc *d, int32_t *bm, int32_t *bn, int32_t *incremental);
/* The cross-view fusion GEMM with its input generated inside the kernel (rot_mv.py:44-50 ImageFeatFuser
 * first layer on cat([img_feat_i, (R_ij @ F_j).flatten]), :234-239; and the gaze head's first layer on
 * cat([img_feat_i, F_i.flatten]), :249-254, with rel = NULL):
 *   y[m] = [relu]( W @ [ img_feat[row_img[m]] (cf) | rel[m] (3x3) @ feat[row_src[m]] (3 x nvec, axis-major) ] + bias )
 * for m < rows.  The concatenated / rotated row is built by the GEMM's operand loader (three loads and
 * three fmas per 16 bytes of the rotated part) - it is never written to memory; mvg_fuser_wgrad is the
 * backward-weight twin (dw += dy^T X, db += column sums of dy) with X generated the same way.
 * img_feat [img_rows][cf], feat [feat_rows][3*nvec], rel [rows][9] or NULL (identity), W [fout][cf + 3*nvec].
 * Workspaces like mvg_linear_fprop / mvg_linear_wgrad (fin = cf + 3*nvec). */
int mvg_fuser_fprop(const float *img_feat, const float *feat, const float *rel, const int32_t *row_img,
                    const int32_t *row_src, const float *w, const float *bias, int relu, float *y, int rows, int cf,
                    int nvec, int fout, int img_rows, int feat_rows, float *workspace, size_t ws_floats, void *stream);
int mvg_fuser_wgrad(const float *img_feat, const float *feat, const float *rel, const int32_t *row_img,
                    const int32_t *row_src, const float *dy, float *dw, float *db, int rows, int cf, int nvec, int fout,
                    int img_rows, int feat_rows, float *workspace, int splits, int accumulate, void *stream);

/* nn.Linear backward-weight (blocks.py:41-47 under autograd): dw[fout][fin] (+)= dy^T x and, in the SAME
 * launch, the bias gradient db[fout] (+)= column sums of dy (the kernel streams dy anyway; db may be NULL).
 * splits = mvg_conv_wgrad_splits(linear descriptor); workspace: splits * (fout*fin + fout) floats when
 * splits > 1. */
int mvg_linear_wgrad(const float *x, const float *dy, float *dw, float *db, int rows, int fin, int fout,
                     float *workspace, int splits, int accumulate, void *stream);

/* nn.Linear forward / backward-data (backbones/blocks.py:41-47 inside Mlp): the conv kernels with
 * h = w = r = s = 1 plus split-K - with a few hundred rows the tile grid cannot fill 256 CUs, so
 * K is cut into slices whose partial tiles land in `workspace` (mvg_linear_workspace_floats()
 * floats) and are summed, in fixed order, by a reduce kernel that applies the epilogue.
 *   fprop: y = [relu](x @ w^T + bias);   dgrad: dx = (dy @ w) * (mask > 0) + addend. */
size_t mvg_linear_workspace_floats(int rows, int fin, int fout);
int mvg_linear_fprop(const float *x, const float *w, const float *bias, int relu, float *y, int rows,
                     int fin, int fout, float *workspace, size_t ws_floats, void *stream);
int mvg_linear_dgrad(const float *dy, const float *w, const float *mask, const float *addend, float *dx,
                     int rows, int fin, int fout, float *workspace, size_t ws_floats, void *stream);

/* ---------------------------------------------------------------- BatchNorm2d (train + eval)
 * Replaces nn.BatchNorm2d (eps 1e-5, momentum 0.1, affine, track_running_stats) as constructed
 * at resnet.py:185,72-76,119-125 and the ReLU / residual add around it (:74,93-94,140-146). */

/* Merge the conv epilogue's partials into per-(group, channel) batch statistics, produce the
 * fused affine (scale = gamma*invstd, shift = beta - mean*scale) and update the running stats
 * once per group IN GROUP ORDER (view 0 first: rot_mv.py:196-197) with the unbiased variance.
 *   stats        [groups][partials][2][c]     rows_per_partial, rows_per_group as given
 *   mean,invstd  [groups][c] (saved for backward), scale, shift [groups][c]
 *   running_mean/var [c] updated in place unless NULL; num_batches_tracked is host-side. */
int mvg_bn_finalize(const float *stats, int groups, int partials, int rows_per_partial,
                    int64_t rows_per_group, int c, const float *gamma, const float *beta,
                    float *running_mean, float *running_var, float momentum, float eps,
                    float *mean, float *invstd, float *scale, float *shift, void *stream);
/* eval mode: scale/shift from the running statistics (same for every group). */
int mvg_bn_eval_affine(int groups, int c, const float *gamma, const float *beta,
                       const float *running_mean, const float *running_var, float eps,
                       float *scale, float *shift, void *stream);
/* Every BatchNorm of a network folded by ONE launch (the inference session's bind; 20 / 53 records for ResNet-18 / -50).
 * items_dev: n records in DEVICE memory of
 *   { const float *gamma, *beta, *running_mean, *running_var; float *scale, *shift; int32 c; int32 pad; }  (56 bytes);
 * scale[c] / shift[c] of every record receive the bits mvg_bn_eval_affine(1, c, ...) leaves (one device function serves
 * both kernels).  max_c: the widest record's channel count (it sizes the grid). */
int mvg_bn_eval_affine_batch(const void *items_dev, int n, int max_c, float eps, void *stream);
/* out = [relu]( y*scale[g] + shift[g] [+ residual] );  y,out,residual: [groups][rows][c].
 * res_scale/res_shift ([groups][c], both or neither): the residual is the RAW output of the block's
 * downsample conv and its BatchNorm (residual*res_scale + res_shift) is applied here, so the normalised
 * downsample map is never written (resnet.py:88-93,137-145). */
int mvg_bn_apply(const float *y, const float *scale, const float *shift, const float *residual,
                 const float *res_scale, const float *res_shift, int relu, float *out, int groups,
                 int64_t rows_per_group, int c, void *stream);
/* mvg_bn_apply for a residual unit (relu = 1) that also records the ReLU mask: relu_bits holds one byte per
 * 16-byte access of `out` (bit k = element k > 0; groups*rows*c/4 bytes in fp32, /8 in bf16).
 * mvg_bn_bwd_reduce_bits takes the mask from those bytes instead of `act`: 1/16 of the bytes of reading the
 * activation again (resnet.py:93-94,145-146 under autograd: the ReLU after the residual add). */
int mvg_bn_apply_bits(const float *y, const float *scale, const float *shift, const float *residual,
                      const float *res_scale, const float *res_shift, float *out, uint8_t *relu_bits, int groups,
                      int64_t rows_per_group, int c, void *stream);
int mvg_bn_bwd_reduce_bits(const float *g, const uint8_t *relu_bits, const float *y, const float *mean,
                           const float *invstd, int groups, int64_t rows_per_group, int c, float *s1, float *s2,
                           float *dgamma, float *dbeta, int accumulate, float *workspace, float *dz_out, void *stream);
int mvg_bn_apply_bits_bf16(const uint16_t *y, const float *scale, const float *shift, const uint16_t *residual,
                           const float *res_scale, const float *res_shift, uint16_t *out, uint8_t *relu_bits,
                           int groups, int64_t rows_per_group, int c, void *stream);
int mvg_bn_bwd_reduce_bits_bf16(const uint16_t *g, const uint8_t *relu_bits, const uint16_t *y, const float *mean,
                                const float *invstd, int groups, int64_t rows_per_group, int c, float *s1,
                                float *s2, float *dgamma, float *dbeta, int accumulate, float *workspace,
                                uint16_t *dz_out, void *stream);
/* Backward, step 1: per (group, channel) s1 = sum(dz), s2 = sum(dz * xhat), xhat = (y - mean) * invstd,
 * dz = g masked by the unit's ReLU.  The mask comes from `act` (the unit's output: act > 0) or, for
 * a ReLU without residual, from (relu_scale, relu_shift) = the scale/shift mvg_bn_apply used:
 * fma(y, scale, shift) > 0 is the same bit pattern and saves reading act.  Both NULL: no ReLU.
 * Also dgamma[c] (+)= sum_g s2, dbeta[c] (+)= sum_g s1 (accumulate flag).
 * dz_out (may be NULL, may alias g): the masked gradient dz is written out, so that mvg_bn_bwd_apply can
 * run on it without reading the mask again and the residual branch gets its gradient from the same buffer.
 * workspace: mvg_bn_bwd_workspace_floats() floats. */
int mvg_bn_bwd_reduce(const float *g, const float *act, const float *y, const float *mean,
                      const float *invstd, const float *relu_scale, const float *relu_shift,
                      int groups, int64_t rows_per_group, int c, float *s1, float *s2, float *dgamma,
                      float *dbeta, int accumulate, float *workspace, float *dz_out, void *stream);
size_t mvg_bn_bwd_workspace_floats(int groups, int64_t rows_per_group, int c);
/* Backward, step 2: dy = gamma*invstd*(dz - s1/n - xhat*s2/n); dz_out (optional, may alias g)
 * receives the masked gradient for the residual branch. */
int mvg_bn_bwd_apply(const float *g, const float *act, const float *y, const float *mean,
                     const float *invstd, const float *gamma, const float *s1, const float *s2,
                     const float *relu_scale, const float *relu_shift, int groups,
                     int64_t rows_per_group, int c, float *dy, float *dz_out, void *stream);
/* Eval mode (model.eval() with gradients): backward of BatchNorm2d on its RUNNING statistics - what autograd
 * differentiates for F.batch_norm(training=False) in resnet.py:84,88,132,136,140 (:91,143: the downsample
 * BatchNorm) - in ONE pass, since nothing depends on batch sums:
 *   dz = g masked by the unit's ReLU,  dy = gamma*invstd_r*dz,  invstd_r = 1/sqrt(running_var + eps),
 *   dbeta[c] (+)= sum dz,  dgamma[c] (+)= sum dz*(y - running_mean)*invstd_r  (over every row of every group).
 * The mask, as the forward decided it: act > 0, relu_bits (mvg_bn_apply_bits' layout), or fma(y, relu_scale,
 * relu_shift) > 0 with the [groups][c] scale / shift of mvg_bn_eval_affine; all NULL: no ReLU (downsample branch).
 * dy may alias g; dz_out (optional, may alias g, not dy) receives dz for the residual branch.  The sums are left
 * per (group, chunk, channel) in `workspace` and a second launch adds them in a fixed order (reproducible);
 * dgamma / dbeta NULL: no sums.  workspace: mvg_bn_eval_bwd_workspace_floats() floats (both entry points). */
int mvg_bn_eval_bwd(const float *g, const float *act, const uint8_t *relu_bits, const float *y, const float *relu_scale,
                    const float *relu_shift, const float *gamma, const float *running_mean, const float *running_var,
                    float eps, int groups, int64_t rows_per_group, int c, float *dy, float *dz_out, float *dgamma,
                    float *dbeta, int accumulate, float *workspace, void *stream);
size_t mvg_bn_eval_bwd_workspace_floats(int groups, int64_t rows_per_group, int c);

/* Host-only plan query of the BatchNorm passes (ABI v13; tests guard with it which form a shape runs): answered by the
 * functions the launches plan with, for the CUs the planners may use now (mvg_set_reserved_cus; 256 without a device);
 * nothing is launched.  -1 (and a message) for sizes the launch would reject.  `pass` names the launch, `elem` the
 * storage family (SP: mvg_bn_apply_split / mvg_bn_bwd_apply_split / the _split reduce entry points, which read fp32 and
 * keep a third workspace row).  rows_per_group: rows of [rows][c] (ignored by the POOL passes, which take n_per_group, h,
 * w of the conv output and pool 3x3 / 2 / 1); partials and scratch_floats (the floats registered for the stream with
 * mvg_set_scratch, 0: none) matter to FINALIZE only.  Fields a pass does not have stay 0.  out may be NULL. */
enum { MVG_BN_PASS_APPLY = 0, MVG_BN_PASS_BWD_APPLY = 1, MVG_BN_PASS_BWD_REDUCE = 2, MVG_BN_PASS_EVAL_BWD = 3,
       MVG_BN_PASS_POOL_BWD_REDUCE = 4, MVG_BN_PASS_POOL_EVAL_BWD = 5, MVG_BN_PASS_FINALIZE = 6 };
enum { MVG_BN_ELEM_FP32 = 0, MVG_BN_ELEM_BF16 = 1, MVG_BN_ELEM_SP = 2 };
enum { MVG_BN_MERGE_WALK_GROUPS = 0, MVG_BN_MERGE_ALL_GROUPS = 1, MVG_BN_MERGE_PER_GROUP = 2 };
typedef struct {
  /* streaming passes (APPLY, BWD_APPLY) */
  int64_t accesses_per_group; /* 16-byte accesses (sp: 8-channel chunks) per group */
  int32_t grid_x;             /* workgroups of 256 lanes per group (at most 4096) */
  int32_t trips;              /* loop trips of the busiest lane */
  int32_t step;               /* column groups a lane advances by per trip (0: it keeps its channels) */
  /* reduce-type passes (BWD_REDUCE, EVAL_BWD, POOL_BWD_REDUCE, POOL_EVAL_BWD) */
  int32_t cwn, cw;            /* column groups per row, and per column block */
  int32_t column_blocks;      /* grid.y; the last block is partly masked when cw does not divide cwn */
  int32_t row_lanes;          /* 256 / cw */
  int32_t chunks;             /* grid.x: row ranges (POOL_BWD_REDUCE: ranges of pooled lines; POOL_EVAL_BWD: workgroups) */
  int32_t empty_chunks;       /* trailing chunks that receive no rows */
  int64_t rows_per_chunk;     /* rows (pooled lines) per chunk; 0 for POOL_EVAL_BWD's grid-stride loop */
  int64_t workspace_floats;   /* what the reported chunks write of the caller's workspace */
  /* FINALIZE */
  int32_t form;               /* MVG_BN_MERGE_*: one workgroup walks the groups / 2 - 4 groups share a workgroup's lanes /
                               * one workgroup per group, then the running-statistics update */
  int32_t lanes_per_group;    /* partial lanes merging one (channel, group) */
  int32_t slices;             /* slices per group the partials are first collapsed to (0: unsliced) */
  int32_t partials_per_slice; /* 0 when unsliced */
  int64_t scratch_floats;     /* what the stream must have registered for the fastest form of these sizes (0: none) */
} mvg_bn_plan;
int mvg_bn_plan_query(int pass, int elem, int groups, int64_t rows_per_group, int c, int n_per_group, int h, int w,
                      int partials, size_t scratch_floats, mvg_bn_plan *out);

/* ---------------------------------------------------------------- pooling / layout
 * nn.MaxPool2d(3,2,1) resnet.py:189; nn.AdaptiveAvgPool2d((1,1)) resnet.py:200 + rot_mv.py:126;
 * NCHW float input of FeatRotationSymm.forward (rot_mv.py:188-189) -> NHWC4. */
int mvg_maxpool3x3s2_fwd(const float *x, float *y, uint8_t *argmax, int n, int h, int w, int c,
                         int ho, int wo, void *stream);
int mvg_maxpool3x3s2_bwd(const float *dy, const uint8_t *argmax, float *dx, int n, int h, int w,
                         int c, int ho, int wo, void *stream);
/* Stem tail fused: pooled = MaxPool2d(3,2,1)(relu(y*scale + shift)) without materialising the
 * normalised activation (torchvision resnet.py:187-189 conv1 -> bn1 -> relu -> maxpool, called from
 * /root/reference/models/rot_mv.py:204-205).  y [groups][n_per_group][h][w][c]; scale/shift
 * [groups][c] from mvg_bn_finalize / mvg_bn_eval_affine.  The backward pair rebuilds the gradient
 * of the BN output from (g_pooled, argmax) and the ReLU mask from y: same results as
 * mvg_maxpool3x3s2_bwd -> mvg_bn_bwd_reduce -> mvg_bn_bwd_apply, 2.3 GB less traffic at C2. */
int mvg_bn_relu_maxpool_fwd(const float *y, const float *scale, const float *shift, float *pooled,
                            uint8_t *argmax, int groups, int n_per_group, int h, int w, int c,
                            int ho, int wo, void *stream);
int mvg_bn_relu_maxpool_bwd_reduce(const float *g_pooled, const uint8_t *argmax, const float *y,
                                   const float *mean, const float *invstd, const float *scale,
                                   const float *shift, int groups, int n_per_group, int h, int w,
                                   int c, int ho, int wo, float *s1, float *s2, float *dgamma,
                                   float *dbeta, int accumulate, float *workspace, void *stream);
int mvg_bn_relu_maxpool_bwd_apply(const float *g_pooled, const uint8_t *argmax, const float *y,
                                  const float *mean, const float *invstd, const float *gamma,
                                  const float *scale, const float *shift, const float *s1,
                                  const float *s2, int groups, int n_per_group, int h, int w, int c,
                                  int ho, int wo, float *dy, void *stream);
/* The stem tail in eval mode (resnet.py:262-265 with bn1 on its running statistics): max-pool backward through
 * argmax, the ReLU mask fma(y, scale, shift) > 0 (scale / shift [groups][c] of mvg_bn_eval_affine), and
 * dy = gamma*invstd_r*dz in one pass that writes dy [groups][n_per_group][h][w][c] once; dgamma / dbeta as
 * mvg_bn_eval_bwd.  c/4 must divide 256. */
int mvg_bn_relu_maxpool_eval_bwd(const float *g_pooled, const uint8_t *argmax, const float *y, const float *scale,
                                 const float *shift, const float *gamma, const float *running_mean,
                                 const float *running_var, float eps, int groups, int n_per_group, int h, int w,
                                 int c, int ho, int wo, float *dy, float *dgamma, float *dbeta, int accumulate,
                                 float *workspace, void *stream);
int mvg_avgpool_fwd(const float *x, float *y, int n, int hw, int c, void *stream);
int mvg_avgpool_bwd(const float *dy, float *dx, int n, int hw, int c, void *stream);
int mvg_nchw_to_nhwc4(const float *src, float *dst, int n, int c, int h, int w, void *stream);
int mvg_nhwc4_to_nchw(const float *src, float *dst, int n, int c, int h, int w, void *stream);
/* GPU input pipeline: raw uint8 [n][h][w][3] face patches (the HDF5
 * `face_patch` layout, dataset/gaze.py:122) -> optional BGR->RGB (:108-109) -> /255 (ToTensor) ->
 * (x - mean)/std (Normalize, main.py:38-39,54) -> NHWC4 fp32, the backbone's input layout. */
int mvg_preprocess_u8hwc(const uint8_t *src, float *dst, int n, int h, int w, float mean0, float mean1,
                         float mean2, float std0, float std1, float std2, int swap_rb, void *stream);
/* The same with the Resize((oh, ow), antialias=True) of main.py:46,53 between ToTensor and Normalize, for
 * patches that are not already oh x ow (h == oh && w == ow is mvg_preprocess_u8hwc: torchvision returns
 * the input unchanged).  Resize on a float tensor is torch.nn.functional.interpolate(mode="bilinear",
 * antialias=True, align_corners=False) (ATen _upsample_bilinear2d_aa): width pass, then height.
 * dst [n][oh][ow][4]. */
int mvg_preprocess_u8hwc_resize(const uint8_t *src, float *dst, int n, int h, int w, int oh, int ow, float mean0,
                                float mean1, float mean2, float std0, float std1, float std2, int swap_rb,
                                void *stream);
/* RandomMultiErasing.__call__ utils/augment.py:38-47 on a device batch: img [n][c][h][w] *= the
 * nearest-neighbour upsampling (F.interpolate default, augment.py:21) of masks[n] (grid[n] x grid[n]
 * floats in a gmax*gmax slot); grid[n] == 0 leaves image n untouched.  The random draws stay on the
 * host (rot_mvgaze_amd/augment.py replays the reference's RNG calls). */
int mvg_multi_erase_nchw(float *img, const float *masks, const int32_t *grid, int gmax, int n, int c,
                         int h, int w, void *stream);
/* The random part of the reference's training transform (main.py:41-49) on raw uint8 patches, one launch per batch:
 * ColorJitter(brightness, contrast, saturation) and RandomAffine(degrees=0, scale, translate), bit for bit what
 * torchvision computes on the PIL image - Pillow's ImageEnhance.{Brightness, Contrast, Color} (ImagingBlend against
 * a degenerate image; every op quantises to uint8) in a per-image order, then Image.transform(AFFINE, NEAREST) on its
 * scale-only path (per-axis source-index tables built by repeated double additions; outside = 0).
 * One record per image, in a DEVICE array: packed on the host from the reference's RNG calls in its order (the default,
 * rot_mvgaze_amd/augment.py TrainAugment.draw) or written on the device by mvg_augment_draw below. */
typedef struct mvg_augment_rec {
  float factor[3];   /* brightness, contrast, saturation factor (1 = identity) */
  int32_t order[3];  /* the ops in the order applied: a permutation of 0 brightness, 1 contrast, 2 saturation */
  double a0, cx;     /* inverse affine map, x axis: src_x = a0 * (x + 0.5) + cx (torchvision's matrix[0], matrix[2]) */
  double a4, cy;     /* ... y axis (matrix[4], matrix[5]); the off-diagonal terms are zero */
} mvg_augment_rec;
/* src [n][h][w][3] uint8 (swap_rb: stored BGR, swapped first: grey is computed on RGB).  Destinations, at least one:
 * dst_u8 [n][h][w][3], the augmented RGB image, and / or dst_nhwc4 [n][h][w][4] fp32, that image through ToTensor and
 * Normalize exactly as mvg_preprocess_u8hwc computes them (channel 3 zero), then - masks / grid non-null - times the
 * RandomMultiErasing keep-mask by mvg_multi_erase_nchw's index rule (masks [n][gmax*gmax], grid [n]; the uint8
 * destination is the image before ToTensor and is not erased).  recs_host (optional): the same n records in host
 * memory, checked before the launch (the order must be a permutation).  h, w <= 8192 and h*w <= 16843009. */
int mvg_augment_u8hwc(const uint8_t *src, const mvg_augment_rec *recs, const mvg_augment_rec *recs_host,
                      uint8_t *dst_u8, float *dst_nhwc4, const float *masks, const int32_t *grid, int gmax, int n,
                      int h, int w, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                      int swap_rb, void *stream);
/* The same launch straight into the bf16 stem's operand (training steps of the bf16 storage path on raw patches: no
 * fp32 image in between).  Every value is mvg_augment_u8hwc's dst_nhwc4 value - normalised, times the keep-mask -
 * rounded once to bf16 (nearest even).  Destinations, at least one, both from one launch allowed:
 * dst_nhwc8 [n][h][w][8], channels 3..7 zero (mvg_preprocess_u8hwc_resize_bf16's layout), and / or dst_rw
 * [n][h][w/4][64], mvg_stem_rowwindow_bf16's folded row windows: window m of an image row holds image columns
 * 4m-4 .. 4m+11 x (r, g, b, 0); columns outside [0, w) are bf16 zero (padding - the pixels the affine map fills are
 * inside the image and carry normalised black).  dst_rw needs w % 4 == 0.  The launch writes every byte of its
 * destinations, which may arrive uninitialised.  The other arguments and checks are mvg_augment_u8hwc's.
 * (Added under ABI v13: additive.) */
int mvg_augment_u8hwc_bf16(const uint8_t *src, const mvg_augment_rec *recs, const mvg_augment_rec *recs_host,
                           uint16_t *dst_nhwc8, uint16_t *dst_rw, const float *masks, const int32_t *grid, int gmax,
                           int n, int h, int w, float mean0, float mean1, float mean2, float std0, float std1,
                           float std2, int swap_rb, void *stream);
/* The per-image draws of that transform made on the device: one launch writes the n records, and with an erase the
 * keep-masks [n][gmax*gmax] and grid sizes [n], that the two entry points above read - no host draw, no copy, no
 * synchronisation, so an augmented step can be captured.  The distributions are the reference's; the RNG stream is not
 * (TrainAugment(draws="host") replays that).  cfg: a host mvg_augment_draw_cfg (rotmvgaze_augment_draw.h), read during
 * the call.  masks and grid may both be NULL (no erase: gmax is then 0); with them, gmax == (int)(1.0 / cfg->dot_lo) <= 64.
 * Generator: Philox4x32-10, key (seed low word, seed high word), counter (image i, block j, launch counter low word,
 * high word).  The launch counter is a uint64 in DEVICE memory at counter_dev: every draw of a launch uses the value it
 * had when the launch began, and the launch adds one to it in stream order - a replayed graph draws afresh on every
 * replay, and (seed, counter) reproduces a launch.  The word assignment does not depend on which ops are enabled:
 *   block 0: order, brightness, contrast, saturation     block 1: tx, ty, scale, erase-apply
 *   block 2: dot size, proportion, two unused            block 3 + c/4, word c%4: mask cell c = row * g + column
 * Arithmetic, every operation rounded on its own (no fused multiply-add), so that it can be restated exactly:
 *   u = (float)(x >> 8) * 2^-24;  order = the k-th permutation of (0, 1, 2) in lexicographic order, k = (x * 6) >> 32;
 *   a factor = u * (hi - lo) + lo in fp32 (torch's uniform_);  tx = (int)rintf(u * (2 max_dx) - max_dx), ty likewise;
 *   the scale s in fp32 like a factor, then in doubles a0 = a4 = 1.0 / s, cx = a0 * (-w/2 - tx) + w/2, cy likewise with h;
 *   the erase applies unless (double)u > p;  dot = dot_lo + (dot_hi - dot_lo) * (double)u,  g = (int)(1.0 / dot) clamped
 *   to [1, gmax],  prop likewise from the proportion range,  cell keep = (double)u > prop ? 1 : 0.
 * Every byte of recs, masks and grid is written by every launch (they may arrive uninitialised): mask cells past g*g
 * are 0, and an image that is not erased gets grid 0 and an all-zero mask slot.  (Added under ABI v13: additive.) */
int mvg_augment_draw(mvg_augment_rec *recs, float *masks, int32_t *grid, int gmax, int n, int h, int w, const void *cfg,
                     uint64_t seed, uint64_t *counter_dev, void *stream);

/* ---------------------------------------------------------------- geometry
 * rotation_matrix_2d utils/math.py:188-219; relative rotations rot_mv.py:193-194. */
int mvg_rotation_matrix_2d(const float *pitch_yaw /*[n][2]*/, float *rot /*[n][3][3]*/, int n,
                           int inverse, void *stream);
/* rel[d][b] = rot[b][vi[d]] @ rot[b][vj[d]]^T for d < dirs; rot [b][views][3][3]. */
int mvg_relative_rotation(const float *rot, const int32_t *vi, const int32_t *vj, float *rel,
                          int batch, int views, int dirs, void *stream);

/* ---------------------------------------------------------------- cross-view fusion operands
 * ImageFeatFuser.forward's cat([img_feat, (R @ F).flatten]) rot_mv.py:44-50,234-239 and the head's
 * cat([img_feat, F.flatten]) :249-254.  Row (d, b) of x = [ img_feat[view_of[d]][b] (cf floats),
 * rel[d][b] @ feat[src_of[d]][b] (3*nvec floats, axis-major) ]; rel == NULL means identity. */
int mvg_rotcat_fwd(const float *img_feat /*[views][batch][cf]*/, const float *feat /*[dirs][batch][3][nvec]*/,
                   const float *rel /*[dirs][batch][3][3] or NULL*/, const int32_t *view_of,
                   const int32_t *src_of, float *x /*[dirs][batch][cf+3*nvec]*/, int batch, int dirs,
                   int cf, int nvec, void *stream);
/* dfeat[src_of[d]][b] = rel[d][b]^T @ dx_rot  (src_of must be injective: every slot written once). */
int mvg_rotcat_bwd(const float *dx, const float *rel, const int32_t *src_of, float *dfeat, int batch,
                   int dirs, int cf, int nvec, void *stream);
/* ---------------------------------------------------------------- ablation variants
 * encode_rotmat, ImageRotmatFeatFuser.forward rot_mv.py:62-69: row (d, b) of x (row length ld,
 * zero-padded) = [ img_feat[view_of[d]][b] | (rel_apply[d][b] @) feat[src_of[d]][b] | rel_append[d][b]
 * flattened (9) ]; either rel may be NULL (no rotation applied / nothing appended). */
int mvg_rotcat_ext_fwd(const float *img_feat, const float *feat, const float *rel_apply,
                       const float *rel_append, const int32_t *view_of, const int32_t *src_of,
                       float *x, int ld, int batch, int dirs, int cf, int nvec, void *stream);
int mvg_rotcat_ext_bwd(const float *dx, int ld, const float *rel, const int32_t *src_of, float *dfeat,
                       int batch, int dirs, int cf, int nvec, void *stream);
/* share_feature: IntensityBatchNorm rot_mv.py:13-32 as used by RotFeatFuser.forward :82-86.  The
 * 2*dirs calls of one iteration (direction d: a[view_of[d]] then feat[src_of[d]]) run in order on
 * the fuser's running_mean [nvec] (updated in place when training); scales [2*dirs][nvec] =
 * 1 / (running_mean + eps) as each call saw it. */
int mvg_ibn_scales(const float *a /*[views][batch][3][nvec]*/, const float *feat /*[srcs][batch][3][nvec]*/,
                   const int32_t *view_of, const int32_t *src_of, float *running_mean, int training,
                   float momentum, float eps, float *scales, int batch, int dirs, int nvec,
                   void *stream);
/* x[(d,b)][axis][0:nvec] = scales[2d] * a[view_of[d]][b][axis], [nvec:2nvec] = scales[2d+1] * (rel[d][b] @
 * feat[src_of[d]][b])[axis]: cat([.,.], dim=-1).flatten(-2,-1) of rot_mv.py:85 (scales) and :241-247
 * (gaze head input, scales == NULL, rel == NULL).  Backward: da_dir [(d,b)][3][nvec] (sum it over
 * directions with mvg_segment_sum) and dfeat[src_of[d]][b] = rel^T @ (...). */
int mvg_paircat_fwd(const float *a, const float *feat, const float *rel, const float *scales,
                    const int32_t *view_of, const int32_t *src_of, float *x, int batch, int dirs,
                    int nvec, void *stream);
int mvg_paircat_bwd(const float *dx, const float *rel, const float *scales, const int32_t *src_of,
                    float *da_dir, float *dfeat, int batch, int dirs, int nvec, void *stream);
/* out[v][b][0:width] (+)= sum over d with seg_of[d] == v, ascending d (reproducible), of
 * x[(d*batch + b)*row_stride + 0:width].  Gradient fan-in of the per-view features that several
 * directed pairs read (img_feat in every fuser/head input, the lifted feature at iteration 0). */
int mvg_segment_sum(const float *x, int64_t row_stride, int width, const int32_t *seg_of, float *out,
                    int batch, int dirs, int segments, int accumulate, void *stream);

/* y = a*x + b*y (n floats) - gradient fan-in accumulation. */
int mvg_axpby(const float *x, float *y, float a, float b, int64_t n, void *stream);
/* out = x * scale[0] with the scale read on the device (upstream gradient of a scalar loss). */
int mvg_scale_by(const float *x, const float *scale, float *out, int64_t n, void *stream);

/* Linear with out_features <= 4 (the gaze head's Linear(512 -> 2), rot_mv.py:179-184), for which a
 * 32-wide MFMA tile would be >90% padding.  bwd: dx = (dy @ w) * (mask > 0) [mask optional],
 * dw (+)= dy^T @ x, db (+)= colsum(dy); dx / dw may be NULL to skip. */
int mvg_linear_skinny_fwd(const float *x, const float *w, const float *bias, float *y, int rows, int k,
                          int nout, void *stream);
/* dx_absmax (may be NULL): a device float slot that receives max |dx| (its bits, by atomicMax: the caller clears it) */
int mvg_linear_skinny_bwd(const float *dy, const float *x, const float *w, const float *mask, float *dx,
                          float *dw, float *db, int rows, int k, int nout, int accumulate, float *dx_absmax, void *stream);

/* ---------------------------------------------------------------- optimizer
 * torch.optim.Adam step (trainer.py:54,141-143: betas (0.9, 0.999), eps 1e-8, coupled L2
 * weight_decay 1e-6, bias correction) over flat fp32 arenas - the model keeps parameters and
 * gradients in two arenas with identical offsets, so one launch updates every parameter. */
int mvg_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step, void *stream);
/* The same step with nothing from the host but the launch itself (a step captured in a hipGraph replays it): lr_dev = one
 * device float (CyclicLR writes it when it steps, trainer.py:58-62,147), state3 = three device floats {step, 1 - beta1^step,
 * sqrt(1 - beta2^step)} - zero-initialised, advanced by a one-thread launch in front of the update. */
int mvg_adam_step_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const float *lr_dev,
                      float *state3, float beta1, float beta2, float eps, float weight_decay, void *stream);
/* The step of mvg_adam_step over SEGMENTS of the arenas only - parameter groups with their own hyper-parameters, parameters
 * without a gradient left out (fine-tuning: optim.Adam).  Segment i is the element range [host_bounds[2 i], host_bounds[2 i + 1])
 * (both multiples of 4, begin < end, inside [0, n)), updated with host_hyper[5 i ..] = {lr, beta1, beta2, eps, weight_decay} and
 * the bias corrections of its OWN step count host_steps[i] >= 1 (computed on the host in double, as mvg_adam_step does).  The
 * three arrays are HOST memory, sorted by begin and disjoint; anything else is rejected before the first launch.  Each launch
 * takes up to MVG_ADAM_MAX_SEGMENTS segments by value in its kernel arguments (no device table, no copy); more segments are more
 * launches.  Elements outside every segment are neither read nor written: a launch moves 28 B per element of its segments.
 * A segment's result equals, bit for bit, mvg_adam_step over that slice with the same hyper-parameters and step. */
enum { MVG_ADAM_MAX_SEGMENTS = 16 };
int mvg_adam_step_segments(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                           const int64_t *host_bounds, const float *host_hyper, const int32_t *host_steps, int n_segments,
                           void *stream);
/* mvg_adam_step_segments with nothing from the host but the launch itself (a fine-tuning step captured in a hipGraph replays
 * it).  The segments travel by value as above - host_bounds as there, host_hyper[4 i ..] = {beta1, beta2, eps, weight_decay},
 * host_lr_index[i] in [0, n_lr): constants of a captured plan - and two things live on the DEVICE: lr_dev[n_lr], one float per
 * parameter group (the host rewrites an entry between replays when a scheduler moved that group's learning rate; segment i
 * reads lr_dev[host_lr_index[i]]), and state3_dev[n_segments][3], one row {step, 1 - beta1^step, sqrt(1 - beta2^step)} per
 * segment (a row starts as {count so far, 0, 0}).  Per MVG_ADAM_MAX_SEGMENTS segments there are two launches: a small one that
 * advances those segments' rows, each exactly once and with its segment's betas (the arithmetic of mvg_adam_step_dev's tick),
 * then the update, which reads lr_dev[..] / row[1] and row[2].  Null pointers, an lr index outside [0, n_lr) and segments that
 * are unsorted, overlapping, not aligned to 4, outside [0, n) or empty are rejected before the first launch, the tick included:
 * a rejected call has advanced no row and updated nothing.  Elements outside every segment are neither read nor written.  A
 * segment's result equals, bit for bit, mvg_adam_step_dev over that slice with a one-element lr_dev and the same row. */
int mvg_adam_step_segments_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                               const int64_t *host_bounds, const float *host_hyper, const int32_t *host_lr_index, int n_segments,
                               const float *lr_dev, int n_lr, float *state3_dev, void *stream);
/* Global-norm gradient clipping and the non-finite guard of the segmented steps.  mvg_grad_norm_segments reads the gradients of
 * the segments (host_bounds as above, checked by the same rules before the first launch; nothing outside a segment is read)
 * once and leaves the record clip4_dev = four device floats {norm, coef, skipped, skipped_total}: norm = sqrt(sum of squares),
 * coef = min(1, max_norm / (norm + 1e-6)) formed in double (torch.nn.utils.clip_grad_norm_'s coefficient; max_norm <= 0: no
 * clipping, coef = 1), skipped = 1 when skip_nonfinite is set and the sum is not finite (coef is then 0; with skip_nonfinite
 * clear a non-finite sum gives the NaN / 0 coefficient torch's formula gives), skipped_total += skipped - the one field that is
 * read before it is written, so the caller zeroes the record once.  The sum is accumulated in double: a finite fp32 gradient
 * cannot overflow it, and it is non-finite exactly when an element is.  One partial-sum launch per MVG_ADAM_MAX_SEGMENTS
 * segments, each workgroup storing one double to the caller's workspace ws (at least mvg_grad_norm_workspace_bytes(n_segments)
 * bytes, 8-byte aligned; a smaller one is rejected), then one one-workgroup launch that adds the partials in a fixed order: no
 * atomics, and the grids depend on the segment sizes and the CU count alone, so equal inputs give equal bits.  Nothing is
 * allocated and nothing synchronises.
 * mvg_adam_step_segments_clip / mvg_adam_step_segments_dev_clip are the two segmented steps reading that record: the gradient is
 * multiplied by coef as it is loaded (rounded to fp32 on its own: the result equals, bit for bit, the unclipped entry point on a
 * gradient scaled by coef in fp32; the gradient arena is not rewritten), and with skipped != 0 the update - and the device
 * form's tick - leave parameters, moments and state rows as they are. */
int64_t mvg_grad_norm_workspace_bytes(int n_segments);
int mvg_grad_norm_segments(const float *grad, int64_t n, const int64_t *host_bounds, int n_segments, float max_norm,
                           int skip_nonfinite, void *ws, int64_t ws_bytes, float *clip4_dev, void *stream);
int mvg_adam_step_segments_clip(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                                const int64_t *host_bounds, const float *host_hyper, const int32_t *host_steps, int n_segments,
                                const float *clip4_dev, void *stream);
int mvg_adam_step_segments_dev_clip(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                                    const int64_t *host_bounds, const float *host_hyper, const int32_t *host_lr_index, int n_segments,
                                    const float *lr_dev, int n_lr, float *state3_dev, const float *clip4_dev, void *stream);
/* DECOUPLED weight decay (torch.optim.AdamW; optim.AdamW and optim.Adam(decoupled_weight_decay=True)) on every step form.  One
 * element:  f = 1 - lr * weight_decay (float, formed on the device by every form as one fused multiply-add; lr is the plain
 * learning rate, not lr / bc1),  q = p * f,  m' = b1 m + (1 - b1) g,  v' = b2 v + (1 - b2) g^2,
 * p' = q - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps) - the gradient alone enters the moments (already multiplied by coef in
 * a clipped step).  With weight_decay = 0 the result equals the coupled entry point's, bit for bit.
 * mvg_adamw_step / mvg_adamw_step_dev are mvg_adam_step / mvg_adam_step_dev in that mode: the same arguments, checks, grid and -
 * for the device form - the same tick on the same state3 (lr_dev[0] is also the lr of f). */
int mvg_adamw_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, void *stream);
int mvg_adamw_step_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const float *lr_dev,
                       float *state3, float beta1, float beta2, float eps, float weight_decay, void *stream);
/* The two segmented steps with a MODE per segment: host_decoupled[i] (host memory, like the other per-segment arrays) is 0 for
 * the coupled update of mvg_adam_step_segments and 1 for the decoupled one; anything else is rejected.  The mode travels by
 * value in the kernel arguments, so one launch may hold coupled and decoupled segments side by side.  host_hyper is that of
 * mvg_adam_step_segments (stride 5) resp. mvg_adam_step_segments_dev (stride 4).  clip4_dev may be NULL: no clipping and no
 * guard (the bits of coef = 1); otherwise the record is read as mvg_adam_step_segments_clip / _dev_clip read it, and with
 * skipped != 0 nothing is updated and no row advances.  Every rule of those entry points holds here, checked before the first
 * launch (the tick included): a rejected call has advanced no row and updated nothing.  Elements outside every segment are
 * neither read nor written.  A coupled segment's result equals, bit for bit, that of mvg_adam_step_segments (_dev, _clip,
 * _dev_clip) on the same data; a decoupled segment's equals mvg_adamw_step (mvg_adamw_step_dev with a one-element lr_dev and
 * the same row) over that slice. */
int mvg_adam_step_segments_ex(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                              const int64_t *host_bounds, const float *host_hyper, const int32_t *host_steps,
                              const int32_t *host_decoupled, int n_segments, const float *clip4_dev, void *stream);
int mvg_adam_step_segments_dev_ex(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                                  const int64_t *host_bounds, const float *host_hyper, const int32_t *host_lr_index,
                                  const int32_t *host_decoupled, int n_segments, const float *lr_dev, int n_lr, float *state3_dev,
                                  const float *clip4_dev, void *stream);

/* ---------------------------------------------------------------- loss
 * gaze_angular_loss losses/gaze_loss.py:42-52 over pitchyaw_to_vector utils/math.py:52-60:
 * theta_i = acos(clamp(cos_sim(v(gt_i), v(pred_i), eps 1e-6), -1, 1)) * 180/pi;
 * loss[0] (+)= sum_i row_weight * theta_i ; dpred_i = row_weight * dtheta_i/dpred_i (optional).
 * (row_weight = 1/batch gives the reference's batch mean.)  theta_out optional [n]. */
int mvg_gaze_angular_loss(const float *pred, const float *gt, int n, float row_weight,
                          float *loss, int accumulate, float *dpred, float *theta_out, void *stream);

/* gaze_l1_loss / gaze_l2_loss losses/gaze_loss.py:56-64 (GazeLoss loss_type 'l1' / 'l2', :21-29; not used by
 * StereoL1Loss, which fixes 'angular'): loss[0] = mean over the n elements of |pred - label|^p, p in {1, 2};
 * dpred (optional, n floats) = d loss / d pred (zero where pred == label, like torch.abs). */
int mvg_gaze_lp_loss(const float *pred, const float *label, int n, int p, float *loss, float *dpred, void *stream);
/* IterationLoss(StereoL1Loss) (stereo_loss.py:46-54,65-84) over the head's stacked predictions in ONE launch: pred
 * [iters][dirs * batch][2], gt [dirs * batch][2]; host_weights [iters * dirs] (HOST array, copied into the launch): row r of
 * iteration i weighs host_weights[i * dirs + r / batch] / batch.  loss[0] = the weighted sum of the angular errors (degrees),
 * dpred (may be NULL) = its gradient. */
int mvg_gaze_angular_loss_multi(const float *pred, const float *gt, int iters, int dirs, int batch, const float *host_weights,
                                float *loss, float *dpred, void *stream);

/* Gaze error meter: the evaluation metric the trainer prints (trainer.py:128,187-192: np.mean(angular_error(pred, gt)), degrees)
 * accumulated on the DEVICE in double, with no copy to the host per batch.  preds fp32 [iters][dirs][batch][2] (the heads'
 * stacked (pitch, yaw) buffer, mvg_session_forward's preds), gt fp32 [dirs][batch][2] (row d = the labels of the view direction
 * d predicts for, the layout of mvg_gaze_angular_loss_multi's gt).  record = double [iters * dirs][MVG_GAZE_ERR_FIELDS], one
 * cell per (iteration, direction): COUNT, SUM, SUMSQ, MAX of the rows' errors and NONFINITE, the rows left out (counts are
 * doubles holding integers).  All zero is the empty record; reset is a stream-ordered memset of it (there is no entry point).
 * Per row, in double: utils/math.py:105-120 (angular_error_numpy) - both pairs to vectors with sin / cos, norms clipped at 1e-7,
 * similarity = dot / (na nb), acos, * 180 / pi - with ONE deviation: the similarity is clamped to [-1, 1] before acos (the
 * reference returns NaN where pred == gt rounds to 1 + 2e-16; here such a row is 0).  A row with a NaN or Inf in pred or gt
 * increments NONFINITE only.  err_out (may be NULL) fp32 [iters * dirs][capacity], the device form of pred_gaze_all /
 * gt_gaze_all (trainer.py:169-189): row b of this call goes to slot seen_before + b of its cell's row, seen_before = COUNT +
 * NONFINITE at kernel entry; a non-finite row stores NaN; slots >= capacity are not written while the counters still advance
 * (the reader sees COUNT + NONFINITE > capacity).  One launch, one workgroup of 256 threads per cell, fixed-order reduction, no
 * atomics: updates of one record are ordered by the stream, and equal updates leave equal bits.  Nothing is allocated and
 * nothing synchronises (capturable).  NULL preds / gt / record, iters / dirs / batch < 1, capacity < 0 and err_out with
 * capacity == 0 are rejected before any HIP call. */
enum { MVG_GAZE_ERR_COUNT = 0, MVG_GAZE_ERR_SUM = 1, MVG_GAZE_ERR_SUMSQ = 2, MVG_GAZE_ERR_MAX = 3, MVG_GAZE_ERR_NONFINITE = 4,
       MVG_GAZE_ERR_FIELDS = 5 };
int mvg_gaze_error_update(const float *preds, const float *gt, int iters, int dirs, int batch, double *record, float *err_out,
                          int64_t capacity, void *stream);

/* Multi-view consensus gaze: ONE estimate per sample from all D = views (views - 1) directed pair predictions, by the model's own
 * premise that views relate through the head-pose rotations (mvg_relative_rotation: rel = rot_i rot_j^T): rot[b][s]^T takes a
 * prediction made in view s's camera frame to the head frame, where predictions can be averaged.  preds fp32
 * [iters][D][batch][2] (pitch, yaw), the heads' stacked buffer: for pair p = (i < j) direction 2p predicts for view s = i with
 * partner q = j, direction 2p + 1 for s = j with q = i.  rot fp32 [batch][views][3][3].  weights fp32 [batch][views] or NULL
 * (all 1): a per-view confidence, 0 = the view is missing.  Per item (it, b), in double:
 *   w_d = weights[b][s(d)] * weights[b][q(d)];  contribution d is active iff w_d > 0.  Inactive contributions are SKIPPED, not
 *   multiplied by zero: a NaN in their preds row, or in the rot of a view that appears in no active contribution, reaches no sum.
 *   v_d = (cos p sin y, sin p, cos p cos y);   h = sum_active w_d rot[b][s(d)]^T v_d;   W = sum_active w_d;   e = h / |h|.
 *   head[it][b] = e.   For EVERY view t, whatever its weight: u = rot[b][t] e, views_out[it][t][b] = (asin(clamp(u.y, -1, 1)),
 *   atan2(u.x, u.z)); a non-finite rot[b][t] gives a NaN row for that t only.
 *   stats (may be NULL) [it][b] = (|h| / W, the resultant length in [0, 1];  sum_active w_d acos(clamp(e . rot^T v_d, -1, 1))
 *   180 / pi / W, the weighted mean disagreement in degrees).  head and views_out have the same bits with and without stats.
 * An item is degenerate - head, every views_out row and stats are NaN - when no contribution is active, a weight of the sample is
 * negative or non-finite, an active preds row or the rot of an active source view is non-finite, or |h| <= 1e-4 W (a
 * definition: below it the predictions cancel).  One thread per item, no LDS, no atomics: equal calls leave equal bits.  Nothing is
 * allocated and nothing synchronises (capturable).  A NULL preds / rot / head / views_out, views outside 2..8, iters or batch
 * < 1, iters * batch > INT32_MAX and a preds / views_out pointer that is not 8-byte aligned are rejected before any HIP call.
 * (Added under ABI v13: additive.) */
int mvg_gaze_consensus_fwd(const float *preds, const float *rot, const float *weights, int iters, int views, int batch, float *head,
                           float *views_out, float *stats, void *stream);
/* Its backward: dviews fp32 [iters][views][batch][2] -> dpreds fp32 [iters][D][batch][2]; every row is written (the caller clears
 * nothing).  With u = rot[b][t] e as above, the gradient on u is g_t = (dyaw u.z / r2, dpitch / sqrt(1 - u.y^2), -dyaw u.x / r2),
 * r2 = u.x^2 + u.z^2; a target whose forward row is NaN, or with r2 == 0 or u.y^2 >= 1, is left out.  g_e = sum_t rot[b][t]^T g_t,
 * g_h = (g_e - (g_e . e) e) / |h|, g_v = w_d rot[b][s(d)] g_h, dpitch_d = g_v . (-sin p sin y, cos p, -sin p cos y), dyaw_d = g_v .
 * (cos p cos y, 0, -cos p sin y).  Inactive rows and all rows of a degenerate item are exactly 0.  No gradient goes to rot or
 * weights.  Same checks (dviews, preds, rot, dpreds required; the three row buffers 8-byte aligned), same guarantees. */
int mvg_gaze_consensus_bwd(const float *dviews, const float *preds, const float *rot, const float *weights, int iters, int views,
                           int batch, float *dpreds, void *stream);

/* ---------------------------------------------------------------- stereo pair index (HOST)
 * GazeDataset.__init__'s idx_to_kv build, dataset/gaze.py:39-73, driven by CPython's
 * random.seed(int)/random.choice stream (MT19937 + getrandbits rejection).  Pure host integer
 * code; state (625 words: mt[624] + index) persists across calls like Python's global RNG.
 *   camera_tag: 0 = all, 1 = novel_train, 2 = novel_test.
 * Returns the number of tuples written (<= capacity) or -1 on error. */
int mvg_mt19937_seed(uint32_t *host_state /*[625]*/, uint64_t seed);
int64_t mvg_pair_index_build(uint32_t *host_state, const int64_t *host_file_rows, int n_files,
                             int camera_tag, int64_t *host_out /*[capacity][3]*/, int64_t capacity);


/* ---------------------------------------------------------------------------------------------
 * bf16 storage path (BASELINE.json configs[4]: "bf16 MFMA path").  Nothing in the reference
 * corresponds to it (the reference is fp32 everywhere: models/resnet.py:31-47, models/backbones/
 * blocks.py:41-47); these entry points are the same operators as above with activations, their
 * gradients and the conv weights held as bf16 (uint16_t storage) in HBM.  Matrix products run on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation; BatchNorm statistics, scale/shift, biases, weight
 * gradients and the loss stay fp32.  Channels (cin, cout) must be multiples of 8 (16-byte vectors);
 * the 3-channel stem input is padded to 8 by mvg_nchw_to_nhwc8_bf16.  The parity bar of this path is
 * declared in tests/test_bf16_gpu.py (it cannot meet the fp32 path's 1e-4).
 * --------------------------------------------------------------------------------------------- */
/* fp32 KRSC weights (cin_src <= d->cin channels per tap, the rest zero) -> bf16 KRSC `w_krsc`
 * [cout][r][s][d->cin] and, when w_crsk != NULL, the transposed copy [d->cin][r][s][cout] that
 * mvg_conv_dgrad_bf16 reads (one cast per weight per step: the master weights stay fp32). */
int mvg_cast_weights_bf16(const mvg_conv_desc *d, const float *w, int cin_src, void *w_krsc, void *w_crsk,
                          void *stream);
/* like mvg_conv_fprop / mvg_conv_stats_partials; x, wgt (KRSC), y are bf16, bias/stats fp32 */
int mvg_conv_fprop_bf16(const mvg_conv_desc *d, const void *x, const void *wgt, void *y, const float *bias,
                        int relu, float *stats, void *stream);
int mvg_conv_stats_partials_bf16(const mvg_conv_desc *d, int32_t *out_rows_per_partial);
/* Inference on the bf16 storage path (like mvg_conv_fprop_affine / mvg_conv_fprop_split_affine): BatchNorm on its running
 * statistics folded into the conv epilogue,
 *     out = bf16( [relu]( acc * scale[cout] + shift[cout] [+ residual] ) )
 * acc = the fp32 accumulator; scale / shift fp32 from mvg_bn_eval_affine (one row: every group uses the same); residual
 * (may be NULL) bf16, shaped like out; the ReLU follows the add; ONE rounding, at the store - no raw conv output, no
 * mvg_bn_apply_bf16 pass.  Same shapes and kernel choice as mvg_conv_fprop_bf16, in instantiations of their own (the
 * training kernels are unchanged).  With scale = 1, shift = 0, no residual, no ReLU the result equals
 * mvg_conv_fprop_bf16's as values. */
int mvg_conv_fprop_bf16_affine(const mvg_conv_desc *d, const void *x, const void *wgt, void *out, const float *scale,
                               const float *shift, const void *residual, int relu, void *stream);
/* like mvg_conv_dgrad; wgt_crsk = the transposed bf16 weights; mask/addend (bf16) like dx */
int mvg_conv_dgrad_bf16(const mvg_conv_desc *d, const void *dy, const void *wgt_crsk, void *dx,
                        const void *mask, const void *addend, void *stream);
/* mvg_conv_dgrad_bf16 fused with the BatchNorm-backward reduce pass of the unit whose output gradient dx is (the bf16
 * form of mvg_conv_dgrad_split_bnreduce below; resnet.py:113-133 backward): dx is stored masked by that unit's ReLU
 * (bn_bits from mvg_bn_apply_bits_bf16 - one byte per 8 channels -, or fma(bn_y, relu_scale, relu_shift) > 0, or no mask)
 * and s1 / s2 / dgamma / dbeta - sums of the ROUNDED gradient, what mvg_bn_bwd_reduce_bf16 would read back - come
 * out of the same launch + a finalize.  Stride 1 or 2; cin, cout multiples of 64; bn_y bf16 shaped like dx.
 * partials: groups * mvg_conv_dgrad_bn_partials_bf16(d) * 2 * cin floats. */
int mvg_conv_dgrad_bn_partials_bf16(const mvg_conv_desc *d);
int mvg_conv_dgrad_bf16_bnreduce(const mvg_conv_desc *d, const void *dy, const void *wgt_crsk, void *dx, const void *addend,
                                 const void *bn_y, const uint8_t *bn_bits, const float *bn_mean, const float *bn_invstd,
                                 const float *relu_scale, const float *relu_shift, float *partials, float *s1, float *s2,
                                 float *dgamma, float *dbeta, int accumulate, void *stream);
/* The 7x7 stride-2 stem (resnet.py:184) on the LDS-DMA bf16 kernels as FOLDED row windows: xw [images][h][w/4][16][4]
 * bf16 - window m holds image columns 4 m - 4 .. 4 m + 11 x (R, G, B, 0), zero outside the image, made straight from
 * the NCHW fp32 input - serves output columns 2 m and 2 m + 1 as 2 * cout GEMM columns, so the kernel's output
 * [.., wo/2, 2 cout] is y [.., wo, cout] in memory.  d = the stem's descriptor (r = s = 7, stride 2, pad 3; w % 4 == 0;
 * n * ho * wo / 2 a multiple of 64).  w_fold: bf16 [2 cout][7][16][4] with w_fold[par * cout + o][r][j][c] =
 * w[o][r][j - 1 - 2 par][c] (zero elsewhere).  stats: BatchNorm partials of y, groups * 2 P * 2 * cout floats with
 * P = mvg_conv_stats_partials_bf16 of a descriptor with n, ho, wo / 2 (64 outputs per partial, like every bf16 forward).
 * mvg_stem_wgrad_bf16: dw_fold fp32 in the same layout (the caller adds the two parities' taps);
 * workspace = splits * 2 cout * 448 floats, splits = mvg_stem_wgrad_splits_bf16(d). */
int mvg_stem_rowwindow_bf16(const float *x_nchw, void *xw, int64_t images, int h, int w, void *stream);
int mvg_stem_fprop_bf16(const mvg_conv_desc *d, const void *xw, const void *w_fold, void *y, float *stats, void *stream);
int mvg_stem_wgrad_splits_bf16(const mvg_conv_desc *d);
int mvg_stem_wgrad_bf16(const mvg_conv_desc *d, const void *xw, const void *dy, float *dw_fold, float *workspace, int splits,
                        int accumulate, void *stream);
/* like mvg_conv_wgrad / mvg_conv_wgrad_splits; x, dy bf16, dw (and the slabs in workspace) fp32 */
int mvg_conv_wgrad_bf16(const mvg_conv_desc *d, const void *x, const void *dy, float *dw, float *workspace,
                        int splits, int accumulate, void *stream);
int mvg_conv_wgrad_splits_bf16(const mvg_conv_desc *d);
/* the launch without its slab reduce (splits > 1), for mvg_wgrad_reduce_batch - see mvg_conv_wgrad_split_slabs */
int mvg_conv_wgrad_bf16_slabs(const mvg_conv_desc *d, const void *x, const void *dy, float *workspace, int splits, void *stream);
/* Host-only plan queries of the bf16 kernels (like mvg_conv_plan_query / mvg_conv_wgrad_tile: tests guard with them which
 * form a shape runs): answered by the code the launches plan with; nothing is launched and no device is needed.  -1 (and
 * a message) for a descriptor or kind the launch would reject.
 * mvg_conv_plan_query_bf16: `kind` names the launch - MVG_PLAN_BF16_FPROP (mvg_conv_fprop_bf16), MVG_PLAN_BF16_DGRAD
 * (mvg_conv_dgrad_bf16), MVG_PLAN_BF16_DGRAD_BNREDUCE (mvg_conv_dgrad_bf16_bnreduce: classes without taps stay in the
 * launch, with 0 K-steps), MVG_PLAN_BF16_AFFINE (mvg_conv_fprop_bf16_affine), MVG_PLAN_BF16_LINEAR_FPROP_MIXED /
 * MVG_PLAN_BF16_LINEAR_DGRAD_MIXED (mvg_linear_fprop_mixed / mvg_linear_dgrad_mixed with the descriptor {1, rows, 1, 1, fin,
 * fout, 1, 1, 1, 0, 1, 1}); the stem's folded forms are not covered.  The plan: bm = 128, bk = 64, bn = 128 or 64, fasta
 * (the uniform-tap loader), ncls / cls_tiles / cls_kt as in mvg_conv_plan_query, streamk_grid = 0, splitk = 1,
 * scratch_floats = 0.  The kernel follows: the LDS-DMA kernel iff fasta and the kind is not a mixed one (those run the
 * register-staged kernel with fp32 operands, fasta choosing its loader); otherwise the register-staged kernel.  out may be NULL.
 * mvg_conv_wgrad_tile_bf16: the tile (bm rows of cout x bn columns of r*s*cin) mvg_conv_wgrad_bf16 (f32in = 0) or
 * mvg_linear_wgrad_mixed (f32in != 0) runs `d` on, and whether its loader steps the pixel coordinates incrementally (never
 * with fp32 operands); every out-pointer may be NULL. */
enum { MVG_PLAN_BF16_FPROP = 0, MVG_PLAN_BF16_DGRAD = 1, MVG_PLAN_BF16_DGRAD_BNREDUCE = 2, MVG_PLAN_BF16_AFFINE = 3,
       MVG_PLAN_BF16_LINEAR_FPROP_MIXED = 4, MVG_PLAN_BF16_LINEAR_DGRAD_MIXED = 5 };
int mvg_conv_plan_query_bf16(const mvg_conv_desc *d, int kind, mvg_conv_plan *out);
int mvg_conv_wgrad_tile_bf16(const mvg_conv_desc *d, int f32in, int32_t *bm, int32_t *bn, int32_t *incremental);
/* The stem's folded forms (d = the stem's own descriptor, as mvg_stem_fprop_bf16 takes it): *fwd = the forward's plan of the
 * folded descriptor (2 cout GEMM columns, K-steps of 64 over 7 taps) and the weight gradient's tile over (2 cout) x 448 with its
 * pixel addressing (incremental when ho * wo / 2 >= 128).  Every out-pointer may be NULL; launches nothing; 0, or -1 (and a message)
 * for a descriptor the stem launches reject. */
int mvg_stem_plan_query_bf16(const mvg_conv_desc *d, mvg_conv_plan *fwd, int32_t *wgrad_bm, int32_t *wgrad_bn, int32_t *wgrad_incremental);
/* nn.Linear of the fusion block in the bf16 path ("mixed"): activations, gradients, biases and outputs stay
 * fp32 in memory, the operand loaders round to bf16 on the way into LDS and the product runs on the bf16
 * matrix cores against the bf16 weight copies (w_bf16 [fout][fin]; wt_bf16 [fin][fout] for backward-data).
 * No split-K: meant for the large row counts of the bf16 configuration (C5: 3584 rows per GPU).
 *   fprop: y = [relu](x @ w^T + bias);  dgrad: dx = (dy @ w) * (mask > 0) + addend;
 *   wgrad: dw (+)= dy^T x, db (+)= column sums of the fp32 dy; splits = mvg_conv_wgrad_splits_bf16(linear
 *   descriptor), workspace splits * (fout*fin + fout) floats when splits > 1. */
int mvg_linear_fprop_mixed(const float *x, const void *w_bf16, const float *bias, int relu, float *y, int rows, int fin,
                           int fout, void *stream);
int mvg_linear_dgrad_mixed(const float *dy, const void *wt_bf16, const float *mask, const float *addend, float *dx,
                           int rows, int fin, int fout, void *stream);
int mvg_linear_wgrad_mixed(const float *x, const float *dy, float *dw, float *db, int rows, int fin, int fout,
                           float *workspace, int splits, int accumulate, void *stream);
/* the BatchNorm / pooling passes with bf16 activations (same arguments as the fp32 entry points) */
int mvg_bn_apply_bf16(const uint16_t *y, const float *scale, const float *shift, const uint16_t *residual,
                      const float *res_scale, const float *res_shift, int relu, uint16_t *out, int groups,
                      int64_t rows_per_group, int c, void *stream);
int mvg_bn_bwd_reduce_bf16(const uint16_t *g, const uint16_t *act, const uint16_t *y, const float *mean,
                           const float *invstd, const float *relu_scale, const float *relu_shift, int groups,
                           int64_t rows_per_group, int c, float *s1, float *s2, float *dgamma, float *dbeta,
                           int accumulate, float *workspace, uint16_t *dz_out, void *stream);
int mvg_bn_bwd_apply_bf16(const uint16_t *g, const uint16_t *act, const uint16_t *y, const float *mean,
                          const float *invstd, const float *gamma, const float *s1, const float *s2,
                          const float *relu_scale, const float *relu_shift, int groups, int64_t rows_per_group,
                          int c, uint16_t *dy, uint16_t *dz_out, void *stream);
int mvg_bn_relu_maxpool_fwd_bf16(const uint16_t *y, const float *scale, const float *shift, uint16_t *pooled,
                                 uint8_t *argmax, int groups, int n_per_group, int h, int w, int c, int ho,
                                 int wo, void *stream);
int mvg_bn_relu_maxpool_bwd_reduce_bf16(const uint16_t *g_pooled, const uint8_t *argmax, const uint16_t *y,
                                        const float *mean, const float *invstd, const float *scale,
                                        const float *shift, int groups, int n_per_group, int h, int w, int c,
                                        int ho, int wo, float *s1, float *s2, float *dgamma, float *dbeta,
                                        int accumulate, float *workspace, void *stream);
int mvg_bn_relu_maxpool_bwd_apply_bf16(const uint16_t *g_pooled, const uint8_t *argmax, const uint16_t *y,
                                       const float *mean, const float *invstd, const float *gamma,
                                       const float *scale, const float *shift, const float *s1,
                                       const float *s2, int groups, int n_per_group, int h, int w, int c,
                                       int ho, int wo, uint16_t *dy, void *stream);
/* mvg_bn_eval_bwd / mvg_bn_relu_maxpool_eval_bwd with bf16 g, act, y, dy, dz_out (g_pooled, y, dy): a training step that
 * keeps BatchNorm on its running statistics (frozen BatchNorm) on the bf16 path.  Same contracts: one mask source at most,
 * dy and dz_out may alias g but not each other, NULL dgamma and dbeta skip the finalize launch; the same workspace.  The
 * arithmetic is the fp32 entry points' on the widened values, every stored value rounded to bf16 once.  relu_bits: one
 * byte per 8 elements (mvg_bn_apply_bits_bf16's layout).  Sizes: mvg_bn_bwd_reduce_bf16's (c/8 divides 256 or exceeds it);
 * the stem tail moves 4 channels per lane in both storage types (c/4 divides 256). */
int mvg_bn_eval_bwd_bf16(const uint16_t *g, const uint16_t *act, const uint8_t *relu_bits, const uint16_t *y,
                         const float *relu_scale, const float *relu_shift, const float *gamma, const float *running_mean,
                         const float *running_var, float eps, int groups, int64_t rows_per_group, int c, uint16_t *dy,
                         uint16_t *dz_out, float *dgamma, float *dbeta, int accumulate, float *workspace, void *stream);
int mvg_bn_relu_maxpool_eval_bwd_bf16(const uint16_t *g_pooled, const uint8_t *argmax, const uint16_t *y, const float *scale,
                                      const float *shift, const float *gamma, const float *running_mean,
                                      const float *running_var, float eps, int groups, int n_per_group, int h, int w,
                                      int c, int ho, int wo, uint16_t *dy, float *dgamma, float *dbeta, int accumulate,
                                      float *workspace, void *stream);
/* bf16 feature map -> fp32 pooled features and back (the fusion block stays fp32) */
int mvg_avgpool_fwd_bf16(const uint16_t *x, float *y, int n, int hw, int c, void *stream);
int mvg_avgpool_bwd_bf16(const float *dy, uint16_t *dx, int n, int hw, int c, void *stream);
/* fp32 NCHW images (rot_mv.py:188-189) -> bf16 NHWC with the channels zero-padded to 8 */
int mvg_nchw_to_nhwc8_bf16(const float *src, uint16_t *dst, int n, int c, int h, int w, void *stream);
/* mvg_preprocess_u8hwc_resize (h == oh && w == ow: mvg_preprocess_u8hwc) straight to the bf16 stem's input: the same
 * arithmetic (one device function serves both), the result rounded once to bf16 and stored NHWC8, dst [n][oh][ow][8] with
 * channels 3..7 zero - bit for bit what mvg_nchw_to_nhwc8_bf16 makes of the fp32 kernel's output.  One launch per view. */
int mvg_preprocess_u8hwc_resize_bf16(const uint8_t *src, uint16_t *dst, int n, int h, int w, int oh, int ow, float mean0,
                                     float mean1, float mean2, float std0, float std1, float std2, int swap_rb,
                                     void *stream);

/* ---- "split" operands: fp32-accurate convolutions on the fp16 matrix cores (csrc/conv_split.hip) ----------------
 * An fp32 tensor in "sp" format holds every value v - times a per-tensor power-of-two scale 2^k chosen by its producer -
 * as TWO fp16 pieces, h1 = fp16(v 2^k), h2 = fp16(v 2^k - h1): |v - (h1 + h2) 2^-k| <= 2^-23 |v| (at most the last of the
 * 24 significand bits is lost; three values in four are exact).  Channels go in chunks of 8 with the two pieces of a chunk adjacent (4 bytes per element).
 * Three fp16 MFMAs per 32 k (h1 g1 + h1 g2 + h2 g1, fp32 accumulation) reproduce the fp32 product to fp32-accumulation
 * accuracy (conv_split.hip header; tests/test_split_gpu.py holds every kernel to 2e-6 against fp64 and to the
 * fp32-MFMA kernel's own error), so these entries serve the same 1e-4 parity path as mvg_conv_fprop / _dgrad / _wgrad
 * (resnet.py:31-47: F.conv2d forward and its autograd backward) - outputs (y, dx, dw) are plain fp32.
 * Scales travel as DEVICE scalars "sinv" = 2^-k next to their tensor (NULL = 1): activations are stored unscaled,
 * gradients dy get theirs from mvg_bn_bwd_apply_split, weight copies from the weight prep; a consumer multiplies its
 * accumulators by the sinv of both operands.  Shapes: cin, cout multiples of 32, r*s <= 32 (everything in the
 * backbone but the 3-channel stem). */
int mvg_split_f32(const float *x, void *out_sp, int64_t n, float scale, void *stream);        /* n % 8 == 0; out = sp(x * scale) */
int mvg_merge_sp(const void *x_sp, float *out, int64_t n, float inv_scale, void *stream);     /* out = (h1 + h2) * inv_scale */
/* fp32 KRSC weights -> sp KRSC (fprop) and, when w_crsk_sp != NULL, the sp transposed copy CRSK (dgrad), both scaled by the
 * 2^k that puts max |w| just below 2^15.  stat2: two device floats, receive {max |w| (bits), 2^-k}: pass stat2 + 1 as the
 * w_sinv of the consumers.  items_dev: 64 bytes of device memory (staging of the one-record table). */
int mvg_split_weights(const mvg_conv_desc *d, const float *w, void *w_krsc_sp, void *w_crsk_sp, float *stat2, void *items_dev,
                      void *stream);
/* All weight copies of a training step in two launches (max |w| per conv, then the copies).  items_dev: n records in
 * DEVICE memory of
 *   { const float *w (fp32 KRSC); void *wk; void *wt (NULL: no transposed copy); int32 cout, rs, cin, cin_pad;
 *     float *stat (mode 1: two device floats per conv, stat[0] CLEARED by the caller, receive {max |w| bits, 2^-k}); }  (48 bytes)
 * mode 1: wk / wt = the sp KRSC / CRSK copies of mvg_split_weights (cin_pad unused); mode 0: the bf16 KRSC (cin
 * zero-padded to cin_pad) / CRSK copies of mvg_cast_weights_bf16 (stat unused). */
int mvg_weights_prep_batch(const void *items_dev, int n, int mode, int blocks_per_item /* 0: 64 */, void *stream);
/* partial-statistics geometry of mvg_conv_fprop_split (like mvg_conv_stats_partials) */
int mvg_conv_stats_partials_split(const mvg_conv_desc *d, int32_t *rows_per_partial);
int mvg_conv_fprop_split(const mvg_conv_desc *d, const void *x_sp, const float *x_sinv, const void *w_sp, const float *w_sinv,
                         float *y, float *stats, void *stream);
/* inference forward with BatchNorm folded into the epilogue (like mvg_conv_fprop_affine): out = relu?(conv * scale +
 * shift (+ residual)); residual fp32 or sp (residual_sp; unscaled), the result fp32 or sp (out_sp; unscaled) - in sp the
 * next conv reads it directly (resnet.py:60-75,113-133 in eval mode) */
int mvg_conv_fprop_split_affine(const mvg_conv_desc *d, const void *x_sp, const float *x_sinv, const void *w_sp, const float *w_sinv,
                                void *out, int out_sp, const float *scale, const float *shift, const void *residual,
                                int residual_sp, int relu, void *stream);
/* The guarded inference forward (see "Inference on the split kernels" below): the launch above with an sp output
 * (out_sp != 0 is required) plus the activation RANGE RECORD of what it stores.  *range_word (required; device memory;
 * cleared by the caller before the forward) receives, by an unsigned-integer atomic max, the largest bit pattern of |v|
 * over the stored elements, v being the fp32 value handed to the fp16 split - after scale, shift, residual and ReLU.  The
 * integer order is the float order for non-negative floats and ranks inf / NaN above every finite value.  The tensor has
 * overflowed iff the word is >= 0x477FF000 (|v| >= 65520.0f: where fp16 round-to-nearest-even gives inf).  Rows and columns
 * beyond the map's edge take no part.  Same tiles, launch plan and output bits as mvg_conv_fprop_split_affine.
 * mvg_split_f32_ranged: mvg_split_f32 plus the same record (the stem's pooled map). */
int mvg_conv_fprop_split_affine_ranged(const mvg_conv_desc *d, const void *x_sp, const float *x_sinv, const void *w_sp,
                                       const float *w_sinv, void *out, int out_sp, const float *scale, const float *shift,
                                       const void *residual, int residual_sp, int relu, uint32_t *range_word, void *stream);
int mvg_split_f32_ranged(const float *x, void *out_sp, int64_t n, float scale, uint32_t *range_word, void *stream);
/* relu_mask_sp (may be NULL; stride-1 launches): an sp tensor shaped like dx - dx is zeroed where it is <= 0 (the ReLU of a
 * Linear's hidden layer, whose activation the forward wrote in sp) */
int mvg_conv_dgrad_split(const mvg_conv_desc *d, const void *dy_sp, const float *dy_sinv, const void *w_crsk_sp,
                         const float *w_sinv, float *dx, const float *addend, const void *relu_mask_sp, void *stream);
/* The BatchNorm passes on the split path: the conv output y and every gradient g stay fp32; what the next conv
 * reads is written in sp - the normalised activation (mvg_bn_apply_split, residual = the previous block's sp output
 * when residual_sp != 0, else the raw fp32 downsample output with its res_scale / res_shift), the stem's pooled map
 * (mvg_bn_relu_maxpool_fwd_split) and dy (mvg_bn_bwd_apply_split: g already masked, or the mask from relu_scale /
 * relu_shift).  relu_bits as in mvg_bn_apply_bits (1 byte per 4 channels).  mvg_avgpool_fwd_split pools an sp map.
 * dy is stored times 2^k, k from the bound  max over (group, channel) of |gamma invstd| (mx + |s1|/n + sqrt(n) |s2|/n) >= |dy|,
 * mx [groups][c] = max |masked gradient| per (group, channel), left by mvg_bn_bwd_reduce_split or
 * mvg_conv_dgrad_split_bnreduce; *dy_sinv receives 2^-k for mvg_conv_dgrad_split / _wgrad_split.  The reduce entries
 * (mvg_bn_bwd_reduce_split, mvg_conv_dgrad_split_bnreduce, mvg_bn_relu_maxpool_bwd_reduce_split) take the unit's gamma and
 * dy_sinv (both NULL, or both given): their finalize then leaves *dy_sinv itself - bn_bwd_finalize_kernel (partials -> s1 / s2 /
 * mx), then the single-workgroup bn_bwd_dgamma_dyscale_kernel (dgamma / dbeta and the bound's 2^-k) in place of the plain
 * dgamma / dbeta launch - and the apply entry is told so (dy_sinv_ready != 0). */
int mvg_bn_apply_split(const float *y, const float *scale, const float *shift, const void *residual, int residual_sp,
                       const float *res_scale, const float *res_shift, int relu, void *out_sp, uint8_t *relu_bits,
                       int groups, int64_t rows_per_group, int c, void *stream);
int mvg_bn_bwd_reduce_split(const float *g, const uint8_t *relu_bits, const float *y, const float *mean, const float *invstd,
                            const float *relu_scale, const float *relu_shift, int groups, int64_t rows_per_group, int c,
                            float *s1, float *s2, float *dgamma, float *dbeta, int accumulate, float *workspace,
                            float *dz_out, float *mx, const float *gamma, float *dy_sinv, void *stream);
int mvg_bn_bwd_apply_split(const float *g, const float *y, const float *mean, const float *invstd, const float *gamma,
                           const float *s1, const float *s2, const float *relu_scale, const float *relu_shift,
                           int groups, int64_t rows_per_group, int c, void *dy_sp, const float *mx, float *dy_sinv,
                           int dy_sinv_ready, void *stream);
int mvg_bn_relu_maxpool_fwd_split(const float *y, const float *scale, const float *shift, void *pooled_sp,
                                  uint8_t *argmax, int groups, int n_per_group, int h, int w, int c, int ho, int wo,
                                  void *stream);
int mvg_avgpool_fwd_split(const void *x_sp, float *y, int n, int hw, int c, void *stream);
/* Backbone activations of a TRAINING step carry a per-tensor power-of-two scale too (the reference - resnet.py:60-75,
 * 113-133,261-275 - computes them in plain fp32 and has no range limit; fp16 pieces overflow at 65 520 and lose small
 * values absolutely).  The scale comes from a bound that needs no pass over any activation: a unit writes
 * [relu](gamma xhat + beta [+ identity]) with xhat a z-score of n = B Ho Wo samples per view, |xhat| <= sqrt(n - 1), so
 *   bound(unit) = max_c (|gamma_c| sqrt(n - 1) + |beta_c|),  bound(block output) = bound(last unit) + bound(identity),
 * identity = the previous block's output (first block: the stem's pooled map, bound(stem unit)) or the downsample
 * BatchNorm's output.  2^k = 1 while 1 <= bound < 2^15 (every value fits unscaled: the stored bits are those of an
 * unscaled tensor), else the power of two that maps the bound just below 2^15; a zero, infinite or NaN bound gives 1.
 *   mvg_act_scales: ONE single-workgroup launch for a whole step.  items_dev: n <= 256 records in DEVICE memory of
 *     { const float *gamma, *beta; int32 c; float sqrt(n - 1); int32 ident; int32 slot; }  (32 bytes) in forward order;
 *     ident = an EARLIER record whose (chained) bound is added, or -1; slots[slot] receives 2^-k (slot -1: none).
 *   The _scaled / _xs entry points are the ones above with those device scalars (NULL = unscaled: the results of the old
 *   entry point, bit for bit; the new ones also reject null required pointers and non-positive sizes, the old ones keep
 *   exactly the argument checks they had): out_sinv / pooled_sinv of the tensor written, res_sinv of an sp identity, x_sinv of the tensor read
 *   (the conv forward takes it as mvg_conv_fprop_split's x_sinv).  The ReLU mask bits are decided on the unscaled value.
 *   Readers that use an sp activation only for its SIGN (relu_mask_sp, the backward's mask forms) need no scale.
 * Inference on the split kernels (mvg_conv_fprop_split_affine) has no z-score bound - running statistics give none, and a
 * bound chained from the input grows by every layer's L1 gain - and stays unscaled: an activation that reaches 65 520 is
 * stored as inf and merges to NaN, which a later ReLU can turn into 0.  The caller who cannot vouch for the checkpoint
 * runs the guarded forward instead: mvg_conv_fprop_split_affine_ranged / mvg_split_f32_ranged leave one range word per sp
 * tensor (same launches, same output bits), and a word >= 0x477FF000 says that tensor overflowed - rerun on the fp32-MFMA
 * kernels (mvg_conv_fprop_affine; Backbone.split_eval_guard = "fallback" does that, mvg_session_set_range_record reports). */
int mvg_act_scales(const void *items_dev, int n, float *slots, int n_slots, void *stream);
int mvg_bn_apply_split_scaled(const float *y, const float *scale, const float *shift, const void *residual, int residual_sp,
                              const float *res_scale, const float *res_shift, const float *res_sinv, int relu, void *out_sp,
                              const float *out_sinv, uint8_t *relu_bits, int groups, int64_t rows_per_group, int c,
                              void *stream);
int mvg_bn_relu_maxpool_fwd_split_scaled(const float *y, const float *scale, const float *shift, void *pooled_sp,
                                         const float *pooled_sinv, uint8_t *argmax, int groups, int n_per_group, int h, int w,
                                         int c, int ho, int wo, void *stream);
int mvg_avgpool_fwd_split_scaled(const void *x_sp, const float *x_sinv, float *y, int n, int hw, int c, void *stream);
/* Frozen-BatchNorm training steps on the split kernels (Backbone.split_frozen; added under ABI v13: additive).  A unit on the
 * running statistics has no z-score bound, so its activation scale comes from the conv launch's own statistics partials
 * (mvg_conv_fprop_split / mvg_stem_fprop_split: `stats`, the layout mvg_bn_finalize reads) - no pass over an activation.  With
 * mean_b, var_b (biased) of the n = rows_per_group conv outputs of a (group, channel), every element obeys
 * |y - mean_b| <= sqrt((n - 1) var_b), hence
 *   |gamma invstd_r (y - rm) + beta| <= |gamma| invstd_r (|mean_b - rm| + sqrt((n - 1) var_b)) + |beta|,
 *   bound(unit) = max over (group, channel) of that,  bound(block output) = bound(last unit) + bound(identity).
 * mvg_bn_frozen_finalize, ONE launch per unit in place of mvg_bn_eval_affine:
 *   scale, shift [groups][c]   the bits mvg_bn_eval_affine writes;
 *   mean, invstd [groups][c]   running_mean and 1 / sqrt(running_var + eps), broadcast over the groups: what the reduce entry
 *                              points of the backward (mvg_conv_dgrad_split_bnreduce, mvg_bn_bwd_reduce_split, the stem's) read;
 *   state                      4 device floats of the unit, state[0] and state[1] ZERO on entry (an integer maximum and an
 *                              arrival count: the last workgroup to arrive finishes the unit); state[2] receives the chained
 *                              bound = bound(unit) (+ *ident_bound, the state[2] of an EARLIER unit, or NULL);
 *   slot (may be NULL)         receives 2^-k by mvg_act_scales' rule: 1 while 1 <= bound < 2^15, else the power of two that
 *                              maps the bound just below 2^15; a zero, infinite or NaN bound gives 1.
 * Rounding may only enlarge the bound: the partials are merged in float64 (mvg_bn_finalize's pivoted Chan merge), the
 * expression is evaluated in float64, and a final factor 1 + 2^-7 (ops.FROZEN_BOUND_MARGIN) covers the fp32 rounding of the
 * partials themselves and of the chained sum.  The 2^15 target leaves another factor of two below 65 520.  The running
 * statistics are read, never written.
 * mvg_bn_frozen_bwd_apply_split: the backward apply pass of such a unit, dy = sp(gamma_c invstd_c dz 2^k) in one pass - no batch
 * sums.  g already masked, or the mask from fma(y, relu_scale, relu_shift) > 0 (y is read in this form only), or no ReLU
 * (both NULL).  invstd [groups][c] as mvg_bn_frozen_finalize left it; *dy_sinv = 2^-k as the reduce entry points leave it from
 * |gamma invstd| (mx + |s1|/n + sqrt(n) |s2|/n), which only adds non-negative terms to |gamma invstd| mx >= |dy|: the
 * train-mode bound holds for the frozen dy and is kept.  c % 8 == 0. */
int mvg_bn_frozen_finalize(const float *stats, int groups, int partials, int rows_per_partial, int64_t rows_per_group, int c,
                           const float *gamma, const float *beta, const float *running_mean, const float *running_var, float eps,
                           const float *ident_bound, float *mean, float *invstd, float *scale, float *shift, float *state,
                           float *slot, void *stream);
int mvg_bn_frozen_bwd_apply_split(const float *g, const float *y, const float *invstd, const float *gamma, const float *relu_scale,
                                  const float *relu_shift, int groups, int64_t rows_per_group, int c, void *dy_sp,
                                  const float *dy_sinv, void *stream);
/* mvg_conv_dgrad_split fused with the BatchNorm-backward reduce pass of the unit whose output gradient dx is (stride 1
 * or 2: a stride-2 launch's parity classes - those a 1x1 filter never touches included - each bring their partials): dx is stored masked by that unit's ReLU (bn_bits from mvg_bn_apply_split, or fma(bn_y, relu_scale,
 * relu_shift) > 0, or no mask) and s1 / s2 / dgamma / dbeta come out of the same launch + a finalize; mx [groups][cin] (may be
 * NULL) receives max |dx| per (group, channel).  partials: groups * mvg_conv_dgrad_bn_partials_split(d) * 3 * cin floats. */
int mvg_conv_dgrad_bn_partials_split(const mvg_conv_desc *d);
int mvg_conv_dgrad_split_bnreduce(const mvg_conv_desc *d, const void *dy_sp, const float *dy_sinv, const void *w_crsk_sp,
                                  const float *w_sinv, float *dx, const float *addend, const float *bn_y, const uint8_t *bn_bits,
                                  const float *bn_mean, const float *bn_invstd, const float *relu_scale, const float *relu_shift,
                                  float *partials, float *s1, float *s2, float *dgamma, float *dbeta, int accumulate,
                                  float *mx, const float *bn_gamma, float *dx_dy_sinv, void *stream);
/* mvg_bn_bwd_apply_split (g already masked, dy_sinv ready) and mvg_conv_dgrad_split_bnreduce of the same unit in ONE launch, for a
 * 1x1 / stride 1 / pad 0 unit with cin = 64 or 128 (one column tile of backward-data: every dy element is consumed by exactly one
 * workgroup) and cout % 32 == 0, cout <= 512: the loader forms dy = BatchNorm backward of (dz, y) with the unit's mean / invstd
 * [groups][cout], gamma [cout] and sums un_s1 / un_s2 [groups][cout] over rows_per_group = n * ho * wo rows, times 2^k = 1 / *dy_sinv,
 * multiplies it and WRITES it to dy_sp (an output here: the weight gradient reads it afterwards).  Everything from w_crsk_sp on is
 * mvg_conv_dgrad_split_bnreduce's.  dy_sp, dx, the sums and mx hold the bits the two calls leave. */
int mvg_conv_dgrad_split_bnapply_bnreduce(const mvg_conv_desc *d, void *dy_sp, const float *dy_sinv, const float *dz, const float *y,
                                          const float *mean, const float *invstd, const float *gamma, const float *un_s1,
                                          const float *un_s2, int64_t rows_per_group, const void *w_crsk_sp, const float *w_sinv,
                                          float *dx, const float *addend, const float *bn_y, const uint8_t *bn_bits,
                                          const float *bn_mean, const float *bn_invstd, const float *relu_scale,
                                          const float *relu_shift, float *partials, float *s1, float *s2, float *dgamma, float *dbeta,
                                          int accumulate, float *mx, const float *bn_gamma, float *dx_dy_sinv, void *stream);
/* mvg_bn_apply_split_scaled (residual + ReLU) of the unit that PRODUCES a conv's input and mvg_conv_fprop_split of that conv in ONE
 * launch, for a 1x1 / stride 1 / pad 0 conv with cout = 64 or 128 (one column tile of the forward GEMM: every input element is
 * consumed by exactly one workgroup) and cin % 32 == 0, cin <= 512 - a residual block's first conv after a bottleneck: the loader
 * forms relu(bn_y * scale + shift + residual) with the producer's scale / shift [groups][cin]; the residual [groups][n][h][w][cin] is
 * an sp identity (residual_sp = 1; read times *res_sinv, NULL = 1) or the raw fp32 downsample output with res_scale / res_shift
 * [groups][cin]; multiplies it and WRITES it times 1 / *out_sinv to out_sp (an output here: later readers find it as the apply pass
 * leaves it), and the ReLU mask to relu_bits (may be NULL).  Everything from w_sp on is mvg_conv_fprop_split's.  out_sp, relu_bits,
 * y and stats hold the bits the two calls leave.  The launch runs the single-stage K loop: mvg_conv_fprop_split_stages tells which
 * form mvg_conv_fprop_split picks for a descriptor on this device (1 = single-stage, 2 = two-stage pipeline, -1 = bad descriptor).
 * mvg_conv_dgrad_split_stages answers the same for mvg_conv_dgrad_split (fused_reduce = 0) and mvg_conv_dgrad_split_bnreduce
 * (fused_reduce != 0: the launch keeps the stride-2 parity classes without taps, so it has more tiles).  Both are host arithmetic
 * by the launch's own plan - device CUs minus mvg_set_reserved_cus - and launch nothing: a test asserts with them which kernel
 * form a shape ran. */
int mvg_conv_fprop_split_stages(const mvg_conv_desc *d);
int mvg_conv_dgrad_split_stages(const mvg_conv_desc *d, int fused_reduce);
int mvg_conv_fprop_split_bnapply(const mvg_conv_desc *d, void *out_sp, const float *out_sinv, const float *bn_y, const float *scale,
                                 const float *shift, const void *residual, int residual_sp, const float *res_scale,
                                 const float *res_shift, const float *res_sinv, uint8_t *relu_bits, const void *w_sp,
                                 const float *w_sinv, float *y, float *stats, void *stream);
/* The 7x7 stride-2 stem (resnet.py:184, ResNet.forward :262) on the split kernels, "row-window" form: the 3-channel image
 * (stored NHWC with 4 channels) is rewritten as xw [images][h][w/2][8][4] in sp - window ox holds image columns 2 ox - 4 ..
 * 2 ox + 3, zero outside the image - and the stem becomes a 7 x 1 filter over 32 "channels" (vertical stride 2 / pad 3,
 * horizontal stride 1 / pad 0): K = 224.  d = the stem's own descriptor (r = s = 7, stride 2, pad 3, cin = 4, even w).
 *   mvg_stem_rowwindow_split: x_nhwc4 fp32 -> xw_sp (32 * images * h * w/2 sp elements);
 *   w_sp: the sp copy (mvg_split_weights on a [cout][7][1][32] descriptor) of w'[o][r][j][c] = w[o][r][j - 1][c], zero for
 *         j = 0 and c = 3;   mvg_stem_fprop_split: y fp32 [groups][n][ho][wo][cout] + BatchNorm partials like
 *         mvg_conv_fprop_split (mvg_conv_stats_partials_split of a descriptor with the same n, ho, wo);
 *   mvg_stem_wgrad_split: dw_rw [cout][7][8][4] fp32 in the same tap layout (the caller drops j = 0 and c = 3);
 *         workspace = splits * cout * 224 floats, splits = mvg_stem_wgrad_splits_split(d).
 * The stem tail's backward with dy in sp: mvg_bn_relu_maxpool_bwd_reduce_split also leaves mx [groups][c], a bound on a
 * pixel's gradient (4 x the largest masked window gradient); mvg_bn_relu_maxpool_bwd_apply_split scales dy by the 2^k that
 * bound allows and writes 2^-k to *dy_sinv. */
int mvg_stem_rowwindow_split(const float *x_nhwc4, void *xw_sp, int64_t images, int h, int w, void *stream);
int mvg_stem_rowwindow_split_nchw(const float *x_nchw, void *xw_sp, int64_t images, int h, int w, void *stream);   /* from [images][3][h][w] */
int mvg_stem_fprop_split(const mvg_conv_desc *d, const void *xw_sp, const void *w_sp, const float *w_sinv, float *y, float *stats,
                         void *stream);
int mvg_stem_wgrad_splits_split(const mvg_conv_desc *d);
int mvg_stem_wgrad_split(const mvg_conv_desc *d, const void *xw_sp, const void *dy_sp, const float *dy_sinv, float *dw_rw,
                         float *workspace, int splits, int accumulate, void *stream);
/* What the two stem launches run for `d` (the stem's own descriptor) with the CUs the planners may use now: the forward's tile
 * (*fwd_bm x *fwd_bn: 128 x 64, 128 x 128, or 256 x 64 from 65536 output rows per group with 64 columns) and K loop (*fwd_stages:
 * 1, or 2 = the two-stage pipeline, 128 x 128 tiles only), the weight gradient's tile over cout x 224 and its pixel addressing
 * (as mvg_conv_wgrad_split_tile).  Every out-pointer may be NULL; launches nothing; 0, or -1 (and a message) for a descriptor the
 * stem launches reject. */
int mvg_stem_plan_query_split(const mvg_conv_desc *d, int32_t *fwd_bm, int32_t *fwd_bn, int32_t *fwd_stages, int32_t *wgrad_bm,
                              int32_t *wgrad_bn, int32_t *wgrad_incremental);
int mvg_bn_relu_maxpool_bwd_reduce_split(const float *g_pooled, const uint8_t *argmax, const float *y, const float *mean,
                                         const float *invstd, const float *scale, const float *shift, int groups,
                                         int n_per_group, int h, int w, int c, int ho, int wo, float *s1, float *s2,
                                         float *dgamma, float *dbeta, int accumulate, float *workspace, float *mx, const float *gamma,
                                         float *dy_sinv, void *stream);
int mvg_bn_relu_maxpool_bwd_apply_split(const float *g_pooled, const uint8_t *argmax, const float *y, const float *mean,
                                        const float *invstd, const float *gamma, const float *scale, const float *shift,
                                        const float *s1, const float *s2, int groups, int n_per_group, int h, int w, int c,
                                        int ho, int wo, void *dy_sp, const float *mx, float *dy_sinv, int dy_sinv_ready, void *stream);
int mvg_conv_wgrad_splits_split(const mvg_conv_desc *d);   /* pixel-split count; workspace = splits * cout*r*s*cin floats */
/* The tile mvg_conv_wgrad_split runs a descriptor on: *bm x *bn (cout rows x r*s*cin columns; 128 x 256, 128 x 192, 128 x 128,
 * 128 x 64, 64 x 192, 64 x 128 or 64 x 64) and *incremental = 1 when the kernel addresses pixels incrementally (ho * wo >= 32).
 * Each pointer may be NULL.  Host arithmetic by the launch's own choice, launches nothing; 0, or -1 for a bad descriptor. */
int mvg_conv_wgrad_split_tile(const mvg_conv_desc *d, int32_t *bm, int32_t *bn, int32_t *incremental);
int mvg_conv_wgrad_split(const mvg_conv_desc *d, const void *x_sp, const void *dy_sp, const float *dy_sinv, float *dw,
                         float *workspace, int splits, int accumulate, void *stream);
/* The same launch WITHOUT its slab reduce (splits > 1: workspace receives the per-split partial gradients), and the reduces
 * of up to 8 such gradients in ONE launch (a residual block's convs): dw[i] (+)= the sum over host_splits[i] slabs of
 * host_n[i] floats, fixed order.  Host arrays; the launch copies them. */
int mvg_conv_wgrad_split_slabs(const mvg_conv_desc *d, const void *x_sp, const void *dy_sp, const float *dy_sinv, float *workspace,
                               int splits, void *stream);
/* ... with x_sinv, the 2^-k of a scaled activation operand (mvg_act_scales; NULL = unscaled) */
int mvg_conv_wgrad_split_xs(const mvg_conv_desc *d, const void *x_sp, const float *x_sinv, const void *dy_sp, const float *dy_sinv,
                            float *dw, float *workspace, int splits, int accumulate, void *stream);
int mvg_conv_wgrad_split_slabs_xs(const mvg_conv_desc *d, const void *x_sp, const float *x_sinv, const void *dy_sp,
                                  const float *dy_sinv, float *workspace, int splits, void *stream);
int mvg_wgrad_reduce_batch(const float *const *host_slabs, float *const *host_dw, const int64_t *host_n, const int32_t *host_splits,
                           const int32_t *host_accumulate, int n, void *stream);

/* ---------------------------------------------------------------- the fusion block on the split kernels
 * ImageFeatFuser / gaze head Linears (rot_mv.py:35-50,179-184,234-254; blocks.py:41-47) with >= 1024 rows: every tensor a
 * split kernel reads carries a per-tensor power-of-two scale (the reference computes these in plain fp32 and has no range
 * limit; fp16 pieces do), found WITHOUT extra passes: fp32 results leave max |.| in a device slot from the producing
 * launch's epilogue (float bits, atomicMax: order-independent; the caller clears the slots once per step), sp results are
 * stored times the 2^k a bound allows.
 *   mvg_absmax_multi: max |x| of up to 8 small tensors (HOST arrays of device pointers / counts / slots) in one launch.
 *   mvg_fuse_build_split: the operands built from a feature tensor F [.][3][nvec], straight into sp:
 *       xf[m] = [ img_feat[row_img[m]] | rel[m] @ F[row_src_f[m]] ]  (next iteration's fuser input; NULL = not wanted)
 *       xh[m] = [ img_feat[row_img[m]] |          F[row_src_h[m]] ]  (this iteration's head input;  NULL = not wanted)
 *     scaled from am_img / am_feat (max |img_feat|, max |F|: |rel @ f| <= sqrt(3) max |f|); *xf_sinv / *xh_sinv = 2^-k.
 *   mvg_linear_fprop_split: out = relu?(x W^T + bias); out fp32 (out_absmax, may be NULL, receives max |out|) or sp
 *     (out_sp: stored times 2^k from the bound fin * 2^30 * x_sinv * w_sinv + *bias_absmax >= |out|; *out_sinv = 2^-k).
 *   mvg_linear_dgrad_split: dx = (dy W) [* (relu_mask_sp > 0)] [+ addend], out_absmax as above.
 *   mvg_linear_wgrad_split: dw (+)= dy^T x with BOTH operands scaled (x_sinv may be NULL).
 *   mvg_split_colsum: g [rows][cols] fp32 -> sp times the 2^k that *absmax (max |g| bits) allows, *out_sinv = 2^-k, and
 *     db (may be NULL) (+)= the column sums of g - the Linear's bias gradient - in one pass (cols % 32 == 0).
 *   mvg_fuse_unbuild: the backward of mvg_fuse_build_split for one iteration: dfeat [segments][batch][3][nvec] =
 *     dxh[.][cf:] + sum over d with seg[d] == s of rel[d]^T @ dxn[d][cf:]; da [views][batch][cf] (+)= sum over d with
 *     vi[d] == v of (dxh + dxn)[d][:cf]; max |dfeat| into *absmax (may be NULL).  dxh / dxn: [dirs][batch][cf + 3 nvec]. */
int mvg_absmax_multi(const float *const *host_ptrs, const int64_t *host_counts, float *const *host_out_slots, int n, void *stream);
int mvg_fuse_build_split(const float *img_feat, const float *feat, const float *rel, const int32_t *row_img, const int32_t *row_src_f,
                         const int32_t *row_src_h, void *xf_sp, void *xh_sp, const float *am_img, const float *am_feat,
                         float *xf_sinv, float *xh_sinv, int rows, int cf, int nvec, void *stream);
int mvg_fuse_unbuild(const float *dxh, const float *dxn, const float *rel, const int32_t *seg, const int32_t *vi, float *dfeat, float *da,
                     int da_accumulate, int segments, int views, int dirs, int batch, int cf, int nvec, float *absmax, void *stream);
int mvg_linear_fprop_split(int rows, int fin, int fout, const void *x_sp, const float *x_sinv, const void *w_sp, const float *w_sinv,
                           const float *bias, int relu, void *out, int out_sp, float *out_sinv, const float *bias_absmax,
                           float *out_absmax, void *stream);
int mvg_linear_dgrad_split(int rows, int fin, int fout, const void *dy_sp, const float *dy_sinv, const void *wt_sp, const float *w_sinv,
                           float *dx, const float *addend, const void *relu_mask_sp, float *out_absmax, void *stream);
int mvg_linear_wgrad_split(int rows, int fin, int fout, const void *x_sp, const float *x_sinv, const void *dy_sp, const float *dy_sinv,
                           float *dw, float *workspace, int splits, int accumulate, void *stream);
int mvg_split_colsum(const float *g, int rows, int cols, const float *absmax, void *out_sp, float *out_sinv, float *db, int accumulate,
                     void *stream);
/* What mvg_linear_fprop_split (dgrad == 0) / mvg_linear_dgrad_split (dgrad != 0) run for a Linear with the CUs the planners may use now,
 * answered by the code those launches plan with: the tile (*bm x *bn: 128 x 128, or 128 x 64 for fewer than 128 columns or where
 * 128-column tiles would leave half the CUs idle) and the K loop (*stages: 1, or 2 = the two-stage pipeline, which the Linear
 * kernels have at both widths).  Every out-pointer may be NULL; launches nothing; 0, or -1 (and a message) for sizes the launches
 * refuse. */
int mvg_linear_plan_query_split(int rows, int fin, int fout, int dgrad, int32_t *bm, int32_t *bn, int32_t *stages);

/* ---------------------------------------------------------------- inference session (no Python needed)
 * An opaque handle, made for ONE (architecture, views, batch, height, width) shape, that queues the complete eval-mode
 * forward of the fp32 model - input layout, backbone with BatchNorm folded into the conv epilogues (trainer.py:164-199
 * under model.eval()), pools, lifter, fusion iterations, gaze heads (rot_mv.py:188-263) - from one call.  It calls the
 * entry points above, in the order and with the arguments the Python module uses, so the results are bit-identical.
 *
 * Ownership: the caller owns the workspace, the model tensors, the inputs and the outputs; the session keeps pointers
 * only.  mvg_session_forward allocates nothing, never synchronises and touches no host memory after its launches are
 * queued.  The workspace holds the sp copies of the conv / Linear weights (KRSC only), the folded (scale, shift) of every
 * BatchNorm, the pair / row index tables, the split head path's 64 scale slots, the activation arena (buffers share
 * bytes when their live ranges do not intersect; create verifies that plan and fails if it is unsound) and a scratch
 * region of mvg_scratch_bytes() that the launches of a forward use instead of the mvg_set_scratch registry.
 *
 * split: 1 = the kernels the fp32 module runs by default (split-operand convs unless a view's largest sp tensor would reach
 * 2 GiB - decided from the cfg's real sizes -, split-operand fuser / head Linears from 1024 rows), 0 = the fp32-MFMA kernels
 * everywhere (MVG_SPLIT=0).  raw_u8: the views are uint8 [batch][in_h][in_w][3] patches put through
 * mvg_preprocess_u8hwc_resize (mean / std of main.py:38-39) instead of fp32 [batch][3][height][width] images.
 *
 * Two compute forms (mvg_session_create_ex): MVG_SESSION_FP32, the above, and MVG_SESSION_BF16, the eval-mode forward of the
 * bf16 storage path as the module queues it with compute_dtype = bfloat16 - uint8 patches or fp32 images straight to the bf16
 * NHWC8 stem input, the stem as mvg_conv_fprop_bf16 + mvg_bn_relu_maxpool_fwd_bf16, every residual unit one
 * mvg_conv_fprop_bf16_affine, mvg_avgpool_fwd_bf16, and the lifter / fuser / head Linears on mvg_linear_fprop_mixed over
 * materialised mvg_rotcat_fwd inputs.  Its workspace holds bf16 weight copies (KRSC only, the stem's 3 channels padded to 8)
 * and a 2-byte activation arena; split is ignored; there are no range units.  Bit-identical to the module, like the fp32 form.
 * Not representable: the encode_rotmat and share_feature variants, training. */
typedef struct mvg_session mvg_session;
typedef struct {
  int32_t depth;          /* 18 | 50 */
  int32_t num_iter;       /* >= 1 (reference: 3); at most 5 when the head runs on the split kernels */
  int32_t views, batch;   /* 2 <= views <= 8, batch >= 1 */
  int32_t height, width;  /* network input size, >= 32 */
  int32_t share_weights, ignore_rotmat;
  int32_t split;
  int32_t raw_u8;
  int32_t in_h, in_w, input_bgr;          /* raw_u8 only */
} mvg_session_cfg;

/* HOST ONLY (no HIP call: runs on a machine without a GPU): builds the layer table, the conv descriptors, the kernel-family
 * decisions and the buffer plan, and checks the plan.  Non-zero + mvg_last_error() for a configuration outside the scope;
 * *out is NULL then. */
int mvg_session_create(const mvg_session_cfg *cfg, mvg_session **out);
/* HOST ONLY.  mvg_session_create with the compute form chosen: mvg_session_create(cfg, out) is
 * mvg_session_create_ex(cfg, MVG_SESSION_FP32, out).  MVG_SESSION_BF16 accepts and ignores cfg->split, and also rejects here
 * every shape one of the bf16 entry points would reject in mvg_session_forward.  Any other `compute` is rejected.
 * mvg_session_compute returns the form a handle was made for (-1 for NULL). */
#define MVG_SESSION_FP32 0
#define MVG_SESSION_BF16 1
int mvg_session_create_ex(const mvg_session_cfg *cfg, int32_t compute, mvg_session **out);
int mvg_session_compute(const mvg_session *s);
/* Frees the handle (host memory only; the workspace is the caller's).  NULL is allowed. */
void mvg_session_destroy(mvg_session *s);
/* The model tensors the session reads, by state_dict key, in the order mvg_session_bind takes their pointers: per conv
 * weight (KRSC), BatchNorm weight, bias, running_mean, running_var; then the lifter, fuser and head Linears (weight, bias).
 * With share_weights only iteration 0's fuser / head appear. */
int mvg_session_num_tensors(const mvg_session *s);
const char *mvg_session_tensor_name(const mvg_session *s, int i);
int64_t mvg_session_tensor_numel(const mvg_session *s, int i);
/* Bytes of the workspace mvg_session_bind wants (host only). */
size_t mvg_session_workspace_bytes(const mvg_session *s);
/* Library calls one mvg_session_forward queues (host only; a stream-K / split-K GEMM adds its fix-up kernel on the device):
 * the plan's steps, one more while mvg_session_set_error_record holds a record, and one more while mvg_session_set_consensus
 * holds its outputs. */
int mvg_session_launches(const mvg_session *s);
/* The plan's steps in the order mvg_session_forward queues them (host only, both forms): how many, and the entry point step
 * i calls, without the "mvg_" prefix, e.g. "conv_fprop_bf16_affine" (a step that records ranges still names the plain entry
 * point; the split head path's slot clear is "memset").  NULL out of range. */
int mvg_session_num_steps(const mvg_session *s);
const char *mvg_session_step_name(const mvg_session *s, int i);
/* host_tensor_ptrs: a HOST array of mvg_session_num_tensors() device pointers (fp32, contiguous; conv weights KRSC).
 * workspace: 256-byte aligned device memory of at least mvg_session_workspace_bytes().  Queues on `stream` the work that
 * depends on the weights only: the index tables, the stem filter padded to 4 channels, every sp weight copy (two
 * mvg_weights_prep_batch calls; MVG_SESSION_BF16: the bf16 copies, mode 0, and no padded stem filter) and every BatchNorm
 * fold (one mvg_bn_eval_affine_batch).  Call it again after the
 * weights changed (same or new pointers).  Forwards must be ordered after it (same stream, or an event). */
int mvg_session_bind(mvg_session *s, const void *const *host_tensor_ptrs, void *workspace, size_t bytes, void *stream);
/* Queues one forward on `stream`: only the launches that depend on the input.  host_view_ptrs: a HOST array of `views`
 * device pointers (fp32 NCHW images, or uint8 HWC patches with raw_u8); rot fp32 [batch][views][3][3].  Outputs (device,
 * fp32, D = views (views - 1) directed pairs, I = num_iter, Cf = 512 | 2048): img_feat [views][batch][Cf], lifted
 * [views][batch][3][512], feats [I][D][batch][3][512], preds [I][D][batch][2]. */
int mvg_session_forward(mvg_session *s, const void *const *host_view_ptrs, const float *rot, float *img_feat, float *lifted,
                        float *feats, float *preds, void *stream);
/* The activation range record of a session whose backbone runs on the split kernels (mvg_conv_fprop_split_affine_ranged):
 * one 32-bit word per sp tensor the forward stores - the stem's pooled map (named by the stem's conv), then every block
 * conv in forward order; the downsample branches stay fp32 and have none.  _num_range_units (host only): how many, 0 when
 * the backbone is not on the split kernels (split = 0, the 2 GiB guard, or MVG_SESSION_BF16); _range_unit_name (host only): the conv's
 * state_dict prefix, NULL out of range.  _set_range_record (host only: the pointer is only stored): record_dev = device
 * memory of _num_range_units words, or NULL (the default) for no record.  With a record mvg_session_forward clears it with
 * one stream-ordered memset and calls the ranged entry points: same mvg_session_launches, same outputs, still no
 * synchronisation and no allocation.  There is no fallback inside a session: a caller who reads a word >= 0x477FF000
 * builds a split = 0 session. */
int mvg_session_num_range_units(const mvg_session *s);
const char *mvg_session_range_unit_name(const mvg_session *s, int i);
int mvg_session_set_range_record(mvg_session *s, uint32_t *record_dev);
/* The gaze error record of a session (host only: the pointers are only stored; both compute forms).  gt_dev: the caller's static
 * fp32 [D][batch][2] label buffer (row d = the labels of the view direction d predicts for), refilled before each forward;
 * record_dev, err_out, capacity: as mvg_gaze_error_update takes them, cells = num_iter * D.  record_dev = NULL (the default)
 * restores the plain forward exactly.  With a record mvg_session_forward queues one mvg_gaze_error_update over its own preds
 * after the plan's last step: the four outputs are unchanged, still no synchronisation and no allocation; the plan - its steps,
 * their names, mvg_session_num_steps - is untouched, and mvg_session_launches reports one more.  A record without gt_dev,
 * capacity < 0 and err_out with capacity == 0 are rejected. */
int mvg_session_set_error_record(mvg_session *s, const float *gt_dev, double *record_dev, float *err_out, int64_t capacity);
/* The consensus gaze of a session (host only: the pointers are only stored; both compute forms).  head [num_iter][batch][3],
 * views_out [num_iter][views][batch][2], stats [num_iter][batch][2] or NULL and weights_dev [batch][views] or NULL: the caller's
 * static device buffers, as mvg_gaze_consensus_fwd takes them.  views_out = NULL (the default) restores the plain forward exactly.
 * With views_out mvg_session_forward queues one mvg_gaze_consensus_fwd over its own preds and rot after the plan's last step and
 * before the error update, if one is set: the four outputs are unchanged, still no synchronisation and no allocation; the plan -
 * its steps, their names, mvg_session_num_steps - is untouched, and mvg_session_launches reports one more.  views_out without
 * head is rejected.  (Added under ABI v13: additive.) */
int mvg_session_set_consensus(mvg_session *s, const float *weights_dev, float *head, float *views_out, float *stats);

#ifdef __cplusplus
}
#endif
#endif /* ROTMVGAZE_H */
