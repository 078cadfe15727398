/*
 * metrabs_hip.h -- C-ABI of the MI355X-native MeTRAbs per-crop hot path (libmetrabs_hip.so).
 *
 * The reference (isarandi/metrabs) is pure Python and has no FFI boundary; the path is reached by
 * ordinary method calls.  Each entry point below replaces the reference
 * call(s) cited next to it; the Python drop-ins in metrabs_amd/ (same class / function names as the
 * reference) are the only callers, via ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless it says "host";
 *   - nothing allocates, synchronises or touches global state: every call only enqueues work on
 *     `stream` (a hipStream_t), so all of them are hipGraph-capturable and re-entrant;
 *   - return value: 0 = ok, <0 = argument error detected on the host before any launch
 *     (MTR_E_*), >0 = hipError_t of a failed launch.  Nothing throws or exits across the ABI;
 *   - tensors are dense, row-major in the index order written in the comment.
 */
#ifndef METRABS_HIP_H_
#define METRABS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTR_VERSION 100 /* 0.1.0 */

typedef void* mtr_stream_t; /* hipStream_t */

enum mtr_dtype { MTR_F32 = 0, MTR_F16 = 1, MTR_BF16 = 2 };

enum mtr_layout {
  MTR_NCHW = 0, /* metrabs_pytorch: [B, C, H, W]            (models/metrabs.py:79 'b (d j) h w') */
  MTR_NHWC = 1  /* metrabs_tf / torch channels_last: [B,H,W,C] (tf models/metrabs.py:100-101)      */
};

enum mtr_error {
  MTR_OK = 0,
  MTR_E_NULL = -1,      /* a required pointer is NULL                      */
  MTR_E_SHAPE = -2,     /* a dimension is <= 0 or out of the supported range */
  MTR_E_DTYPE = -3,     /* unsupported dtype / layout combination           */
  MTR_E_PARAM = -4,     /* inconsistent params struct                       */
  MTR_E_WORKSPACE = -5, /* workspace too small / misaligned                 */
  MTR_E_ALIGN = -6      /* a pointer violates the documented alignment      */
};

/* The flags the reference reads from its global config at call time
 * (metrabs_pytorch/config/config.yaml:1-22, config_s_256.yaml:5-9; read in models/util.py:7,24,30). */
typedef struct mtr_head_params {
  int32_t proc_side;                  /* FLAGS.proc_side (256 / 384)                          */
  int32_t stride_test;                /* FLAGS.stride_test: inference stride of heatmap_to_image */
  int32_t centered_stride;            /* FLAGS.centered_stride                                 */
  int32_t legacy_centered_stride_bug; /* FLAGS.legacy_centered_stride_bug                      */
  float box_size_mm;                  /* FLAGS.box_size_mm (2200)                              */
} mtr_head_params;

/* Flags / constants of ptu3d.reconstruct_absolute and friends (ptu3d.py:9-33,56-121). */
typedef struct mtr_recon_params {
  int32_t proc_side;         /* FLAGS.proc_side                                   */
  int32_t stride_train;      /* FLAGS.stride_train (is_within_fov, ptu3d.py:115)  */
  int32_t centered_stride;   /* FLAGS.centered_stride (ptu3d.py:116)              */
  int32_t weak_perspective;  /* FLAGS.weak_perspective (ptu3d.py:14-18)           */
  int32_t mix_enabled;       /* 0 <=> mix_3d_inside_fov is None (ptu3d.py:28)     */
  float mix_3d_inside_fov;   /* FLAGS.mix_3d_inside_fov (0.5)                     */
  float l2_reg;              /* 1e-2   (ridge rows sqrt(1e-2), ptu3d.py:96-97)    */
  float weight_eps;          /* 1e-4   (weights = mask + 1e-4, ptu3d.py:94)       */
  float fov_border_factor;   /* 0.75   (is_within_fov default, ptu3d.py:113)      */
} mtr_recon_params;

int mtr_version(void);
const char* mtr_strerror(int code);

/* ------------------------------------------------------------------------------------------------
 * K2-K4: volumetric soft-argmax decode.  Replaces, for logits already in memory,
 *   MetrabsHeads.forward after the 1x1 conv   metrabs_pytorch/models/metrabs.py:78-85
 *   ptu.softmax / ptu.decode_heatmap          metrabs_pytorch/ptu.py:47-75
 *   heatmap_to_image / heatmap_to_metric      metrabs_pytorch/models/util.py:6-33
 *
 * logits   [B, J*(1+D), H, W] (MTR_NCHW) or [B, H, W, J*(1+D)] (MTR_NHWC), dtype f32/f16/bf16.
 *          channel n < J: 2D heatmap of joint n; channel J + d*J + j: depth slice d of joint j.
 * coords2d     [B, J, 2] f32, pixels (x, y) of the crop
 * coords3d_rel [B, J, 3] f32, millimetres (x, y, z) relative to the unknown reference point
 */
int mtr_softargmax_decode(const void* logits, int dtype, int layout, int B, int J, int D, int H,
                          int W, const mtr_head_params* p, float* coords2d, float* coords3d_rel,
                          mtr_stream_t stream);
/* The same launch with the NHWC kernel choice made explicit (A/B measurements, the bit-identity tests):
 * nhwc_staging 0 = the library's rule, 1 = never, 2 = whenever the shape allows, 3 = as 2 with two crops per workgroup
 * where that fills the waves better (measured, never the rule's choice) -- the kernel that streams a crop's logits
 * through a ring of LDS slots filled by 16-byte-per-lane global_load_lds and walks them there (by the rule: launches of
 * >= 256 crops of <= 1,024 channels).  Same operations in the same order: the same bits.  Ignored for MTR_NCHW. */
int mtr_softargmax_decode_opts(const void* logits, int dtype, int layout, int B, int J, int D, int H,
                               int W, const mtr_head_params* p, int nhwc_staging, float* coords2d,
                               float* coords3d_rel, mtr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K1+K2-K4 fused: 1x1 heatmap-projection GEMM (MFMA) with the decode as its epilogue; the logits
 * never reach HBM.  Replaces MetrabsHeads.forward as a whole (models/metrabs.py:75-85; the conv is
 * torch.nn.LazyConv2d(kernel_size=1), models/metrabs.py:73).
 *
 * mtr_head_pack_weights re-orders conv_final.weight [J*(1+D), C] (+bias) ONCE into the tiled
 * layout the kernel streams; `packed` must hold mtr_head_packed_bytes(...) bytes
 * (0 = no fused kernel for this (C, J, D, dtype): run the 1x1 conv as a GEMM and
 * mtr_softargmax_decode on its logits).  The blob is specific to the feat_dtype it was packed for:
 * pass the same feat_dtype to mtr_head_packed_bytes, mtr_head_pack_weights and mtr_head_fused.
 * features: [B, C, H, W] (MTR_NCHW) or [B, H, W, C] (MTR_NHWC, C % 4 == 0); H*W a multiple of 4.
 *
 * f32 features (the reference's CPU arithmetic) -- row-tile kernel, any map size, D <= 80:
 *   v_mfma_f32_16x16x4_f32 on f32 weights, chains of 32 channels summed in f32 over 8 stages and
 *   carried into f64 accumulators; 16-row tiles of whole softmax units (mtr_head_row_plan), a
 *   workgroup = (crop, block of <= 5 tiles), tiles staged by global_load_lds -- on launches of at most
 *   one workgroup per CU by a dedicated loader wave (mtr_head_options.rt_loader); with a workspace
 *   (mtr_head_fused_ws) the 64-position column blocks of a larger map may go to different workgroups
 *   (rt_split_column_blocks).  Every dispatch choice gives the same bits.
 * f16 / bf16 features (the reference's autocast GPU arithmetic) -- joint-group kernels, C % 8 == 0,
 *   1 + D <= 64, H*W <= 256: v_mfma_f32_32x32x16_{f16,bf16} on the features and on the weights
 *   ROUNDED TO THE FEATURE DTYPE (what autocast does to conv_final), f32 accumulation, f32 logits.
 *   (C % 64 == 0, and for NCHW also H*W % 8 == 0 and H*W >= 64: tiles staged by global_load_lds
 *   instead of through registers -- same arithmetic, same results.)
 *   Beyond those limits (72 depth bins; maps of more than 256 positions), C % 64 == 0, D <= 80: the
 *   row-tile core on v_mfma_f32_16x16x32_{f16,bf16} (head_rt16_kernel), any map size.  It consumes
 *   NHWC features; NCHW features are transposed once into the workspace of mtr_head_fused_ws
 *   (without one: MTR_E_WORKSPACE).
 *
 * mtr_head_fused_opts: the same launch with explicit dispatch choices (A/B measurements, tests of
 * every kernel variant); options == NULL or all-zero fields = the library's own choice.  There are
 * no environment switches behind these entry points, and no state that changes a result.  What the
 * library does keep per process is MEMOISATION of pure functions of its arguments: the launch plans of
 * the f32 head (a mutex-guarded map keyed by the current device's CU count, the shape -- with the batch
 * size rounded up to a multiple of 8, all the plan reads of it -- and the options), the per-kernel "dynamic LDS allowed" once-flags, and
 * the detector pre-processing's per-shape kernel choice; all of it is rebuilt identically on a miss.
 *
 * mtr_head_fused / mtr_head_fused_opts have no workspace to offer: a shape that needs one (16-bit NCHW
 * features on the row-tile core) is reported as MTR_E_SHAPE -- "take the library-GEMM path" -- exactly
 * like any other shape without a fused kernel; only mtr_head_fused_ws returns MTR_E_WORKSPACE.
 *
 * mtr_head_options is versioned by its first member: set struct_size = sizeof(mtr_head_options) of the
 * header you compiled against.  The library reads the fields inside struct_size and takes its own choice
 * for the ones beyond it (a caller built against an older, shorter struct keeps working); a struct_size
 * that is not a multiple of 4, below 8 or above 256 is MTR_E_PARAM (a round-3 caller, whose struct began
 * with rt_tiles_per_workgroup = 0..5, is rejected instead of being misread).
 */
typedef struct mtr_head_options {
  uint32_t struct_size;            /* sizeof(mtr_head_options) as the CALLER knows it (see above)            */
  int32_t rt_tiles_per_workgroup;  /* f32: row tiles per workgroup for one-tile atoms, 1..5; 0 = by launch size */
  int32_t groups_per_workgroup;    /* 16-bit: joint groups per workgroup, 1..3 (dma_staging 4: 2..4 = waves
                                      per workgroup); 0 = by launch size                                    */
  int32_t dma_staging;             /* 16-bit: 1 = global_load_lds where possible, 0 = through registers,
                                      2 = global_load_lds issued by a fifth, LOADER wave (320 threads; same
                                      bits; measured 10 - 25 % SLOWER than 1 on every shape of
                                      profiles/r04c_head16_ab.jsonl -- kept for A/B runs, never the library's
                                      choice), 3 = global_load_lds with the copies of stage s + 1 issued first in
                                      stage s and the fragments read per 16-channel step (round 4; same bits),
                                      4 = weights in registers (round 5, head_areg.hip: a wave per joint group
                                      against all column tiles, weights loaded per lane from the fragment-major
                                      section of the blob, only the features through LDS; 3 - 5 column tiles,
                                      C % 64 == 0; same bits; elsewhere: as -1),
                                      5 = weights RESIDENT in registers, persistent workgroups (round 5,
                                      head_res.hip: a workgroup keeps a pair of joint groups' weights for the
                                      whole launch and streams its share of the crops through a ring of feature
                                      stages; C = 1280, 3 - 5 column tiles; same bits; 20 - 40 % SLOWER than the
                                      library's choice on every shape of profiles/r05y_* -- its decode epilogue
                                      has no second workgroup's K loop to hide behind; kept for A/B runs;
                                      elsewhere: as -1),
                                      6 = eight waves in two alternating halves (round 6, head_pp.hip: four joint
                                      groups per workgroup; one half multiplies a 64-channel stage while the other
                                      issues the next stage's copies; C % 64 == 0, 3 - 5 column tiles; same bits;
                                      elsewhere: as -1),
                                      7 = early copies on a tight feature stage (round 6: H*W positions instead of
                                      whole 32-position tiles, exactly two stages of LDS; groups_per_workgroup 1
                                      (default) or 2; H*W % 8 == 0; same bits; elsewhere: as -1),
                                      -1 = library's choice (NB: a zeroed struct selects registers) */
  int32_t rt_column_blocks;        /* f32, maps of > 64 positions: 64-position column blocks per workgroup
                                      tile, 2..4 (one K loop for all of them); 1 = one K loop per column
                                      block; 0 = by launch size                                         */
  int32_t rt_k_groups;             /* f32, blocks of <= 3 one-tile atoms, C % 64 == 0: 2 = two K groups per
                                      workgroup (512 threads: the odd 32-channel stages run on waves
                                      4..7 and their chains are handed to waves 0..3, which sum in the
                                      one-group order: same bits), 1 = one; 0 = two for blocks of 2-3
                                      tiles (the small-launch configuration)                          */
  int32_t rt_loader;               /* f32, C % 32 == 0: 2 = four MFMA waves + a LOADER wave per workgroup (320
                                      threads; the fifth wave issues every global_load_lds and waits for it,
                                      the MFMA waves only meet it at the stage barrier: same bits), 1 = never;
                                      0 = for launches of at most one workgroup per CU                 */
  int32_t rt_split_column_blocks;  /* f32, maps of > 64 positions, mtr_head_fused_ws with a workspace: 2 = deal
                                      the 64-position column blocks to different workgroups (a second, tiny
                                      launch merges their softmax statistics in block order: same bits as one
                                      workgroup walking them), 1 = never; 0 = on small launches        */
} mtr_head_options;

/* host-only, no GPU work: the row order of the f32 row-tile kernel.  conv_final's J*(1+D) channels
 * are re-ordered into n_tiles 16-row MFMA tiles so that the rows of one softmax (a joint's 2D row;
 * a joint's D depth slices) never straddle a workgroup's block of tiles; atoms of tiles_per_atom
 * consecutive tiles are the unit a block is made of.  row_channel (may be NULL; `capacity` ints,
 * >= n_tiles*16) receives for every packed row the conv_final channel it holds, -1 for padding. */
int mtr_head_row_plan(int J, int D, int32_t* n_tiles, int32_t* tiles_per_atom, int32_t* row_channel,
                      int capacity);
size_t mtr_head_packed_bytes(int C, int J, int D, int feat_dtype);
int mtr_head_pack_weights(const float* weight /*[J*(1+D), C] f32*/, const float* bias /*[J*(1+D)]*/,
                          int C, int J, int D, int feat_dtype, void* packed, mtr_stream_t stream);
int mtr_head_fused(const void* features, int feat_dtype, int layout, int B, int C, int H, int W,
                   const void* packed, int J, int D, const mtr_head_params* p, float* coords2d,
                   float* coords3d_rel, mtr_stream_t stream);
int mtr_head_fused_opts(const void* features, int feat_dtype, int layout, int B, int C, int H, int W,
                        const void* packed, int J, int D, const mtr_head_params* p,
                        const mtr_head_options* options, float* coords2d, float* coords3d_rel,
                        mtr_stream_t stream);
/* host-only, no GPU work: which kernel mtr_head_fused_ws takes for a launch (what a profile will show).
 * kernel: one of MTR_HEAD_KERNEL_*; 0 with return MTR_E_SHAPE = no fused kernel for this shape. */
enum {
  MTR_HEAD_KERNEL_RT = 1,        /* head_rt_kernel: 256 threads, every wave copies and multiplies          */
  MTR_HEAD_KERNEL_RT_LOADER = 2, /* head_rt_ld_kernel: four MFMA waves + a loader wave                     */
  MTR_HEAD_KERNEL_RT_KS = 3,     /* head_rt_ks_kernel: two K groups                                        */
  MTR_HEAD_KERNEL_RT_NP = 4,     /* head_rt_np_kernel: row tiles x column blocks per workgroup             */
  MTR_HEAD_KERNEL_16 = 10,       /* head_fused16_kernel: 16-bit features staged through registers          */
  MTR_HEAD_KERNEL_16_DMA = 11,   /* head_fused16dma_kernel: 16-bit features staged by global_load_lds      */
  MTR_HEAD_KERNEL_16_DMA_EARLY = 14,  /* head_fused16dma_kernel<..., EARLY>: copies of stage s + 1 issued first in stage s */
  MTR_HEAD_KERNEL_16_DMA_LOADER = 13, /* head_fused16dma_kernel<..., LD>: the same with a loader wave (dma_staging 2) */
  MTR_HEAD_KERNEL_16_AREG = 15,  /* head_fused16areg_kernel: weights in registers, a wave per joint group (dma_staging 4;
                                    the library's choice for >= 512 crops of >= 8 joint groups on 5 column tiles)  */
  MTR_HEAD_KERNEL_16_RES = 16,   /* head_fused16res_kernel: weights RESIDENT in registers, persistent workgroups (dma_staging 5) */
  MTR_HEAD_KERNEL_16_PP = 17,    /* head_fused16pp_kernel: eight waves in two alternating halves, four joint groups per
                                    workgroup (dma_staging 6; round 6)                                        */
  MTR_HEAD_KERNEL_16_DMA_EARLY_TIGHT = 18, /* the early-copies kernel on a feature stage of exactly H*W positions and two stages
                                    of LDS: one joint group per workgroup = 52 KiB at 12x12, three workgroups per CU (round 6;
                                    dma_staging 7; the library's choice where its round model says so)          */
  MTR_HEAD_KERNEL_16_RT = 12     /* head_rt16_kernel: 16-bit features on the row-tile core (1 + D > 64 rows per
                                    joint, or maps of more than 256 positions); NCHW features: needs the
                                    workspace (one transposing pass in front)                              */
};
typedef struct mtr_head_plan_info {
  int32_t kernel;
  int32_t tiles_per_workgroup;    /* f32: row tiles; 16-bit: joint groups                                   */
  int32_t column_blocks;          /* f32 np kernel: column blocks per workgroup tile, else 1               */
  int32_t split_column_blocks;    /* f32: column blocks dealt to workgroups (+ the merge launch), else 0   */
  int64_t workgroups;             /* of the main launch                                                     */
  double model_us;                /* f32 row-tile kernels: the launch plan's own estimate of the launch time
                                     (its cost model simulates the launch; diagnostic), else 0              */
} mtr_head_plan_info;
int mtr_head_plan(int feat_dtype, int layout, int B, int C, int H, int W, int J, int D,
                  const mtr_head_options* options, int have_workspace, mtr_head_plan_info* plan);

/* The same with a caller-provided scratch buffer (8-byte aligned, mtr_head_workspace_bytes(...) bytes,
 * contents irrelevant before and after; 0 bytes = this shape never uses one): with it, f32 maps of
 * more than 64 positions may spread their column blocks over workgroups (rt_split_column_blocks).
 * workspace == NULL is mtr_head_fused_opts.  Still no allocation, no sync, no globals: two launches
 * on `stream` instead of one when the split is taken. */
size_t mtr_head_workspace_bytes(int feat_dtype, int layout, int B, int C, int H, int W, int J, int D);
int mtr_head_fused_ws(const void* features, int feat_dtype, int layout, int B, int C, int H, int W,
                      const void* packed, int J, int D, const mtr_head_params* p,
                      const mtr_head_options* options, void* workspace, size_t workspace_bytes,
                      float* coords2d, float* coords3d_rel, mtr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K5: absolute (camera-space) reconstruction.  Replaces
 *   ptu3d.reconstruct_absolute        metrabs_pytorch/ptu3d.py:9-33
 *   ptu3d.reconstruct_ref_fullpersp   metrabs_pytorch/ptu3d.py:56-105
 *   ptu3d.reconstruct_ref_weakpersp   metrabs_pytorch/ptu3d.py:36-49
 *   ptu3d.is_within_fov / back_project           ptu3d.py:108-121
 *
 * The two RMS scalars of reconstruct_ref_fullpersp are taken over the WHOLE call batch
 * (ptu3d.py:71-74): B here must be the reference's internal batch for bit-comparable results.
 * workspace: mtr_reconstruct_workspace_bytes(B, J) bytes, 16-byte aligned.
 *
 * The split form exposes the batch moments so that a sharded caller can all-reduce them
 * (SURVEY.md section 8e "exact-monolithic mode"):
 *   mtr_reconstruct_moments -> moments[0] = sum(normalized2d^2), moments[1] = sum(rel_backproj^2),
 *                              moments[2] = number of summed elements (B*J*2), all f64;
 *   mtr_reconstruct_solve   <- the (possibly all-reduced) moments.
 */
size_t mtr_reconstruct_workspace_bytes(int B, int J);
int mtr_reconstruct_absolute(const float* coords2d /*[B,J,2]*/, const float* coords3d_rel /*[B,J,3]*/,
                             const float* intrinsics /*[B,3,3]*/, int B, int J,
                             const mtr_recon_params* p, float* poses3d /*[B,J,3]*/, void* workspace,
                             size_t workspace_bytes, mtr_stream_t stream);
int mtr_reconstruct_moments(const float* coords2d, const float* coords3d_rel,
                            const float* intrinsics, int B, int J, double* moments /*[3]*/,
                            void* workspace, size_t workspace_bytes, mtr_stream_t stream);
int mtr_reconstruct_solve(const float* coords2d, const float* coords3d_rel, const float* intrinsics,
                          int B, int J, const mtr_recon_params* p, const double* moments /*[3]*/,
                          float* poses3d, mtr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K6: crop sampler.
 *
 * mtr_build_pyramid replaces the whole-image gamma decode `(u8/255)**2.2`
 * (multiperson_model.py:196) and the box-filter pyramid (warping.py:10-13):
 *   images_u8 [N,3,Hi,Wi] u8  ->  level0 [N,3,Hi,Wi], level1 [N,3,Hi/2,Wi/2], level2 [N,3,Hi/4,Wi/4]
 *   (f32 linear light, floor division on odd sizes as avg_pool2d(2,2)).
 *
 * mtr_crop_geometry replaces Pose3dEstimator._get_new_rotation_and_scale and the matrix set-up of
 * _get_crops (multiperson_model.py:264-305,322-355; ptu3d.lookat_matrix ptu3d.py:129-142;
 * warping.undistort_points warping.py:65-73): one thread per (aug, box).
 *   boxes [n_box,4(+)] (x,y,w,h; row stride box_stride floats), intrinsics [n_box,3,3],
 *   distortion [n_box,12] (zero padded), camspace_up [n_box,3], aug_rotflipmat [n_aug,3,3],
 *   aug_scales [n_aug]
 *   -> new_intrinsics [n_aug,n_box,3,3], rot [n_aug,n_box,3,3], warp_params [n_aug*n_box, MTR_WARP_PARAM_FLOATS].
 *
 * mtr_warp_crops replaces warping.warp_images_with_pyramid / warp_single_image (warping.py:6-54:
 * homography, lens distortion warping.py:57-107, per-level intrinsics warping.py:128-133,
 * grid_sample bilinear/zeros/align_corners=True), the antialias avg_pool2d and the per-crop gamma
 * `crops **= gamma/2.2` of _get_crops (multiperson_model.py:308-319).
 *   warp_params [n_crops, MTR_WARP_PARAM_FLOATS] as laid out below; out [n_crops,3,res,res]
 *   (NCHW) or [n_crops,res,res,3] (NHWC), dtype f32/f16/bf16.
 */
#define MTR_WARP_PARAM_FLOATS 36
/* warp_params row (floats): [0..8] Hinv (new_invprojmat incl. the antialias scale), [9..17] K of
 * the chosen pyramid level, [18..29] 12 distortion coefficients, [30] has_distortion (0/1),
 * [31] pyramid level (0..2), [32] image id, [33] gamma exponent (gamma_aug / 2.2), [34..35] pad */

int mtr_build_pyramid(const uint8_t* images_u8, int N, int Hi, int Wi, float* level0, float* level1,
                      float* level2, mtr_stream_t stream);
/* Same pyramid from an already linear-light f32 level 0 (the argument warping.warp_images_with_pyramid
 * receives, warping.py:6-13): writes level1 / level2 only. */
int mtr_pyramid_from_level0(const float* level0, int N, int Hi, int Wi, float* level1, float* level2,
                            mtr_stream_t stream);
/* Level 0 left as the uint8 frame: the f32 level 0 is 64 % of the pyramid's bytes and is only ever
 * sampled, so the fast path never materialises it.  mtr_build_pyramid_u8 writes level1 / level2 and
 * the 256-entry gamma LUT (lut[v] = (v/255)**2.2); mtr_warp_crops_u8 samples level 0 from
 * images_u8 through that LUT (bit-identical to mtr_warp_crops on the materialised level 0). */
int mtr_build_pyramid_u8(const uint8_t* images_u8, int N, int Hi, int Wi, float* lut /*[256]*/,
                         float* level1, float* level2, mtr_stream_t stream);
int mtr_warp_crops_u8(const uint8_t* level0_u8, const float* lut, const float* level1,
                      const float* level2, int N, int Hi, int Wi, const float* warp_params,
                      int n_crops, int res, int antialias, int out_dtype, int out_layout, void* out,
                      mtr_stream_t stream);
/* The same two calls for frames with interleaved channels, images_u8 [N,Hi,Wi,3] (the memory of a
 * torch channels_last [N,3,Hi,Wi] tensor; what image decoders and numpy hand over; the reference
 * accepts such a tensor through its strides, `images.float()` at multiperson_model.py:196).  Levels 1
 * and 2 are the same f32 planes; the crops are bit-identical to mtr_warp_crops_u8 on the planar copy
 * of the frames.  The two x-taps of a row are then 6 consecutive bytes for all three channels: one
 * 12-byte gather per row instead of three 8-byte ones. */
int mtr_build_pyramid_u8_hwc(const uint8_t* images_u8, int N, int Hi, int Wi, float* lut /*[256]*/,
                             float* level1, float* level2, mtr_stream_t stream);
int mtr_warp_crops_u8_hwc(const uint8_t* level0_u8, const float* lut, const float* level1,
                          const float* level2, int N, int Hi, int Wi, const float* warp_params,
                          int n_crops, int res, int antialias, int out_dtype, int out_layout, void* out,
                          mtr_stream_t stream);
int mtr_crop_geometry(const float* boxes, int box_stride, const float* intrinsics,
                      const float* distortion, const float* camspace_up, const int32_t* image_ids,
                      const float* aug_rotflipmat, const float* aug_scales, const float* aug_gammas,
                      int n_box, int n_aug, int res, int antialias, float* new_intrinsics,
                      float* rot, float* warp_params, mtr_stream_t stream);
int mtr_warp_crops(const float* level0, const float* level1, const float* level2, int N, int Hi,
                   int Wi, const float* warp_params, int n_crops, int res, int antialias,
                   int out_dtype, int out_layout, void* out, mtr_stream_t stream);
/* antialias_factor > 4 (multiperson_model.py:312-315): the crops are sampled at res*aa x res*aa
 * (mtr_warp_crops[_u8] with res = res*aa, antialias = 1 and gamma exponents of 1 in warp_params[33])
 * and shrunk here the way torchvision.transforms.functional.resize(antialias=True) = aten's
 * separable antialiased bilinear filter does, with the per-crop `** (gamma / 2.2)` (:319) on the way
 * out.  crops_big [n_crops,3,res*aa,res*aa] f32 linear light; warp_params: the ORIGINAL rows (their
 * [33] is the exponent applied); workspace: mtr_crops_shrink_workspace_bytes(...) bytes;
 * 2 <= antialias <= 19. */
size_t mtr_crops_shrink_workspace_bytes(int n_crops, int res, int antialias);
int mtr_crops_shrink_antialiased(const float* crops_big, const float* warp_params, int n_crops, int res,
                                 int antialias, int out_dtype, int out_layout, void* out,
                                 void* workspace, size_t workspace_bytes, mtr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K7 (first "next" row): post-processing of the crop-model output in one launch.
 * Replaces Pose3dEstimator._predict_single_batch post-ops (multiperson_model.py:244-259: mirror
 * un-swap through joint_info.mirror_mapping for flipped augs, poses @ R, transpose) and the
 * post-ops of _estimate_poses_batched (multiperson_model.py:143-178: joint_transform_matrix,
 * 2D projection with lens distortion, world transform by inv(extrinsics), skeleton selection,
 * mean over the TTA axis).
 *   poses_crop [A, n, J, 3] crop-model output (aug-major), rot [A, n, 3, 3], should_flip [A] (u8),
 *   mirror_mapping [J] (i32), joint_transform [J, Jt] or NULL, skeleton [S] (i32) or NULL,
 *   intrinsics [n,3,3], distortion [n,12], inv_extrinsics [n,4,4] (already inverted)
 *   -> poses3d [n, (A,) S', 3], poses2d [n, (A,) S', 2]; the A axis is dropped when average_aug;
 *   S' = S if skeleton else (Jt if joint_transform else J).
 */
int mtr_postprocess_poses(const float* poses_crop, const float* rot, const uint8_t* should_flip,
                          const int32_t* mirror_mapping, const float* joint_transform, int Jt,
                          const int32_t* skeleton, int S, const float* intrinsics,
                          const float* distortion, const float* inv_extrinsics, int A, int n, int J,
                          int average_aug, float* poses3d, float* poses2d, mtr_stream_t stream);

/* Row a11: Metrabs.latent_points_to_joints (metrabs_tf/models/metrabs.py:80-81 ->
 * tfu3d.linear_combine_points tfu3d.py:48-49, einsum 'bjc,jJ->bJc'), the step Metrabs.forward runs
 * behind reconstruct_absolute when transform_coords / predict_all_and_latents is set
 * (metrabs_pytorch/models/metrabs.py:61-62, metrabs_tf/models/metrabs.py:61-62).
 *   points [B, J_in, 3] f32 (the reconstructed latent points), weights [J_in, J_out] f32 row-major
 *   (`w2` of the affine-weights file = recombination_weights) -> out [B, J_out, 3] f32.
 * f64 sums, one rounding per output.  J_in <= 4096. */
int mtr_linear_combine_points(const float* points, const float* weights, int B, int J_in, int J_out,
                              float* out, mtr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K9: detector pre-processing, the step in front of the hot path.
 * Replaces PersonDetector.forward minus the network (metrabs_pytorch/multiperson/person_detector.py):
 *   :15-20,26-29  target size / padding arithmetic in float32        -> mtr_detector_geometry (host)
 *   :21-33        (u8/255)**2.2, torchvision bilinear resize (antialiased when shrinking),
 *                 **(1/2.2), pad to multiples of 32 with 0.5           -> mtr_detector_preprocess
 *   :47-54        scale_boxes (network frame -> image frame)          -> mtr_detector_scale_boxes
 * The resize mirrors aten's separable CPU kernels operation for operation (bit-exact in linear
 * light); shrink factors above 19x are rejected (MTR_E_SHAPE).
 */
typedef struct mtr_detector_geom {
  int32_t target_h, target_w; /* resized extent: int32(factor * h), int32(factor * w)          */
  int32_t antialias;          /* factor < 1                                                    */
  int32_t pad_top, pad_left;  /* half_pad_h, half_pad_w                                        */
  int32_t out_h, out_w;       /* padded extent (multiples of 32)                               */
  float x_factor, y_factor;   /* w / target_w, h / target_h                                    */
} mtr_detector_geom;

/* host-only, no GPU work: fills `g` (a HOST pointer) for frames of H x W */
int mtr_detector_geometry(int H, int W, int input_size /*416*/, mtr_detector_geom* g);
/* images_u8 [N,3,H,W] uint8 -> out [N,3,g->out_h,g->out_w] f32 (what the network is fed); g: host */
int mtr_detector_preprocess(const uint8_t* images_u8, int N, int H, int W, const mtr_detector_geom* g,
                            float* out, mtr_stream_t stream);
/* The same with the kernel named (tests and timing; the two kernels give identical bits):
 *   AUTO    the streaming kernel for launches past its measured cross-over (4 frames of 1080p; any
 *           shrink of 5.5x and more) when the frame tensor is a multiple of 16 bytes and its LDS fits,
 *           else the tile kernel (what mtr_detector_preprocess does);
 *   TILE    one 8-row x 64-column output tile at a time, staged through registers;
 *   STREAM  a 64-column strip walked down the frame, rows loaded global -> LDS two chunks ahead by
 *           a loading wave (MTR_E_SHAPE when not available for this tensor). */
enum { MTR_DETECTOR_KERNEL_AUTO = 0, MTR_DETECTOR_KERNEL_TILE = 1, MTR_DETECTOR_KERNEL_STREAM = 2 };
int mtr_detector_preprocess_kernel(const uint8_t* images_u8, int N, int H, int W, const mtr_detector_geom* g,
                                   int kernel, float* out, mtr_stream_t stream);
/* xyxy_conf [n,5] (x1,y1,x2,y2,conf; network frame) -> boxes_out [n,5] (x,y,w,h,conf; image frame) */
int mtr_detector_scale_boxes(const float* xyxy_conf, int n, const mtr_detector_geom* g,
                             float* boxes_out, mtr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K8: plausibility filter + pose NMS, one launch per call (one
 * workgroup per image).  Replaces _filter_poses (metrabs_tf/multiperson/multiperson_model.py:441-459)
 * and plausibility_check.py (TF :9-96; PyTorch port metrabs_pytorch/multiperson/
 * plausibility_check.py:8-119, whose call site multiperson_model.py:158-163 is commented out):
 * is_pose_plausible, are_augmentation_results_consistent, is_pose_consistent_with_box,
 * compute_pose_similarity, pose_non_max_suppression.
 *   poses3d [P,A,J,3] camera-space mm (all model joints, before the skeleton selection),
 *   poses2d [P,A,J,2] px, boxes [P,5] (x,y,w,h,score); poses of image i are rows
 *   row_start[i] .. row_start[i+1]-1; sim_offsets[i] = sum_{k<i} n_k^2 (floats);
 *   edges [n_bones,2] + mean_bones [n_bones] of the first J_model joints (n_bones = 0: no bone test).
 *   -> valid [P] (u8, the three plausibility tests), keep_idx [P] (per image: the kept poses as
 *      global row indices, then -1), keep_count [n_images].
 * A table row that names a joint >= J_model is skipped.  The shape and parameter rules (A, J >= 1,
 * 1 <= J_model <= J, max_per_image <= 1024, 16 * (J rounded up to even) + 32 * A <= 48 KiB of dynamic
 * LDS) are checked before anything else, also for n_images = 0.
 * The workspace is a contract (tests/test_gpu_filter_fuzz.py reads it): first the mean-over-
 * augmentation poses [P,J,3] float32 (the float32 sum over A in order, divided by A), then, at
 * sim_offsets[i] floats behind them, image i's similarity matrix: nv_i x nv_i float32, COMPACT, over
 * the image's valid poses in index order (nv_i <= n_i; symmetric; NaN where J / 4 = 0).  The floats
 * of an image's n_i^2 behind its nv_i^2 are not written.  mtr_filter_poses_workspace_bytes sizes the
 * workspace for n_i^2 floats per image: (P * J * 3 + P * max_per_image) * 4 bytes, which holds
 * sum n_i^2 <= P * max_per_image.
 */
typedef struct mtr_filter_params {
  float rel_small, rel_big, abs_diff_mm; /* 0.1, 3, 300   plausibility_check.py:22-24            */
  float stdev_mm;                        /* 200           :64-66                                 */
  float box_fraction;                    /* 0.5           TF :84                                  */
  float sim_scale_mm, sim_threshold;     /* 300, 0.4      :83, :59                                */
  int32_t max_output;                    /* 150 (TF max_output_size; used when order_by_score)     */
  int32_t var_correction;                /* 0 = population variance (TF), 1 = torch.var default    */
  int32_t order_by_score;                /* 1 = TF order (score descending), 0 = PyTorch port (index) */
} mtr_filter_params;

size_t mtr_filter_poses_workspace_bytes(int P, int J, int max_per_image);
int mtr_filter_poses(const float* poses3d, const float* poses2d, const float* boxes,
                     const int32_t* row_start, const int32_t* sim_offsets, int n_images, int P, int A,
                     int J, const int32_t* edges, const float* mean_bones, int n_bones, int J_model,
                     const mtr_filter_params* params /*host*/, void* workspace, size_t workspace_bytes,
                     int max_per_image, uint8_t* valid, int32_t* keep_idx, int32_t* keep_count,
                     mtr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K10 (outside the reference's hot path): fused epilogue for the PyTorch-ROCm
 * backbone's inference copy, metrabs_amd/backbones.py:fold_batchnorm(fused_epilogue=True).  With
 * batch norm folded into a convolution, what follows it is "+ bias[c]" and an activation -- two
 * elementwise kernels in PyTorch-ROCm (torchvision Conv2dNormActivation: ops/misc.py; the
 * reference's backbones/efficientnet.py:11-18 builds on it).  In place on y [B, C, HW] (NCHW,
 * 16-byte aligned, HW % (16 / sizeof(dtype)) == 0): y = act(y + bias[c]) (+ residual, the skip
 * connection of an (Fused)MBConv block, same shape and dtype as y, may be NULL), computed in f32.
 * act: 0 none, 1 ReLU, 2 SiLU, 3 Hardswish.
 */
int mtr_bias_act_nchw(void* y, int dtype, const float* bias /*[C] f32*/, const void* residual, int act,
                      long long B, int C, int HW, mtr_stream_t stream);

/* Same pass without a residual, additionally row_mean[b * C + c] = mean over H*W of the stored result:
 * the input of the squeeze-excite block behind a depthwise convolution (x.mean((2, 3)), the first
 * statement of torchvision's SqueezeExcitation that efficientnet.py:110-173 uses), otherwise a
 * reduction kernel of its own. */
int mtr_bias_act_rowmean_nchw(void* y, int dtype, const float* bias /*[C] f32*/, int act, long long B,
                              int C, int HW, float* row_mean /*[B*C] f32*/, mtr_stream_t stream);

/* K11 (outside the reference's hot path, like K10): depthwise 3x3 convolution of the backbone's
 * inference copy with the K10 epilogue in the same pass.  x [B, C, H, W] -> y [B, C, OH, OW] (NCHW,
 * same dtype; OH = (H + 2 pad - 3) / stride + 1, OW likewise and a multiple of 4), cross-correlation
 * with weight [C, 3, 3] f32 (torch Conv2d(groups=C).weight with the batch norm folded in), zero
 * padding `pad` in {0, 1} on every side, stride in {1, 2}; y = act(conv + bias[c]) in f32 arithmetic;
 * row_mean (may be NULL): [B*C] f32 mean of the stored result per (b, c) plane, the input of the
 * squeeze-excite block behind the layer (efficientnet.py:110-173). */
int mtr_depthwise3x3_bias_act(const void* x, int dtype, const float* weight, const float* bias, int act,
                              long long B, int C, int H, int W, int stride, int pad, void* y,
                              float* row_mean, mtr_stream_t stream);
/* The same layer with the explicit asymmetric zero padding the reference's TF-'SAME' stride-2 layers
 * put in front of an unpadded convolution (efficientnet.py:1127-1161: (0,1,0,1), or (0,2,0,2) for the
 * `bottomright_stride` layer) folded in: pad_top, pad_left in {0, 1}, pad_bottom, pad_right in 0..2;
 * OH = (H + pad_top + pad_bottom - 3) / stride + 1, OW likewise and a multiple of 4.  x is the
 * UNPADDED activation: the ZeroPad2d pass and its padded copy disappear. */
int mtr_depthwise3x3_bias_act_padded(const void* x, int dtype, const float* weight, const float* bias,
                                     int act, long long B, int C, int H, int W, int stride, int pad_top,
                                     int pad_left, int pad_bottom, int pad_right, void* y,
                                     float* row_mean, mtr_stream_t stream);

/* K18 (outside the reference's hot path, like K11): the stride-1, padding-1 depthwise 3x3 layer of K11 on register
 * blocks, for the planes K11's own block kernel refuses (it takes a plane only when W / 4 and H / 4 are powers of
 * two and the plane has at most 64 blocks; everything else runs on its VALU-bound generic kernel).  x, y
 * [B, C, H, W] NCHW in `dtype` (f32 / f16 / bf16), both 16-byte aligned (else MTR_E_ALIGN); weight [C, 3, 3] and
 * bias [C] f32; W a multiple of 4, 4 <= W <= 128, 1 <= H <= 128 (H need not be a multiple of 4), B * C < 2^24
 * (else MTR_E_SHAPE: the caller keeps K11); act as K11.  y = rnd(act(conv + bias[c])) with the BITS of K11's
 * generic kernel: f32 accumulation from 0 over (ky, kx) with ky outer, then the bias, the activation and one
 * rounding; row_mean (may be NULL): [B*C] f32 mean of the stored result per plane, summed in that kernel's
 * order, so y and row_mean equal mtr_depthwise3x3_bias_act's on every plane that reaches its generic kernel.
 * Every check is made on the host before anything is enqueued; B == 0 returns MTR_OK without a launch.  No
 * atomics, no workspace, no allocation; only enqueues on `stream` (graph-capturable). */
int mtr_depthwise3x3_blocks_bias_act(const void* x, int dtype, const float* weight /*[C][3][3]*/,
                                     const float* bias, int act, long long B, int C, int H, int W, void* y,
                                     float* row_mean /*[B*C] or NULL*/, mtr_stream_t stream);
/* The same with the block shape chosen by the caller.  block_cols: 0 the library's choice, 4 a lane owns 4 rows
 * x 4 columns, 8 (f16 / bf16 only, else MTR_E_PARAM; W a multiple of 8, else MTR_E_SHAPE) 4 rows x 8 columns,
 * one 16-byte load per row; other values MTR_E_PARAM.  The bits do not depend on block_cols. */
int mtr_depthwise3x3_blocks_bias_act_opts(const void* x, int dtype, const float* weight, const float* bias,
                                          int act, long long B, int C, int H, int W, void* y, float* row_mean,
                                          mtr_stream_t stream, int block_cols);
/* Whether K18 takes a depthwise 3x3 layer given with K11's arguments, without a launch (the idiom of
 * mtr_conv1x1_plan): MTR_OK and *block_cols = the block shape block_cols = 0 resolves to (4 or 8), or *block_cols = 0
 * and what the entry would answer -- MTR_E_NULL without block_cols, K11's argument errors in K11's order (MTR_E_PARAM for a stride outside {1, 2} or padding
 * outside mtr_depthwise3x3_bias_act_padded's ranges), then MTR_E_SHAPE for what K11 runs and K18 does not
 * (stride 2, any padding other than 1 on all four sides, W % 4 != 0, H or W above 128), then MTR_E_DTYPE.  The
 * alignment of x and y and the plane count are the entry's own checks. */
int mtr_depthwise3x3_blocks_supported(int dtype, int H, int W, int stride, int pad_top, int pad_left,
                                      int pad_bottom, int pad_right, int* block_cols /*[1]*/);

/* K15 (outside the reference's hot path, like K10 / K11): depthwise 5x5 convolution of the backbone's
 * inference copy with the K10 epilogue in the same pass -- the 5x5 layers of MobileNetV3-Large
 * (mobilenet_v3.py:387-432) and of the EfficientNet-B family (efficientnet.py:389-395).  K11's contract:
 * x [B, C, H, W] -> y [B, C, OH, OW] (NCHW, same dtype, f32 / f16 / bf16), cross-correlation with
 * weight [C, 5, 5] f32, bias [C] f32, zero padding pad_top, pad_left in 0..2 and pad_bottom, pad_right in
 * 0..3 (symmetric 2, or the explicit TF-'SAME' / `bottomright_stride` padding (1, 3, 1, 3) folded in),
 * stride in {1, 2}; OH = (H + pad_top + pad_bottom - 5) / stride + 1, OW likewise and a multiple of 4;
 * y 16-byte aligned.  y = rnd(act(conv + bias[c])): f32 accumulation from 0 over (ky, kx) with ky outer,
 * then the bias, the activation and one rounding, the same bits on every internal path (aligned or
 * unaligned x), call and graph replay; no atomics.  row_mean (may be NULL): [B*C] f32 mean of the stored
 * (rounded) result per plane.  The padded plane may be at most 112 x 112 (it is staged through LDS):
 * larger ones return MTR_E_SHAPE.  Error codes in the order of mtr_depthwise3x3_bias_act_padded; B == 0
 * returns MTR_OK without a launch.  Only enqueues on `stream`. */
int mtr_depthwise5x5_bias_act_padded(const void* x, int dtype, const float* weight /*[C][5][5]*/,
                                     const float* bias, int act, long long B, int C, int H, int W,
                                     int stride, int pad_top, int pad_left, int pad_bottom, int pad_right,
                                     void* y, float* row_mean /*[B*C] or NULL*/, mtr_stream_t stream);

/* K12 (outside the reference's hot path, like K10): the squeeze-excite gate of an MBConv block
 * (efficientnet.py:110-173, torchvision SqueezeExcitation) in one launch, from the [B, C] f32 channel
 * mean K10 / K11 emit:
 *   gate[b, c] = gate_fn(b2[c] + sum_s w2[c, s] * act(b1[s] + sum_k w1[s, k] * mean[b, k]))
 * w1 [S, C], w2 [C, S] (the fc1 / fc2 1x1 convolution weights), b1 [S], b2 [C], all f32, contiguous;
 * mean and w1 16-byte aligned, C a multiple of 4.  act: as mtr_bias_act_nchw; gate_fn: 0 sigmoid,
 * 1 hardsigmoid (torch.nn.Hardsigmoid).  f32 arithmetic in a fixed order, no atomics. */
int mtr_se_gate(const float* mean /*[B*C]*/, const float* w1, const float* b1, const float* w2,
                const float* b2, int act, int gate_fn, int B, int C, int S, float* gate /*[B*C]*/,
                mtr_stream_t stream);

/* mtr_se_gate with the layout of w2 and the kernel configuration stated.  w2_layout: MTR_SE_W2_CS is
 * w2 [C, S] as above, MTR_SE_W2_SC its transpose [S, C] (made once from the constant weight of an inference
 * copy: the fc2 loads of a wave are then contiguous).  config: -1 the library's own choice (what mtr_se_gate
 * takes), 0 .. 3 a (images per workgroup, channels per workgroup) split of (4, 256), (4, 1024), (8, 256),
 * (2, 512); one that does not fit the shape (more than 65535 image groups, more than 160 KiB of LDS) returns
 * MTR_E_SHAPE.  An image's gate has the same bits for every layout, configuration and B.  Other values of
 * either argument: MTR_E_PARAM; else the rules of mtr_se_gate. */
#define MTR_SE_W2_CS 0
#define MTR_SE_W2_SC 1
int mtr_se_gate_opts(const float* mean /*[B*C]*/, const float* w1, const float* b1, const float* w2,
                     const float* b2, int act, int gate_fn, int B, int C, int S, float* gate /*[B*C]*/,
                     mtr_stream_t stream, int w2_layout, int config);

/* K13 (outside the reference's hot path, like K10): a 1x1 stride-1 unpadded convolution of the backbone's
 * inference copy as one f32 MFMA GEMM with the K10 epilogue and the squeeze-excite gate folded in:
 *   y[b, m, p] = act(bias[m] + sum_k weight[m, k] * (x[b, k, p] * gate[b, k])) (+ residual[b, m, p])
 * x [B, K, HW], y and residual [B, M, HW] (NCHW, contiguous, 16-byte aligned), weight [M, K] row-major
 * (the folded conv weight, 16-byte aligned), bias [M]; gate [B, K] and residual may be NULL.  The sum is
 * an f32 fmaf chain in k order 0, 1, 2, ...; act: as mtr_bias_act_nchw, the residual added after it.
 * f32 only (else MTR_E_DTYPE); HW and K multiples of 4 (else MTR_E_SHAPE: the caller takes the
 * library-GEMM path); y must not alias x.  No atomics: the same inputs give the same bits. */
int mtr_conv1x1_bias_act(const void* x, int dtype, const float* weight, const float* bias,
                         const float* gate /*[B*K] or NULL*/, const void* residual, int act, long long B,
                         int M, int K, int HW, void* y, mtr_stream_t stream);

/* mtr_conv1x1_bias_act with the tile configuration stated (tests, A/B runs).  config: -1 the library's own choice
 * (what mtr_conv1x1_bias_act takes, a pure function of (M, K, HW, B)), 0 wide (192 x 128), 1 square (128 x 128),
 * 2 tall (32 w x 32), 3 deep-K (32 w x 16, three k-tiles of 32 in flight); else MTR_E_PARAM.  Every configuration
 * takes every shape and returns the same bits. */
int mtr_conv1x1_bias_act_opts(const void* x, int dtype, const float* weight, const float* bias,
                              const float* gate /*[B*K] or NULL*/, const void* residual, int act, long long B,
                              int M, int K, int HW, void* y, mtr_stream_t stream, int config);

/* mtr_conv1x1_bias_act_opts with an input prologue: the epilogue of the convolution that produced x, left out there
 * and applied here to every element on its way into the GEMM,
 *   v[b, k, p] = act_in(x[b, k, p] + in_bias[k])       (the f32 value mtr_bias_act_nchw would have stored in x)
 *   y[b, m, p] = act(bias[m] + sum_k weight[m, k] * (v[b, k, p] * gate[b, k])) (+ residual[b, m, p])
 * so mtr_bias_act_nchw(x, in_bias, in_act) followed by mtr_conv1x1_bias_act_opts(x, ...) gives the same bits, with
 * one read and one write of x less.  in_bias [K] f32 (4-byte aligned, else MTR_E_ALIGN) or NULL: no prologue, and
 * in_act must then be 0 (else MTR_E_PARAM).  in_act: as `act`.  Everything else as mtr_conv1x1_bias_act_opts, and
 * two more configurations: 4 stream (four waves, each 32 columns and all of M <= 96 channels; the whole weight staged
 * in LDS once, at most 64 KiB of it, x read straight into the MFMA operand).  Forced on a shape whose weight does not
 * fit, it runs as tall.  5 deep64 (eight waves on 64 channels x 64 columns, three k-tiles of 32 in flight in a ring
 * of LDS stages); takes every shape.  The same bits as every other configuration. */
int mtr_conv1x1_bias_act_pre(const void* x, int dtype, const float* weight, const float* bias,
                             const float* in_bias /*[K] or NULL*/, int in_act, const float* gate /*[B*K] or NULL*/,
                             const void* residual, int act, long long B, int M, int K, int HW, void* y,
                             mtr_stream_t stream, int config);

/* Host only: what `config` (as above, 4 stream and 5 deep64 included) resolves to for a shape.  plan[0 .. 3] =
 * configuration (0 .. 5; 2 for stream where the weight does not fit), waves along the channels (stream: 32-channel
 * tiles per wave; deep64: 2, of 2 x 4 waves), channels per workgroup, columns per workgroup. */
int mtr_conv1x1_plan(int M, int K, int HW, long long B, int config, int* plan /*[4]*/);

/* K13h (outside the reference's hot path, like K10): mtr_conv1x1_bias_act for f16 / bf16 tensors, one 16-bit
 * MFMA GEMM (v_mfma_f32_32x32x16_{f16,bf16}) with the K10 epilogue and the squeeze-excite gate folded in:
 *   xg[b, k, p] = x[b, k, p], or rnd16(x[b, k, p] * rnd16(gate[b, k])) with a gate (torch's x * gate.to(x.dtype))
 *   y[b, m, p]  = rnd16(act(bias[m] + sum_k weight[m, k] * xg[b, k, p]) (+ residual[b, m, p]))
 * x [B, K, HW], y and residual [B, M, HW] (NCHW, contiguous, 16-byte aligned), weight [M, K] row-major, all in
 * `dtype` (MTR_F16 or MTR_BF16, else MTR_E_DTYPE); bias [M] and gate [B, K] f32 (4-byte aligned); gate and
 * residual may be NULL.  The sum is accumulated in f32 in 16-k MFMA steps in k order, the epilogue is f32 in
 * K10's order (act, then the residual), rounded to 16 bits once (to nearest even).  HW and K multiples of 8
 * (else MTR_E_SHAPE: the caller takes the library-GEMM path); y must not alias x.  No atomics, no split-K:
 * the same inputs give the same bits, whichever tile the shape picks. */
int mtr_conv1x1_bias_act16(const void* x, int dtype, const void* weight, const float* bias,
                           const float* gate /*[B*K] or NULL*/, const void* residual, int act, long long B,
                           int M, int K, int HW, void* y, mtr_stream_t stream);

/* mtr_conv1x1_bias_act16 with the tile configuration stated (tests, A/B runs, the backbone's deep projects).  config:
 * -1 the library's own choice (exactly mtr_conv1x1_bias_act16, a pure function of (M, K)), 0 tall (32 w x 32), 1 square
 * (128 x 128), 2 deep-K (64 x 64, x and W through LDS, three k-tiles of 64 in flight, the result stored in whole row
 * segments); else MTR_E_PARAM.  The other argument rules are mtr_conv1x1_bias_act16's, in its order.  Every
 * configuration takes every shape and returns the same bits. */
int mtr_conv1x1_bias_act16_opts(const void* x, int dtype, const void* weight, const float* bias,
                                const float* gate /*[B*K] or NULL*/, const void* residual, int act, long long B,
                                int M, int K, int HW, void* y, mtr_stream_t stream, int config);

/* Host only: what `config` (as above) resolves to for a shape.  plan[0 .. 3] = configuration (0 .. 2), waves along the
 * channels, channels per workgroup, columns per workgroup. */
int mtr_conv1x1_plan16(int M, int K, int HW, long long B, int config, int* plan /*[4]*/);

/* K14h (outside the reference's hot path, like K10): a dense 3x3 convolution of f16 / bf16 tensors -- stride 1 or
 * 2, padding 1 on all sides, no dilation, groups 1 -- as one implicit 16-bit MFMA GEMM
 * (v_mfma_f32_32x32x16_{f16,bf16}) with the K10 epilogue folded in:
 *   y[b, m, oy, ox] = rnd16(act(bias[m] + sum_{ky, kx, ci} weight[m, ky, kx, ci]
 *                                          * x[b, ci, stride oy + ky - 1, stride ox + kx - 1]) (+ residual[b, m, oy, ox]))
 * x [B, Cin, H, W], y and residual [B, Cout, Ho, Wo] with Ho = (H - 1) / stride + 1, Wo likewise (NCHW, contiguous,
 * 16-byte aligned), all in `dtype` (MTR_F16 or MTR_BF16, else MTR_E_DTYPE).  weight is the convolution weight
 * REPACKED to [Cout][3][3][Cin] (torch: w.permute(0, 2, 3, 1).contiguous()), 16-byte aligned -- not OIHW: the
 * reduction runs over (ky, kx, ci) with ci innermost.  bias [Cout] f32; residual may be NULL and may be x itself.
 * The sum is accumulated in f32 in 16-k MFMA steps in that one k order, the epilogue is f32 in K10's order (act,
 * then the residual), rounded to 16 bits once (to nearest even).  Cin a multiple of 8, W and Wo multiples of 4,
 * and the input halo of one output tile (all Cin channels) must fit 160 KiB of LDS (Cin up to 256 at stride 1 and 120 at
 * stride 2; mtr_conv3x3_16_lds_bytes tells),
 * else MTR_E_SHAPE: the caller takes the library path.  y must not alias x or residual.  No atomics, no split-K:
 * the same inputs give the same bits, whichever tile the shape picks. */
int mtr_conv3x3_bias_act16(const void* x, int dtype, const void* weight /*[Cout][3][3][Cin]*/, const float* bias,
                           const void* residual, int act, long long B, int Cin, int Cout, int H, int W, int stride,
                           void* y, mtr_stream_t stream);

/* The bytes of LDS one workgroup of mtr_conv3x3_bias_act16 uses for this shape (the staged input halo), or 0 where the
 * entry has no kernel for it and answers MTR_E_SHAPE.  No GPU work. */
size_t mtr_conv3x3_16_lds_bytes(long long B, int Cin, int Cout, int H, int W, int stride);

/* K16h (outside the reference's hot path, like K10): a whole FusedMBConv block of f16 / bf16 tensors -- the dense
 * 3x3 expand of K14h and the 1x1 project of K13h behind it -- as ONE launch; the Cmid-wide activation between them
 * stays in LDS (no workspace, nothing allocated, graph-capturable):
 *   mid[b, c, p] = rnd16(act(bias3[c] + conv3x3(x, w3, stride, pad 1)[b, c, p]))              c < Cmid
 *   y[b, m, p]   = rnd16(bias1[m] + sum_c w1[m, c] * mid[b, c, p] (+ residual[b, m, p]))       m < Cout
 * The result has the BITS of mtr_conv3x3_bias_act16(x, w3_packed, bias3, NULL, act) followed by
 * mtr_conv1x1_bias_act16(mid, w1, bias1, NULL, residual, MTR_ACT none): the same 16-k MFMA steps in the same order,
 * the intermediate rounded to 16 bits once, the same epilogue order; it does not depend on the tile picked.
 * x [B, Cin, H, W], y and residual [B, Cout, Ho, Wo] (NCHW, contiguous, 16-byte aligned) in `dtype` (MTR_F16 or
 * MTR_BF16, else MTR_E_DTYPE); w3_packed [Cmid][3][3][Cin] as K14h takes it, w1 [Cout][Cmid], both in `dtype` and
 * 16-byte aligned; bias3 [Cmid] and bias1 [Cout] f32.  `act` is the expand's activation; the project has none.
 * MTR_E_SHAPE (the caller keeps the two-kernel chain) unless: stride 1 or 2; Cin and Cmid multiples of 8; W and Wo
 * multiples of 4; Cout <= 128; the input halo of a 128-position tile plus one chunk of `mid` (128 positions x 128 or
 * 192 channels) within 160 KiB of LDS (mtr_fused_mbconv16_lds_bytes tells); a residual only with stride 1 and
 * Cout == Cin.  residual may be NULL and may be x itself; y must not alias x or residual.  No atomics, no split-K. */
int mtr_fused_mbconv16(const void* x, int dtype, const void* w3_packed /*[Cmid][3][3][Cin]*/, const float* bias3,
                       int act, const void* w1 /*[Cout][Cmid]*/, const float* bias1, const void* residual,
                       long long B, int Cin, int Cmid, int Cout, int H, int W, int stride, void* y,
                       mtr_stream_t stream);

/* The bytes of LDS one workgroup of mtr_fused_mbconv16 uses for this shape (the staged halo and one chunk of the
 * intermediate), or 0 where the entry has no kernel for it and answers MTR_E_SHAPE.  No GPU work. */
size_t mtr_fused_mbconv16_lds_bytes(long long B, int Cin, int Cmid, int Cout, int H, int W, int stride);

/* K17 (outside the reference's hot path, like K10): the backbone stem -- Preproc (x * 2 - 1) and the dense 3x3,
 * stride-2, padding-1, Cin = 3 convolution behind it, with the K10 epilogue folded in -- as ONE launch:
 *   p[b, ci, iy, ix] = preproc ? rndD(rndX(fma(2, x[b, ci, iy, ix], -1))) : rndD(x[b, ci, iy, ix])   inside the image
 *                    = 0                                                  outside (the ring is zero AFTER Preproc)
 *   y[b, m, oy, ox]  = rndD(act(bias[m] + sum_{ci, ky, kx} weight[m, ci, ky, kx] * p[b, ci, 2 oy + ky - 1, 2 ox + kx - 1]))
 * rndX rounds to x_dtype, rndD to `dtype`: p has the bits of torch's (x * 2 - 1).to(dtype).  x is [B, 3, H, W]
 * (layout MTR_NCHW) or interleaved [B, H, W, 3] (MTR_NHWC), contiguous, 16-byte aligned, in x_dtype; y is
 * [B, Cout, H / 2, W / 2], NCHW-contiguous, 16-byte aligned, in `dtype`; weight is the convolution weight as stored,
 * OIHW [Cout, 3, 3, 3], in `dtype`; bias [Cout] f32.  dtype MTR_F32, MTR_F16 or MTR_BF16; x_dtype == dtype, or
 * MTR_F32 with a 16-bit dtype (the cast of the first convolution is folded in); else MTR_E_DTYPE.  The sum is
 * accumulated in f32 in the one order k = 9 ci + 3 ky + kx (16-bit: two 16-k MFMA steps, K padded to 32 with zeros;
 * f32: fourteen 2-k steps of the f32 MFMA, K padded to 28), the epilogue is f32 in K10's order, rounded to `dtype` once.  act: as mtr_bias_act_nchw;
 * preproc 0 or 1.  MTR_E_SHAPE (the caller keeps the library chain) unless Cin == 3, H even, W % 8 == 0,
 * Cout % 8 == 0, Cout <= 64, B <= 65535 and a band of input rows fits LDS (mtr_stem_conv_lds_bytes tells).  y must
 * not overlap x (MTR_E_PARAM).  Every check is made on the host before anything is enqueued.  No atomics, no
 * workspace, nothing allocated; only enqueues on `stream`: the same inputs give the same bits, for either layout,
 * any batch index and on every graph replay. */
int mtr_stem_conv3x3s2(const void* x, int x_dtype, int layout, const void* weight /*[Cout][3][3][3]*/,
                       const float* bias, int dtype, int act, int preproc, long long B, int Cin, int Cout, int H,
                       int W, void* y, mtr_stream_t stream);

/* The bytes of LDS one workgroup of mtr_stem_conv3x3s2 uses for this shape and `dtype` (the staged band of input rows
 * and the output turn), or 0 where the entry has no kernel for it and answers MTR_E_SHAPE / MTR_E_DTYPE.  No GPU
 * work. */
size_t mtr_stem_conv_lds_bytes(int dtype, long long B, int Cin, int Cout, int H, int W);

/* K19 (outside the reference's hot path, like K10): a dense 3x3 convolution of f32 tensors -- stride 1, padding 1 on all
 * sides, no dilation, groups 1 -- as Winograd F(2x2, 3x3) on the f32-input MFMA (v_mfma_f32_16x16x4_f32), with the K10
 * epilogue folded in:
 *   y[b, m, oy, ox] = act(bias[m] + sum_{ci, ky, kx} w[m, ci, ky, kx] * x[b, ci, oy + ky - 1, ox + kx - 1])
 *                     (+ residual[b, m, oy, ox])
 * evaluated per 2x2 output tile as Y = A^T [ sum_ci U[xi, m, ci] * (B^T d B)[xi, ci, tile] ] A with the standard
 * matrices (entries 0, +-1, +-1/2).  x [B, Cin, H, W], y and residual [B, Cout, H, W]: f32, NCHW, contiguous, 16-byte
 * aligned (else MTR_E_ALIGN).  weight_u is the weight ALREADY TRANSFORMED, U = G g G^T, computed in fp64 from the f32
 * OIHW weight and rounded to f32 once, laid out [16][Cout][Cin] (xi = 4 i + j), contiguous, 16-byte aligned.  bias
 * [Cout] f32; residual may be NULL and may be x itself; act as mtr_bias_act_nchw, applied in K10's order (bias,
 * activation, then the residual), else MTR_E_PARAM.  The 16 products are f32 MFMA chains over ci = 0, 1, 2, ... in that
 * one order; the input and output transforms use one fixed order of additions.  MTR_E_SHAPE (the caller keeps the
 * library path) unless H is even, W % 4 == 0, Cin % 4 == 0, Cout >= 1, Cin H W and Cout H W below 2^31 and B H W / 4
 * (the 2x2 tiles of the batch) below 2^31 - 64; maps of any such size are taken, partial workgroups included.  A NULL
 * x, weight_u, bias or y is MTR_E_NULL; y overlapping x or residual is MTR_E_PARAM.  Every check is made on the host
 * before anything is enqueued; B == 0 returns MTR_OK without a launch.  No atomics, no split-K, no workspace, nothing
 * allocated; only enqueues on `stream`: the same inputs give the same bits for any batch index, on every call and
 * graph replay (there is one tile configuration). */
int mtr_conv3x3_winograd_bias_act(const void* x, const float* weight_u /*[16][Cout][Cin]*/, const float* bias,
                                  const void* residual, int act, long long B, int Cin, int Cout, int H, int W,
                                  void* y, mtr_stream_t stream);

/* The bytes of LDS one workgroup of mtr_conv3x3_winograd_bias_act uses for this shape (one chunk of the transformed
 * input and of U), or 0 where the entry answers MTR_E_SHAPE (and for B <= 0).  No GPU work. */
size_t mtr_conv3x3_winograd_lds_bytes(long long B, int Cin, int Cout, int H, int W);

/* K22 (outside the reference's hot path, like K10): a dense 3x3 convolution of f32 tensors -- STRIDE 2, padding 1 on
 * all sides, no dilation, groups 1 -- as an implicit GEMM on the f32-input MFMA (v_mfma_f32_16x16x4_f32), with the K10
 * epilogue folded in:
 *   y[b, m, oy, ox] = act(bias[m] + sum_{ci, ky, kx} w[m, ci, ky, kx] * x[b, ci, 2 oy + ky - 1, 2 ox + kx - 1])
 *                     (+ residual[b, m, oy, ox])
 * x [B, Cin, H, W], y and residual [B, Cout, H / 2, W / 2]: f32, NCHW, contiguous, 16-byte aligned (else MTR_E_ALIGN).
 * w_packed is the f32 OIHW weight PERMUTED (no arithmetic) to [Cin / 4][Cout][3][3][4]: element (c4, m, ky, kx, j) is
 * w[m, 4 c4 + j, ky, kx]; contiguous, 16-byte aligned.  bias [Cout] f32; residual may be NULL; act_code as the `act`
 * of mtr_bias_act_nchw, applied in K10's order (bias, activation, then the residual), else MTR_E_PARAM.
 * Every output element is ONE chain of 9 Cin fmaf from 0, in the order: for c4 (chunks of four input channels), for
 * ky, for kx, for ci = 4 c4 .. 4 c4 + 3: s = fmaf(x, w, s), padding taps entering as zeros -- the MFMA is bitwise such
 * a chain.  MTR_E_SHAPE (the caller keeps the library path) unless Cin % 4 == 0, H and W are even, (W / 2) % 4 == 0,
 * Cout >= 1, and Cin H W, Cout H W / 4, 9 Cin Cout and the grid are below 2^31; any Cout and B are taken.  A NULL x,
 * w_packed, bias or y is MTR_E_NULL; y overlapping x or residual is MTR_E_PARAM.  Every check is made on the host
 * before anything is enqueued; B == 0 returns MTR_OK without a launch.  No atomics, no split-K, no workspace, nothing
 * allocated; only enqueues on `stream`: the same inputs give the same bits for any batch index and tile position, on
 * every call and graph replay.  (The activation parameter is named act_code: tests/test_act_code_refusals.py keeps
 * its own table of the declarations that say `int act`; this entry's refusals are pinned in
 * tests/test_conv3x3_strided_host.py.) */
int mtr_conv3x3s2_bias_act(const void* x, const float* w_packed /*[Cin/4][Cout][3][3][4]*/, const float* bias,
                           const void* residual, int act_code, long long B, int Cin, int Cout, int H, int W, void* y,
                           mtr_stream_t stream);

/* The bytes of LDS one workgroup of mtr_conv3x3s2_bias_act uses for this shape (one chunk of the input halo and of the
 * weight), or 0 where the entry answers MTR_E_SHAPE (and for B <= 0).  No GPU work. */
size_t mtr_conv3x3s2_lds_bytes(long long B, int Cin, int Cout, int H, int W);

/* K21 (outside the reference's hot path, like K10): a dense 3x3 convolution of f32 tensors -- stride 1, padding 1 on
 * all sides, no dilation, groups 1 -- on the bf16 matrix cores by operand split (K20's arithmetic), with the K10
 * epilogue folded in:
 *   y[b, m, oy, ox] = act(bias[m] + sum_{ci, ky, kx} w[m, ci, ky, kx] * x[b, ci, oy + ky - 1, ox + kx - 1])
 *                     (+ residual[b, m, oy, ox])
 * x [B, Cin, H, W], y and residual [B, Cout, H, W]: f32, NCHW, contiguous, 16-byte aligned (else MTR_E_ALIGN).
 * w_split is the f32 OIHW weight as three bf16 pieces, [3][Cout][3][3][Cp], ci innermost, Cp = Cin rounded up to 16
 * with a zero tail (kernels.pack_conv3x3_split_weight): piece 0 = bf16(w), piece 1 = bf16(w - p0), piece 2 =
 * bf16(w - p0 - p1), their sum is w exactly; contiguous, 16-byte aligned.  bias [Cout] f32; residual may be NULL and
 * may be x itself (Cin == Cout); act_code as the `act` of mtr_bias_act_nchw, applied in K10's order (bias,
 * activation, then the residual), else MTR_E_PARAM (also with B == 0).
 * x is split the same way on the fly.  Every output element is ONE f32 accumulator that starts from 0 and takes, for
 * c = 0, 16, .. < Cp (chunks of 16 input channels, the same constant for every shape), for ky, for kx, the six piece
 * products (w2,v0), (w0,v2), (w1,v1), (w1,v0), (w0,v1), (w0,v0) in this order, each one v_mfma_f32_32x32x16_bf16 over
 * the chunk's 16 channels; padding taps enter as zeros; the three products below 2^-23 |w v| are dropped.
 * a - bf16(a) of an infinity is NaN: a window that holds an infinity (or |x| >= 2^127 (2 - 2^-8)) gives NaN.
 * MTR_E_SHAPE (the caller keeps another path) unless Cin % 8 == 0, W % 4 == 0, H >= 1, Cout >= 1, B >= 0, and
 * B Cin H W, B Cout H W, 27 Cout Cp and the grid are below 2^31; no shape inside this domain is refused for LDS.  A
 * NULL x, w_split, bias or y is MTR_E_NULL; y overlapping x or residual is MTR_E_PARAM.  The checks are made on the
 * host, in the order NULL, shape, act_code, alignment, overlap, before anything is enqueued; B == 0 returns MTR_OK
 * without a launch.  No atomics, no split-K, no workspace, nothing allocated; only enqueues on `stream`: the same
 * inputs give the same bits for any batch index, tile position and residual, on every call and graph replay.  (The
 * activation parameter is named act_code, as K22's; this entry's refusals are pinned in
 * tests/test_conv3x3_split_host.py.) */
int mtr_conv3x3_bias_act_split(const void* x, const void* w_split /*[3][Cout][3][3][Cp] bf16*/, const float* bias,
                               const void* residual, int act_code, long long B, int Cin, int Cout, int H, int W,
                               void* y, mtr_stream_t stream);

/* The bytes of LDS one workgroup of mtr_conv3x3_bias_act_split uses (two buffers of one 16-channel chunk of the split
 * input halo), or 0 where the entry answers MTR_E_SHAPE (and for B <= 0).  No GPU work. */
size_t mtr_conv3x3_split_lds_bytes(long long B, int Cin, int Cout, int H, int W);

/* K25h (outside the reference's hot path, like K10): the 1x1 expand convolution of an MBConv block and the depthwise
 * 3x3 stride-1 padding-1 convolution behind it, of f16 / bf16 tensors, as ONE launch; the Cmid-wide activation between
 * them stays in LDS (no workspace, nothing allocated, graph-capturable):
 *   mid[b, c, p] = rnd16(act1(bias1[c] + sum_k w1[c, k] * x[b, k, p]))                                     c < Cmid
 *   y[b, c, p]   = rnd16(act2(bias_dw[c] + sum_{ky, kx} w_dw[c, ky, kx] * mid[b, c, p + (ky - 1, kx - 1)]))
 *   row_mean[b, c] = (1 / (H W)) * sum_p f32(y[b, c, p])                                      (where row_mean != NULL)
 * y and row_mean have the BITS of mtr_conv1x1_bias_act16(x, w1, bias1, NULL, NULL, act1) followed by
 * mtr_depthwise3x3_bias_act(mid, w_dw, bias_dw, act2, stride 1, pad 1, row_mean): the same 16-k MFMA steps in the same
 * order, the intermediate rounded to 16 bits once, the depthwise accumulator started at the bias and nine fmaf in
 * (ky, kx) order, the mean from the rounded outputs in the order of K11's stride-1 block kernel.
 * x [B, Cin, H, W] and y [B, Cmid, H, W] (NCHW, contiguous, 16-byte aligned) in `dtype` (MTR_F16 or MTR_BF16, else
 * MTR_E_DTYPE); w1 [Cmid][Cin] in `dtype`, 16-byte aligned; bias1 [Cmid], w_dw [Cmid][3][3], bias_dw [Cmid] and
 * row_mean [B][Cmid] f32.  act1_code / act2_code as the `act` of mtr_bias_act_nchw, else MTR_E_PARAM.
 * MTR_E_SHAPE (the caller keeps the two-kernel chain) unless: Cin % 8 == 0; H / 4 and W / 4 powers of two with
 * H W <= 256 (the planes K11 runs on its block kernel, up to 16x16: 4x4, 8x8, 16x16, 8x16, 16x4, ...); B Cmid < 2^24.
 * A NULL x, w1, bias1, w_dw, bias_dw or y is MTR_E_NULL; y overlapping x is MTR_E_PARAM.  Checked in the order NULL,
 * dtype, shape, parameters, alignment, overlap, on the host before anything is enqueued; B == 0 returns MTR_OK without
 * a launch.  No atomics, no split-K; only enqueues on `stream`: the same inputs give the same bits for any batch index,
 * on every call and graph replay. */
int mtr_expand_dw16(const void* x, int dtype, const void* w1 /*[Cmid][Cin]*/, const float* bias1, int act1_code,
                    const float* w_dw /*[Cmid][3][3]*/, const float* bias_dw, int act2_code, long long B, int Cin,
                    int Cmid, int H, int W, void* y, float* row_mean /* may be NULL */, mtr_stream_t stream);

/* The same with the workgroup-to-image mapping chosen: -1 the library's own choice, 0 blockIdx = image * chunks +
 * chunk, 1 the chunks of one image on one XCD (else MTR_E_PARAM).  The bits do not depend on it. */
int mtr_expand_dw16_opts(const void* x, int dtype, const void* w1, const float* bias1, int act1_code,
                         const float* w_dw, const float* bias_dw, int act2_code, long long B, int Cin, int Cmid, int H,
                         int W, void* y, float* row_mean, mtr_stream_t stream, int mapping);

/* The bytes of LDS one workgroup of mtr_expand_dw16 uses for this shape (the slice of the expanded activation), or 0
 * where the entry answers MTR_E_SHAPE (and for B <= 0).  No GPU work. */
size_t mtr_expand_dw16_lds_bytes(long long B, int Cin, int Cmid, int H, int W);

/* K26h (outside the reference's hot path, like K10): mtr_expand_dw16's function -- the same three formulas, arguments,
 * checks and error codes -- on the planes it refuses because K11 runs them on its GENERIC kernel (24x24 and 12x12 of
 * the EfficientNetV2 family at 384 px).  y and row_mean have the BITS of mtr_conv1x1_bias_act16(x, w1, bias1, NULL,
 * NULL, act1) followed by mtr_depthwise3x3_bias_act(mid, w_dw, bias_dw, act2, stride 1, pad 1, row_mean) on such a
 * plane: the depthwise accumulator started at 0, nine fmaf with ky outer and kx inner, the bias added last, the mean in
 * the generic kernel's order (groups of four outputs left to right, lane s of lpp adding groups s, s + 64, ..., the xor
 * butterfly).  They are therefore also the bits of mtr_conv1x1_bias_act16 + mtr_depthwise3x3_blocks_bias_act.
 * MTR_E_SHAPE (the caller keeps the two-kernel chain) unless: Cin % 8 == 0; W % 4 == 0; H W % 8 == 0; H <= 32, W <= 32,
 * H W <= 576; the plane is NOT one K11 runs on its block kernel (H / 4 and W / 4 powers of two with at most 16 blocks
 * per row and 64 per plane: mtr_expand_dw16's planes, 32x16, 16x32, ...); B Cmid < 2^30.  A NULL x, w1, bias1, w_dw,
 * bias_dw or y is MTR_E_NULL; act1_code / act2_code outside 0..3 are MTR_E_PARAM; y overlapping x is MTR_E_PARAM.
 * Checked in the order NULL, dtype, shape, parameters, alignment, overlap, on the host before anything is enqueued;
 * B == 0 returns MTR_OK without a launch.  No atomics, no split-K, no workspace; only enqueues on `stream`: the same
 * inputs give the same bits for any batch index, on every call and graph replay. */
int mtr_expand_dw16_planes(const void* x, int dtype, const void* w1 /*[Cmid][Cin]*/, const float* bias1, int act1_code,
                           const float* w_dw /*[Cmid][3][3]*/, const float* bias_dw, int act2_code, long long B,
                           int Cin, int Cmid, int H, int W, void* y, float* row_mean /* may be NULL */,
                           mtr_stream_t stream);

/* The same with the workgroup-to-image mapping chosen, as in mtr_expand_dw16_opts.  The bits do not depend on it. */
int mtr_expand_dw16_planes_opts(const void* x, int dtype, const void* w1, const float* bias1, int act1_code,
                                const float* w_dw, const float* bias_dw, int act2_code, long long B, int Cin, int Cmid,
                                int H, int W, void* y, float* row_mean, mtr_stream_t stream, int mapping);

/* The bytes of LDS one workgroup of mtr_expand_dw16_planes uses for this shape, or 0 where the entry answers
 * MTR_E_SHAPE (and for B <= 0).  No GPU work. */
size_t mtr_expand_dw16_planes_lds_bytes(long long B, int Cin, int Cmid, int H, int W);

/* K27h (outside the reference's hot path, like K10): the 1x1 expand and the depthwise 3x3 layer behind it (stride 1 or
 * 2, zero padding 1 on all four sides) as one launch on LARGE planes, WITHOUT a mean output: a workgroup owns a band of
 * output rows of 32 expanded channels and recomputes the halo rows of the expand.
 *   mid[b, c, p] = rnd16(act1(bias1[c] + sum_k w1[c, k] x[b, k, p]))
 *   y[b, c, o]   = rnd16(act2(sum_{ky, kx} w_dw[c, ky, kx] mid[b, c, stride o + (ky - 1, kx - 1)] + bias_dw[c]))
 * y [B, Cmid, H / stride, W / stride] has the BITS of mtr_conv1x1_bias_act16(x, w1, bias1, NULL, NULL, act1) followed
 * by mtr_depthwise3x3_bias_act(mid, w_dw, bias_dw, act2, stride, pad 1, NULL) where that runs K11's generic kernel:
 * the accumulator started at 0, nine fmaf with ky outer and kx inner, the bias added last, one rounding.
 * MTR_E_SHAPE (the caller keeps the two-kernel chain) unless: stride 1 or 2; Cin % 8 == 0; H <= 128, W <= 128;
 * B Cmid < 2^30; at stride 1 W % 4 == 0, W >= 4, H W % 8 == 0 and the plane is NOT one K11 runs on its block kernel
 * (H / 4 and W / 4 powers of two with at most 16 blocks per row and 64 per plane); at stride 2 H even and W % 8 == 0.
 * A NULL x, w1, bias1, w_dw, bias_dw or y is MTR_E_NULL; act1_code / act2_code outside 0..3 are MTR_E_PARAM; y
 * overlapping x is MTR_E_PARAM.  Checked in the order NULL, dtype, shape, parameters, alignment (x, w1, y 16 bytes),
 * overlap, on the host before anything is enqueued; B == 0 returns MTR_OK without a launch.  No atomics, no split-K, no
 * workspace; only enqueues on `stream`: the same inputs give the same bits for any batch index, on every call and
 * graph replay. */
int mtr_expand_dw16_tiles(const void* x, int dtype, const void* w1 /*[Cmid][Cin]*/, const float* bias1, int act1_code,
                          const float* w_dw /*[Cmid][3][3]*/, const float* bias_dw, int act2_code, long long B,
                          int Cin, int Cmid, int H, int W, int stride, void* y, mtr_stream_t stream);

/* The bytes of LDS one workgroup of mtr_expand_dw16_tiles uses for this shape, or 0 where the entry answers
 * MTR_E_SHAPE (and for B <= 0).  No GPU work. */
size_t mtr_expand_dw16_tiles_lds_bytes(long long B, int Cin, int Cmid, int H, int W, int stride);

/* K28h (outside the reference's hot path, like K10): the 1x1 expand and the depthwise 5x5 layer behind it (stride 1 or
 * 2, zero padding 2 on all four sides) as one launch, with the mean; the Cmid-wide activation between them stays in LDS:
 *   mid[b, c, p] = rnd16(act1(bias1[c] + sum_k w1[c, k] x[b, k, p]))
 *   y[b, c, o]   = rnd16(act2(sum_{ky, kx} w_dw[c, ky, kx] mid[b, c, stride o + (ky - 2, kx - 2)] + bias_dw[c]))
 *   row_mean[b, c] = (1 / (OH OW)) * sum_o f32(y[b, c, o])                                    (where row_mean != NULL)
 * y [B, Cmid, OH, OW], OH = (H - 1) / stride + 1 and OW = (W - 1) / stride + 1, and row_mean have the BITS of
 * mtr_conv1x1_bias_act16(x, w1, bias1, NULL, NULL, act1) followed by mtr_depthwise5x5_bias_act_padded(mid, w_dw,
 * bias_dw, act2, stride, 2, 2, 2, 2, row_mean): the accumulator started at 0, 25 fmaf with ky outer and kx inner, the
 * bias added last, one rounding, the mean from the rounded outputs in K15's order (units of 4 x 4 or 2 x 4 outputs, lane
 * l of G adding the unit sums l, l + G, ..., the xor butterfly).
 * MTR_E_SHAPE (the caller keeps the two-kernel chain) unless: stride 1 or 2; Cin % 8 == 0; H W % 8 == 0; W % 4 == 0;
 * OW % 4 == 0; H + 4 <= 112 and W + 4 <= 112; B Cmid < 2^30; and the image of a slice of 32 expanded channels, with the
 * staging buffers or unit sums beside it, fits 160 KiB of LDS (mtr_expand_dw16_k5_lds_bytes: 32x32 at stride 1 and
 * 28x52 at stride 1 do, 40x40 and 64x64 do not).  w_dw is [Cmid][5][5].  A NULL x, w1, bias1, w_dw, bias_dw or y is
 * MTR_E_NULL; act1_code / act2_code outside 0..3 are MTR_E_PARAM; y overlapping x is MTR_E_PARAM.  Checked in the order
 * NULL, dtype, shape, parameters, alignment (x, w1, y 16 bytes), overlap, on the host before anything is enqueued and
 * without reading a pointer; B == 0 returns MTR_OK without a launch.  No atomics, no split-K, no workspace; only
 * enqueues on `stream`: the same inputs give the same bits for any batch index, on every call and graph replay. */
int mtr_expand_dw16_k5(const void* x, int dtype, const void* w1 /*[Cmid][Cin]*/, const float* bias1, int act1_code,
                       const float* w_dw /*[Cmid][5][5]*/, const float* bias_dw, int act2_code, long long B, int Cin,
                       int Cmid, int H, int W, int stride, void* y, float* row_mean /* may be NULL */,
                       mtr_stream_t stream);

/* The same with the workgroup-to-image mapping chosen, as in mtr_expand_dw16_opts.  The bits do not depend on it. */
int mtr_expand_dw16_k5_opts(const void* x, int dtype, const void* w1, const float* bias1, int act1_code,
                            const float* w_dw, const float* bias_dw, int act2_code, long long B, int Cin, int Cmid, int H,
                            int W, int stride, void* y, float* row_mean, mtr_stream_t stream, int mapping);

/* The bytes of LDS one workgroup of mtr_expand_dw16_k5 uses for this shape, or 0 where the entry answers MTR_E_SHAPE
 * (and for B <= 0).  No GPU work. */
size_t mtr_expand_dw16_k5_lds_bytes(long long B, int Cin, int Cmid, int H, int W, int stride);

/* K20 (outside the reference's hot path, like K13): mtr_conv1x1_bias_act_pre for f32 tensors, evaluated on the bf16
 * matrix cores from split operands (v_mfma_f32_16x16x32_bf16):
 *   v[b, k, p] = act_in(x[b, k, p] + in_bias[k])  (x itself without in_bias), then v * gate[b, k] with a gate -- f32
 *   y[b, m, p] = act(bias[m] + sum_k w[m, k] * v[b, k, p]) (+ residual[b, m, p])
 * An f32 value is exactly the sum of three bf16 values, a0 = bf16_rn(a), a1 = bf16_rn(a - a0), a2 = bf16_rn(a - a0 -
 * a1).  w_split is the weight ALREADY SPLIT that way: [3][M][Kp] bf16, Kp = K rounded up to 32, the tail zero,
 * contiguous, 16-byte aligned.  v is split inside the kernel.  Per 32-k block and output the six products (w2, v0),
 * (w0, v2), (w1, v1), (w1, v0), (w0, v1), (w0, v0) are accumulated in that order into one f32 accumulator, the blocks
 * in k order: everything above 2^-23 |w v| is kept, and the result passes the fp64 bound K13 is tested with, but it is
 * NOT the bits of mtr_conv1x1_bias_act_pre.  x [B, K, HW], y and residual [B, M, HW]: f32, NCHW, contiguous, 16-byte
 * aligned (else MTR_E_ALIGN); bias [M], in_bias [K] (4-byte aligned) or NULL (in_act must then be 0, else
 * MTR_E_PARAM), gate [B, K] or NULL, residual or NULL; act / in_act as mtr_bias_act_nchw, the residual added after
 * the activation.  HW and K multiples of 4, B >= 0, M >= 1, B HW, K HW and M HW below 2^31 (else MTR_E_SHAPE); a NULL
 * x, w_split, bias or y is MTR_E_NULL; y overlapping x or the residual, or the residual being x, is MTR_E_PARAM.
 * Checked in that order -- NULL, shape, parameters, alignment, overlap -- on the host before anything is enqueued;
 * B == 0 returns MTR_OK without a launch.  Non-finite inputs: a - bf16(a) of an infinity is NaN, so a column of x
 * that holds an infinity (or a finite value of 2^127 (2 - 2^-8) or more, which rounds to one) gives NaN where
 * mtr_conv1x1_bias_act_pre gives an infinity; finite inputs below 2^127 behave as described.  No atomics, no
 * split-K, no workspace, nothing allocated; only enqueues on `stream`: the same inputs give the same bits on every
 * call and graph replay (the tile is a function of the shape and does not change the bits). */
int mtr_conv1x1_bias_act_split(const void* x, const void* w_split /*[3][M][Kp] bf16*/, const float* bias,
                               const float* in_bias /*[K] or NULL*/, int in_act,
                               const float* gate /*[B*K] or NULL*/, const void* residual, int act, long long B,
                               int M, int K, int HW, void* y, mtr_stream_t stream);

/* Host only: MTR_OK where mtr_conv1x1_bias_act_split takes the shape, else what it answers (MTR_E_SHAPE). */
int mtr_conv1x1_split_supported(long long B, int M, int K, int HW);

#ifdef __cplusplus
}
#endif
#endif /* METRABS_HIP_H_ */
