/*
 * lightplane_hip.h -- C ABI of liblightplane_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary of the Renderer / Splatter hot path.  Every entry
 * point replaces one Triton kernel launch site of the reference
 * (facebookresearch/lightplane @ 2024-08-07):
 *
 *   lp_renderer_forward   <- LightplaneFunction.forward  fw_kernel[grid](...)
 *                            lightplane/lightplane_renderer.py:505-555
 *                            (kernel: lightplane/triton_src/templates/renderer_fw.py:85-375)
 *   lp_renderer_backward  <- LightplaneFunction.backward bw_kernel[grid](...)
 *                            lightplane/lightplane_renderer.py:657-711
 *                            (kernel: lightplane/triton_src/templates/renderer_bw.py:89-627)
 *   lp_splatter_forward   <- LightplaneSplatterFunction.forward, BOTH launches
 *                            (features :505 and unit weights :507-539 in one march)
 *                            lightplane/lightplane_splatter.py:503-539
 *                            (kernels: templates/splatter_fw.py:71-165, :168-309 with MLP)
 *   lp_splatter_normalize <- weight clamp + divide, lightplane_splatter.py:541,584
 *   lp_splatter_backward  <- LightplaneSplatterFunction.backward bw_kernel[grid](...)
 *                            lightplane/lightplane_splatter.py:608,664
 *                            (kernels: templates/splatter_bw.py:75-180, :183-394 with MLP)
 *   lp_hash_randn         <- int_to_randn_kernel, triton_src/shared/rand_util.py:20-35
 *
 * Conventions
 *   - plain C: raw device pointers + host integers; no torch / C++ types.
 *   - the library never allocates device memory and keeps no state besides a
 *     thread-local error string; the caller owns every buffer.
 *   - all tensors are fp32, contiguous, resident on the device of `stream`.
 *   - every non-NULL device pointer of LpRendererArgs, LpSplatterArgs and LpRayEmbedArgs (per-grid
 *     LpGrid.data and the gradient lists included) and `feature` / `weight` of
 *     lp_splatter_normalize is 16-byte aligned: the kernels read and write caller memory
 *     16 and 8 bytes at a time.  Checked on the host for every pointer, whatever n_rays
 *     is, before anything touches the device: LP_EINVAL, the message names the field.
 *     Row offsets inside a flat grid tensor are not pointers and carry no such rule.
 *     (hipMalloc and every framework allocator return at least 256-byte alignment; what
 *     needs care is a view at an element offset into a larger buffer: copy it.)  The
 *     lp_grid_tv_* and lp_grid_resample_* entry points take any 4-byte-aligned grid (scalar path when under-aligned).
 *   - accumulation targets (grad_*, splat feature/weight grids) MUST be zeroed by
 *     the caller: kernels accumulate with atomics (reference does the same:
 *     lightplane_renderer.py:470-476, 642-651; lightplane_splatter.py:404-410).
 *   - every function returns 0 on success, a negative LP_E* code on invalid
 *     arguments, or the positive hipError_t of a failed launch; lp_last_error()
 *     describes the last failure of the calling thread.
 *   - `stream` is a hipStream_t (NULL = default stream).  Calls are asynchronous.
 *
 * Grid-list layout (reference lightplane/misc_utils.py:25-46): one flat
 * [sum_g B*D_g*H_g*W_g, C] channels-last tensor; grid g begins at row
 * grids[g].row_offset, cell (b,z,y,x) is row ((b*D+z)*H+y)*W+x inside it.
 * Coordinates: x<->W, y<->H, z<->D; a grid with exactly one singleton spatial
 * dim is a plane sampled bilinearly (D==1: xy, H==1: xz, W==1: yz).
 *
 * MLP parameter layout (reference lightplane/mlp_utils.py:390-456): see LpMlp.
 */
#ifndef LIGHTPLANE_HIP_H
#define LIGHTPLANE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LP_VERSION 207 /* 0.2.0: per-grid base pointers (zero-copy grid-lists), fused bg-colour / alpha epilogue,
                           ray-embedding entry points; grad replicas removed
                           0.2.1: segment-parallel backward for small batches (LpRendererArgs.seg_prefix)
                           0.2.2: no struct change; lp_*_kernel_family() report family 3 (layer-looped MFMA kernels: Renderer
                                  decoders of 1-4 layers per MLP / up to 32 colour channels, MLP-Splatter of 2-4 layers and
                                  widths 16 / 32 / 64), 64-channel Splatter walks
                           0.2.3: no struct change; 64-channel Renderer grid-lists on family 3; the Renderer's family 1 is the tuned
                                  default decoder shape only (every other shallow shape reports 3), lp_splatter_kernel_family() no
                                  longer returns 2; lp_version() was negative for a library built with experiment switches (since
                                  retired: every build returns LP_VERSION)
                           0.2.4: no struct change; lp_renderer_kernel_family() no longer returns 2 (2/2/2 x 64 decoders run the
                                  layer-looped family's two-block kernels and report 3); family 3 takes up to 256 beyond-far samples
                                  and two-grid decoders of hidden width 64 (heads of at most 2 layers, 16 / 32 grid channels)
                           0.2.5: no struct change; new test hook lp_renderer_backward_relu_dump(); the dX chains of the MFMA
                                  backwards take the gradient operand as two bf16 limbs
                           0.2.6: LpRendererArgs.arithmetic (LP_ARITH_FP32: every product of the backward fp32-equivalent, selectable
                                  per call); lp_build_info(); lp_renderer_relu_dump_words() and dump twins for the layer-looped
                                  family (the dump of family 1 keeps its five words per sample); LpRendererArgs.march_order
                                  (LP_MARCH_SAMPLES_PER_WAVE: transposed march of the tuned backward for incoherent ray batches)
                           0.2.7: no struct change; LP_SEG_LEN 16 -> 8: LpRendererArgs.seg_prefix holds a record per 8 samples
                                  (lp_renderer_backward_segments() returns ceil(S / 8) for a small batch): batches of up to ~2 000 rays
                                  are dealt to the CUs in 8-sample segments, larger ones in 16-sample segments as before; the MFMA
                                  families take grid-lists of any byte size below 2^31 rows (were: below 4 GB); later, without a
                                  version change (additive: no struct or behaviour change, every existing entry point as before):
                                  the MLP-Splatter test hooks lp_mlp_splatter_backward_relu_dump() and
                                  lp_mlp_splatter_relu_dump_words(), the launch-shape query lp_mlp_splatter_launch_shape(); the total-variation
                                  regulariser of a grid-list, lp_grid_tv_workspace_bytes() / _forward() / _backward() / _fused()
                                  (lp_build_info() then has a "grid_tv" entry)
                                  later still, again without a version change (no struct change; every call whose pointers come from an
                                  allocator answers as before): a device pointer of LpRendererArgs / LpSplatterArgs / LpRayEmbedArgs or
                                  of lp_splatter_normalize() that is not 16-byte aligned is refused with LP_EINVAL (Conventions above;
                                  the kernels always assumed it, nothing checked it); and, additive again: resampling of a grid-list
                                  to new spatial sizes, lp_grid_resample_forward() / _backward() (lp_build_info() then has a
                                  "grid_resample" entry)
                                  and once more without a version change (additive: a new struct and three new entry points, nothing
                                  existing touched): the occupancy scaffold of a grid-list, LpScaffoldArgs with
                                  lp_scaffold_workspace_bytes() / lp_scaffold_opacity() / lp_scaffold_build() (lp_build_info() then
                                  has a "scaffold" entry; lp_abi_sizeof(8) answers for the new struct)
                                  and again (additive: a new struct and two new entry points): the decoder at arbitrary points,
                                  LpPointsArgs with lp_points_forward() / lp_points_backward() (lp_build_info() then has a "points"
                                  entry; lp_abi_sizeof(10) answers for the new struct)
                                  and again (additive: a new struct and one new entry point): rays clipped to the occupied span of a
                                  scaffold, LpRayClipArgs with lp_rays_clip() (lp_build_info() then has a "ray_clip" entry;
                                  lp_abi_sizeof(12) answers for the new struct)
                                  and again (additive: a new struct and four new entry points): gather and splat of a grid-list at
                                  arbitrary points, LpPointGridArgs with lp_point_gather() / lp_point_splat() / lp_point_normalize() /
                                  lp_point_grad_points() (lp_build_info() then has a "point_grid" entry; lp_abi_sizeof(14) answers
                                  for the new struct)
                                  and again (additive: a new struct and three new entry points): the triangle mesh of a lattice's
                                  level set, LpMeshArgs with lp_mesh_workspace_bytes() / lp_mesh_count() / lp_mesh_emit()
                                  (lp_build_info() then has a "mesh" entry; lp_abi_sizeof(16) answers for the new struct) */

#define LP_MAX_GRIDS 8   /* grids per grid-list                         */
#define LP_MAX_LAYERS 8  /* layers per MLP                              */
#define LP_MAX_WIDTH 128 /* widest layer / grid channel count supported */
/* The forward pass saves the running -log T every LP_NLT_CKPT regular samples (and at the
 * last regular sample) and after EVERY beyond-far sample, so that the backward sweep
 * (far -> near) never reconstructs the transmittance across more than LP_NLT_CKPT
 * subtractions.  Every checkpoint is a float PAIR (hi, lo): -log T is accumulated as an unevaluated sum so
 * that the backward's subtraction of the same products recovers the intermediate values exactly.
 * One more pair per ray closes the list: (index of the last sample the forward marched, low word of
 * the final -log T) -- the backward starts there (see stop_neg_log_t).  The forward writes every pair of a ray up to the one of
 * that sample and the closing pair; with early termination the pairs of checkpoints BEHIND the last marched sample are not
 * written, and the backward never reads them (it takes no sample behind that index).  Without early termination every pair of
 * every ray is written.
 * O(N) memory: 2 * (ceil(S/LP_NLT_CKPT) + S_inf + 1) floats per ray. */
#define LP_NLT_CKPT 32
/* samples per state record of the segment-parallel march of a small batch (LpRendererArgs.seg_prefix); a workgroup marches one or more
 * such blocks (16 before 0.2.7) */
#define LP_SEG_LEN 8

/* error codes (negative; positive values are hipError_t) */
#define LP_OK 0
#define LP_EINVAL (-1)      /* malformed argument (see lp_last_error)          */
#define LP_EUNSUPPORTED (-2) /* shape outside what the kernels are built for    */
#define LP_ENULL (-3)       /* required pointer is NULL                        */

/* kernel selection hints (LpRendererArgs.kernel) */
#define LP_KERNEL_AUTO 0    /* MFMA kernel when the shape allows it, else generic */
#define LP_KERNEL_GENERIC 1 /* force the shape-generic VALU kernel               */
#define LP_KERNEL_MFMA 2    /* force the MFMA kernel (LP_EUNSUPPORTED if n/a)    */

/* arithmetic of the Renderer BACKWARD (LpRendererArgs.arithmetic).  The forward products -- the outputs, the backward's decoder
 * recompute and its ReLU decisions -- are fp32-equivalent in every mode (bf16x3: three exact bf16 limbs per operand, six limb
 * products, fp32 accumulation; the shape-generic kernels: plain fp32 FMAs).
 *   LP_ARITH_DEFAULT  the gradient operand of the dX chains and both operands of the weight gradients as TWO bf16 limbs (16
 *                     significand bits, three of nine limb products) where the kernel family does so -- lp_build_info() names the
 *                     limb counts of the library at hand; results stay inside 1e-4 of the fp32 reference
 *   LP_ARITH_FP32     the reference's arithmetic (triton_src/shared/const.py:9 ALLOW_TF32 = False): three limbs for every operand
 *                     of the dX chains, weight gradients on v_mfma_f32_16x16x4_f32.  The tuned family (kernel family 1) has
 *                     instantiations for it; every other shape runs the shape-generic fp32 kernels (family 0: slow, exact). */
#define LP_ARITH_DEFAULT 0
#define LP_ARITH_FP32 1

/* march order of the Renderer BACKWARD (LpRendererArgs.march_order; same results up to fp32 summation order).  The grid-gradient
 * scatter merges the taps of consecutive lanes that fall into one cell into a single row-contiguous atomic:
 *   LP_MARCH_RAYS_PER_WAVE     a wavefront = 32 consecutive rays at one sample: merges neighbouring rays (image-coherent batches:
 *                              consecutive rays = neighbouring pixels).  Default.
 *   LP_MARCH_SAMPLES_PER_WAVE  a wavefront = 32 consecutive samples of ONE ray (its rays one after the other): merges the samples a
 *                              ray spends in one cell -- for batches of unrelated rays (random training batches; the reference's speed
 *                              benchmark, tests/renderer_speed_benchmark.py:228-246), where every ray is its own run otherwise and
 *                              the backward is bound by the chip's atomic rate.  Tuned family, no beyond-far samples, no early
 *                              termination, >= 32 samples; ignored elsewhere (the rays-per-wavefront kernels run). */
#define LP_MARCH_RAYS_PER_WAVE 0
#define LP_MARCH_SAMPLES_PER_WAVE 1

typedef struct LpGrid {
  int32_t B, D, H, W;  /* batch and spatial extent                         */
  int64_t row_offset;  /* first row of this grid in the tensor that holds it */
  /* Zero-copy grid-lists (reference misc_utils.py:42-45 concatenates a list of grids on every call): a grid may
   * live in its own allocation.  NULL = the grid lives in LpGridList.data (one flat tensor, increasing
   * row_offsets); otherwise the [rows, C] tensor holding this grid, whose row `row_offset` (normally 0) is the
   * grid's first cell.  Gradient buffers mirror this through the *_list fields of the argument structs. */
  const float* data;
} LpGrid;

typedef struct LpGridList {
  const float* data;   /* [rows, channels] fp32; may be NULL when n_grids == 0 or every grid carries its own pointer */
  int32_t n_grids;     /* 0 .. LP_MAX_GRIDS                                 */
  int32_t channels;    /* C                                                  */
  int64_t n_rows;      /* total rows (for bounds checks)                     */
  LpGrid grids[LP_MAX_GRIDS];
} LpGridList;

/* rays: reference lightplane/ray_utils.py:19-57 */
typedef struct LpRays {
  int64_t n_rays;
  const float* directions;  /* [N,3] */
  const float* origins;     /* [N,3] */
  const int32_t* grid_idx;  /* [N]   batch element each ray belongs to */
  const float* near_t;      /* [N]   */
  const float* far_t;       /* [N]   */
  const float* encoding;    /* [N,encoding_dim] (Renderer: colour-MLP input width;
                               Splatter: splatted feature) */
  int32_t encoding_dim;
  int32_t row_length;       /* > 0: the batch is made of image rows in scanline order, row_length consecutive rays each (neighbouring
                               pixels).  A hint (0 = unknown; ABI 0.2.6, the former padding): the Splatter's backward walk then deals
                               2 x 4 PIXEL PATCHES to a wavefront -- four image rows walked column by column, alternating direction --
                               instead of 8 pixels of one row: the rays a wave gathers for are neighbours in both image directions
                               (cfg 3 backward -14 %).  Results are per ray and unchanged.  (The Renderer kernels ignore it: dealt
                               8 x 4 patches they measured SLOWER -- profiles/r06_ray_order.txt.) */
} LpRays;

/* ray-march schedule: reference naive_renderer.py:218-257, ray_util.py:48-58 */
typedef struct LpMarch {
  int32_t num_samples;         /* S  : equispaced in [near, far], both ends included */
  int32_t num_samples_inf;     /* S_inf : extra samples beyond far, linear in disparity */
  int32_t mask_out_of_bounds;  /* zero samples outside [-1,1]^3                      */
  int32_t contract_coords;     /* MeRF contraction (+ x0.5) before sampling          */
  double disparity_at_inf;
} LpMarch;

/* one MLP inside a flat parameter vector: all weights W_0..W_{n-1} ([in,out]
 * row-major, y = x @ W + b) followed by all biases b_0..b_{n-1}, starting at
 * float index `offset`.  dims[0] = input width, dims[l+1] = output width of layer l. */
typedef struct LpMlp {
  int32_t n_layers;                /* 0 .. LP_MAX_LAYERS */
  int32_t dims[LP_MAX_LAYERS + 1];
  int64_t offset;
} LpMlp;

typedef struct LpRendererArgs {
  LpRays rays;            /* encoding_dim == colour MLP input width            */
  LpGridList grid;        /* feature grid-list                                  */
  LpGridList color_grid;  /* n_grids == 0: single-grid mode (trunk MLP used)    */
  const float* scaffold;  /* NULL or [B, D*H*W] occupancy (0/1 floats)          */
  LpGrid scaffold_shape;  /* B,D,H,W of the scaffold (row_offset ignored)       */
  LpMarch march;
  /* decoder: trunk -> {opacity, color}; ReLU after every trunk layer and between
   * head layers; opacity = gain*softplus(raw); color = sigmoid(raw)              */
  const float* mlp_params;
  int64_t n_mlp_params;
  LpMlp trunk, opacity, color;
  int32_t color_chn;      /* real colour channels (<= color.dims[last]; the
                             remaining columns are zero padding, never evaluated) */
  float gain;
  float noise_sigma;      /* > 0: add sigma * hash_randn to the raw opacity      */
  int32_t noise_seed;
  int32_t kernel;         /* LP_KERNEL_*                                         */
  int32_t seg_forward_off; /* 1: with seg_prefix, the forward still marches every ray in one sweep (see seg_prefix) */
  /* forward outputs (written, not accumulated) */
  float* ray_length;      /* [N]                                                 */
  float* neg_log_t;       /* [N]  negative log transmittance after the last sample */
  float* feature;         /* [N, color_chn]                                      */
  float* neg_log_t_ckpt;  /* [N, n_ckpt, 2] written by forward, read by backward; NULL:
                             backward reconstructs from neg_log_t alone (less accurate) */
  /* backward inputs: upstream gradients (NULL = zeros) + neg_log_t from forward */
  const float* grad_ray_length; /* [N]            */
  const float* grad_neg_log_t;  /* [N]            */
  const float* grad_feature;    /* [N, color_chn] */
  /* backward outputs, accumulated with atomics: caller zero-fills. NULL = skip. */
  float* grad_grid;        /* like grid.data        */
  float* grad_color_grid;  /* like color_grid.data  */
  float* grad_mlp_params;  /* [n_mlp_params]        */
  float* grad_encoding;    /* [N, encoding_dim] (written, not accumulated) */
  /* per-grid gradient buffers for grids that carry their own LpGrid.data pointer: entry g (shaped like the tensor
   * grids[g].data points to, same row_offset) receives the gradient of grid g; NULL entries fall back to
   * grad_grid / grad_color_grid. */
  float* grad_grid_list[LP_MAX_GRIDS];
  float* grad_color_grid_list[LP_MAX_GRIDS];
  /* Fused epilogue of the module front-end (reference renderer_module.py:552-561; all optional):
   *   bg_color != NULL : feature[r, c] += T_r * bg_color[c],  T_r = exp(-neg_log_t[r])
   *   alpha    != NULL : alpha[r] = 1 - T_r (alpha_mode 1)  or  log T_r = -neg_log_t[r] (alpha_mode 2)
   * neg_log_t is always written raw (the backward needs it).  The backward takes grad_feature w.r.t. the
   * composited feature and grad_alpha [N] and folds both into the gradient of -log T. */
  const float* bg_color;    /* [color_chn] */
  float* alpha;             /* [N] */
  const float* grad_alpha;  /* [N] (backward) */
  int32_t alpha_mode;       /* 0 none, 1 alpha = 1 - T, 2 log transmittance */
  /* early ray termination (extension; the reference always marches every sample): > 0 = a wavefront stops
   * marching once -log T of all its rays has reached this value (their transmittance is below
   * exp(-stop_neg_log_t)); the backward skips the same samples.  ray_length / feature then miss
   * contributions of at most exp(-stop_neg_log_t) per unit of depth / colour, and neg_log_t is the value
   * reached at the stop (>= stop_neg_log_t) instead of the value after the last sample.  0 = exact. */
  float stop_neg_log_t;
  /* Segment-parallel backward for small batches (extension).  A backward sweep is serial along the ray, so a batch
   * with fewer rays than the GPU has wave slots (65 536 fill an MI355X once) leaves most of the chip idle.  With seg_prefix != NULL the
   * forward also saves, per ray and per block of LP_SEG_LEN regular samples, the state after the block's last sample
   * -- [N, lp_renderer_backward_segments(args), 8] floats: ray_length, feature[0..3], -log T (hi, lo), 0 -- and the
   * backward sweeps every block of a ray in its own workgroup (the part of d loss / d opacity_s that depends on the
   * samples behind the block comes from the saved sums).  grad_encoding is then ACCUMULATED (caller zero-fills).
   * The forward itself is segment-parallel too unless seg_forward_off is set: one workgroup per (128 rays, segment)
   * writes segment-local sums into the records and a combine pass chains them (compositing is associative) -- outputs
   * then differ from the single sweep by rounding (~1e-7 relative).
   * Pass the same pointer to forward and backward, and only when lp_renderer_backward_segments() > 1. */
  float* seg_prefix;
  int32_t arithmetic;     /* LP_ARITH_* (backward only; the forward is fp32-equivalent in every mode) */
  int32_t march_order;    /* LP_MARCH_* (backward only): how (ray, sample) pairs are dealt to the lanes of a wavefront */
} LpRendererArgs;

typedef struct LpSplatterArgs {
  LpRays rays;             /* encoding = splatted feature [N, encoding_dim]       */
  LpMarch march;
  LpGridList out;          /* output grid-list shape; out.data = feature accumulator
                              [rows, C] (zero-filled by caller)                   */
  float* out_feature;      /* == (float*)out.data, writable alias                 */
  float* out_weight;       /* [rows] splat-weight accumulator (zero-filled)       */
  /* MLP-splatter only (mlp.n_layers > 0): MLP(sample(input_grid) + encoding) is
   * splatted instead of the encoding                                            */
  LpGridList input_grid;
  const float* mlp_params;
  int64_t n_mlp_params;
  LpMlp mlp;               /* dims[0] == encoding_dim == input_grid.channels,
                              dims[last] == out.channels                          */
  int32_t kernel;
  int32_t march_order;     /* LP_MARCH_* (plain Splatter forward): LP_MARCH_SAMPLES_PER_WAVE walks 32 consecutive samples of ONE ray per
                              wavefront instead of 32 rays -- for batches of unrelated rays (reference tests/splatter_speed_benchmark.py):
                              the run merge of the atomic walk then works along the ray.  0 = rays per wavefront (image-coherent batches) */
  /* backward */
  const float* grad_out;   /* [rows, C] gradient w.r.t. the NORMALISED output grid */
  const float* weight;     /* [rows] un-clamped splat weights saved by forward     */
  float* grad_encoding;    /* [N, encoding_dim] (written)                          */
  float* grad_input_grid;  /* like input_grid.data (accumulated; MLP-splatter)     */
  float* grad_mlp_params;  /* [n_mlp_params]      (accumulated; MLP-splatter)      */
  float* grad_input_grid_list[LP_MAX_GRIDS]; /* per-grid buffers (see LpGrid.data); NULL entries -> grad_input_grid */
} LpSplatterArgs;

/* Ray-direction embedding of the module front-end, fused into one kernel (reference renderer_module.py:578-601
 * `_get_ray_embedding`: F.normalize -> harmonic embedding (ray_utils.py:181-212) -> Linear):
 *   d = directions / max(|directions|, 1e-12)
 *   emb = [sin(d_c 2^k)]_{c<3,k<n} ++ [sin(d_c 2^k + pi/2)]_{c<3,k<n} ++ d          (3 + 6 n values, index (p*3+c)*n+k)
 *   out[r, e] = bias[e] + sum_i weight[e, i] emb[i]                                  (torch.nn.Linear layout)
 * backward: grad_weight / grad_bias accumulate (atomics; caller zero-fills); directions get no gradient. */
typedef struct LpRayEmbedArgs {
  int64_t n_rays;
  const float* directions;  /* [N,3] */
  int32_t n_harmonics;      /* 0 .. 10 */
  int32_t out_dim;          /* E <= LP_MAX_WIDTH */
  const float* weight;      /* [E, 3 + 6 n] */
  const float* bias;        /* [E] */
  float* out;               /* [N, E] (forward) */
  const float* grad_out;    /* [N, E] (backward) */
  float* grad_weight;       /* [E, 3 + 6 n] */
  float* grad_bias;         /* [E] */
} LpRayEmbedArgs;

int lp_version(void); /* LP_VERSION */
/* What this binary was built from, as one JSON object (static storage): "version", "src_hash" (sha256 over csrc/ *.hip, *.h,
 * build.py and this header, as lightplane_amd/csrc/build.py source_hash() computes it -- compare with the tree), "flags" (global
 * + per-file compiler flags), and per kernel family the limb counts / matrix instructions its backward was compiled with
 * ("tuned_bwd", "loop_bwd_deep", "loop_bwd_shallow", "mlp_splatter_bwd"), "test_hooks" (1 = the DUMP twins are in). */
const char* lp_build_info(void);
const char* lp_last_error(void);
/* sizeof() of the ABI structs as compiled into the library, for binding self-checks:
 * which = 0 LpGrid, 1 LpGridList, 2 LpRays, 3 LpMarch, 4 LpMlp, 5 LpRendererArgs,
 * 6 LpSplatterArgs, 7 LpRayEmbedArgs, 8 LpScaffoldArgs, 10 LpPointsArgs, 12 LpRayClipArgs, 14 LpPointGridArgs, 16 LpMeshArgs; anything
 * else returns -1 -- 9, 11, 13 and 15 among them: the scaffold's, the point evaluation's, the ray clip's and the point gather's tests
 * pin those answers as "the first selector that does not exist", so the next addition took the one after.
 * (18 and 20 answer for the two structs of lightplane_hip_samples.h -- sample placement and compositing of the march as entry
 * points of their own, declared in that header so that the tables of this one stay as they are; 17, 19 and 21 return -1.
 * 22 answers for LpImportanceArgs of lightplane_hip_importance.h, importance resampling of those samples; 23 returns -1.
 * 24 and 26 answer for LpDistortionArgs and LpInterlevelArgs of lightplane_hip_losses.h, two losses on those samples; 25 and 27
 * return -1.) */
int lp_abi_sizeof(int which);

/* Number of ray segments the backward of these arguments can be split into (see LpRendererArgs.seg_prefix): 1 when the
 * selected kernel has no segmented form, when the march has beyond-far samples or early termination, or when the
 * batch fills the GPU without it; otherwise ceil(num_samples / LP_SEG_LEN).  Depends on shapes only (no launch). */
int lp_renderer_backward_segments(const LpRendererArgs* args);

/* Which kernel family LP_KERNEL_AUTO selects for these arguments (no launch; shapes only):
 *   lp_renderer_kernel_family: the BACKWARD's family = the family of lp_renderer_forward (lp_renderer_forward_ws has its own answer,
 *                              lp_renderer_forward_family below): 0 shape-generic VALU kernels, 1 tuned bf16x3 MFMA kernels of the default decoder (2/2/2 x 32),
 *                              3 layer-looped bf16x3 MFMA family (1-4 layers per MLP, one hidden width of 16 / 32 and <= 32
 *                              colour channels -- or width 64 / 64 grid channels with at most 2 layers per MLP and <= 4 colour
 *                              channels); 2 (the fp32-MFMA hidden-64 family of 0.1 - 0.2.3) is no longer returned
 *   lp_splatter_kernel_family: 0 shape-generic kernels, 1 run-merged walk (plain Splatter, C in {16,32,64}),
 *                              3 layer-looped bf16x3 MFMA MLP-Splatter (2-4 layers, widths 16 / 32 / 64, Cout 16 / 32);
 *                              2 (the two-layer fp32-MFMA family of 0.1 - 0.2.2) is no longer returned
 * The generic kernels are correctness anchors, one to two orders of magnitude slower. */
int lp_renderer_kernel_family(const LpRendererArgs* args);
int lp_splatter_kernel_family(const LpSplatterArgs* args);

int lp_renderer_forward(const LpRendererArgs* args, void* stream);
int lp_renderer_backward(const LpRendererArgs* args, void* stream);

/* Forward with a caller-provided workspace: the layer-looped MFMA forward also for the decoders lp_renderer_kernel_family() turns down
 * ONLY for their depth -- hidden width 64 (or 64 grid channels) with 3 or 4 layers in any of the three MLPs; default arithmetic,
 * <= 4 colour channels, everything else as family 3.  Their backward stays on the shape-generic kernels (lp_renderer_backward,
 * unchanged): this forward leaves neg_log_t and neg_log_t_ckpt exactly as that backward reads them, and stops early-terminated
 * rays per 64 consecutive rays, the wavefront of the generic kernels.  For every other shape -- and for LP_KERNEL_GENERIC and
 * LP_ARITH_FP32 -- it IS lp_renderer_forward (workspace ignored).
 *   lp_renderer_forward_family: what lp_renderer_forward_ws runs (no launch; shapes only): 0 / 1 / 3 as lp_renderer_kernel_family,
 *     3 also for a deep decoder whose weight images fit the 160 KB LDS without the backward's tiles (e.g. 3/2/2 x 64), 4 = the
 *     layer-looped forward with STREAMED weight images (a resident prefix of layers + a two-slot LDS ring for the rest).
 *     A decoder with a separate colour grid is laid out WITH the ring's two slots reserved (the resident kernel has no eight-wave form
 *     for it): 0/3/3 x 64 still fits whole and reports 3 (four-wave resident kernel), 0/4/4 x 64 reports 4 (its last layers pass
 *     through the ring) although its 20 block images alone would fit the LDS.
 *   lp_renderer_forward_workspace_bytes: 0 unless the family is 4; then the bytes of the streamed layers' pre-split block images,
 *     back to back, no header (per layer ceil(rows_in / 32) * ceil(cols / 32) * 6528).  Depends on shapes only.  A block image is
 *     three limbs of 2176 bytes in the LDS layout: 32 rows of 64 bytes, every group of four rows 16 bytes further on; the 8 x 16
 *     bytes of that skew are padding -- the packing pass does not write them, and nothing that is computed reads them (the copy into
 *     LDS carries them along).
 *   lp_renderer_forward_ws: packs the images into `workspace` (device memory, 16-byte aligned, at least that many bytes; owned by the
 *     caller, free to reuse once the call's work on `stream` is done) and runs the forward on `stream`.  LP_EINVAL, before any launch, when
 *     the family is 4 and the workspace is NULL, short or misaligned. */
int lp_renderer_forward_family(const LpRendererArgs* args);
int64_t lp_renderer_forward_workspace_bytes(const LpRendererArgs* args);
int lp_renderer_forward_ws(const LpRendererArgs* args, void* workspace, int64_t workspace_bytes, void* stream);

int lp_splatter_forward(const LpSplatterArgs* args, void* stream);
/* feature[r, :] /= max(weight[r], 1e-5) for r in [0, n_rows) (in place). */
int lp_splatter_normalize(float* feature, const float* weight, int64_t n_rows, int32_t channels,
                          void* stream);
int lp_splatter_backward(const LpSplatterArgs* args, void* stream);

/* <- LightplaneRenderer._get_ray_embedding (lightplane/renderer_module.py:578-601) and its autograd backward */
int lp_ray_embedding_forward(const LpRayEmbedArgs* args, void* stream);
int lp_ray_embedding_backward(const LpRayEmbedArgs* args, void* stream);

/* Total-variation regulariser of a grid-list (an extension: the reference has no such operator; lp_grid_tv.hip).
 * For one grid x [B, D, H, W, C] and p in {1, 2}, phi_1(d) = |d|, phi_2(d) = d * d:
 *   T_a    = sum of phi_p(x[.., i + 1, ..] - x[.., i, ..]) over all adjacent pairs along the spatial axis a, all B and all C;
 *            N_a = the number of those pairs
 *   loss_g = sum over the axes a in {D, H, W} with extent > 1 of T_a / N_a      (a plane [B, 1, H, W, C] gets its 2-D TV; a
 *            grid with no axis > 1 has loss 0)
 *   loss   = sum_g grid_weights[g] * loss_g
 * The derivative of phi_1 at a zero difference is 0.  There are no pairs across batch entries or across list entries.
 * `grid`: a grid-list as everywhere in this header (flat tensor + row offsets, or per-grid base pointers), with two relaxations:
 * a grid may have ANY positive extents (a line [B, 1, 1, W] and a single cell are valid), and the grids need not share a batch
 * size.  1 .. LP_MAX_WIDTH channels (rows are read 16 bytes at a time where C % 4 == 0 and every pointer is 16-byte aligned, float
 * by float otherwise); every tensor below 2^31 rows, element offsets are 64-bit.
 * `grid_weights`: HOST array of n_weights == grid->n_grids floats, or NULL with n_weights == 0 (every weight 1).
 * No atomics: loss and gradient are bit-reproducible.  No host synchronisation and no allocation: graph-capturable.
 *   lp_grid_tv_workspace_bytes: bytes of device workspace the loss needs for this list (one fp64 partial per workgroup of the sweep;
 *     shapes only, no device; never decreases when an extent grows), or a negative LP_E* code for a malformed list.
 *   lp_grid_tv_forward:  *loss (device, fp32) = loss.  `workspace`: device memory, 8-byte aligned, >= that many bytes, free to reuse
 *     once the call's work on `stream` is done.  It is scratch: the call writes one partial per workgroup it launches, from the
 *     start of the buffer, and reads back exactly those; the query sizes for the float-by-float sweep, so with 16-byte rows the tail
 *     of the buffer is neither written nor read.  The contents before the call do not matter.
 *   lp_grid_tv_backward: gradient = scale * (*grad_loss) * d loss / d grid, computed per element from its six neighbours and written
 *     (accumulate == 0) or added to what the buffer holds (accumulate != 0).  grad_loss: DEVICE scalar (the upstream gradient; NULL =
 *     1).  Where the gradient goes: `grad_list` -- a HOST array of n_grad_list == n_grids device pointers, entry g shaped like the
 *     tensor that holds grid g (same row_offset) -- and / or `grad`, the buffer that mirrors the flat tensor grid->data, which serves
 *     every grid without an own LpGrid.data pointer whose list entry is NULL or absent (grad_list == NULL needs n_grad_list == 0).
 *   lp_grid_tv_fused:    both in ONE sweep over the grid: *loss = loss (not scaled), gradient buffers += scale * (*grad_loss) * d loss /
 *     d grid -- for a training step on a grid too large for a second sweep to be free.
 * Before anything touches the device: LP_EINVAL for p outside {1, 2}, a weight count != n_grids, a short or misaligned workspace, a
 * gradient list that does not match the grid list; LP_ENULL for a NULL list / loss / workspace / missing data or gradient pointers;
 * LP_EUNSUPPORTED for a channel count outside [1, LP_MAX_WIDTH] or a tensor of 2^31 rows or more. */
int64_t lp_grid_tv_workspace_bytes(const LpGridList* grid);
int lp_grid_tv_forward(const LpGridList* grid, const float* grid_weights, int32_t n_weights, int32_t p, float* loss, void* workspace,
                       int64_t workspace_bytes, void* stream);
int lp_grid_tv_backward(const LpGridList* grid, const float* grid_weights, int32_t n_weights, int32_t p, const float* grad_loss,
                        float scale, float* grad, float* const* grad_list, int32_t n_grad_list, int32_t accumulate, void* stream);
int lp_grid_tv_fused(const LpGridList* grid, const float* grid_weights, int32_t n_weights, int32_t p, float* loss, void* workspace,
                     int64_t workspace_bytes, const float* grad_loss, float scale, float* grad, float* const* grad_list,
                     int32_t n_grad_list, void* stream);

/* Resampling of a grid-list to new spatial sizes, on the channels-last layout (lp_grid_resample.hip; the role of the reference's
 * examples/utils/util/grid_util.py grid_up_sample = permute + torch.nn.functional.interpolate + permute, without the copies).
 * `src` and `dst` are grid-lists as everywhere in this header (flat tensor + row offsets, or per-grid base pointers; any positive
 * extents, as for lp_grid_tv_*) with the same number of grids, the same channel count and, grid by grid, the same B: grid g of `src`
 * [B, D, H, W, C] is resampled to the extents of grid g of `dst` [B, D', H', W', C].  Batch and channels are never resampled.
 * Per spatial axis with input extent n_in, output extent n_out and one fp32 coefficient a:
 *   align_corners == 1: src(o) = a * o;   align_corners == 0: src(o) = max(0, a * (o + 0.5) - 0.5)
 *   i0 = min(floor(src), n_in - 1), i1 = min(i0 + 1, n_in - 1), lambda = clamp(src - i0, 0, 1)
 * and an output cell is the tensor product over the three axes: the sum of 8 input rows with weights prod (1 - lambda | lambda) --
 * torch's trilinear interpolation (bilinear for a plane: an axis with n_in == 1 replicates).  fp32, every operation individually rounded.
 * `coeffs`: HOST array of 3 * n_grids floats, a of grid g and axis D, H, W at [3 g], [3 g + 1], [3 g + 2] -- torch takes
 * (float)(1.0 / scale_factor) when it is given a scale factor and align_corners is off -- or NULL: derived from the sizes, with
 * align_corners (n_in - 1) / (n_out - 1) (0 for n_out == 1), without n_in / n_out, both as fp32 divisions.
 *   lp_grid_resample_forward:  dst = R src.  The memory `dst` describes is WRITTEN (the struct's pointers are const for the readers).
 *   lp_grid_resample_backward: the adjoint.  `grad_dst` (read) is shaped like the forward's dst, `grad_src` (WRITTEN) like its src:
 *     grad_src[i] = sum_o w(o, i) grad_dst[o] with exactly the forward's weights, stored (accumulate == 0) or added to what the
 *     buffer holds (accumulate != 0).  A gather per input cell in a fixed order: no atomics, bit-reproducible, any size ratio.
 * 1 .. LP_MAX_WIDTH channels: rows move 16 bytes at a time where C % 4 == 0 and every pointer is 16-byte aligned, float by float
 * otherwise (any 4-byte-aligned pointer is accepted).  No allocation, no state, no host synchronisation: graph-capturable.
 * Before anything touches the device: LP_ENULL for a NULL list or a grid without a data pointer; LP_EINVAL for lists that differ in
 * the number of grids, in channels or in a grid's B, an empty extent, align_corners outside {0, 1}, a coefficient that is not finite
 * and positive, a tensor of 2^31 rows or more, a source that overlaps its destination, a pointer that is not 4-byte aligned;
 * LP_EUNSUPPORTED for a channel count outside [1, LP_MAX_WIDTH]. */
int lp_grid_resample_forward(const LpGridList* src, const LpGridList* dst, int32_t align_corners, const float* coeffs, void* stream);
int lp_grid_resample_backward(const LpGridList* grad_src, const LpGridList* grad_dst, int32_t align_corners, const float* coeffs,
                              int32_t accumulate, void* stream);

/* Occupancy scaffold of a grid-list (lp_scaffold.hip; the role of the reference's LightplaneRenderer.calculate_scaffold,
 * renderer_module.py:349-417, without the lattice of points, the encoding and the float max-pool).  The decoder's opacity is evaluated
 * on the regular lattice of a [B, D, H, W] scaffold -- x along W, y along H, z along D; the coordinate of index i on an axis of n points
 * is the fp32 value of torch.linspace(0, 1, n)[i] * 2 - 1 (torch's two-sided formula; n == 1 gives -1) --:
 *   features = sum over the grids of `grid` of their tri- / bi-linear sample at the point (the Renderer's gather: align_corners off,
 *              zero padding; all zero at a point outside [-1, 1]^3 when mask_out_of_bounds is set)
 *   raw      = opacity MLP(ReLU(trunk MLP(features)))   (ReLU after every trunk layer and between the head's layers), or, with
 *              trunk.n_layers == 0 (the two-grid decoder), opacity MLP(ReLU(features))
 *   opacity  = gain * softplus(raw)
 * in plain fp32 FMA arithmetic.  `mlp_params` is the decoder's flat vector as LpRendererArgs takes it (trunk | opacity | colour);
 * trunk.offset is 0, opacity.offset the trunk's size, and the colour MLP behind them is never read: n_mlp_params only has to cover
 * the two MLPs that are.  Any layer counts, widths up to LP_MAX_WIDTH, 1 .. LP_MAX_WIDTH grid channels.
 *   lp_scaffold_opacity: opacity[b, z, y, x] = that value (the raw lattice; threshold and dilate are ignored).
 *   lp_scaffold_build:   scaffold = max_pool3d(opacity, 2 * dilate + 1, stride 1, padding dilate) > threshold as 0 / 1 floats, computed as
 *     the binary OR-dilation of (opacity > threshold) -- the same thing: the pool's padding never wins and max commutes with a monotone
 *     threshold -- in three separable byte passes.  `workspace`: device memory of lp_scaffold_workspace_bytes() bytes (one byte per
 *     lattice point when dilate > 0, else 0 and the pointer may be NULL), free to reuse once the call's work on `stream` is done.  The
 *     result tensor itself serves as the second byte buffer.  A window at least as wide as an axis covers the whole axis.
 *   lp_scaffold_workspace_bytes: shapes only (shape and dilate; no device), or a negative LP_E* code.
 * One launch for the lattice and three for the dilation, all on `stream`: no atomics, no allocation, no host synchronisation
 * (graph-capturable).  Every device pointer -- the grids, mlp_params, the result, the workspace -- is 16-byte aligned (Conventions).
 * Before anything touches the device: LP_ENULL for NULL args / mlp_params / result or a grid without data; LP_EINVAL for a scaffold
 * extent < 1, shape.B different from the grid-list's batch, dilate < 0, a threshold that is NaN, MLPs that do not chain (trunk input
 * != grid channels, head input != trunk output, head output != 1) or do not fit n_mlp_params, an under-aligned pointer, a workspace
 * that is NULL, short or misaligned when bytes are needed; LP_EUNSUPPORTED for widths or channels outside [1, LP_MAX_WIDTH]. */
typedef struct LpScaffoldArgs {
  LpGridList grid;             /* feature grid-list, as in LpRendererArgs */
  const float* mlp_params;     /* the decoder's flat parameter vector */
  int64_t n_mlp_params;
  LpMlp trunk, opacity;        /* as in LpRendererArgs; trunk.n_layers == 0: two-grid decoder */
  float gain;
  int32_t mask_out_of_bounds;  /* zero the features of a lattice point outside [-1, 1]^3 (fp32 round-off at the faces only) */
  LpGrid shape;                /* B, D, H, W of the scaffold (row_offset and data ignored) */
  float threshold;             /* occupied: opacity > threshold */
  int32_t dilate;              /* radius r of the dilation window 2 r + 1; 0 = none */
} LpScaffoldArgs;
int64_t lp_scaffold_workspace_bytes(const LpScaffoldArgs* args);
int lp_scaffold_opacity(const LpScaffoldArgs* args, float* opacity, void* stream);
int lp_scaffold_build(const LpScaffoldArgs* args, float* scaffold, void* workspace, int64_t workspace_bytes, void* stream);

/* The decoder at arbitrary 3-D points (lp_points.hip; the role of the reference's lightplane_eval_mlp / lightplane_eval_mlp_opacity_only,
 * naive_renderer.py:328-598, as its LightplaneRenderer.eval_decoder_at_points / eval_opacity_at_points call them).  For point
 * p = points[r, n] of ray r, batch element b = grid_idx[r] (clamped to the grid-list's batch) and encoding e = encoding[r]:
 *   q        = p, or with contract_coords the Renderer's contraction of p (LpMarch.contract_coords: MeRF contraction, then x 0.5)
 *   features = sum over the grids of `grid` of their tri- / bi-linear sample at q (the Renderer's gather: align_corners off, zero
 *              padding; all zero outside [-1, 1]^3 when mask_out_of_bounds is set); cfeatures the same of `color_grid`
 *   single grid-list:  t = ReLU(trunk MLP(features)) (ReLU(features) without trunk layers), raw = opacity MLP(t), craw = colour MLP(t + e)
 *   two-grid decoder (color_grid.n_grids > 0, no trunk layers): raw = opacity MLP(ReLU(features)), craw = colour MLP(ReLU(cfeatures) + e)
 *   opacity_out[r, n]   = gain * softplus(raw) * occ,   color_out[r, n, c] = sigmoid(craw[c]) * occ, c < color_chn
 *   occ = 1, or with a scaffold its nearest-neighbour value at q (0 outside [-1, 1]^3), as in LpRendererArgs.
 * lp_points_forward: one lane per point, activations in LDS column tiles, weights through wave-uniform scalar loads, plain fp32 FMA
 *   chains (the lattice kernel of lp_scaffold_opacity with points read from memory).  color_out == NULL: opacity only -- the colour
 *   MLP, the colour grid-list and the encoding are never read (color.n_layers may then be 0 and encoding NULL; n_mlp_params has to cover
 *   the MLPs that are read).  The grad_* fields are ignored.
 * lp_points_backward: the shape-generic Renderer backward without the march.  It reads nothing the forward wrote: it recomputes the
 *   decoder of every point (fp32 matrix-core products for the wide layers: the same values to fp32 round-off, and the gradient
 *   returned is that of the branch of every ReLU this recompute took), forms d raw = grad_opacity * gain * occ * softplus'(raw) and
 *   d craw[c] = grad_color[c] * occ * sigmoid'(craw[c]), and goes back through the heads, the trunk and the gather.  grad_opacity /
 *   grad_color: NULL = zeros; with grad_color == NULL the colour head is not evaluated (its parameters and the colour grid-list get no
 *   contribution; color.n_layers may be 0 and encoding NULL).  Every result pointer may be NULL (that gradient is skipped); all but
 *   grad_points are ACCUMULATED with atomics into buffers the caller has zeroed, as in lp_renderer_backward:
 *   grad_grid / grad_grid_list, grad_color_grid / grad_color_grid_list (as in LpRendererArgs), grad_mlp_params [n_mlp_params],
 *   grad_encoding [n_rays, encoding_dim] (a ray's points span wavefronts), and grad_points [n_rays, n_pts, 3] (WRITTEN):
 *   d L / d p = J^T sum over both grid-lists, their grids and corners k of (d w_k / d q) <row_k, d features>, with d w_k / d q the
 *   derivative of the tri- / bi-linear weight times size / 2 and J the Jacobian of the contraction; the out-of-bounds mask and the
 *   scaffold are piecewise constant and contribute nothing.  The opacity_out / color_out fields are ignored.
 * Any layer counts, widths and channels up to LP_MAX_WIDTH (backward: layer widths summing to at most 1024, as the generic Renderer).
 * n_rays * n_pts == 0 launches nothing.  No allocation, no host synchronisation: graph-capturable.  Every device pointer is 16-byte
 * aligned (Conventions).  Before anything touches the device: LP_ENULL for NULL args / points / grid_idx / mlp_params / opacity_out
 * (forward), a grid without data, or a NULL encoding where the colour head runs; LP_EINVAL for negative n_rays / n_pts, MLPs that do
 * not chain or do not fit n_mlp_params, encoding_dim != the colour head's input width, color_chn outside the colour head's output, a
 * colour grid-list with trunk layers or with another batch size / channel count than `grid`, a scaffold of another batch size or an
 * extent < 1, gradient buffers for some grids of a list only, an under-aligned pointer; LP_EUNSUPPORTED for widths or channels
 * outside [1, LP_MAX_WIDTH], more than 2^31 x 64 points, or (backward) layer widths beyond 1024 in total. */
typedef struct LpPointsArgs {
  LpGridList grid;             /* feature grid-list */
  LpGridList color_grid;       /* n_grids == 0: single grid-list (trunk MLP used) */
  const float* mlp_params;     /* the decoder's flat parameter vector: trunk | opacity | colour */
  int64_t n_mlp_params;
  LpMlp trunk, opacity, color; /* as in LpRendererArgs */
  int32_t color_chn;           /* real colour channels (<= color.dims[last]) */
  float gain;
  int32_t mask_out_of_bounds;
  int32_t contract_coords;
  const float* points;         /* [n_rays, n_pts, 3] */
  const int32_t* grid_idx;     /* [n_rays] batch element of each ray's points, as LpRays.grid_idx */
  const float* encoding;       /* [n_rays, encoding_dim] */
  int32_t encoding_dim;        /* == the colour head's input width */
  int32_t reserved;            /* 0 */
  int64_t n_rays, n_pts;
  const float* scaffold;       /* NULL or [B, D, H, W] occupancy (0 / 1 floats) */
  LpGrid scaffold_shape;       /* B, D, H, W of the scaffold (row_offset and data ignored) */
  /* forward results (written).  (The MLP fields above carry the names `opacity` and `color`, as in every struct here.) */
  float* opacity_out;          /* [n_rays, n_pts] */
  float* color_out;            /* [n_rays, n_pts, color_chn]; NULL = opacity only */
  /* backward: upstream gradients (NULL = zeros) */
  const float* grad_opacity;   /* [n_rays, n_pts] */
  const float* grad_color;     /* [n_rays, n_pts, color_chn] */
  /* backward results (NULL = skip) */
  float* grad_grid;            /* like grid.data */
  float* grad_color_grid;      /* like color_grid.data */
  float* grad_grid_list[LP_MAX_GRIDS];        /* per-grid buffers, as in LpRendererArgs */
  float* grad_color_grid_list[LP_MAX_GRIDS];
  float* grad_mlp_params;      /* [n_mlp_params] */
  float* grad_encoding;        /* [n_rays, encoding_dim] (accumulated) */
  float* grad_points;          /* [n_rays, n_pts, 3] (written) */
} LpPointsArgs;
int lp_points_forward(const LpPointsArgs* args, void* stream);
int lp_points_backward(const LpPointsArgs* args, void* stream);

/* Rays clipped to the occupied span of a scaffold (lp_ray_clip.hip).  The Renderer reads a scaffold with nearest-neighbour,
 * align_corners = False indexing: scene b is tiled by W x H x D axis-aligned boxes, cell i along x covering
 * [-1 + 2 i / W, -1 + 2 (i + 1) / W], and a cell is occupied iff its value != 0.  For ray r (any direction length; a zero component is
 * legal) the kernel intersects [near, far] with the box [-1, 1]^3 (slab test), walks the cells the ray crosses (3-D DDA, one lane per
 * ray) forward to the first occupied cell (near*) and backward from the far end to the last (far*), and writes
 *   near_out[r] = max(near, near* - pad_t - e),  far_out[r] = min(far, far* + pad_t + e),  hit_out[r] = 1
 * with pad_t = pad * h / |d|, h = 2 / max(D, H, W), and e >= 0 the kernel's bound on the fp32 rounding of the crossing it stopped at
 * (14 * 2^-24 * (1 + |o_a|) / |d_a| for a crossing of axis a): no sample of the Renderer on [near, far] outside
 * [near_out, far_out] has a non-zero scaffold value.  A ray without an occupied cell on [near, far] -- also one with far < near, a NaN
 * or Inf entry, or grid_idx outside [0, B) -- is a miss: hit_out[r] = 0 and near_out / far_out carry near / far bit for bit.
 * scaffold == NULL: the box alone (one occupied cell, h = 2; scaffold_shape is ignored, any grid_idx >= 0 is in range).
 * rays.encoding, encoding_dim and row_length are ignored.  near_out / far_out may be rays.near_t / rays.far_t (a lane reads its
 * values before it writes).  No atomics, no workspace, no host synchronisation: graph-capturable and bit-reproducible.
 * Every device pointer except hit_out (bytes) is 16-byte aligned (Conventions).  Before anything touches the device: LP_ENULL for
 * NULL args / results or, with n_rays > 0, a NULL ray field; LP_EINVAL for an under-aligned pointer, n_rays < 0, a pad that is
 * negative or not finite, or (with a scaffold) a shape with an extent < 1.  n_rays == 0 succeeds without a launch. */
typedef struct LpRayClipArgs {
  LpRays rays;             /* directions, origins, grid_idx, near_t, far_t */
  const float* scaffold;   /* NULL or [B, D, H, W] occupancy (!= 0: occupied) */
  LpGrid scaffold_shape;   /* B, D, H, W of the scaffold (row_offset and data ignored) */
  float pad;               /* margin in cells of the finest axis, >= 0 */
  int32_t reserved;        /* 0 */
} LpRayClipArgs;
int lp_rays_clip(const LpRayClipArgs* args, float* near_out, float* far_out, uint8_t* hit_out, void* stream);

/* Gather and splat of a grid-list at arbitrary 3-D points, without a decoder (lp_point_grid.hip; an extension: the counterpart at
 * points of the Renderer's gather and the Splatter's scatter along rays).  For the grid-list G (C channels), points P [n_rays, n_pts, 3],
 * per-point vectors U [n_rays, n_pts, C], q = p or, with contract_coords, the Renderer's contraction of p, and batch element
 * b = grid_idx[r] (clamped to the grid-list's batch) for every point of row r, the four entry points are the partial derivatives of
 *   B(G, P, U) = sum over points, grids g and corners k of  w_k(q) <G_g[row_k(q)], U[point]>
 * with row_k / w_k the Renderer's corner rows and tri- / bi-linear weights (align_corners off, zero padding: a corner outside its grid
 * contributes nothing; with mask_out_of_bounds a point outside [-1, 1]^3 -- after the contraction -- contributes nothing at all):
 *   lp_point_gather:      out_features[r, n, :] = dB/dU = sum_g sum_k w_k G_g[row_k]  (WRITTEN; no atomics: bit-reproducible).  With
 *                         row_weight[g] != NULL a row of grid g is divided by max(row_weight[g][row_k], 1e-5) as it is read.  A
 *                         sub-group of C / 4 lanes per point moves whole rows 16 bytes per lane where C % 4 == 0; one lane per point
 *                         and float by float otherwise.  `vectors` is ignored.
 *   lp_point_splat:       dB/dG: vectors[r, n, :] * w_k is ADDED atomically to row row_k of every grid -- the memory `grid` describes is
 *                         accumulated into (the struct's pointers are const for the readers) and zeroed by the caller.  Lanes =
 *                         channels: one atomic instruction writes 64 / CW whole rows, CW = 16 / 32 / 64 lanes per row; channels
 *                         64 .. 127 take a second pass.  With row_weight[g] != NULL for EVERY grid, w_k is also added to
 *                         row_weight[g][row_k] (the Splatter's weight grid; zeroed by the caller).
 *   lp_point_normalize:   the epilogue of lp_point_splat with the same arguments: grid g row i /= max(row_weight[g][i], 1e-5) for every
 *                         row of every grid, in place, one pass (the Splatter's epilogue; true division).  row_weight is required for
 *                         every grid; the point, vector and result pointers are not looked at.
 *   lp_point_grad_points: grad_points[r, n, :] = dB/dP = J^T sum_g sum_k (d w_k / d q) <G_g[row_k], vectors[r, n]>  (WRITTEN, one lane
 *                         per point, no atomics), J the Jacobian of the contraction, as lp_points_backward forms grad_points; the mask is
 *                         piecewise constant and contributes nothing.  row_weight is ignored.
 * row_weight[g] indexes rows as grids[g] does: entry i belongs to row i of the tensor that holds grid g (its own allocation, or the
 * flat tensor -- then every entry may be one [n_rows] buffer).  Rows are 64-bit: grid-lists beyond 4 GB index correctly.
 * 1 .. LP_MAX_GRIDS grids, 1 .. LP_MAX_WIDTH channels.  No workspace, no allocation, no host synchronisation: graph-capturable.
 * Every device pointer is 16-byte aligned (Conventions).  Before anything touches the device: LP_ENULL for NULL args, a grid without
 * data, a NULL points / grid_idx / vectors / result the call uses (with n_rays * n_pts > 0), or (normalize) a grid without row_weight;
 * LP_EINVAL for negative n_rays / n_pts, a malformed grid-list, channels != grid.channels, row_weight for some grids only (splat), an
 * under-aligned pointer;
 * LP_EUNSUPPORTED for channels outside [1, LP_MAX_WIDTH] or more than 2^31 x 64 points.  n_rays * n_pts == 0 returns LP_OK without
 * a launch (lp_point_normalize too: a splat of no points added nothing, and a zero row divided by the clamp stays zero). */
typedef struct LpPointGridArgs {
  LpGridList grid;                 /* read (gather, grad_points), accumulated into (splat), divided in place (normalize) */
  float* row_weight[LP_MAX_GRIDS]; /* per-grid [rows] fp32 or NULL: read (gather, normalize), accumulated into (splat) */
  const float* points;             /* [n_rays, n_pts, 3] */
  const int32_t* grid_idx;         /* [n_rays] batch element of each row's points, as LpRays.grid_idx */
  int64_t n_rays, n_pts;
  const float* vectors;            /* U [n_rays, n_pts, C]: the features to splat / the upstream gradient of the gather */
  float* out_features;             /* gather: [n_rays, n_pts, C] (written) */
  float* grad_points;              /* grad_points: [n_rays, n_pts, 3] (written) */
  int32_t channels;                /* C of vectors / out_features as the caller laid them out: has to equal grid.channels */
  int32_t mask_out_of_bounds;
  int32_t contract_coords;
  int32_t reserved;                /* 0 */
} LpPointGridArgs;
int lp_point_gather(const LpPointGridArgs* args, void* stream);
int lp_point_splat(const LpPointGridArgs* args, void* stream);
int lp_point_normalize(const LpPointGridArgs* args, void* stream);
int lp_point_grad_points(const LpPointGridArgs* args, void* stream);

/* Triangle mesh of the level set {volume = level} of a [B, D, H, W] lattice: marching cubes (lp_mesh.hip; an extension -- the
 * reference has no mesh extraction).  Lattice point n = ((b D + z) H + y) W + x sits at the scaffold's coordinates
 * (lin(W)[x], lin(H)[y], lin(D)[z]), lin(n) = linspace(-1, 1, n); a point is inside when volume >= level (a NaN is outside).  A
 * lattice edge belongs to its endpoint with the lower coordinate and carries a vertex when exactly one endpoint is inside:
 *   vertex = p_lo + t (p_hi - p_lo),  t = clamp((level - v_lo) / (v_hi - v_lo), 0, 1) in fp32 (a NaN quotient -- an infinite or NaN
 *   endpoint -- counts as 0; finite values whose difference overflows fp32 are halved first, so +-3e38 around level 0 still gives 0.5).
 * Each cell (min corner n) contributes the triangles of the table lp_mc_table.h (generated by scripts/gen_mc_table.py; watertight by
 * construction, normals towards the lower values).  The output order is part of the contract:
 *   vertices: by owner point n, then axis x, y, z;   faces: by cell n, then table order;   scenes concatenated.
 * A face holds three vertex ids local to its scene (global id - vertex_offsets[b]).  An axis of size 1 has no cells: the mesh is empty.
 *   lp_mesh_workspace_bytes: shapes only (no device): 4 bytes per lattice point + 16 bytes per 256 points (+ the small upper levels
 *                            of the scan), or a negative LP_E* code.
 *   lp_mesh_count:  count pass + scan.  WRITES every element of vertex_offsets / face_offsets ([B + 1] int64: entry b = vertices /
 *                   faces of the scenes before b, entry B = the totals) and the workspace.  Reads volume.
 *   lp_mesh_emit:   after lp_mesh_count with the same arguments and workspace (which it reads, with vertex_offsets).  WRITES
 *                   vertices[i], normals[i] for every i < min(total vertices, max_vertices) and faces[i] for every
 *                   i < min(total faces, max_faces); touches nothing at or beyond a capacity -- the offsets keep the true counts, so
 *                   the caller detects the overflow.  normals == NULL: none; else the unit vector along -(gradient), the gradient by
 *                   central differences (one-sided at the border) in scene coordinates at the two endpoints, interpolated with t;
 *                   (0, 0, 0) where it vanishes or is not finite.
 * No atomics, nothing waits on another workgroup (the scan is a hierarchy of separate launches), no host synchronisation, no
 * allocation: graph-capturable and bit-reproducible.  Every device pointer is 16-byte aligned (Conventions).  Before anything touches
 * the device: LP_ENULL for NULL args / volume / offsets / workspace, or a NULL vertices / faces with a capacity > 0; LP_EINVAL for an
 * extent < 1, a negative capacity, an under-aligned pointer, a workspace smaller than lp_mesh_workspace_bytes(); LP_EUNSUPPORTED
 * for B D H W >= 2^31.  The vertices of one scene have to stay below 2^31 (int32 ids). */
typedef struct LpMeshArgs {
  const float* volume;      /* [B, D, H, W] (read) */
  LpGrid shape;             /* B, D, H, W (row_offset and data ignored) */
  float level;
  int32_t reserved;         /* 0 */
  int64_t* vertex_offsets;  /* [B + 1] (count: written; emit: read) */
  int64_t* face_offsets;    /* [B + 1] (count: written) */
  float* vertices;          /* emit: [max_vertices, 3] (written below the count) */
  int32_t* faces;           /* emit: [max_faces, 3] (written below the count) */
  float* normals;           /* emit: NULL or [max_vertices, 3] (written below the count) */
  int64_t max_vertices, max_faces;
} LpMeshArgs;
int64_t lp_mesh_workspace_bytes(const LpMeshArgs* args);
int lp_mesh_count(const LpMeshArgs* args, void* workspace, int64_t workspace_bytes, void* stream);
int lp_mesh_emit(const LpMeshArgs* args, void* workspace, int64_t workspace_bytes, void* stream);

/* out[i] = hash_randn(x1[i], x2[i], seed), i < n (test hook for the opacity-noise RNG). */
int lp_hash_randn(const int32_t* x1, const int32_t* x2, float* out, int64_t n, int32_t seed,
                  void* stream);

/* Debug / parity hook: integer corner rows of the Renderer march.  For grid g of
 * args->grid writes rows[(ray*S_tot + step)*K_tot + k] (int64, -1 = corner out of
 * range), K_tot = sum over grids of 8 (voxel) / 4 (plane), grids concatenated in
 * list order.  Used by the tests to prove bit-exact integer indexing vs the oracle. */
int lp_renderer_corner_rows(const LpRendererArgs* args, int64_t* rows, void* stream);

/* Debug / parity hook: lp_renderer_backward() through the DUMP twin of the kernel it would launch (same template, same
 * instruction sequence, stores added), which also writes the ReLU decisions of the backward's decoder recompute:
 * dump[(ray * S_tot + sample) * 5 + {0: trunk layer 1, 1: trunk layer 2 (the trunk output), 2: opacity hidden, 3: colour
 * hidden}] = bit f set when unit f is active, word 4 = 1 (sample contributed), 2 (visited, not contributing: beyond the ray's
 * last marched sample), 0 (never visited).  dump_words must be n_rays * S_tot * lp_renderer_relu_dump_words(args).  Every kernel
 * family has dump twins -- the tuned bf16x3 family (1; four-wave workgroups, default arithmetic), the layer-looped family (3) and the
 * shape-generic kernels (0): LP_EUNSUPPORTED for LP_ARITH_FP32, for the tuned family's eight-wave workgroups (> 64 beyond-far samples)
 * and in a library built without -DLP_TEST_HOOKS (lp_build_info() "test_hooks": 0).  The tests force these decisions onto the
 * fp64 oracle and require every gradient entry within 1e-4 (tests/test_gpu_config_scale.py::test_flips_are_flips). */
int lp_renderer_backward_relu_dump(const LpRendererArgs* args, uint32_t* dump, int64_t dump_words, void* stream);
/* Words per (ray, sample) of that dump for these arguments (shapes only, no launch), or LP_EUNSUPPORTED:
 *   family 1: 5 (above);
 *   family 3 (layer-looped): NB * n_sites + 1, NB = 32-bit words per ReLU site (1 up to 32 units, 2 for hidden width 64 / 64 grid
 *     channels), sites in the reference's evaluation order (naive_renderer.py:328-501) -- single grid-list: trunk layers 1 .. n_t,
 *     opacity hidden layers, colour hidden layers; two-grid decoder: relu(sampled feature), opacity hidden layers, relu(sampled
 *     colour feature), colour hidden layers -- word k * NB + b holds units 32 b .. 32 b + 31 of site k, the last word the
 *     visited flag (1 / 2 / 0 as above);
 *   family 0 (shape-generic, also LP_KERNEL_GENERIC): the same layout with NB = ceil(widest site / 32). */
int lp_renderer_relu_dump_words(const LpRendererArgs* args);

/* Debug / parity hook: lp_splatter_backward() of an MLP-Splatter through the DUMP twin of the kernel it would launch (layer-looped
 * family 3 -- every instantiation, two-layer kernel included -- or the shape-generic kernel), which also writes the ReLU decisions of
 * the backward's MLP recompute: per (ray, sample) lp_mlp_splatter_relu_dump_words(args) words -- for each hidden layer l (the ReLU
 * sites in the oracle's call order) ceil(dims[l + 1] / 32) words, bit f of word b set when unit 32 b + f is active, then one flag
 * word: 1 (live sample), 2 (visited, masked out of bounds), 0 (never visited).  dump_words must be n_rays * S_tot * that count; the
 * caller zero-fills.  LP_EUNSUPPORTED in a library built without -DLP_TEST_HOOKS. */
int lp_mlp_splatter_backward_relu_dump(const LpSplatterArgs* args, uint32_t* dump, int64_t dump_words, void* stream);
/* Words per (ray, sample) of that dump for these arguments (shapes only, no launch). */
int lp_mlp_splatter_relu_dump_words(const LpSplatterArgs* args);
/* How an MLP-Splatter of these arguments is launched (shapes and batch size only, no launch): shape[0] kernel family (3 / 0, as
 * lp_splatter_kernel_family, 0 also for LP_KERNEL_GENERIC), shape[1] forward waves per workgroup (4 or 8; 1 for the generic
 * kernels), shape[2] backward segments per ray (1 = one sweep), shape[3] layers the backward instantiation is unrolled for (2: the
 * two-layer kernel at two waves per SIMD, 4: the deep one, 0: generic), shape[4] 32-unit blocks per layer (0: generic), shape[5]
 * forward segments per ray.  shape must hold 6 int32. */
int lp_mlp_splatter_launch_shape(const LpSplatterArgs* args, int32_t* shape);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTPLANE_HIP_H */
