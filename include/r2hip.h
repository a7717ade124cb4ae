/*
 * r2hip.h -- C ABI of libr2hip.so, the MI355X (gfx950) implementation of the R2-Gaussian hot path:
 * differentiable X-ray rasterizer, 3D voxelizer and simple-knn.
 *
 * Every entry point replaces one function of the reference's native layer L0/L1
 * (paths relative to r2_gaussian/submodules/xray-gaussian-rasterization-voxelization/ = SUB):
 *
 *   r2_raster_forward     <- CudaRasterizer::Rasterizer::forward      SUB/cuda_rasterizer/rasterizer.h:36-56,  rasterizer_impl.cu:196-331
 *   r2_raster_backward    <- CudaRasterizer::Rasterizer::backward     SUB/cuda_rasterizer/rasterizer.h:58-85,  rasterizer_impl.cu:335-421
 *   r2_mark_visible       <- CudaRasterizer::Rasterizer::markVisible  SUB/cuda_rasterizer/rasterizer.h:29-34,  rasterizer_impl.cu:141-153
 *   r2_voxel_forward      <- CudaVoxelizer::Voxelizer::forward        SUB/cuda_voxelizer/voxelizer.h:28-47,    voxelizer_impl.cu:171-302
 *   r2_voxel_backward     <- CudaVoxelizer::Voxelizer::backward       SUB/cuda_voxelizer/voxelizer.h:49-72,    voxelizer_impl.cu:307-389
 *   r2_knn_dist2          <- simple_knn._C.distCUDA2 (un-vendored submodule; call site r2_gaussian/gaussian/gaussian_model.py:145-150)
 *
 * Conventions (identical to the reference's L0):
 *   - all data pointers are DEVICE pointers to contiguous float32 / int32 arrays owned by the caller;
 *   - "absent" optional inputs (scales/rotations vs cov3D_precomp) are passed as NULL;
 *   - 4x4 matrices are 16 floats indexed m[col*4+row] (== row-major memory of the transposed
 *     matrices torch hands over: world_view_transform, full_proj_transform);
 *   - the library never allocates result/state memory: it asks the caller for bytes through the
 *     three r2_alloc_fn callbacks, the C form of the reference's std::function<char*(size_t)>
 *     (SUB/utility.h:7-13).  The layout inside those buffers is private to the library;
 *   - gradient outputs of the backward calls are FULLY WRITTEN by the library (all-zero rows for culled
 *     Gaussians, for the scale/rotation gradients on the cov3D_precomp path, and the unused third component of
 *     dL_dmean2D): the zero-initialisation the reference's torch boundary performs
 *     (SUB/rasterize_points.cu:124-131, SUB/voxelize_points.cu:130-136) is not required;
 *   - `stream` is a hipStream_t (NULL = the null stream).  Work is enqueued on it; the forward
 *     calls synchronise that stream once to learn num_rendered (the reference's cudaMemcpy D2H,
 *     rasterizer_impl.cu:279), the backward calls do not synchronise;
 *   - return value: >= 0 on success (forward: num_rendered), < 0 = -(hipError_t) or R2_ERR_*;
 *     r2_last_error() gives a message.  With debug != 0 the stream is synchronised and checked after
 *     every stage (the reference's CHECK_CUDA, SUB/cuda_rasterizer/auxiliary.h:170-177).
 */
#ifndef R2HIP_H
#define R2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define R2_API __attribute__((visibility("default")))
#else
#define R2_API
#endif

#define R2_ABI_VERSION 3
#define R2_ERR_INVALID (-10001) /* bad argument (NULL where data is required, negative size ...) */
#define R2_ERR_ALLOC   (-10002) /* an r2_alloc_fn callback returned NULL */

/* Returns a device pointer to at least `bytes` bytes (128-byte aligned), valid until the matching
 * backward call has been enqueued.  `user` is passed through untouched.
 * The rasterizer forward may call the binning and image callbacks a SECOND time within one call (tile-first chain: the state
 * was sized by a prediction that fell short and is asked for again with the exact size, see r2_tile_first_control).  Kernels
 * enqueued on `stream` before the second request still hold pointers into the first buffer (they find the true count on the
 * device and do nothing, but they do read and write a few words of it), so a callback that releases or reuses the first buffer
 * must do so IN STREAM ORDER on `stream` -- true of a stream-ordered allocator such as torch's caching allocator on the
 * current stream, of hipFreeAsync on `stream`, and of a synchronous hipFree; a callback that recycles memory on ANOTHER
 * stream must keep the first buffer alive until `stream` has passed the forward.  The buffer the backward must be given is the
 * one returned LAST. */
typedef char *(*r2_alloc_fn)(size_t bytes, void *user);

R2_API int r2_abi_version(void);
R2_API const char *r2_last_error(void);

/* Alignment.  All pointers are device pointers to float / int arrays and must be 4-byte aligned; the kernels move the
 * following arrays 16 bytes at a time, so THESE must be 16-byte aligned (any fresh torch / hipMalloc allocation is):
 *   rotations [P,4], dL_dpix [H,W] (rasterizer backward, when width % 16 == 0), dL_dconic [P,2,2], dL_drot [P,4] (both
 *   backwards), and the state buffers handed out by the r2_alloc_fn callbacks (128-byte aligned).
 * The torch boundaries (r2_gaussian_amd/_C.py, csrc/torch_shim.cpp) copy an input whose data pointer is not 16-byte
 * aligned (e.g. a view into a flat parameter buffer at an odd offset) before passing it down.
 * Devices / threads.  Calls take the caller's HIP stream; the device that stream belongs to must be current (hipSetDevice)
 * in the calling thread, as for every HIP API that takes a stream.  A host thread may drive several devices.
 * num_rendered.  The forward calls return the number of (tile, Gaussian) instances as a non-negative int; a scene whose
 * instance count does not fit 31 bits is rejected with R2_ERR_INVALID (the reference's int num_rendered has the same range).
 */

/* ---- rasterizer ------------------------------------------------------------------------------ */
R2_API int r2_raster_forward(
    r2_alloc_fn geometryBuffer, void *geometry_user,
    r2_alloc_fn binningBuffer, void *binning_user,
    r2_alloc_fn imageBuffer, void *image_user,
    int P, int width, int height,
    const float *means3D,      /* [P,3] */
    const float *opacities,    /* [P]   activated density */
    const float *scales,       /* [P,3] or NULL */
    float scale_modifier,
    const float *rotations,    /* [P,4] (r,x,y,z) or NULL */
    const float *cov3D_precomp,/* [P,6] or NULL */
    const float *viewmatrix,   /* [16] */
    const float *projmatrix,   /* [16] */
    const float *cam_pos,      /* [3], unused by the X-ray path (kept for signature parity) */
    float tan_fovx, float tan_fovy,
    int prefiltered,
    int mode,                  /* 0 parallel beam, 1 cone beam */
    float *out_color,          /* [1,H,W] */
    int *radii,                /* [P] */
    int debug,
    void *stream);

R2_API int r2_raster_backward(
    int P, int R, int width, int height,
    const float *means3D, const float *scales, float scale_modifier, const float *rotations,
    const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, const float *campos,
    float tan_fovx, float tan_fovy,
    const int *radii,
    char *geom_buffer, char *binning_buffer, char *img_buffer,
    const float *dL_dpix,      /* [1,H,W] */
    float *dL_dmean2D,         /* [P,3] (z stays 0) */
    float *dL_dconic,          /* [P,2,2] (slots 0,1,3); 16-byte aligned */
    float *dL_dopacity,        /* [P,1] */
    float *dL_dmu,             /* [P,1] */
    float *dL_dmean3D,         /* [P,3] */
    float *dL_dcov3D,          /* [P,6] */
    float *dL_dscale,          /* [P,3] */
    float *dL_drot,            /* [P,4] */
    int mode, int debug, void *stream);

R2_API int r2_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                    uint8_t *present /* [P] bool */, void *stream);

/* ---- rasterizer, batched views (NEW functionality: the reference renders one view per call) ----
 * V views of the SAME Gaussians (same detector size, tan_fov and mode; V camera poses) through one pass of the pipeline:
 * the views become V * P "view instances" on a tile grid that stacks the views' grids, so every latency-bound stage
 * (preprocess, depth order, instance emission, tile sort) runs once on V times the work.  A trainer that accumulates
 * several views per optimiser step (view-sharded data parallelism) calls these instead of V single-view
 * calls.  Every view is evaluated with exactly the arithmetic of r2_raster_forward / r2_raster_backward: out_color[v] and
 * radii[v] are bit-identical to the single-view call's, tile lists too.
 *   forward : viewmatrices / projmatrices [V,16]; out_color [V,H,W]; radii [V,P]; returns num_rendered over all views;
 *             width * height need not be tile-aligned.
 *   backward: dL_dpix [V,H,W]; per view: dL_dmean2D [V,P,3], dL_dconic [V,P,2,2], dL_dmu [V,P]; SUMMED over the views (in
 *             view order, deterministic): dL_dopacity [P], dL_dmean3D [P,3], dL_dcov3D [P,6], dL_dscale [P,3], dL_drot [P,4]. */
R2_API int r2_raster_forward_batch(
    r2_alloc_fn geometryBuffer, void *geometry_user,
    r2_alloc_fn binningBuffer, void *binning_user,
    r2_alloc_fn imageBuffer, void *image_user,
    int P, int V, int width, int height,
    const float *means3D, const float *opacities, const float *scales, float scale_modifier, const float *rotations,
    const float *cov3D_precomp,
    const float *viewmatrices, /* [V,16] */
    const float *projmatrices, /* [V,16] */
    float tan_fovx, float tan_fovy, int mode,
    float *out_color,          /* [V,H,W] */
    int *radii,                /* [V,P] */
    int debug, void *stream);

R2_API int r2_raster_backward_batch(
    int P, int V, int R, int width, int height,
    const float *means3D, const float *scales, float scale_modifier, const float *rotations,
    const float *cov3D_precomp, const float *viewmatrices, const float *projmatrices,
    float tan_fovx, float tan_fovy,
    const int *radii,          /* [V,P] */
    char *geom_buffer, char *binning_buffer, char *img_buffer,
    const float *dL_dpix,      /* [V,H,W] */
    float *dL_dmean2D,         /* [V,P,3] */
    float *dL_dconic,          /* [V,P,2,2]; 16-byte aligned */
    float *dL_dopacity,        /* [P,1]   summed over the views */
    float *dL_dmu,             /* [V,P] */
    float *dL_dmean3D,         /* [P,3]   summed */
    float *dL_dcov3D,          /* [P,6]   summed */
    float *dL_dscale,          /* [P,3]   summed */
    float *dL_drot,            /* [P,4]   summed */
    int mode, int debug, void *stream);

/* ---- loss stack of the training iteration (r2_gaussian/utils/loss_utils.py:19-104, train.py:118-147) ----
 * r2_loss_l1_ssim: loss = w_l1 * mean|img - gt| + w_ssim * (1 - SSIM(img, gt)) (11x11 Gaussian window, sigma 1.5, zero
 * padding) of one [height,width] projection AND its gradient dL/dimg, in two launches; scalars = {l1 mean, ssim mean, loss}.
 * r2_loss_tv3d: tv = tv_3d_loss(vol, "mean") of a [nx,ny,nz] volume and dL/dvol = weight * d tv / d vol; scalars = {tv,
 * weight * tv}; a volume without neighbour pairs (1 x 1 x 1) gives tv = NaN (0 / 0, as the reference) and a zero gradient.
 * scratch: device floats, at least r2_loss_*_scratch_floats(...).  Per-block sums are folded in a fixed order in double.
 * r2_loss_l1_ssim_batch: V >= 1 projections imgs [V,height,width] against V ground truths, for the loss
 *   mean over the views v of  w_l1 * mean|img_v - gt_v| + w_ssim * (1 - SSIM(img_v, gt_v)),
 * forward and gradient, by the kernels of r2_loss_l1_ssim: their grid's third dimension is the view, and r2_loss_l1_ssim is
 * their launch with one view and no batch row (so it refuses an image beyond the grid bound below as well).  gts_host: a
 * HOST array of V device pointers, each to a [height,width] image (a step's ground truths are picks from a training set and
 * need not be contiguous with each other; they are read in place).  The table travels to the kernels by value,
 * R2_LOSS_BATCH_CHUNK views per pair of launches: ceil(V / R2_LOSS_BATCH_CHUNK) * 2 launches, no host synchronisation, no
 * allocation, no copy.  V is bounded only by the grid: V * ceil(width / 16) * ceil(height / 16) must fit 31 bits.
 *   scalars [V + 1][3]: row v < V = {l1 mean, ssim mean, loss} of view v, bit-identical to what r2_loss_l1_ssim(img_v, gt_v,
 *     w_l1, w_ssim) writes; row V = the means of those float rows over the views, summed in view order in double.
 *   dL_dimg [V,height,width]: the gradient of the batch loss; dL_dimg[v] is bit-identical to what r2_loss_l1_ssim(img_v,
 *     gt_v, w_l1 / V, w_ssim / V) writes, the two quotients formed in float.
 *   scratch: at least r2_loss_l1_ssim_batch_scratch_floats(V, width, height) device floats, 8-byte aligned ([V][3][height]
 *     [width] derivative maps, then every view's per-block partial sums); 0 for sizes the call rejects.
 *   R2_ERR_INVALID: V < 1, width or height <= 0, a NULL imgs / gts_host / gts_host[v] / dL_dimg / scratch / scalars, a
 *     grid beyond the bound above (also more than 65535 tiles of 16 rows: height > 1048560).  r2_loss_l1_ssim: the same
 *     with V = 1. */
R2_API size_t r2_loss_l1_ssim_scratch_floats(int width, int height);
R2_API int r2_loss_l1_ssim(int width, int height, const float *img, const float *gt, float w_l1, float w_ssim,
                           float *dL_dimg, float *scratch, float *scalars /* [3] */, void *stream);
#define R2_LOSS_BATCH_CHUNK 16 /* ground-truth pointers per launch of r2_loss_l1_ssim_batch */
R2_API size_t r2_loss_l1_ssim_batch_scratch_floats(int V, int width, int height);
R2_API int r2_loss_l1_ssim_batch(int V, int width, int height, const float *imgs /* [V,H,W] */,
                                 const float *const *gts_host /* V device pointers */, float w_l1, float w_ssim,
                                 float *dL_dimg /* [V,H,W] */, float *scratch, float *scalars /* [V + 1][3] */, void *stream);
/* r2_loss_l1_ssim_weighted: the same loss with per-pixel weights w [height,width] (a 0/1 mask is the special case; the
 * penalised weighted least squares of CT reconstruction).  A weight counts only where it is > 0: a negative, zero or NaN
 * weight is 0; the others must be finite.  A pixel of weight 0 is unmeasured: its gt is never used as a value (it may hold
 * NaN, Inf or anything else), the measurement taken in its place is the image's own value there, held constant:
 *   y'(p) = w(p) > 0 ? gt(p) : img(p),  sum_w = sum_p w(p),  S = the SSIM map of (img, y') as r2_loss_l1_ssim forms it,
 *   l1 = sum w |img - y'| / sum_w,  ssim = sum w S / sum_w,  loss = w_l1 * l1 + w_ssim * (1 - ssim),
 *   dL/dimg(p) = w_l1 w(p) sign(img(p) - y'(p)) / sum_w
 *                - w_ssim / sum_w * sum_q W(q - p) w(q) [D1(q) + 2 img(p) D2(q) + y'(p) D3(q)]
 * (r2_loss_l1_ssim's formula with 1 / N -> 1 / sum_w, D_i -> w D_i, gt -> y'; an unmeasured pixel still receives the SSIM part
 * through its weighted neighbours).  sum_w = 0 (no measured pixel): l1 = 0, ssim = 1, loss = 0 and a gradient of zeros, no
 * NaN.  weights == NULL is a weight of 1 everywhere; that, and an array of ones, give the bits of r2_loss_l1_ssim.  Scaling
 * all weights by a power of two changes no bit of the gradient or of the first three scalars.
 *   scalars [4] = {l1, ssim, loss, sum_w}: per-block sums folded in a fixed order in double, sum_w rounded to float once.
 *   Three launches (forward, a one-block fold of sum_w and the scalars, backward); no atomics, no host synchronisation, no
 *   allocation; bit-reproducible.  scratch: at least r2_loss_l1_ssim_weighted_scratch_floats(width, height) device floats,
 *   8-byte aligned; 0 for sizes the call rejects.
 *   R2_ERR_INVALID: width or height <= 0, a NULL img / gt / dL_dimg / scratch / scalars, a grid beyond the batch bound.
 * r2_loss_l1_ssim_weighted_batch: V >= 1 views for the mean over the views of each view's own weighted loss (every view is
 * normalised by its own sum_w), three launches per R2_LOSS_BATCH_CHUNK views.  weights_host: NULL (unit weights for every
 * view), or a HOST array of V device pointers, each to a [height,width] array or NULL (unit weights for that view).
 *   scalars [V + 1][4]: row v < V is bit-identical to what r2_loss_l1_ssim_weighted(img_v, gt_v, weights_v, w_l1, w_ssim)
 *     writes; row V = the means of the first three columns of those float rows over the views, summed in view order in
 *     double, and the sum of their sum_w.  A view with sum_w = 0 contributes loss 0 and a zero gradient and still counts in V.
 *   dL_dimg [V,height,width]: dL_dimg[v] is bit-identical to what r2_loss_l1_ssim_weighted(img_v, gt_v, weights_v,
 *     w_l1 / V, w_ssim / V) writes, the two quotients formed in float.
 *   scratch: at least r2_loss_l1_ssim_weighted_batch_scratch_floats(V, width, height) device floats, 8-byte aligned.
 *   R2_ERR_INVALID: those of r2_loss_l1_ssim_batch; a NULL weights_host or weights_host[v] is allowed. */
R2_API size_t r2_loss_l1_ssim_weighted_scratch_floats(int width, int height);
R2_API int r2_loss_l1_ssim_weighted(int width, int height, const float *img, const float *gt,
                                    const float *weights /* [H,W] or NULL = 1 */, float w_l1, float w_ssim,
                                    float *dL_dimg, float *scratch, float *scalars /* [4] */, void *stream);
R2_API size_t r2_loss_l1_ssim_weighted_batch_scratch_floats(int V, int width, int height);
R2_API int r2_loss_l1_ssim_weighted_batch(int V, int width, int height, const float *imgs /* [V,H,W] */,
                                          const float *const *gts_host /* V device pointers */,
                                          const float *const *weights_host /* NULL, or V device pointers, each may be NULL = 1 */,
                                          float w_l1, float w_ssim, float *dL_dimg /* [V,H,W] */, float *scratch,
                                          float *scalars /* [V + 1][4] */, void *stream);
R2_API size_t r2_loss_tv3d_scratch_floats(int nx, int ny, int nz);
R2_API int r2_loss_tv3d(int nx, int ny, int nz, const float *vol, float weight, float *dL_dvol, float *scratch,
                        float *scalars /* [2] */, void *stream);

/* ---- evaluation metrics (r2_gaussian/utils/image_utils.py:90-184: metric_vol, metric_proj; forward only) ----
 * r2_metric_slices: for every 2D slice of a C-contiguous float32 [n0,n1,n2] array taken along `axis` (slice i of axis 1 is
 * a[:, i, :], rows n0, columns n2; of axis 2 a[:, :, i], rows n0, columns n1), per_slice[i] = {mean of the SSIM map (11x11
 * Gaussian window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2), sum (gt - pred)^2, max gt, max pred}, written on the
 * device.  flags: R2_METRIC_SSIM computes the SSIM field (NaN without it: an SSE / maximum pass only); R2_METRIC_NORMALIZE
 * divides each slice of both inputs by its own maximum first, as metric_proj does (the maxima fields stay those of the
 * inputs).  No host synchronisation; sums are formed in a fixed order, in double per slice (bit-reproducible).  scratch:
 * device floats, 16-byte aligned, at least r2_metric_slices_scratch_floats(n0, n1, n2, axis) (axis 2 includes a transposed
 * copy of both inputs).  At most 65535 slices. */
#define R2_METRIC_SSIM      1
#define R2_METRIC_NORMALIZE 2
R2_API size_t r2_metric_slices_scratch_floats(int n0, int n1, int n2, int axis);
R2_API int r2_metric_slices(int n0, int n1, int n2, int axis, const float *gt, const float *pred, int flags,
                            float *per_slice /* [n_axis][4] */, float *scratch, void *stream);

/* ---- adaptive density control on the device (r2_gaussian/gaussian/gaussian_model.py:320-556, train.py:151-168) ----
 * r2_densify_stats: max_radii2D / xyz_gradient_accum / denom update of one rendered view (in place, one launch).
 * r2_densify_stats_batch: the same for the V >= 1 views of a batched render (radii [V,P], dL_dmeans2D [V,P,3], the layouts of
 *   r2_raster_forward_batch / r2_raster_backward_batch) in ONE launch: for every view in order and every Gaussian with
 *   radii > 0: max_radii2D = max(., radii), grad_accum += grad_scale * ||dL_dmeans2D[:2]||, denom += 1.  A thread owns a
 *   Gaussian and walks the views in order, so with grad_scale == 1 the result is bit-identical to V calls of r2_densify_stats
 *   in view order.  grad_scale: a step whose loss is the MEAN over its V views leaves 1 / V of each view's own gradient in
 *   dL_dmeans2D; grad_scale = V gives the statistics of the views' own losses (exact for V a power of two), which keeps the
 *   densification threshold a per-view quantity.  P == 0 enqueues nothing; P < 0, V < 1 or a NULL array: R2_ERR_INVALID.
 * r2_densify_classify + r2_densify_emit: densify_and_prune -- clone (small Gaussians with a large view-space gradient; both
 * copies get half the density), split (large ones: two children sampled from N(0, scale) in the local frame, scale / 1.6,
 * half the density, parent removed), prune (density below density_min, outside the box) -- with the Adam moments carried
 * along (zeros for new rows) and the statistics reset, written in the reference's row order.  classify decides, counts and
 * synchronises the stream ONCE to return the four survivor counts (originals, clones, first children, second children);
 * the caller allocates sum(counts) rows and calls emit with the same arguments and the same scratch.  normals: [2,P,3]
 * N(0,1) samples indexed by the PARENT's row (only rows of split parents are read).  scale_lo < scale_hi: bounded-sigmoid
 * scaling activation, else exp.  max_screen_size / max_scale: the reference's optional prune thresholds (rows whose
 * max_radii2D / largest activated scale exceed them are pruned, gaussian_model.py:540-545); <= 0 switches them off (None).
 * params / exp_avg / exp_avg_sq (+ _out): 4 device pointers each in the order xyz[.,3], density[.,1], scaling[.,3], rotation[.,4].
 * The moment tables may be NULL; an array's moments move when its four moment arrays (in and out) are all there.  P <= 0, a
 * NULL array, or an array with some but not all four of its moment arrays: R2_ERR_INVALID before anything is launched. */
R2_API int r2_densify_stats(int P, const int *radii, const float *dL_dmeans2D /* [P,3] */, float *max_radii2D, float *grad_accum,
                            float *denom, void *stream);
R2_API int r2_densify_stats_batch(int P, int V, const int *radii /* [V,P] */, const float *dL_dmeans2D /* [V,P,3] */,
                                  float grad_scale, float *max_radii2D, float *grad_accum, float *denom, void *stream);
R2_API size_t r2_densify_scratch_bytes(int P);
R2_API int r2_densify_classify(int P, const float *xyz, const float *density, const float *scaling, const float *rotation,
                               const float *max_radii2D, const float *grad_accum, const float *denom, const float *normals,
                               float grad_thr, float scale_thr, float density_min,
                               const float *bbox_host /* 6 host floats: lo xyz, hi xyz */, float scale_lo, float scale_hi,
                               int do_densify, float max_screen_size, float max_scale, void *scratch,
                               unsigned int *counts_host /* [4] */, void *stream);
R2_API int r2_densify_emit(int P, const float *const *params, const float *const *exp_avg, const float *const *exp_avg_sq,
                           const float *max_radii2D, const float *grad_accum, const float *denom, const float *normals,
                           float grad_thr, float scale_thr, float density_min, const float *bbox_host, float scale_lo,
                           float scale_hi, int do_densify, float max_screen_size, float max_scale, const void *scratch,
                           float *const *params_out, float *const *exp_avg_out,
                           float *const *exp_avg_sq_out, float *max_radii2D_out, float *grad_accum_out, float *denom_out,
                           void *stream);

/* ---- model step of a training iteration (r2_gaussian/gaussian/gaussian_model.py:38-64, 112-126, 188-254; train.py:174-176) ----
 * r2_gaussian_activate replaces the activation properties get_density / get_scaling / get_rotation (gaussian_model.py:112-126):
 *   density_act = softplus(density) with torch's beta 1, threshold 20 (x > 20: x); scaling_act = sigmoid(x) * (hi - lo) + lo with
 *   a scale bound, exp(x) without one; rotation_act = q / max(|q|, 1e-12).  xyz's activation is the identity (no output).
 * r2_gaussian_adam_step replaces torch.optim.Adam.step() over the model's four parameter groups (gaussian_model.py:188-215:
 *   betas (0.9, 0.999) and eps 1e-15, FIXED; no weight decay, no amsgrad) together with the backward of the activations, and
 *   writes the NEXT iteration's activated parameters in the same pass.  grads[k] is dL/d(activated parameter k) -- what autograd
 *   leaves in the .grad of the activated leaves -- and is chained through the activation's derivative as torch's backward
 *   formulas compute it (softplus_backward's threshold, the sigmoid derivative (1 - y) y, exp, the normalize Jacobian
 *   (g - q^(q^.g)) / |q|); then, in torch's non-fused order:  m = m + (1 - b1)(g - m);  v = v b2 + (1 - b2) g g;
 *   denom = sqrt(v) / sqrt(bias_correction2[k]) + eps;  p = p - (lr[k] / bias_correction1[k]) m / denom.  The host computes
 *   lr and both bias corrections in double from the group's step count (1 - beta^step); the call reads nothing back from the
 *   device and does not synchronise.  grads[k] == NULL: group k is left untouched (no parameter, moment or step change),
 *   as torch skips a parameter without .grad; its activated output is still written.
 * params / grads / exp_avg / exp_avg_sq: 4 device pointers each in the order xyz [P,3], density [P,1], scaling [P,3],
 *   rotation [P,4]; parameters and moments are updated in place.  Validation (R2_ERR_INVALID): P < 0; a NULL pointer array
 *   or activation output; a NULL parameter; NULL moments of a group with a gradient; lr < 0 or a bias correction <= 0 in such
 *   a group; a scale bound other than scale_lo < scale_hi (bounded sigmoid) or scale_lo == scale_hi == 0 (exp, no bound);
 *   rotation arrays not 16-byte aligned.  P == 0 enqueues nothing. */
R2_API int r2_gaussian_activate(int P, const float *density, const float *scaling, const float *rotation, double scale_lo,
                                double scale_hi, float *density_act /* [P,1] */, float *scaling_act /* [P,3] */,
                                float *rotation_act /* [P,4] */, void *stream);
R2_API int r2_gaussian_adam_step(int P, float *const *params, const float *const *grads, float *const *exp_avg,
                                 float *const *exp_avg_sq, const double *lr /* [4] */, const double *bias_correction1 /* [4] */,
                                 const double *bias_correction2 /* [4] */, double scale_lo, double scale_hi,
                                 float *density_act, float *scaling_act, float *rotation_act, void *stream);

/* ---- voxelizer ------------------------------------------------------------------------------- */
R2_API int r2_voxel_forward(
    r2_alloc_fn geometryBuffer, void *geometry_user,
    r2_alloc_fn binningBuffer, void *binning_user,
    r2_alloc_fn imageBuffer, void *image_user,
    int P,
    int nVoxel_x, int nVoxel_y, int nVoxel_z,
    float sVoxel_x, float sVoxel_y, float sVoxel_z,
    float center_x, float center_y, float center_z,
    const float *means3D, const float *opacities, const float *scales, float scale_modifier,
    const float *rotations, const float *cov3D_precomp,
    int prefiltered,
    float *out_volume,         /* [nx,ny,nz] */
    int *radii_x, int *radii_y, int *radii_z, /* [P] each */
    int debug, void *stream);

R2_API int r2_voxel_backward(
    int P, int R,
    int nVoxel_x, int nVoxel_y, int nVoxel_z,
    float sVoxel_x, float sVoxel_y, float sVoxel_z,
    float center_x, float center_y, float center_z,
    const float *means3D, const float *scales, float scale_modifier, const float *rotations,
    const float *cov3D_precomp,
    const int *radii_x, const int *radii_y, const int *radii_z,
    char *geom_buffer, char *binning_buffer, char *img_buffer,
    const float *dL_dvol,      /* [nx,ny,nz] */
    float *dL_dmean3D_norm,    /* [P,3] */
    float *dL_dconic3D,        /* [P,6] */
    float *dL_dopacity,        /* [P,1] */
    float *dL_dmean3D,         /* [P,3] */
    float *dL_dcov3D,          /* [P,6] */
    float *dL_dscale,          /* [P,3] */
    float *dL_drot,            /* [P,4] */
    int debug, void *stream);

/* ---- voxelizer, one x-slab of the grid (NEW functionality: the unit of the sharded full-volume query) ----
 * Tile layers [tile_x0, tile_x1) along x (layers of 8 voxels; 0 <= tile_x0 < tile_x1 <= ceil(nVoxel_x / 8)) of the volume the
 * other arguments describe -- nVoxel / sVoxel / center are the FULL volume's, exactly as for r2_voxel_forward.  The call evaluates
 * the full grid's arithmetic (voxel size, voxel-space positions, radii, tile cubes, distances to the voxel centres) and bins /
 * renders only the slab's tiles: out_volume is the [min(8 tile_x1, nVoxel_x) - 8 tile_x0, ny, nz] block of the full volume,
 * BIT-IDENTICAL to the same voxels of r2_voxel_forward's result, and the slab's tile lists are the full call's lists of those tiles
 * (reference: ONE grid with one arithmetic, test.py:105-112, SUB/cuda_voxelizer/forward.cu:58-178, voxelizer_impl.cu:54-101).
 * Slabs are independent: no exchange between them.  radii_{x,y,z}: the full call's radii for Gaussians with a tile in the slab, 0
 * for the others.  Returns the slab's num_rendered.  r2_voxel_forward(...) == r2_voxel_forward_slab(..., 0, ceil(nVoxel_x / 8), ...).
 * The backward takes the same two numbers; dL_dvol is the slab's block. */
R2_API int r2_voxel_forward_slab(
    r2_alloc_fn geometryBuffer, void *geometry_user,
    r2_alloc_fn binningBuffer, void *binning_user,
    r2_alloc_fn imageBuffer, void *image_user,
    int P,
    int nVoxel_x, int nVoxel_y, int nVoxel_z,
    float sVoxel_x, float sVoxel_y, float sVoxel_z,
    float center_x, float center_y, float center_z,
    int tile_x0, int tile_x1,
    const float *means3D, const float *opacities, const float *scales, float scale_modifier,
    const float *rotations, const float *cov3D_precomp,
    int prefiltered,
    float *out_volume,         /* [slab nx,ny,nz] */
    int *radii_x, int *radii_y, int *radii_z, /* [P] each */
    int debug, void *stream);

R2_API int r2_voxel_backward_slab(
    int P, int R,
    int nVoxel_x, int nVoxel_y, int nVoxel_z,
    float sVoxel_x, float sVoxel_y, float sVoxel_z,
    float center_x, float center_y, float center_z,
    int tile_x0, int tile_x1,
    const float *means3D, const float *scales, float scale_modifier, const float *rotations,
    const float *cov3D_precomp,
    const int *radii_x, const int *radii_y, const int *radii_z,
    char *geom_buffer, char *binning_buffer, char *img_buffer,
    const float *dL_dvol,      /* [slab nx,ny,nz] */
    float *dL_dmean3D_norm, float *dL_dconic3D, float *dL_dopacity, float *dL_dmean3D, float *dL_dcov3D, float *dL_dscale,
    float *dL_drot,
    int debug, void *stream);

/* ---- simple-knn ------------------------------------------------------------------------------ */
/* mean of the 3 smallest squared distances to the other points; out[P].  The exact uniform-grid search (P >= 4096) works inside
 * a caller-provided workspace of r2_knn_workspace_bytes(P) bytes (any alignment >= 256 B); without one (NULL / too small) the
 * exhaustive O(P^2) kernel runs, which needs none.  Synchronises the stream twice (bounding box, fullest cell): it is called
 * once per training run (gaussian_model.py:145-150). */
R2_API size_t r2_knn_workspace_bytes(int P);
R2_API int r2_knn_dist2_ws(int P, const float *points /* [P,3] */, float *out /* [P] */, void *workspace, size_t workspace_bytes,
                           void *stream);
/* the reference's signature: obtains the workspace itself (hipMalloc; hipFree after waiting for the stream) -- the one entry
 * point of the library that allocates; callers with an allocator use the two above */
R2_API int r2_knn_dist2(int P, const float *points /* [P,3] */, float *out /* [P] */, void *stream);

/* ---- neighbour graphs and the smoothness loss (no counterpart in the reference) -------------- */
/* r2_knn_graph: the K nearest neighbours of every point, with their indices.
 *   Distance: formed as r2_knn_dist2 forms it, in float32 without contraction: d = other - self per axis, then
 *     (dx*dx + dy*dy) + dz*dz, every operation rounded.
 *   Neighbours of i: all j != i (self excluded by INDEX; a duplicate of i at distance 0 counts), ordered by the pair
 *     (dist2 ascending, j ascending).  Row i of idx / dist2 holds the first K of that order, dist2 next to idx.
 *   The pair is a total order, so the rows do not depend on the order the search visits candidates in: the grid search, the
 *     exhaustive search and every hand-over between them (small P, degenerate or clustered clouds) produce the same bits.
 *   Short rows: where P - 1 < K the missing slots are idx = -1, dist2 = +inf.
 *   Arguments: 1 <= K <= R2_KNN_GRAPH_MAX_K, anything else is R2_ERR_INVALID (checked first); P = 0 is a no-op returning 0;
 *     P < 0, a NULL points / idx / dist2 or P * K >= 2^31: R2_ERR_INVALID.  The workspace rule is r2_knn_dist2_ws's: with
 *     r2_knn_graph_workspace_bytes(P, K) bytes (alignment >= 256 B) the grid search may run (P >= 4096), with NULL or fewer
 *     bytes the exhaustive kernel runs, which needs none.  With a workspace the call synchronises the stream twice.
 *   Non-finite coordinates: a cloud with a NaN or infinite coordinate takes the exhaustive search.  Guaranteed then: nothing
 *     outside the inputs is read, every idx is in [-1, P), rows are ascending in (dist2, idx) and the same on every call.  A
 *     NaN distance is never listed (its slot stays -1 / +inf); a distance that overflowed to +inf is listed like any other.
 * r2_graph_transpose: the incoming edges of every node in a fixed order.  An edge is e = i * K + k with target idx[e]; a
 *   target outside [0, P) (-1 included) makes the edge invalid.  in_edges[in_offsets[j] .. in_offsets[j + 1]) are the valid
 *   edges whose target is j, in ascending e; in_offsets[P] is the number of valid edges; the tail of in_edges [P * K] beyond
 *   that is unspecified.  Any idx is accepted, not only one from r2_knn_graph.  A stable radix sort of the edge ids by target
 *   and a binary search per node: no host read, no atomic.  P = 0 writes in_offsets[0] = 0.  P > 0 needs
 *   r2_graph_transpose_workspace_bytes(P, K) bytes (alignment >= 256 B), else R2_ERR_INVALID; K >= 1, P * K < 2^31.
 * r2_graph_loss: for per-node scalars v [P] and optional edge weights w [P,K] (NULL = 1),
 *     loss[0] = scale * sum over valid edges e = (i, k), j = idx[e], of w[e] * phi(v[i] - v[j]),
 *   phi(x) = |x| (R2_GRAPH_KIND_L1), x * x (R2_GRAPH_KIND_L2) or Huber with delta > 0 (R2_GRAPH_KIND_HUBER):
 *   0.5 * (x * x) for |x| <= delta, else delta * (|x| - 0.5 * delta).  Per term, in float32 without contraction:
 *   x = v[i] - v[j]; phi as written; then w[e] * phi when w is given.  The reduction has a fixed shape whatever P and K:
 *   workgroup b of 256 threads owns edges [2048 b, 2048 b + 2048), thread t adds its terms 2048 b + 256 k + t, k = 0 .. 7,
 *   in that order, a wave folds by xor butterfly (offsets 32 .. 1), the four waves combine as (s0 + s1) + (s2 + s3); the
 *   workgroups' partials (scratch: r2_graph_loss_scratch_floats(P, K) floats) are summed in double in a fixed order,
 *   multiplied by scale and rounded to float once.  R2_GRAPH_LOSS_CHAIN = 8 + 6 + 2 + 1 is the longest chain of float
 *   roundings between a term and the result; the same bits on every call.
 * r2_graph_loss_backward: with in_offsets / in_edges of r2_graph_transpose on the same idx and the upstream scalar g[0] (a
 *   device pointer),
 *     grad[i] = (g * scale) * ( sum_k w[i,k] phi'(v[i] - v[idx[i,k]])  -  sum over incoming e = (s, k) of w[e] phi'(v[s] - v[i]) ),
 *   phi'(x) = sign(x) with phi'(0) = 0, taken from the comparison of the two values (L1); 2 * x (L2); x for |x| <= delta,
 *   else delta with the sign of x (Huber).  One accumulator per node, starting at 0: the own row added in ascending k, then
 *   the incoming terms subtracted in list order; g * scale is formed first and multiplies the sum.  A node with more than
 *   R2_GRAPH_LOSS_HUB incoming edges has its list summed by its wave instead: lane l adds entries l, l + 64, ... of the list
 *   in that order, the 64 sums fold by xor butterfly (offsets 32 .. 1) and the result is subtracted from the own-row sum.
 *   Either order is a function of the lists alone: no atomics, bit-reproducible.  A node without valid edges gets +0.
 *   Differentiable in v only: the graph and the weights are structure.  kind outside 0..2, Huber with delta <= 0 (or NaN),
 *   K < 1, P < 0, P * K >= 2^31 or a NULL array with P > 0: R2_ERR_INVALID.  Targets outside [0, P) are skipped. */
#define R2_KNN_GRAPH_MAX_K 16
#define R2_GRAPH_KIND_L1 0
#define R2_GRAPH_KIND_L2 1
#define R2_GRAPH_KIND_HUBER 2
#define R2_GRAPH_LOSS_CHAIN 17
#define R2_GRAPH_LOSS_HUB 64
R2_API size_t r2_knn_graph_workspace_bytes(int P, int K);
R2_API int r2_knn_graph(int P, const float *points /* [P,3] */, int K, int *idx /* [P,K] */, float *dist2 /* [P,K] */,
                        void *workspace, size_t workspace_bytes, void *stream);
R2_API size_t r2_graph_transpose_workspace_bytes(int P, int K);
R2_API int r2_graph_transpose(int P, int K, const int *idx /* [P,K] */, int *in_offsets /* [P+1] */, int *in_edges /* [P*K] */,
                              void *workspace, size_t workspace_bytes, void *stream);
R2_API size_t r2_graph_loss_scratch_floats(int P, int K);
R2_API int r2_graph_loss(int P, int K, const float *v /* [P] */, const int *idx /* [P,K] */, const float *w /* [P,K] or NULL */,
                         int kind, float delta, float scale, float *scratch, float *loss /* [1] */, void *stream);
R2_API int r2_graph_loss_backward(int P, int K, const float *v, const int *idx, const float *w, const int *in_offsets,
                                  const int *in_edges, int kind, float delta, float scale, const float *g /* device scalar */,
                                  float *grad /* [P] */, void *stream);

/* ---- moment-preserving merging of neighbouring Gaussians (no counterpart in the reference) ---- */
/* Conventions of the three groups.  Gaussian i has mean mu_i, covariance Sigma_i = R^T diag(s^2) R with R = quat_to_rot(r, x, y, z)
 *   of the quaternion AS GIVEN (what cov3d_from_scale_rot forms with mod = 1; the activated rotation is a unit quaternion), and
 *   mass m_i = density_i * s1 s2 s3 (the factor (2 pi)^(3/2) cancels everywhere).  All four arrays are ACTIVATED parameters:
 *   means [P,3], density [P,1], scaling [P,3], rotation [P,4].  Every per-pair operation of r2_merge_cost and r2_merge_emit is
 *   double and the result is rounded to float once, at the store.  No atomics; every call gives the same bits; no host read
 *   except r2_merge_count's.  A graph is idx [P,K] with in_offsets / in_edges of r2_graph_transpose on the same idx; an edge
 *   e = i * K + k is valid when idx[e] is in [0, P), a self edge when idx[e] = i.
 *   Arguments: P = 0 is a no-op returning 0 (r2_merge_count then writes counts = {0, 0}); K < 1, P < 0, P * K >= 2^31 or a
 *   NULL array with P > 0: R2_ERR_INVALID.
 * r2_merge_cost: Runnalls' Kullback-Leibler bound of merging the two ends of every edge, per unit mass.  For a valid edge
 *   e = (i, k), j = idx[e] != i: a = min(i, j), b = max(i, j) (the two directions of a pair run the same operations on the same
 *   operands: the same bits), alpha = m_a / (m_a + m_b), d = mu_a - mu_b,
 *     Sigma_ab = alpha Sigma_a + (1 - alpha) Sigma_b + alpha (1 - alpha) d d^T,
 *     cost[e] = max(0, 1/2 [log det Sigma_ab - alpha log det Sigma_a - (1 - alpha) log det Sigma_b]),
 *   dimensionless and invariant under a common scaling of the cloud.  The determinants are the products of the L D L^T pivots.
 *   cost[e] = +inf: an invalid or self edge; a density or scale <= 0 or a non-finite parameter at either end; a result that is
 *   not finite; max_trace > 0 and trace Sigma_ab > max_trace.  The trace test bounds the merged scales: trace <= hi^2 keeps
 *   every merged scale <= hi, and no merged scale is below the smallest of the parents' (lambda_min(Sigma_ab) >= the smaller
 *   of the parents' lambda_min).
 * r2_graph_match: a matching of ANY graph (not only one of r2_knn_graph) under ANY float costs (the two directions of a pair may
 *   disagree): mate[i] = the partner of node i, or -1.  An edge is eligible when it is valid, no self edge, cost[e] <= max_cost
 *   (a NaN never is; +inf is when max_cost is +inf) and both ends are unmatched.  The key of an eligible directed edge between
 *   i and j is (cost[e], min(i, j), max(i, j)), compared lexicographically: a total order over pairs.  mate starts at -1; each
 *   of `rounds` >= 0 rounds is two launches: POINT, every unmatched node takes the partner of its smallest-key eligible edge
 *   among its own row and its incoming list; PAIR, i and j are matched when they point at each other.  The smallest key of all
 *   is matched in every round, so the rounds end, and what they end in is the sequential greedy matching (take the edges in
 *   key order, an edge when both ends are free); r2_merge_count's `open` tells whether they have.  A node with more than
 *   R2_MERGE_HUB incoming edges has its list walked by its wave (lane l: entries l, l + 64, ...; the minima fold by xor
 *   butterfly): a minimum of a total order, the same whatever the visiting order.  Entries of in_edges that are no edge to the
 *   node they are listed under are skipped; nothing outside the inputs is read.  Workspace: r2_graph_match_workspace_bytes(P)
 *   bytes (alignment >= 256 B), NULL or fewer with P > 0: R2_ERR_INVALID; rounds < 0: R2_ERR_INVALID.
 * r2_merge_count + r2_merge_emit: the two-step shape of r2_densify_classify / r2_densify_emit.  count validates mate -- an entry
 *   that is out of range, a self mate, not an involution (mate[mate[i]] != i), or whose pair has an end of non-positive or
 *   non-finite mass counts as -1 -- scans the surviving rows and synchronises the stream ONCE to return
 *   counts_host = {pairs, open}; open = the unmatched nodes that still have an eligible edge (r2_graph_match's rule, same cost
 *   and max_cost) to an unmatched node: 0 means the matching is maximal.  The caller allocates Pn = P - pairs rows and calls
 *   emit with the same parameters and the same scratch (r2_merge_scratch_bytes(P) bytes, alignment >= 256 B).  emit writes the
 *   rows in ascending order of the original index, a pair at its lower index: src [Pn,2] = (a, b), b = -1 for an unmerged row,
 *   whose four outputs are bit copies of row a.  A merged row: mu = alpha mu_a + (1 - alpha) mu_b; Sigma_ab as above; its
 *   eigenvalues by R2_MERGE_JACOBI_SWEEPS sweeps of cyclic Jacobi (rotations (0,1), (0,2), (1,2)), ordered descending,
 *   s = sqrt(lambda); the rows of R are the eigenvectors, the third flipped when det R < 0; the unit quaternion of R with
 *   r >= 0, the first non-zero component positive when r = 0; density = (m_a + m_b) / (s1 s2 s3) with the scales as stored.
 *   Rows at or beyond Pn are never written. */
#define R2_MERGE_HUB 64
#define R2_MERGE_JACOBI_SWEEPS 8
R2_API int r2_merge_cost(int P, int K, const int *idx /* [P,K] */, const float *means, const float *density, const float *scaling,
                         const float *rotation, float max_trace, float *cost /* [P,K] */, void *stream);
R2_API size_t r2_graph_match_workspace_bytes(int P);
R2_API int r2_graph_match(int P, int K, const int *idx /* [P,K] */, const int *in_offsets /* [P+1] */, const int *in_edges /* [P*K] */,
                          const float *cost /* [P,K] */, float max_cost, int rounds, int *mate /* [P] */, void *workspace,
                          size_t workspace_bytes, void *stream);
R2_API size_t r2_merge_scratch_bytes(int P);
R2_API int r2_merge_count(int P, int K, const int *idx, const int *in_offsets, const int *in_edges, const float *cost, float max_cost,
                          const int *mate /* [P] */, const float *density, const float *scaling, void *scratch,
                          unsigned int *counts_host /* [2] = pairs, open */, void *stream);
R2_API int r2_merge_emit(int P, const float *means, const float *density, const float *scaling, const float *rotation,
                         const void *scratch, int Pn, float *means_out, float *density_out, float *scaling_out,
                         float *rotation_out, int *src /* [Pn,2] */, void *stream);

/* ---- relocation and position noise: a fixed budget of Gaussians (no counterpart in the reference) ---- */
/* The density control of "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al. 2024) for a field that is a plain
 *   sum: n + 1 copies of a Gaussian with density rho / (n + 1) each ARE that Gaussian, so relocation leaves the field and every
 *   projection unchanged and the original method's scale correction is not needed.
 * Randomness (csrc/philox.hpp): Philox4x32-10 as published, key = the 64-bit seed (low word, high word), counter = (index,
 *   purpose, call low word, call high word); purpose 0 = noise, 1 = relocation draw, 2 = spread; `call` is the caller's (the
 *   trainer passes the iteration).  Normals are Box-Muller on words (a, b): u1 = ((a >> 8) + 1) 2^-24, u2 = (b >> 8) 2^-24,
 *   z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2) in float32; the three normals of an index are z0, z1 of
 *   words (0, 1) and z0 of words (2, 3).  R below is quat_to_rot(r, x, y, z) of the quaternion AS GIVEN, R[j][i] = row j,
 *   column i, the covariance R S^2 R^T of r2_query_gaussians and r2_project_gaussians.
 * r2_gaussian_noise: in place on the RAW xyz [P,3]; density [P,1], scaling [P,3], rotation [P,4] are the ACTIVATED arrays
 *   (r2_gaussian_activate's, or r2_gaussian_adam_step's after a step).  One thread per Gaussian, float32, no contraction:
 *     eps = the three normals of (index = row, purpose 0, call);  gate = 1 / (1 + exp(sharpness (rho / density_threshold - 1)));
 *     a_i = (R[0][i] eps_0 + R[1][i] eps_1) + R[2][i] eps_2;  b_i = (s_i s_i) a_i;  d_j = (R[j][0] b_0 + R[j][1] b_1) + R[j][2] b_2;
 *     xyz_j = xyz_j + float(lr * double(gate)) d_j,
 *   that is xyz += lr gate R S^2 R^T eps: Langevin noise shaped by the covariance that fades out above density_threshold (at
 *   density_threshold 0.005 and sharpness 0.5 the gate is the original method's sigmoid(100 (0.005 - rho))).  lr is the host's
 *   product of the xyz learning rate and the noise scale.  A row with a non-finite density, scale or quaternion component is
 *   left untouched.  No atomics, no workspace, no host read; the same (seed, call) gives the same bits.  P = 0 is a no-op;
 *   P < 0, a NULL array, lr or sharpness outside [0, inf), density_threshold outside (0, inf): R2_ERR_INVALID.
 * r2_relocate_plan + r2_relocate_emit: the two-step shape of r2_densify_classify / r2_densify_emit, without the host read: the
 *   result has P + n_new rows whatever the data.  params / exp_avg / exp_avg_sq (+ _out): 4 device pointers each in the order
 *   xyz [.,3], density [.,1], scaling [.,3], rotation [.,4], RAW parameters; density_act [P,1] (and scaling_act, rotation_act for
 *   the spread) their activations.
 *   Dead and alive.  A row is dead when density_act is not inside (dead_density, +inf) or any of its eleven raw parameters is
 *   not finite; every other row is alive.  D = the number of dead rows.  Slot k < D is the k-th dead row in index order, slot
 *   D + j (j < n_new) the appended row P + j.
 *   Weights.  w_i = weights[i], or density_act[i] for weights = NULL, of the alive rows whose w is finite and > 0 (the drawable
 *   rows); w_max their maximum; q_i = max(1, trunc(float(w_i / w_max) * 2^32)) as a 64-bit integer, q_i = 0 for every other
 *   row; cdf = the inclusive prefix sum of q, T = its last entry (P + n_new <= 2^29 keeps it below 2^62).  Integer sums: exact
 *   in any order.
 *   Draws.  Slot k takes words (0, 1) of (index = k, purpose 1, call): r = word0 * 2^32 + word1, t = (r * T) >> 64, and its
 *   source is the first i with cdf[i] > t.  plan writes sources [P + n_new] (slot k's source; -1 for k >= D + n_new and for
 *   T = 0) and draws [P] (n_i = the number of slots whose source is i) and fills the workspace emit reads
 *   (r2_relocate_workspace_bytes(P, n_new) bytes, alignment >= 256 B; its 64-bit scan works in tiles of R2_RELOCATE_SCAN_TILE).
 *   plan synchronises the stream only when counts_host is not NULL: counts_host = {dead, alive, drawable}.
 *   Emit, out of place into arrays of P + n_new rows, one thread per output row, never synchronising.  A source (n_i >= 1)
 *   keeps xyz, scaling and rotation bit for bit, gets the raw density softplus^-1(float(density_act_i / float(n_i + 1))) and
 *   zero moments; softplus^-1(x) = x for x > 20, else log(expm1(x)) evaluated in double and rounded once.  A slot is a bit
 *   copy of its source's xyz, scaling and rotation with that same raw density and zero moments; with spread > 0 its xyz is
 *   xyz_j + spread ((R[j][0] v_0 + R[j][1] v_1) + R[j][2] v_2), v_i = s_i eps_i, eps = the three normals of (index = k, purpose
 *   2, call), s and R the source's ACTIVATED scale and rotation -- sources are never displaced; spread = 0 is the
 *   field-preserving case.  Every other row is copied bit for bit with its moments.  The three statistics are copied for
 *   untouched rows and zeroed for sources and slots.  T = 0 (nothing drawable): every row is copied unchanged, dead ones
 *   included, and appended row j is a copy of row j mod P with raw density -100, zero moments and zero statistics: a finite row
 *   that is dead and is relocated next time.  The moment arrays may be NULL as a whole (no optimizer state), the statistics
 *   too; scaling_act / rotation_act may be NULL when spread = 0.
 *   Arguments: P = 0 with n_new = 0 is a no-op returning 0; P < 0, n_new < 0, P + n_new > 2^29, P = 0 with n_new > 0, a NULL
 *   array, a NaN dead_density, spread outside [0, inf), a workspace that is NULL or too small: R2_ERR_INVALID. */
#define R2_RELOCATE_SCAN_TILE 4096
R2_API int r2_gaussian_noise(int P, float *xyz /* [P,3] raw, in place */, const float *density, const float *scaling,
                             const float *rotation, double lr, float density_threshold, float sharpness,
                             unsigned long long seed, unsigned long long call, void *stream);
R2_API size_t r2_relocate_workspace_bytes(int P, int n_new);
R2_API int r2_relocate_plan(int P, int n_new, const float *const *params, const float *density_act,
                            const float *weights /* [P] or NULL */, float dead_density, unsigned long long seed,
                            unsigned long long call, int *sources /* [P + n_new] */, unsigned int *draws /* [P] */,
                            void *workspace, size_t workspace_bytes, unsigned int *counts_host /* [3] or NULL */, void *stream);
R2_API int r2_relocate_emit(int P, int n_new, const float *const *params, const float *const *exp_avg,
                            const float *const *exp_avg_sq, const float *density_act, const float *scaling_act,
                            const float *rotation_act, const float *max_radii2D, const float *grad_accum, const float *denom,
                            float spread, unsigned long long seed, unsigned long long call, const int *sources,
                            const unsigned int *draws, const void *workspace, size_t workspace_bytes,
                            float *const *params_out, float *const *exp_avg_out, float *const *exp_avg_sq_out,
                            float *max_radii2D_out, float *grad_accum_out, float *denom_out, void *stream);

/* ---- measurement: per-stage HIP-event timing on the caller's stream ---------------------------- */
/* bit i of stage_mask enables stage i (0 = off, the default: no events are recorded).  Enabled stages are
 * bracketed by hipEventRecord on the stream they are launched on; r2_profile_read synchronises the recorded
 * events and returns accumulated milliseconds and launch counts per stage (arrays of r2_profile_stage_count()
 * entries).  Not thread-safe; meant for bench.py. */
R2_API void r2_profile_enable(unsigned long long stage_mask);
R2_API int r2_profile_stage_count(void);
R2_API const char *r2_profile_stage_name(int stage);
R2_API int r2_profile_read(double *total_ms, long long *counts, int reset);
/* host time spent busy-waiting at the forward passes' synchronisation point (the D2H read of num_rendered), and the
 * number of such waits: long waits = GPU-bound, short waits = the host is the bottleneck. */
R2_API int r2_sync_wait_stats(double *total_us, long long *calls, int reset);
/* host time the forward passes spent before that wait (launching the first kernels) and after it (allocation callbacks +
 * launching the rest), accumulated over `calls` forward passes */
R2_API int r2_profile_host(double *pre_sync_us, double *post_sync_us, long long *calls, int reset);

/* ---- FDK reconstruction for the initialisation --------------------------------------------------------
 * Replaces tigre.algorithms.fdk as called by recon_volume() (r2_gaussian/utils/ct_utils.py:17-27) from init_pcd()
 * (initialize_pcd.py:36-90); TIGRE is a third-party CUDA toolbox outside the reference tree.
 * r2_fdk_filter: cosine pre-weight (cone != 0: DSD / sqrt(DSD^2 + u^2 + v^2) at the pixel centres, pixel size du x dv) and
 *   ramp filter along detector rows: out[v][i] = scale * sum_j w(j,v) projs[v][j] * taps[i - j + W - 1], taps = the 2W-1
 *   spatial taps of the (windowed) ramp (host side: r2_gaussian_amd/fdk.py:ramp_taps), scale = (DSD/DSO)(2 pi/V)/(4 du).
 *   The result is stored transposed: filtered_t[V][W][H].  W <= 4096 and V <= 65535, else R2_ERR_INVALID.
 * r2_fdk_backproject: vol[nx][ny][nz] = sum over the views (in order) of the bilinear sample (zero outside the detector) of
 *   filtered_t at the projection of the voxel centre, times (DSO / U)^2 for cone beams (U = p_hom.w, the depth along the
 *   central ray).  projmatrices [V,16] are the full_proj_transform matrices the rasterizer takes (same memory layout), voxel
 *   centres follow the voxelizer: center - sVoxel/2 + (i + 0.5) dVoxel. */
R2_API int r2_fdk_filter(int V, int H, int W, const float *projs /* [V,H,W] */, const float *taps /* [2W-1] */, float scale,
                         int cone, float DSD, float du, float dv, float *filtered_t /* [V,W,H] */, void *stream);
R2_API int r2_fdk_backproject(int V, int H, int W, const float *filtered_t, const float *projmatrices, int cone, float DSO,
                              int nx, int ny, int nz, float sVoxel_x, float sVoxel_y, float sVoxel_z, float center_x,
                              float center_y, float center_z, float *vol /* [nx,ny,nz] */, void *stream);

/* ---- forward projection of a volume (tigre.Ax as generate_data.py:47-69 calls it to make a dataset) ----------------------
 * r2_project_volume: out[V][H][W] = the line integral of the volume along the ray of every detector pixel, ray-driven.
 * Coordinates are voxel-index coordinates q = (x - (center - sVoxel/2)) / dVoxel - 1/2 (voxel (i,j,k) at integer q, the
 * voxelizer's and r2_fdk_backproject's convention).  rays[V][12] per view, in those coordinates: {a[3], p00[3], pu[3], pv[3]};
 * the point of pixel (r, c) is P = p00 + c pu + r pv (the host puts it at the preimage of the pixel centre's detector NDC
 * ((2c+1)/W - 1, (2r+1)/H - 1) under the rasterizer's camera).  cone != 0: the ray runs from the source a through P, t >= 0;
 * cone == 0: the ray passes through P along the direction a, all t.
 * The integrand f is the trilinear interpolant of vol[nx][ny][nz] with zero for neighbours outside [0, n_a - 1] (support
 * [-1, n_a] on each axis).  The ray is clipped to that support ([t0, t1]; a ray that misses writes exactly 0), L = chord
 * length in index units, n = max(1, ceil(L / accuracy)), and out = (t1 - t0)/n * |d_world| * sum over k = 0..n-1 in order of
 * f(q(t0 + (k + 1/2)(t1 - t0)/n)), with d_world the ray direction times dVoxel: world length units.  t0, t1 and n come from
 * separately rounded float32 operations.  No atomics, no allocation, no host synchronisation; bit-reproducible, and a view's
 * output does not depend on the other views of the call.  V <= 65535, ny * nz < 2^32. */
R2_API int r2_project_volume(int V, int H, int W, const float *rays /* [V,12] */, int cone, int nx, int ny, int nz,
                             float dVoxel_x, float dVoxel_y, float dVoxel_z, float accuracy, const float *vol /* [nx,ny,nz] */,
                             float *out /* [V,H,W] */, void *stream);

/* ---- direct volume rendering (pyvista's plotter.add_volume as scripts/plot_volume.py and data_generator/check_volume.py call
 * it to look at a volume; csrc/volume_render.hip) ------------------------------------------------------------------------------
 * The rays, the coordinates, the clip [t0, t1], n, dt = (t1 - t0)/n, wlen = |d_world| and the sample positions
 * q_k = q(t0 + (k + 1/2) dt), k = 0..n-1, are those of r2_project_volume, word for word (the same csrc/ray_sampling.hpp), and
 * f(q_k) is its trilinear value (csrc/trilinear.hpp): a renderer sample is a projector sample.
 *
 * r2_volume_bricks: bricks[bx][by][bz][2], b_a = ceil(n_a / R2_RENDER_BRICK).  Entry (i, j, k) holds the min and the max of vol
 * over the voxel indices [8 b, min(8 b + 8, n_a - 1)] of each axis (nine per axis: the footprint of every trilinear cell whose
 * floor index lies in the brick), widened to contain 0 where the brick touches a face of the volume on any axis (b = 0 or
 * 8 b + 8 > n_a - 1: a sample there mixes in the zero outside), a zero stored as +0; NaN voxels are ignored (fminf / fmaxf).
 * A sample whose floor index on an axis is i belongs to brick clamp(i, 0, n_a - 1) >> 3 of that axis.  The table does not
 * depend on any transfer function and may be reused for as long as vol is unchanged.  No atomics; bit-identical to its NumPy
 * restatement (tests/volume_render_ref.py).  At most 2^31 - 1 bricks; bricks 8-byte aligned.
 *
 * r2_render_volume: out[V][H][W][4] = the emission-absorption image of vol under the transfer function lut[K][4] = rows
 * (r, g, b, ext), row j standing at the value lo + j (hi - lo)/(K - 1) and linear between rows; ext is an extinction per world
 * length.  With scale = (float)(K - 1) / (hi - lo) (float32, computed once), dl = dt * wlen (one product), C = (0, 0, 0), T = 1,
 * per sample k in order, every operation a separately rounded float32 one:
 *     f = f(q_k)
 *     x = fminf(fmaxf((f - lo) * scale, 0), K - 1)          (a NaN lands on 0 and can never index outside the table)
 *     i = min((int)floorf(x), K - 2),   w = x - i
 *     c = lut[i][ch] + w * (lut[i+1][ch] - lut[i][ch])      for ch = r, g, b, ext: a difference, a product, a sum
 *     e = expf(-(ext * dl))                                 (the accurate expf)
 *     C_ch = C_ch + (T * (1 - e)) * c_ch                    for ch = r, g, b
 *     T = T * e
 * and the loop ends after the first sample that leaves T < t_stop (t_stop = 0: never).  out = (C_r, C_g, C_b, 1 - T):
 * premultiplied colour and opacity.  A ray that misses writes four exact zeros.
 * bricks: NULL, or the table of r2_volume_bricks for this vol.  With a table, samples of EMPTY bricks are passed over: a brick
 * with entry (mn, mx) is empty iff every row that the values [mn - 8 u M, mx + 8 u M] can reach has ext == 0, where u = 2^-24,
 * M = max(|mn|, |mx|), both ends are float32 sums rounded outwards by one more float32 where M > 0, and are mapped through the
 * index arithmetic above to the positions xa <= xb in the cells ia <= ib: the rows ia .. ib, and ib + 1 where xb > ib (a brick of
 * exact zeros at x = 0 thus reads row 0 alone, which is what makes air empty under a ramp that starts at 0).  8 u M bounds what
 * the float32 interpolant can exceed its eight voxels by
 * (tests/projector_ref.py).  A passed-over sample would have contributed exactly nothing (ext = 0, e = expf(-0) = 1,
 * T * 1 = T, T * 0 * c = 0), so the output with a table equals the output without, bit for bit; this needs a finite lut, finite
 * dl and NaN-free vol.  The sample index only moves forward, and only over samples whose own brick tested empty.
 * Limits: K in [2, 1024] (the table lives in LDS); hi > lo, both finite; t_stop in [0, 1); lut and out 16-byte aligned;
 * otherwise, and beyond the limits of r2_project_volume, R2_ERR_INVALID with nothing written.  ext >= 0 is the caller's to keep.
 * No atomics, no allocation, no host synchronisation; bit-reproducible, and a view's output does not depend on the other views
 * of the call.
 *
 * r2_render_volume_mip: out[V][H][W] = max_k f(q_k) over the same samples (fmaxf from -inf; a miss writes 0).  With a table a
 * brick is passed over iff mx + 8 u M, rounded outwards as above, <= the running maximum; same bits with and without. */
#define R2_RENDER_BRICK 8
R2_API int r2_volume_bricks(int nx, int ny, int nz, const float *vol /* [nx,ny,nz] */, float *bricks /* [bx,by,bz,2] */,
                            void *stream);
R2_API int r2_render_volume(int V, int H, int W, const float *rays /* [V,12] */, int cone, int nx, int ny, int nz,
                            float dVoxel_x, float dVoxel_y, float dVoxel_z, float accuracy, const float *vol /* [nx,ny,nz] */,
                            const float *bricks /* [bx,by,bz,2] or NULL */, int K, const float *lut /* [K,4] = r, g, b, ext */,
                            float lo, float hi, float t_stop, float *out /* [V,H,W,4] */, void *stream);
R2_API int r2_render_volume_mip(int V, int H, int W, const float *rays /* [V,12] */, int cone, int nx, int ny, int nz,
                                float dVoxel_x, float dVoxel_y, float dVoxel_z, float accuracy,
                                const float *vol /* [nx,ny,nz] */, const float *bricks /* [bx,by,bz,2] or NULL */,
                                float *out /* [V,H,W] */, void *stream);

/* r2_project_volume_siddon: the same rays, coordinates and arguments (no `accuracy`) with the Siddon ray-voxel intersection
 * model: voxel (i,j,k) is the index-space cube [i - 1/2, i + 1/2]^3 with the constant value vol[i][j][k], the volume is
 * [-1/2, n_a - 1/2] on each axis and zero outside, and out = the exact integral of that piecewise-constant function along
 * the ray, in world length units.  With s, d the ray's start and direction (csrc/ray_sampling.hpp: pixel_ray), per axis
 * rd_a = 1 / d_a (one rounded division) and, for the integer m = 0..n_a,
 *     plane_t_a(m) = (((float)m - 1/2) - s_a) * rd_a          (plane m lies at q_a = m - 1/2),
 * a fixed sequence of separately rounded float32 operations, monotone in m, never accumulated along the ray.  The clip to the
 * volume is [t0, t1] = the intersection over the axes of the intervals between plane_t_a(0) and plane_t_a(n_a), with
 * t0 = max(t0, 0) for a cone ray.  An axis is flat when d_a = 0 (or 1 / d_a overflows): it clips nothing, and the ray
 * misses unless -1/2 <= s_a < n_a - 1/2.  A ray that misses, has t1 <= t0, has no direction at all or non-finite
 * parameters writes exactly 0.  For the ray rho of a pixel and voxel v = (i, j, k) the matrix entry is
 *     A[rho, v] = wlen * max(0, min(t1, min_a hi_a) - max(t0, max_a lo_a)),        wlen = |d (.) dVoxel|,
 * lo_a, hi_a the smaller and larger of plane_t_a(m_a) and plane_t_a(m_a + 1) (m_a = i, j, k); a flat axis contributes
 * (-inf, +inf) when m_a - 1/2 <= s_a < m_a + 1/2 and makes the entry 0 otherwise.  The forward walks the cells from t0 to
 * t1 (per-axis integer plane counters, the axis with the smallest next plane_t advances, ties in the order x, y, z, the
 * cell index moves by integer steps) and adds (t_next - t_cur) * vol[cell] segment by segment in order in one thread, then
 * scales the sum by wlen once; the interval it spends in v is the one above.  No atomics, no allocation, no host
 * synchronisation; bit-reproducible, and a view's output does not depend on the other views of the call.  Limits as
 * r2_project_volume.
 * r2_backproject_volume_siddon: vol = A^T projs for that A: vol[v] = sum over the views in order, and over the pixels of
 * a view in row-major order, of A[rho, v] projs[rho], with entries bit-identical to the forward's (csrc/siddon_ray.hpp is
 * shared); only the products and sums round differently.  Voxel-driven: no atomics, no workspace; bit-reproducible, `vol`
 * is overwritten, and a cone source anywhere, inside the volume included, is handled.  Limits as r2_backproject_volume. */
R2_API int r2_project_volume_siddon(int V, int H, int W, const float *rays /* [V,12] */, int cone, int nx, int ny, int nz,
                                    float dVoxel_x, float dVoxel_y, float dVoxel_z, const float *vol /* [nx,ny,nz] */,
                                    float *out /* [V,H,W] */, void *stream);
R2_API int r2_backproject_volume_siddon(int V, int H, int W, const float *rays /* [V,12] */, int cone, int nx, int ny, int nz,
                                        float dVoxel_x, float dVoxel_y, float dVoxel_z, const float *projs /* [V,H,W] */,
                                        float *vol /* [nx,ny,nz] */, void *stream);

/* ---- exact projection of the Gaussian model itself (no counterpart in the reference, whose only Gaussian renderer is the
 * splatting rasterizer: affine at each centre, cut at 3 sigma, culled at the near plane) -------------------------------------
 * r2_project_gaussians: out[V][H][W] = the sum over the P Gaussians of the exact integral of rho exp(-x^T Sigma^-1 x / 2)
 * along the ray of every detector pixel.  Everything is in world (scene) coordinates; rays[V][12] = {a, p00, pu, pv} as for
 * r2_project_volume, read by the same pixel_ray (csrc/ray_sampling.hpp): cone != 0: start s = a, direction d = P - a with
 * P = p00 + c pu + r pv; cone == 0: s = P, d = a.  d is not normalised.
 * One (Gaussian, ray) pair: mean mu, density rho, sigma = scale_modifier * scales (3), quaternion (r, x, y, z) used AS IT
 * COMES (not normalised; the rasterizer's quat_to_rot), R its matrix, Sigma = R S^2 R^T.  With
 *     u = S^-1 R^T d,   w = S^-1 R^T (s - mu),   A = u.u,   B = u.w,   wp = w - (B / A) u,   q = wp.wp,   t* = -B / A,
 *     term = rho sqrt(2 pi / A) exp(-q / 2) |d|,
 * the integral over the WHOLE line.  q is computed from wp, never as w.w - B^2 / A (which cancels when the source is far and
 * sigma small).  For a cone ray a pair with t* <= 0 (closest approach at or behind the source) contributes exactly 0, and a
 * pair with t* > 0 its whole-line term: this differs from the integral over the half line t >= 0 by at most
 * erfc(t* sqrt(A / 2)) / 2 of the term, negligible whenever the source lies several sigma outside the cloud.  There is no
 * near-plane culling and no cut at 3 sigma.
 * Culling: a pair with q <= 32 is always summed; a pair with q > 32 (below exp(-16) of that Gaussian's peak) is summed or
 * skipped: a pixel sums a Gaussian when it lies in the conservative detector rectangle of the sphere of radius
 * 1.01 sqrt(32) sigma_max / s_min(R) around mu (s_min = 1 for a unit quaternion; csrc/gaussian_rays.hpp).  A sphere that
 * contains the cone source or straddles the plane through it parallel to the detector takes the whole detector.
 * A pair with A = 0 or a non-finite result (a ray with no direction) contributes 0, and so does every pair of a Gaussian with
 * a non-finite parameter or a scale <= 0.  P = 0 writes zeros.
 * out[v][r][c] adds its pairs in ascending Gaussian index in one thread: no atomics, no workspace, no allocation and no host
 * synchronisation; bit-reproducible, and a view's image does not depend on the other views of the call.  All arithmetic is
 * separately rounded float32 in the order written above.  V <= 65535, P <= 2^29.
 * r2_project_gaussians_backward: given G = dL/dout [V,H,W], the gradients of L with respect to means [P,3], density [P,1],
 * scales [P,3] (the unmodified ones: the scale_modifier factor is included) and rotations [P,4] (the quaternion as given, no
 * normalisation Jacobian).  Per pair, with T = term / |d|, g_w = -T wp, g_u = T (-u / A + (B / A) wp) and e = s - mu:
 *     d mu = -|d| R S^-1 g_w,     d scale_i = -|d| (g_u,i u_i + g_w,i w_i) / scale_i,     d rho = term / rho (no division),
 *     d R   = |d| (d (x) S^-1 g_u + e (x) S^-1 g_w),  d quaternion = the derivative of quat_to_rot applied to d R,
 * each times G of the pixel.  A pair is differentiated exactly when the forward summed it (same rectangle, same cone rule,
 * same arithmetic: the header is shared).  Gaussian-major: one wave walks the Gaussian's rectangle view by view and adds its
 * 64 partial sums in a fixed order: no atomics, no workspace, bit-reproducible; every output element is written, exact zeros
 * for a Gaussian no ray touches.  H * W < 2^30. */
R2_API int r2_project_gaussians(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P,
                                const float *means /* [P,3] */, const float *density /* [P] */, const float *scales /* [P,3] */,
                                float scale_modifier, const float *rotations /* [P,4] */, float *out /* [V,H,W] */,
                                void *stream);
R2_API int r2_project_gaussians_backward(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P,
                                         const float *means, const float *density, const float *scales, float scale_modifier,
                                         const float *rotations, const float *dL_dout /* [V,H,W] */, float *dL_dmeans /* [P,3] */,
                                         float *dL_ddensity /* [P] */, float *dL_dscales /* [P,3] */,
                                         float *dL_drotations /* [P,4] */, void *stream);
/* r2_project_gaussians_rays_backward: given G = dL/dout [V,H,W], the gradient of L with respect to rays [V,12] = {a, p00, pu,
 * pv}, the cloud held fixed.  A pair is differentiated exactly when the forward summed it (same rectangle, same cone rule,
 * same pair: csrc/gaussian_rays.hpp).  Per pair, with T, g_w, g_u as above, M = S^-1 R^T and G of the pixel:
 *     g_s = (G |d|) M^T g_w                                (the ray start; the negative of d mu above)
 *     g_d = (G |d|) M^T g_u + ((G T) / |d|) d              (the ray direction; the second term is the derivative of |d|)
 * A pixel (r, c) adds g_s and g_d over its pairs in ascending Gaussian index, in one thread, and with P = p00 + c pu + r pv
 * hands on  g_P = g_d, g_a = g_s - g_d  in cone beam (s = a, d = P - a)  and  g_P = g_s, g_a = g_d  in parallel beam (s = P,
 * d = a).  Over the pixels of view v:
 *     dL/da = sum g_a,    dL/dp00 = sum g_P,    dL/dpu = sum c g_P,    dL/dpv = sum r g_P.
 * NOT differentiated, being piecewise constant in the rays: which pairs are summed -- the rectangle and with it the cut of
 * the terms with q > 32, each below exp(-16) of its Gaussian's peak -- and the cone rule t* <= 0.
 * Pixel-major: one workgroup per 16 x 16 tile and view adds its 256 x 12 values in one fixed order into
 * partial[view][tile][12] in `workspace` (r2_project_gaussians_rays_backward_workspace_bytes(V, H, W) = 48 bytes per tile and
 * view; NULL or fewer bytes with P > 0: R2_ERR_INVALID and a message, nothing written), then one workgroup per view adds
 * that view's tiles in one fixed order.  dL_drays is always fully written; P = 0 writes zeros and needs no workspace.  No
 * atomics, no allocation and no host synchronisation; bit-reproducible, and a view's twelve numbers do not depend on the
 * other views of the call.  All arithmetic is separately rounded float32 in the order written above.  V <= 65535,
 * P <= 2^29, H * W < 2^30. */
R2_API size_t r2_project_gaussians_rays_backward_workspace_bytes(int V, int H, int W);
R2_API int r2_project_gaussians_rays_backward(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P,
                                              const float *means, const float *density, const float *scales,
                                              float scale_modifier, const float *rotations, const float *dL_dout /* [V,H,W] */,
                                              float *dL_drays /* [V,12] */, void *workspace, size_t workspace_bytes,
                                              void *stream);

/* ---- exact evaluation of the Gaussian density field at caller-supplied points (no counterpart in the reference, whose only
 * 3D evaluation is the voxelizer: one axis-aligned grid, every Gaussian cut at a cube of ceil(3 max(scale) / dVoxel) voxels
 * and at alpha >= 1e-6) -----------------------------------------------------------------------------------------------------
 * r2_query_gaussians: out[n] = the sum over the P Gaussians of rho exp(-q / 2) at points[n] ([N,3], world (scene)
 * coordinates).  One (Gaussian, point) pair: mean mu, density rho, sigma = scale_modifier * scales (3), quaternion
 * (r, x, y, z) used AS IT COMES (not normalised; the rasterizer's quat_to_rot), R its matrix.  With
 *     e = x - mu,   w = S^-1 R^T e,   q = w.w,   term = rho exp(-q / 2).
 * Culling: a pair with q <= 32 is always summed; a pair with q > 32 (below exp(-16) of that Gaussian's peak) is summed or
 * skipped by one rule that the forward and both backwards share (csrc/gaussian_points.hpp).  That rule cuts per pair, at a
 * float32 q of 32.001, so that values and gradients do not depend on the order of the points; in front of it, and without
 * effect on any bit, the points are taken in blocks of 256 consecutive ones, a block skips a Gaussian whose sphere of radius
 * 1.01 sqrt(32) sigma_max / s_min(R) around mu (s_min = 1 for a unit quaternion; csrc/gaussian_rays.hpp) misses the
 * axis-aligned box of the block's finite points, and a point skips a Gaussian whose sphere it lies outside.  Coherent point
 * sets (planes, lines, patches) therefore cost far less than scattered ones.
 * Every pair of a Gaussian with a non-finite parameter or a scale <= 0 contributes 0, and so does a pair whose q is not
 * a number.  A point with a non-finite coordinate gets out = 0 and zero gradients, and does not enter its block's box.  P = 0
 * writes zeros; N = 0 returns success and touches nothing.  N < 2^31, P <= 2^29.
 * out[n] adds its pairs in ascending Gaussian index in one thread: no atomics, no workspace, no allocation and no host
 * synchronisation; bit-reproducible.  All arithmetic is separately rounded float32 in the order written above.
 * r2_query_gaussians_backward: given G = dL/dout [N], the gradients of L with respect to means [P,3], density [P], scales
 * [P,3] (the unmodified ones: the scale_modifier factor is included) and rotations [P,4] (the quaternion as given, no
 * normalisation Jacobian), and, if dL_dpoints is not NULL, with respect to the points [N,3].  Per pair, with g_w = -term w:
 *     d rho = exp(-q / 2) (no division by rho),   d mu = -R S^-1 g_w,   d x = +R S^-1 g_w,   d scale_i = -g_w,i w_i / scale_i,
 *     d R = e (x) S^-1 g_w,   d quaternion = the derivative of quat_to_rot applied to d R,
 * each times G[n].  A pair is differentiated exactly when the forward summed it (same boxes, same sphere, same arithmetic:
 * the header is shared).  Parameter gradients are Gaussian-major: a first kernel writes the block boxes into `workspace`
 * (r2_query_gaussians_workspace_bytes(N) = 24 bytes per block of 256 points; NULL or fewer bytes with N > 0: R2_ERR_INVALID
 * and a message), then one wave per Gaussian tests the boxes 64 at a time, walks the blocks that meet its sphere in
 * ascending order and adds its 64 partial sums in a fixed order; every output element is written, exact zeros for a
 * Gaussian no point touches (all of them when N = 0).  Point gradients are point-major, in the forward's order.  No atomics,
 * no allocation, no host synchronisation; bit-reproducible. */
R2_API int r2_query_gaussians(int N, const float *points /* [N,3] */, int P, const float *means /* [P,3] */,
                              const float *density /* [P] */, const float *scales /* [P,3] */, float scale_modifier,
                              const float *rotations /* [P,4] */, float *out /* [N] */, void *stream);
R2_API size_t r2_query_gaussians_workspace_bytes(int N);
R2_API int r2_query_gaussians_backward(int N, const float *points /* [N,3] */, int P, const float *means, const float *density,
                                       const float *scales, float scale_modifier, const float *rotations,
                                       const float *dL_dout /* [N] */, float *dL_dmeans /* [P,3] */, float *dL_ddensity /* [P] */,
                                       float *dL_dscales /* [P,3] */, float *dL_drotations /* [P,4] */,
                                       float *dL_dpoints /* [N,3] or NULL */, void *workspace, size_t workspace_bytes,
                                       void *stream);

/* ---- exact line integrals of the Gaussian model along caller-supplied rays (the line form of r2_query_gaussians: curved
 * detectors, measured pixel positions, a random subset of the pixels of many views, per-ray geometry gradients) -------------
 * r2_integrate_gaussians: out[n] = the sum over the P Gaussians of the pair of r2_project_gaussians along ray n, given as
 * rays[n][6] = {start s, direction d} in world (scene) coordinates; d is not normalised.  One (Gaussian, ray) pair is that
 * projector's, operation for operation (csrc/gaussian_rays.hpp: gauss_pair): u, w, A, B, wp = w - (B / A) u, q = wp.wp formed
 * from wp, term = rho sqrt(2 pi / A) exp(-q / 2) |d| over the WHOLE line; half_line != 0 applies the cone rule, a pair with
 * t* = -B / A <= 0 contributes exactly 0 (and one with t* > 0 its whole-line term).
 * Which pairs are summed is a property of the pair alone: a pair is summed when its float32 q is <= 32.001, and only then
 * (every pair with q <= 32 is summed, and of those above, which the projector's contract leaves free, only that sliver; the
 * cut of r2_query_gaussians, for its reason: a tail that depended on the other rays would put gradients outside the float64
 * bracket).  A ray's value and its ray gradient therefore do not depend on which other rays are in the call or on their
 * order, bit for bit; the parameter gradients depend on the order only through the association of their sums.
 * Culling comes in front of the cut, saves work and changes no bit (csrc/gaussian_bundle.hpp derives every allowance below;
 * eps = 2^-24, the allowances are 16 eps of the quantity that rounds).  (0) Two small kernels write the cloud box, the
 * bounding box of the spheres of radius 1.01 sqrt(32) sigma_max / s_min(R) around the means (csrc/gaussian_rays.hpp:
 * gauss_radius; Gaussians that contribute nothing are skipped, an infinite radius makes the box infinite), into the
 * workspace: one partial box per workgroup, then their reduction; no atomics, and min / max are exact in any order.  (1) The
 * rays are taken in blocks of 256 consecutive ones.  Each ray is clipped to the cloud box by the slab method along its unit
 * direction, a half-line ray to t >= 0 as well (the Mahalanobis-closest point of a summed pair lies at t* > 0 and inside its
 * sphere); bounds and t move outwards by 16 eps of themselves.  A ray that misses the cloud box sums nothing.  (2) A block's
 * box is the bounding box of its rays' clipped end points, each moved outwards by 16 eps (|s_k| + |t|); a block skips a
 * Gaussian whose sphere misses its box.  Any point of a line that lies in a sphere lies in the cloud box, hence on the
 * clipped segment, hence in the block's box.  (3) A ray skips a Gaussian whose sphere its line misses,
 * |e x d|^2 > (radius + 16 eps |e|_1)^2 |d|^2 (1 + 1e-5), e = s - mu: the cross product cancels from |e| down to the line's
 * distance, so its rounding is relative to |e| and not to the radius, which the sphere's 1 % could not cover for a small
 * Gaussian seen from afar.  Coherent blocks of rays (a detector tile, sorted rays) cost far less than scattered ones.
 * A ray with a non-finite component or d = 0 (its float32 |d| is 0 or not finite) gets out = 0 and zero gradients and does
 * not enter its block's box.  Every pair of a Gaussian with a non-finite parameter or a scale <= 0 contributes 0.  P = 0
 * writes zeros and needs no workspace; N = 0 returns success and touches nothing.  `workspace`: r2_integrate_gaussians_
 * workspace_bytes(N, P) bytes (24 per box: the cloud box, at most 1024 partial boxes, one box per block of 256 rays; 0 when N
 * or P is 0), not kept between calls; NULL or fewer bytes with N > 0 and P > 0: R2_ERR_INVALID and a message, nothing
 * written.  N < 2^31, P <= 2^29.
 * out[n] adds its pairs in ascending Gaussian index in one thread: no atomics, no allocation, no host synchronisation;
 * bit-reproducible.  All arithmetic is separately rounded float32 in the order written above.
 * r2_integrate_gaussians_backward: given G = dL/dout [N], the gradients of L with respect to means [P,3], density [P], scales
 * [P,3] and rotations [P,4] by the per-pair formulas of r2_project_gaussians_backward, and, if dL_drays is not NULL, with
 * respect to the rays: dL_drays[n] = {sum g_s, sum g_d} over the ray's pairs in ascending Gaussian index, g_s and g_d as
 * r2_project_gaussians_rays_backward has them, written per ray.  A pair is differentiated exactly when the forward summed it;
 * the cut and the cone rule are piecewise constant and NOT differentiated.  Parameter gradients are Gaussian-major: a kernel
 * writes the block boxes into the workspace, then one wave per Gaussian tests the boxes 64 at a time, walks the blocks that
 * meet its sphere in ascending order (lane l takes rays l, l + 64, l + 128, l + 192) and adds its 64 x 11 partial sums in
 * one fixed order; every output element is written, exact zeros for a Gaussian no ray touches (all of them when N = 0, the
 * one thing the backward writes then).  Ray gradients are ray-major, in the forward's skeleton.  No atomics, no allocation,
 * no host synchronisation; bit-reproducible. */
R2_API int r2_integrate_gaussians(int N, const float *rays /* [N,6] = start s, direction d */, int half_line, int P,
                                  const float *means /* [P,3] */, const float *density /* [P] */,
                                  const float *scales /* [P,3] */, float scale_modifier, const float *rotations /* [P,4] */,
                                  float *out /* [N] */, void *workspace, size_t workspace_bytes, void *stream);
R2_API size_t r2_integrate_gaussians_workspace_bytes(int N, int P);
R2_API int r2_integrate_gaussians_backward(int N, const float *rays /* [N,6] */, int half_line, int P, const float *means,
                                           const float *density, const float *scales, float scale_modifier,
                                           const float *rotations, const float *dL_dout /* [N] */, float *dL_dmeans /* [P,3] */,
                                           float *dL_ddensity /* [P] */, float *dL_dscales /* [P,3] */,
                                           float *dL_drotations /* [P,4] */, float *dL_drays /* [N,6] or NULL */,
                                           void *workspace, size_t workspace_bytes, void *stream);

/* ---- the same line integrals, culled by leaves of Gaussians (scattered rays: a random subset of the pixels of many views) ----
 * r2_integrate_gaussians_leaves: the values of r2_integrate_gaussians by the same rule -- a valid ray and a Gaussian with
 * gauss_radius >= 0 are summed exactly when the pair's float32 q, formed from wp, is <= 32.001 (csrc/gaussian_bundle.hpp:
 * bundle_pair), the cone rule with half_line != 0, invalid rays and Gaussians as there -- with the culling done from the other
 * side, so that no ray waits for another ray's Gaussians and N rays make N waves of work.  Culling is by leaves of 64
 * consecutive Gaussians, so an index order that is spatially coherent and keeps large Gaussians together culls well, and any
 * other order costs time and nothing else.
 * A prepare kernel, on every forward and backward call, writes into the workspace a float4 {mean, radius} per Gaussian (the
 * radius of r2_integrate_gaussians' sphere; -1 for a Gaussian that contributes nothing), the 64-byte record S^-1 R^T, 1 / sigma,
 * mean and density of every Gaussian that has a radius (csrc/gaussian_rays.hpp: gauss_rec), and per leaf the bounding box of its
 * members' spheres mu -+ radius (empty, lo > hi, when no member has one; infinite when a radius is; the last leaf may be
 * partial; a min / max butterfly over the wave, exact in any order).  The leaf test: a ray meets a leaf when its line meets the
 * leaf's box under the slab test (1) of r2_integrate_gaussians, with (1)'s allowances: bounds moved outwards by 16 eps of
 * themselves, every t by 16 eps of itself, half-line rays clipped to t >= 0, a ray whose |d|^2 is outside [1e-30, 1e30] meeting
 * every leaf.  A summed pair's closest point lies in the Gaussian's sphere, hence in its leaf's box: the test is conservative
 * for the infinite line and changes which pairs are summed by nothing.  Inside a met leaf a ray skips a Gaussian by (3).
 * Forward: one wave per ray; lane l tests the box of leaf base + l, the wave walks the met leaves in ascending order, lane l
 * taking Gaussian 64 leaf + l and adding its pairs in that order; one fixed xor butterfly adds the 64 lanes and lane 0 writes.
 * out[n] depends on the cloud, its order and ray n alone, bit for bit; an invalid ray gets an exact 0.  Against
 * r2_integrate_gaussians the sums associate differently: the values agree to rounding, and bit for bit where a ray sums one
 * pair.  P = 0 writes zeros and needs no workspace; N = 0 returns success and touches nothing.  `workspace`:
 * r2_integrate_gaussians_leaves_workspace_bytes(N, P) bytes (80 per Gaussian, 24 per leaf; 0 when N or P is 0), aligned to 16
 * bytes, not kept between calls; NULL or fewer bytes with N > 0 and P > 0: R2_ERR_INVALID and a message naming the size
 * needed, nothing launched.  N < 2^31, P <= 2^29.  No atomics, no allocation, no host synchronisation; bit-reproducible.
 * r2_integrate_gaussians_leaves_backward: the gradients of r2_integrate_gaussians_backward, pair for pair.  Parameters: one
 * wave per leaf, one lane per Gaussian; the wave takes the rays 64 at a time, lane l testing ray base + l against the leaf's
 * box, compacts the hits in ray order, and every lane adds the pairs of its own Gaussian: a Gaussian's gradient is summed by
 * one lane in ascending ray index, without butterfly or atomics; every output element is written, exact zeros for a Gaussian
 * no ray touches or one that contributes nothing (all of them when N = 0, the one thing the backward writes then).  Rays, if
 * dL_drays is not NULL: the forward's skeleton with six sums, dL_drays[n] depending on ray n alone. */
R2_API size_t r2_integrate_gaussians_leaves_workspace_bytes(int N, int P);
R2_API int r2_integrate_gaussians_leaves(int N, const float *rays /* [N,6] = start s, direction d */, int half_line, int P,
                                         const float *means /* [P,3] */, const float *density /* [P] */,
                                         const float *scales /* [P,3] */, float scale_modifier,
                                         const float *rotations /* [P,4] */, float *out /* [N] */, void *workspace,
                                         size_t workspace_bytes, void *stream);
R2_API int r2_integrate_gaussians_leaves_backward(int N, const float *rays /* [N,6] */, int half_line, int P, const float *means,
                                                  const float *density, const float *scales, float scale_modifier,
                                                  const float *rotations, const float *dL_dout /* [N] */,
                                                  float *dL_dmeans /* [P,3] */, float *dL_ddensity /* [P] */,
                                                  float *dL_dscales /* [P,3] */, float *dL_drotations /* [P,4] */,
                                                  float *dL_drays /* [N,6] or NULL */, void *workspace, size_t workspace_bytes,
                                                  void *stream);

/* ---- Fisher information and predictive variance on the exact operators (no counterpart in the reference) ---------------------
 * The image of r2_project_gaussians and the field of r2_query_gaussians are plain sums over the Gaussians, so the derivative
 * of one pixel (or of the field at one point) with respect to parameter t of Gaussian i is ONE pair's number: o[t] of
 * r2_project_gaussians_backward's per-pair formulas with G = 1 (csrc/gaussian_rays.hpp: gauss_pair_grad).  The eleven
 * parameters, in that order: mean (3), density, the unmodified scales (3; the scale_modifier factor is included), the
 * quaternion (4; as given, no normalisation Jacobian).  The three entries add squares of these numbers
 * (csrc/gaussian_fisher.hpp: pair_squares, pair_variance); every addend is >= 0 for weights and variances >= 0.
 * What the numbers mean: f is the DIAGONAL of J^T W J, the Fisher information of the parameters under independent pixel noise
 * of variance 1 / w and the Gauss-Newton diagonal of the weighted least-squares fit.  1 / (f + prior precision) taken as a
 * parameter variance, and the two predictive variances computed from it, ignore every correlation between the parameters of
 * a Gaussian and between Gaussians: a Laplace approximation in the given parametrisation, not a posterior.
 * r2_project_gaussians_fisher: f[i][t] = the sum over the pixels (v, r, c) of all V views of
 *     w[v][r][c] * (o[t] * o[t]),     o = the pair's eleven derivatives with G = 1,
 * written to f_means [P,3], f_density [P], f_scales [P,3], f_rotations [P,4].  weights [V,H,W] or NULL for w = 1 (the same
 * bits as an array of ones); they are used as they come and are meant to be >= 0.  The pairs are exactly those
 * r2_project_gaussians_backward differentiates: the detector rectangle of the Gaussian's sphere, then the pair rule of
 * r2_project_gaussians (A > 0, the cone rule, a finite term).  Gaussian-major, the backward's skeleton: one wave per
 * Gaussian, views in order, the rectangle's pixels row-major with lane l taking pixels l, l + 64, ..., eleven sums per lane
 * (acc[t] += w * (o[t] * o[t])), one fixed xor butterfly, lane 0 writes.  No atomics, no workspace, no allocation, no host
 * synchronisation; bit-reproducible; every output element is written, exact zeros for a Gaussian no ray touches and for one
 * with a non-finite parameter or a scale <= 0.  P = 0 returns success and touches nothing.  Cost: that of the backward -- a
 * Gaussian that covers the detector costs its wave V * H * W pairs, and the call waits for it.  P <= 2^29, H * W < 2^30;
 * argument checks as r2_project_gaussians_backward.
 * r2_query_gaussians_variance: out[n] = the sum over the pairs of points[n] of
 *     pair_variance = sum_t v[i][t] * (o[t] * o[t])   (added in ascending t),
 * the variance of the field at the point under independent parameter variances v (v_means [P,3], v_density [P], v_scales
 * [P,3], v_rotations [P,4]; used as they come, meant to be >= 0).  The pairs are those of r2_query_gaussians: the per-pair
 * cut at a float32 q of 32.001 behind the block-box and sphere tests, so out[n] depends on the cloud and point n alone, bit
 * for bit, whatever the order of the points.  Point-major, the forward's skeleton with a 140-byte staged record: one
 * workgroup per block of 256 points, ascending Gaussian index in one thread.  A point with a non-finite coordinate gets 0; P = 0
 * writes zeros; N = 0 returns success and touches nothing.  N < 2^31, P <= 2^29.
 * r2_project_gaussians_variance: out[v][r][c] = the sum over the pixel's pairs of pair_variance, the predictive variance of
 * every pixel of r2_project_gaussians' image.  The pairs are those the forward sums (rectangle, then the pair rule), so
 * sum_pixels w * out = sum_it f[i][t] v[i][t] with f of r2_project_gaussians_fisher up to rounding: the same pairs added in
 * two orders.  Pixel-major, the forward's skeleton: one workgroup per 16 x 16 tile and view, ascending Gaussian index in one
 * thread.  P = 0 writes zeros.  V <= 65535, P <= 2^29.
 * All three: separately rounded float32 in the order written; no atomics, no workspace, no allocation, no host
 * synchronisation; bit-reproducible. */
R2_API int r2_project_gaussians_fisher(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P,
                                       const float *means /* [P,3] */, const float *density /* [P] */,
                                       const float *scales /* [P,3] */, float scale_modifier, const float *rotations /* [P,4] */,
                                       const float *weights /* [V,H,W] or NULL */, float *f_means /* [P,3] */,
                                       float *f_density /* [P] */, float *f_scales /* [P,3] */, float *f_rotations /* [P,4] */,
                                       void *stream);
R2_API int r2_query_gaussians_variance(int N, const float *points /* [N,3] */, int P, const float *means, const float *density,
                                       const float *scales, float scale_modifier, const float *rotations,
                                       const float *v_means /* [P,3] */, const float *v_density /* [P] */,
                                       const float *v_scales /* [P,3] */, const float *v_rotations /* [P,4] */,
                                       float *out /* [N] */, void *stream);
R2_API int r2_project_gaussians_variance(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P, const float *means,
                                         const float *density, const float *scales, float scale_modifier, const float *rotations,
                                         const float *v_means /* [P,3] */, const float *v_density /* [P] */,
                                         const float *v_scales /* [P,3] */, const float *v_rotations /* [P,4] */,
                                         float *out /* [V,H,W] */, void *stream);

/* ---- Jacobian products of the exact projector (no counterpart in the reference) ----------------------------------------------
 * r2_project_gaussians_backward applies J^T, the transpose of the image's Jacobian in the cloud's parameters, and
 * r2_project_gaussians_fisher the diagonal of J^T W J.  These two apply J itself, pixel-major on the forward's skeleton (one
 * workgroup per 16 x 16 tile and view, one thread per pixel, ascending Gaussian index in one thread).
 * r2_project_gaussians_jvp: out[v][r][c] = the sum over the pixel's pairs of
 *     pair_tangent = tan[i][0] * o[0], then + tan[i][t] * o[t] in ascending t,
 * o = the pair's eleven derivatives with G = 1 (csrc/gaussian_rays.hpp: gauss_pair_grad; the parameters and their order as for
 * the Fisher entries above), tan = the tangent of Gaussian i (t_means [P,3], t_density [P], t_scales [P,3], t_rotations
 * [P,4]): the directional derivative (J t) of r2_project_gaussians' image along t.  The pairs are exactly those the forward
 * sums (rectangle, then the pair rule); the culling, the cone rule and the cut are piecewise constant and NOT differentiated,
 * as in the backward.  The tangent of a Gaussian that is staged on no tile (off the detector, behind the source, a non-finite
 * parameter or a scale <= 0) is never read.  The staged record is the projection variance's (156 bytes).  P = 0 writes zeros.
 * Identities: <G, J t> = <J^T G, t> with r2_project_gaussians_backward's J^T G up to rounding (the same pairs added in two
 * orders); linear in t, and exactly so for a factor 2; t = (0, density, 0, 0) gives the forward's image up to rounding.
 * r2_project_gaussians_ray_jacobian: out[v][0..2][r][c] = d pixel / d s and out[v][3..5][r][c] = d pixel / d d, the pixel's
 * derivative in the start s and the direction d of its own ray: the sums over the pixel's pairs of g_s and g_d of
 * r2_project_gaussians_rays_backward with G = 1 (csrc/gaussian_ray_grad.hpp: gauss_pair_ray_grad).  Planar, so that a tile row
 * stores 64 contiguous bytes per plane.  The pixel point is P = p00 + c pu + r pv; cone beam has s = a, d = P - a, parallel
 * beam s = P, d = a: contracting the six planes with G by that rule (pixel_ray_grad) and adding over the pixels gives
 * r2_project_gaussians_rays_backward's dL_drays up to rounding, and contracting them with the tangent of (s, d) gives the
 * image's directional derivative along any change of the geometry.  P = 0 writes zeros.
 * Both: V <= 65535, P <= 2^29; argument checks as r2_project_gaussians_variance; separately rounded float32 in the order
 * written; no atomics, no workspace, no allocation, no host synchronisation; bit-reproducible; a view's output does not
 * depend on the other views. */
R2_API int r2_project_gaussians_jvp(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P, const float *means,
                                    const float *density, const float *scales, float scale_modifier, const float *rotations,
                                    const float *t_means /* [P,3] */, const float *t_density /* [P] */,
                                    const float *t_scales /* [P,3] */, const float *t_rotations /* [P,4] */,
                                    float *out /* [V,H,W] */, void *stream);
R2_API int r2_project_gaussians_ray_jacobian(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P,
                                             const float *means, const float *density, const float *scales, float scale_modifier,
                                             const float *rotations, float *out /* [V,6,H,W] */, void *stream);

/* ---- projection plans: per-tile Gaussian lists for the pixel-major operators of the exact projector -----------------------------
 * r2_project_gaussians, its ray backward, the projection variance, the JVP and the ray Jacobian are pixel-major: every 16 x 16
 * tile of every view walks all P Gaussians and tests each one's detector rectangle against the tile.  For a cloud and a geometry
 * that are projected many times (a Gauss-Newton solve) a plan keeps the answer: with Tx = ceil(W / 16), Ty = ceil(H / 16) and
 * T = Tx Ty, list k = view T + ty Tx + tx is ids[offsets[k] .. offsets[k + 1]), where
 *     offsets  long long [V T + 1], offsets[0] = 0, non-decreasing; offsets[V T] is the number of instances,
 *     ids      int [instances]: the indices of the Gaussians the unplanned kernels stage for that tile -- a radius (no
 *              non-finite parameter, every scale > 0), a detector rectangle (csrc/gaussian_rays.hpp: gauss_radius, gauss_rect)
 *              and the rectangle meets the tile -- ASCENDING within a list.
 * Building (two calls, so that the caller can size ids in between):
 * r2_project_gaussians_plan_count computes every Gaussian's rectangle once per view (V P evaluations where an unplanned call
 * makes V T P) into a table in `workspace` (r2_project_gaussians_plan_workspace_bytes(V, H, W, P) = 8 bytes per view and
 * Gaussian; 0 for P = 0), counts every tile's hits and scans the counts into `offsets`; the caller reads offsets[V T].
 * r2_project_gaussians_plan_fill walks the SAME table (the workspace of the count, untouched in between, and the same
 * arguments) and writes the ids.  It refuses nothing on the device: an id is written only below ids_capacity and below its
 * list's end, so a capacity that is too small loses the instances beyond it and nothing else.
 * No atomics anywhere: a tile's hits are compacted in index order by wave ballots and wave counts, so building twice gives
 * the same bytes, and the ids of a view's lists do not depend on the other views of the call.  Cost: V P rectangles, then
 * 2 V T P tests of four integer compares each on 8-byte entries, against V T P rectangles (about 60 float operations, a
 * square root and two divisions each in cone beam) for ONE unplanned call.  P = 0: the offsets are zeros, no workspace.
 * V <= 65535, Tx <= 65535, Ty <= 65535, P <= 2^29.  NULL or too small a workspace with P > 0: R2_ERR_INVALID, nothing written.
 * Consuming: each *_planned entry takes its parent's arguments and, before the stream, offsets, ids and ids_capacity (the
 * number of ints ids holds), and writes what its parent writes, BIT FOR BIT when the lists are a plan's: an entry is staged
 * as the parent stages a hit (radius and rectangle are computed again, the same record is filled), the test of the pixel
 * against the rectangle and the pair are the parent's, so a pixel adds the same pairs in the same ascending order in one
 * thread.  THE LISTS DRIVE THE KERNEL: a Gaussian that is absent from a tile's list contributes nothing to that tile even if
 * its rectangle meets it, so a caller may hand in lists of their own -- ascending, every id < P; an id outside [0, P) or a
 * Gaussian without radius or rectangle is skipped.  A tile with an empty list still writes its pixels (zeros; its zero partial
 * in the ray backward).  Reads are bounded: both ends of a list are clamped to [0, ids_capacity], so wrong offsets give a
 * wrong image and never a read outside ids.  offsets NULL, ids NULL with ids_capacity > 0, or ids_capacity < 0 (P > 0):
 * R2_ERR_INVALID, nothing written; every other check is the parent's.  P = 0 writes zeros and needs no lists.  The plan is
 * valid for exactly the (V, H, W, rays, cone, cloud, scale_modifier) it was built with; the C ABI does not check that. */
R2_API size_t r2_project_gaussians_plan_workspace_bytes(int V, int H, int W, int P);
R2_API int r2_project_gaussians_plan_count(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P, const float *means,
                                           const float *density, const float *scales, float scale_modifier, const float *rotations,
                                           long long *offsets /* [V T + 1] */, void *workspace, size_t workspace_bytes,
                                           void *stream);
R2_API int r2_project_gaussians_plan_fill(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P, const float *means,
                                          const float *density, const float *scales, float scale_modifier, const float *rotations,
                                          const long long *offsets /* [V T + 1] */, int *ids, long long ids_capacity,
                                          void *workspace, size_t workspace_bytes, void *stream);
R2_API int r2_project_gaussians_planned(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P, const float *means,
                                        const float *density, const float *scales, float scale_modifier, const float *rotations,
                                        float *out /* [V,H,W] */, const long long *offsets, const int *ids, long long ids_capacity,
                                        void *stream);
R2_API int r2_project_gaussians_rays_backward_planned(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P,
                                                      const float *means, const float *density, const float *scales,
                                                      float scale_modifier, const float *rotations,
                                                      const float *dL_dout /* [V,H,W] */, float *dL_drays /* [V,12] */,
                                                      void *workspace, size_t workspace_bytes, const long long *offsets,
                                                      const int *ids, long long ids_capacity, void *stream);
R2_API int r2_project_gaussians_variance_planned(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P,
                                                 const float *means, const float *density, const float *scales,
                                                 float scale_modifier, const float *rotations, const float *v_means,
                                                 const float *v_density, const float *v_scales, const float *v_rotations,
                                                 float *out /* [V,H,W] */, const long long *offsets, const int *ids,
                                                 long long ids_capacity, void *stream);
R2_API int r2_project_gaussians_jvp_planned(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P, const float *means,
                                            const float *density, const float *scales, float scale_modifier, const float *rotations,
                                            const float *t_means, const float *t_density, const float *t_scales,
                                            const float *t_rotations, float *out /* [V,H,W] */, const long long *offsets,
                                            const int *ids, long long ids_capacity, void *stream);
R2_API int r2_project_gaussians_ray_jacobian_planned(int V, int H, int W, const float *rays /* [V,12] */, int cone, int P,
                                                     const float *means, const float *density, const float *scales,
                                                     float scale_modifier, const float *rotations, float *out /* [V,6,H,W] */,
                                                     const long long *offsets, const int *ids, long long ids_capacity,
                                                     void *stream);

/* ---- exact adjoint of the forward projector, and TV descent (tigre.Atb and minimizeTV as the iterative reconstructions of
 * ct_utils.py:60-215 call them; r2_gaussian_amd/recon.py) ----------------------------------------------------------------
 * r2_backproject_volume: vol = A^T projs for the A of r2_project_volume with the same arguments.  For the ray rho of pixel
 * (view, r, c) with the forward's float32 t0, n, dt and |d_world|, and its sample points q_k = fma(fma(k + 1/2, dt, t0), d, s):
 *     A[rho, v] = dt |d_world| sum_k X_k(v_x) Y_k(v_y) Z_k(v_z),
 * X_k(i) = the forward's trilinear weight w0 where i is the floor index of q_k,x, w1 where it is floor + 1, 0 otherwise
 * (likewise Y, Z); vol[v] = sum over the views in order of sum_rho A[rho, v] projs[rho].  The clip, hit or miss, n, the
 * sample positions and the weights are bit-identical to the forward's (csrc/ray_sampling.hpp is shared); only the rounding
 * of the products and sums differs.  Voxel-driven: no atomics, no allocation, no host synchronisation; bit-reproducible,
 * and `vol` is overwritten (its prior contents never matter).  A cone source anywhere, inside the volume included, is
 * handled (the voxels whose support reaches the source plane gather from the whole detector).  The forward's limits plus
 * nx, ny <= 4 * 65535. */
R2_API int r2_backproject_volume(int V, int H, int W, const float *rays /* [V,12] */, int cone, int nx, int ny, int nz,
                                 float dVoxel_x, float dVoxel_y, float dVoxel_z, float accuracy,
                                 const float *projs /* [V,H,W] */, float *vol /* [nx,ny,nz] */, void *stream);
/* r2_tv_descent: n_iter steps of normalised steepest descent on TV_eps(x) = sum_v sqrt(Dx(v)^2 + Dy(v)^2 + Dz(v)^2 + eps),
 * eps = 1e-8, for vol[nx][ny][nz] (z fastest), with forward differences Dx(i,j,k) = x(i+1,j,k) - x(i,j,k) and Dx = 0 at
 * i = nx - 1 (Neumann; likewise y, z).  Its gradient is
 *     g(v) = - (Dx(v) + Dy(v) + Dz(v)) / s(v) + sum_a [v_a > 0] Da(v - e_a) / s(v - e_a),   s = sqrt(Dx^2 + Dy^2 + Dz^2 + eps),
 * and each step is  x <- x - (*step / |g|_2) g,  skipped when |g|_2 = 0 (no division by zero).  |g|_2 is a fixed-order
 * on-device reduction (double partial sums); `step` is a device scalar, read by the kernels: no host synchronisation.
 * scratch: a device buffer of at least r2_tv_descent_scratch_bytes(nx, ny, nz) bytes, 8-byte aligned. */
R2_API size_t r2_tv_descent_scratch_bytes(int nx, int ny, int nz);
R2_API int r2_tv_descent(int nx, int ny, int nz, float *vol, const float *step /* device scalar */, int n_iter, void *scratch,
                         size_t scratch_bytes, void *stream);
/* r2_tv_prox: the proximal operator of the isotropic, unsmoothed total variation with a box constraint (ROF denoising;
 * csrc/tv_prox.hip, recon.py: tv_prox, tv_denoise, fista_tv),
 *     x = argmin_x 1/2 |x - y|^2 + lambda TV(x)  subject to  lo <= x <= hi,      TV(x) = sum_v |(D x)(v)|_2,
 * for y, x [nx][ny][nz] (z fastest), D the forward differences of r2_tv_descent ((D_a x)(v) = x(v + e_a) - x(v), 0 at
 * v_a = n_a - 1), by n_iter iterations of Beck and Teboulle's fast gradient projection on the dual p, r in R^{3 x N}, P_C the
 * clamp to [lo, hi]:  r_1 = p_0 = 0, t_1 = 1, and for k = 1 .. n_iter
 *     x_k = P_C(y - lambda D^T r_k),   q = r_k + (1 / (12 lambda)) D x_k,   p_k(v) = q(v) / max(1, |q(v)|_2),
 *     t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2,   r_{k+1} = p_k + ((t_k - 1) / t_{k+1}) (p_k - p_{k-1});
 * the result is x = P_C(y - lambda D^T p_{n_iter}), with (D^T p)(v) = sum_a (-p_a(v) [v_a < n_a - 1] + p_a(v - e_a) [v_a > 0]);
 * 12 bounds |D|^2 (4 per axis).  n_iter = 0 gives x = P_C(y).
 * lambda: a device scalar, read by the kernels (no host synchronisation).  A lambda that is <= 0 or NaN, or so small or so
 * large that the float32 1 / (12 lambda) is infinite or zero, gives x = P_C(y) with no iteration.  lo, hi: host floats, lo <= hi,
 * -inf / +inf for no bound.  The momentum factors (t_k - 1) / t_{k+1} are computed on the host in double and rounded to float32.
 * Operation order, every operation a separately rounded IEEE float32 one (no FMA; division and square root correctly rounded),
 * which tests/tv_prox_ref.py follows operation for operation:
 *     t_a = (v_a > 0 ? d_a(v - e_a) : 0) - (v_a < n_a - 1 ? d_a(v) : 0),   div = (t_x + t_y) + t_z,   u = y(v) - lambda * div,
 *     P_C(u) = u < lo ? lo : (u > hi ? hi : u)                                  (d = r_k, or p_{n_iter} for the result);
 *     tau = 1 / (12 * lambda);   q_a = r_a + tau * (v_a < n_a - 1 ? x_k(v + e_a) - x_k(v) : 0);
 *     n = sqrt((q_x * q_x + q_y * q_y) + q_z * q_z),   m = n > 1 ? n : 1,   p_a = q_a / m   (one division per component);
 *     r_a' = p_a + mom * (p_a - p_a_previous).
 * No allocation, no atomics, no reduction, no host synchronisation; bit-reproducible and independent of the launch shape.
 * x may be y: the output pass reads y at its own voxel only (and the iterations never write x).  Neither may overlap the
 * scratch: a device buffer of at least r2_tv_prox_scratch_bytes(nx, ny, nz) bytes (nine floats per voxel), 4-byte aligned,
 * whose prior contents never matter. */
R2_API size_t r2_tv_prox_scratch_bytes(int nx, int ny, int nz);
R2_API int r2_tv_prox(int nx, int ny, int nz, const float *y, float *x, const float *lambda /* device scalar */, int n_iter,
                      float lo, float hi, void *scratch, size_t scratch_bytes, void *stream);

/* ---- isosurface extraction (csrc/isosurface.hip, r2_gaussian_amd/mesh.py) -------------------------------------------------
 * The level set {vol = level} of vol[nx][ny][nz] (z fastest; lattice point (i,j,k) has the linear index (i ny + j) nz + k) as an
 * indexed triangle mesh, by marching tetrahedra on the Kuhn (Freudenthal) subdivision: every cell of the lattice is cut into
 * the six tetrahedra 000 -> +e_a -> +e_a+e_b -> 111, one per permutation (a, b, c) of the axes.  All six share the body
 * diagonal and the face diagonals of neighbouring cells agree, so the surface is watertight and there is no ambiguous case.
 *   inside    a point is inside iff vol >= level (float32 compare).
 *   invalid   a value that is NaN, +-inf or above 1e38 in magnitude (!(|v| <= 1e38f)); invalid values are counted, compare as
 *             any float does (a NaN is outside), and the caller decides (mesh.py raises).  Without them fb - fa is finite.
 *   edges     every edge of every tetrahedron runs from a lattice point p to p + d, d in {0,1}^3 \ {0}, both in the lattice;
 *             its direction code is c = dx + 2 dy + 4 dz in 1..7, p OWNS it, and it is CROSSED iff exactly one end is inside.
 *   vertices  one per crossed edge, ordered by (owner's linear index, direction code) ascending.  With fa the owner's value,
 *             fb the other end's, every operation a separately rounded IEEE float32 one (no FMA, division correctly rounded):
 *                 t = (level - fa) / (fb - fa);   index-space coordinate  p_x = float(i) + t dx  (float(i) where dx = 0),
 *                 likewise y, z;   world coordinate  o_a + p_a * s_a  (a multiply, then an add).
 *   normals   (optional) the lattice gradient at a point is (f(q + e_a) - f(q - e_a)) / (2 * s_a), and the one-sided difference
 *             / s_a on a border; the edge gradient is g = ga + t * (gb - ga) (a subtraction, a multiply, an add), n =
 *             sqrt((gx * gx + gy * gy) + gz * gz), and the normal is (-g_a) / n, one division per component; (0, 0, 0) unless
 *             n > 0.  It points from inside to outside.
 *   faces     int32 triples of vertex ids.  Seen from the outside (the low side) the vertices run counter-clockwise: the
 *             geometric normal points from inside to outside.  A tetrahedron with one or three inside corners gives one
 *             triangle, with two a quad split along a fixed diagonal.  Degenerate triangles (a corner value equal to level)
 *             are kept, so that the surface stays closed.  Order: cells by their 000 corner's linear index, in a cell the
 *             tetrahedra by permutation (xyz, xzy, yxz, yzx, zxy, zyx); that order and the first vertex of a face are fixed.
 * A lattice with a dimension of 1 has no cells: no vertices and no faces (invalid values are still counted).
 * r2_isosurface_count reads the volume once, leaves in `ws` (r2_isosurface_workspace_bytes(nx, ny, nz): about six bytes per
 * lattice point, 128-byte aligned, prior contents never matter) every point's mask of crossed owned edges, its cell's triangle
 * count and its first vertex id, and writes counts[0..2] = vertices, triangles, invalid values (device long long [3]).  The
 * caller reads them -- the one host read of the operation -- allocates, and calls r2_isosurface_fill with the same volume,
 * level and workspace (const there: as count left it) and with the world frame o, s (host floats, s_a != 0).  fill writes
 * verts [n_verts,3], normals [n_verts,3] (NULL to skip) and faces [n_tris,3]; it never writes at or beyond row n_verts or
 * n_tris and never reads outside the volume or the workspace, whatever the workspace holds.  No atomics, no allocation, no
 * host synchronisation; two calls give identical bits.
 * R2_ERR_INVALID, nothing written: a dimension below 1, nx ny nz >= 2^31, n_verts or n_tris outside [0, 2^31), a NULL volume,
 * counts, workspace, or verts / faces that a non-zero count needs, too small a workspace. */
R2_API size_t r2_isosurface_workspace_bytes(int nx, int ny, int nz);
R2_API int r2_isosurface_count(int nx, int ny, int nz, const float *vol, float level, void *ws, size_t ws_bytes,
                               long long *counts /* device [3]: vertices, triangles, invalid voxels */, void *stream);
R2_API int r2_isosurface_fill(int nx, int ny, int nz, const float *vol, float level, float ox, float oy, float oz, float sx,
                              float sy, float sz, const void *ws /* as count left it */, size_t ws_bytes, long long n_verts,
                              long long n_tris, float *verts /* [n_verts,3] */, float *normals /* [n_verts,3] or NULL */,
                              int *faces /* [n_tris,3] */, void *stream);

/* ---- cubic-spline resampling of volumes (csrc/spline.hip, r2_gaussian_amd/resample.py) -------------------------------------
 * scipy.ndimage's zoom and map_coordinates for order = 3, mode = "nearest", prefilter = True, grid_mode = False, on
 * vol[nx][ny][nz] (z fastest): a prefilter that turns the samples into the coefficients of the interpolating cubic B-spline,
 * and two evaluators of that spline.  Every float32 operation below is a separately rounded IEEE one (no FMA, division correctly
 * rounded) in the order written, which tests/resample_ref.py follows operation for operation.
 *
 * r2_spline_prefilter: coeffs[nx+24][ny+24][nz+24] from vol.  The input is edge-padded by R2_SPLINE_PAD = 12 on every side,
 *     c(i,j,k) = vol(clamp(i-12, 0, nx-1), clamp(j-12, 0, ny-1), clamp(k-12, 0, nz-1)),
 * (read through clamped indices by the first pass: no padded copy exists), and every line of the padded block is filtered
 * along x, then along y, then along z.  With the pole z = sqrt(3) - 2 and, computed in double and rounded to float32 once each,
 *     Z = z,   G = (1 - z)(1 - 1/z) (= 6),   A = z / (z - 1),   ZP_i = z^i  (i = 1 .. R2_SPLINE_HORIZON),
 * a line c[0 .. n-1] (n >= 25) becomes
 *     g_i = G * c_i                                                  (every i; each pass applies the gain to its own input)
 *     s = g_0;   s = s + ZP_i * g_i  for i = 1 .. R2_SPLINE_HORIZON;   c_0 = g_0 + Z * s              (causal start)
 *     c_i = g_i + Z * c_{i-1}                                        for i = 1 .. n-1
 *     c_{n-1} = c_{n-1} * A                                                                           (anti-causal start)
 *     c_i = Z * (c_{i+1} - c_i)                                      for i = n-2 .. 0.
 * The two starts are those of a half-sample-symmetric extension of the line (what scipy's spline filter uses for "nearest":
 * c_0 += z sum_{i=0}^{n-1} z^i (c_i + z^n c_{n-1-i}) / (1 - z^{2n})), with the start sum cut off after R2_SPLINE_HORIZON = 16
 * terms and the z^n terms dropped: z^17 < 2^-32 and z^n <= z^25 < 2^-47 lie below the float32 rounding of the sum, and no power
 * of the pole becomes denormal.  r2_spline_prefilter_pass runs one pass: axis 0 pads and filters along x (reads vol, writes all
 * of coeffs), axes 1 and 2 filter coeffs in place (vol is not read); r2_spline_prefilter is passes 0, 1, 2.
 * coeffs may not overlap vol.
 *
 * r2_spline_zoom: out[mx][my][mz] from the coefficients, scipy's zoom onto a grid whose first and last nodes are the input's.
 * A first launch writes one table per axis into ws (r2_spline_zoom_workspace_bytes(mx, my, mz), 4-byte aligned, prior contents
 * never matter), in double: for output index o of an axis with n inputs and m outputs
 *     cc = o * ((n-1) / (m-1)) + 12   (the factor is 1 when m = 1),   start = floor(cc) - 1,   t = cc - floor(cc),
 *     w1 = (t*t*(t-2)*3 + 4) / 6;   u = 1 - t;   w2 = (u*u*(u-2)*3 + 4) / 6;   w0 = u*u*u / 6;   w3 = 1 - w0 - w1 - w2,
 * each product and sum left to right, each weight then rounded to float32 once.  Then, in float32,
 *     out(a,b,c) = sum_i wx_i ( sum_j wy_j ( sum_k wz_k * coeffs(sx+i, sy+j, sz+k) ) ),   i, j, k = 0 .. 3,
 * every sum from its first term to its last.  All taps lie inside the padded block.
 *
 * r2_spline_sample: out[N] at points[N][3], float32 index coordinates of the unpadded volume: scipy's map_coordinates.  Per
 * axis, in float32: cc = p + 12, clamped to [-1, n + 24] (one beyond the padded block on either side, as scipy does);
 * start = floor(cc) - 1, t = cc - floor(cc), the weights from t by the formulas above in float32, the tap indices
 * start .. start+3 clamped to the padded block [0, n + 23], and the nesting above.  A point with a NaN or infinite coordinate
 * gives NaN and reads nothing.  N = 0 is a no-op.
 *
 * No allocation, no atomics, no host synchronisation; two calls give identical bits.
 * R2_ERR_INVALID, nothing written: a dimension or an output dimension below 1, (nx+24)(ny+24)(nz+24) >= 2^31, mx my mz >= 2^31,
 * N < 0, an axis outside 0 .. 2, a NULL pointer that the call would use, too small a workspace. */
#define R2_SPLINE_PAD 12
#define R2_SPLINE_HORIZON 16
R2_API int r2_spline_prefilter(int nx, int ny, int nz, const float *vol, float *coeffs /* [nx+24][ny+24][nz+24] */, void *stream);
R2_API int r2_spline_prefilter_pass(int nx, int ny, int nz, const float *vol /* axis 0 only */, float *coeffs, int axis,
                                    void *stream);
R2_API size_t r2_spline_zoom_workspace_bytes(int mx, int my, int mz);
R2_API int r2_spline_zoom(int nx, int ny, int nz, const float *coeffs, int mx, int my, int mz, float *out /* [mx][my][mz] */,
                          void *ws, size_t ws_bytes, void *stream);
R2_API int r2_spline_sample(int nx, int ny, int nz, const float *coeffs, int N, const float *points /* [N,3] */,
                            float *out /* [N] */, void *stream);

/* ---- conditioning of measured projections (csrc/projections.hip, r2_gaussian_amd/projections.py) -----------------------------
 * What a measured projection stack src[V][H][W] (float32, W fastest) needs before it can be trained on: the resize of the
 * reference's real-data converter (cv2.resize with its row shift, clamp and crop) and a median filter against isolated
 * outliers.  Every float32 operation below is a separately rounded IEEE one (no FMA) in the order written, which
 * tests/projections_ref.py follows operation for operation.
 *
 * r2_proj_resize: dst[V][oh][ow] from src, per view: shift, lower clamp, resize to mh x mw, crop -- fused, so that only the
 * cropped outputs are computed and src is read once.
 *   Prepared pixel.  P(r, c) = x < lo ? lo : x  with  x = src(r + sr, c + sc)  where 0 <= r + sr < H and 0 <= c + sc < W, else
 *     P(r, c) = 0 (not lo).  lo = -inf switches the clamp off; a NaN stays a NaN.  sr = 5, lo = 0 is the reference's
 *     proj[proj < 0] = 0; proj_new[:-5] = proj[5:].
 *   Output pixel (i, j), 0 <= i < oh, 0 <= j < ow, is pixel (r0 + i, c0 + j) of the mh x mw resized image.
 *   interp = 0, cv2's INTER_LINEAR for float images.  A first launch writes one table per axis into ws
 *     (r2_proj_resize_workspace_bytes(mh, mw), 4-byte aligned, prior contents never matter; rows use n = H, m = mh, columns
 *     n = W, m = mw).  In double:  inv = (double)m / n,  scale = 1.0 / inv;  for output index d of the axis
 *         fx = (float)((d + 0.5) * scale - 0.5),   s = floor(fx),   f = fx - s  (float32);
 *         s < 0 gives s = 0, f = 0;   s >= n - 1 gives s = n - 1, f = 0;   the taps are s and min(s + 1, n - 1).
 *     Then, in float32, with rows r_0, r_1 and weights b0 = 1.f - f_row, b1 = f_row, columns c_0, c_1 and weights
 *     a0 = 1.f - f_col, a1 = f_col:
 *         h_i = P(r_i, c_0) * a0 + P(r_i, c_1) * a1   (i = 0, 1),       out = h_0 * b0 + h_1 * b1.
 *   interp = 1, box mean; only for H % mh == 0 and W % mw == 0 (fy = H / mh, fx = W / mw; the choice for integer down-sampling
 *     of noisy data).  Resized pixel (y, x):
 *         acc = P(y fy, x fx);   acc = acc + P(y fy + i, x fx + j)  for the remaining (i, j) of the block, row after row, each
 *         row from its first column to its last (i outer, j inner);   out = acc * (float)(1.0 / (fy fx)).
 *     ws is not used and may be NULL.
 *
 * r2_proj_median: dst[V][H][W] from src (dst may not overlap src), per view the median filter of the k x k window, k in {3, 5},
 * with replicated borders: scipy.ndimage.median_filter(size=k, mode="nearest").
 *     m(r, c) = the element of rank k k / 2 (counted from 0, ascending) of the k k values src(clamp(r + i, 0, H - 1),
 *     clamp(c + j, 0, W - 1)), |i|, |j| <= k / 2, a NaN among them read as +inf.
 *     replace(r, c) = !(|x - m| <= threshold)  with x = src(r, c) as it is and the difference in float32: true for a NaN x.
 *     conditional = 0: dst = m.   conditional = 1: dst = replace ? m : x.   flagged[V][H][W] (uint8, may be NULL) = replace,
 *     in either mode.  Where a window holds both -0 and +0 at the rank, which of them comes back is unspecified.
 *
 * No allocation, no atomics, no host synchronisation; two calls give identical bits.  V = 0 is a no-op.
 * R2_ERR_INVALID, nothing launched: V < 0; a dimension below 1; H W, mh mw >= 2^31; V H W or V oh ow >= 2^38; a crop window that
 * is empty or leaves the resized image; |sr| or |sc| above 2^30; a NaN lo; interp outside {0, 1}; interp = 1 with a factor that
 * is not an integer; k outside {3, 5}; conditional outside {0, 1}; a NaN threshold; 2^31 or more tiles of 64 x 16 pixels for the
 * median; a NULL pointer that the call would use; too small a workspace. */
R2_API size_t r2_proj_resize_workspace_bytes(int mh, int mw);
R2_API int r2_proj_resize(int V, int H, int W, const float *src, int sr, int sc, float lo, int interp, int mh, int mw, int r0,
                          int c0, int oh, int ow, float *dst /* [V][oh][ow] */, void *ws, size_t ws_bytes, void *stream);
R2_API int r2_proj_median(int V, int H, int W, const float *src, int k, int conditional, float threshold,
                          float *dst /* [V][H][W] */, unsigned char *flagged /* [V][H][W] or NULL */, void *stream);

/* ---- stripe (ring-artefact) removal along the view axis (csrc/destripe.hip, r2_gaussian_amd/projections.py) -------------------
 * A detector pixel whose gain or offset is slightly wrong adds the same constant to src(v, h, w) in every view v: invisible in
 * one projection, a ring in the reconstruction.  Both entries compare, for a fixed detector row h, neighbouring detector
 * columns w across all V views of src[V][H][W] (float32, W fastest).  They consist of comparisons, selections and the float32
 * and double operations written out below, each separately rounded (no FMA), in the order written: tests/destripe_ref.py
 * restates them in NumPy / SciPy and the results agree bit for bit.  k is the odd width of the window across the columns,
 * 1 <= k <= 31; clamp(x) below is min(max(x, 0), W - 1) (the replicated border), and "the median" of k values is their element
 * of rank k / 2, counted from 0 in ascending order.
 *
 * r2_proj_destripe_sort: dst[V][H][W] from src -- Vo, Atwood and Drakopoulos (2018), algorithm 3.  For every (h, w):
 *     c_v = src(v, h, w), v = 0 .. V-1, a NaN read as +inf (and -0 as +0).
 *     The column is ordered ascending; equal values are ordered by their view index (a stable sort: a clamped projection has
 *     long runs of exact zeros, and which of those views gets which rank changes the result).  S(r, h, w) is the value of rank
 *     r and I(r, h, w) the view it came from.
 *     M(r, h, w) = the median of the k values S(r, h, clamp(w + j)), |j| <= k / 2:
 *     scipy.ndimage.median_filter(S, size=(1, 1, k), mode="nearest").
 *     dst(I(r, h, w), h, w) = M(r, h, w).
 *   With k = 1 that is src itself (its NaNs as +inf), and it is written in one pass: nothing is sorted, ws is checked but not
 *   used.  Which of -0 and +0 comes back where both tie is unspecified.  dst doubles as scratch space while the call runs (it holds the sorted sinogram [H][W][V] before it holds the result); ws needs
 *   r2_proj_destripe_workspace_bytes(V, H, W, 0) = 6 V H W bytes, 4-byte aligned: the filtered sinogram [H][W][V] in float32
 *   and I as uint16.  V <= R2_DESTRIPE_MAX_VIEWS = 4096: a column is sorted as 64-bit keys (the value's order-preserving bits
 *   above the view index, so that the stable order is a plain integer order) in the LDS, padded to a power of two, and 4096
 *   keys are 32 KiB -- five workgroups still share the 160 KiB of a compute unit, and one stays within the 64 KiB that a
 *   workgroup may always have.
 *
 * r2_proj_destripe_mean: the classic normalisation by the mean profile.  For every (h, w):
 *     acc = 0.0 (double);   acc = acc + (double)src(v, h, w)   for v = 0 .. V-1 in this order;   m(h, w) = (float)(acc / V).
 *     s(h, w) = the median of the k values m(h, clamp(w + j)), |j| <= k / 2, a NaN among them read as +inf.
 *     d(h, w) = m(h, w) - s(h, w)                  (float32).
 *     dst(v, h, w) = src(v, h, w) - d(h, w)        (float32),   for every v.
 *   offsets[H][W] = d when the pointer is not NULL: the detector's offsets, a diagnostic.  dst may be NULL when offsets is not:
 *   then only the offsets are computed.  NaN inputs propagate: a pixel with a NaN in any view has a NaN m, hence a NaN d and a
 *   NaN in every view of dst; its neighbours see it as +inf in their windows.  With k = 1, d = m - m (0 for a finite m) and dst
 *   is src.  ws needs r2_proj_destripe_workspace_bytes(V, H, W, 1) = 8 H W bytes, 4-byte aligned (m and d).
 *
 * dst may not overlap src.  A workspace's prior contents never matter.  No allocation, no atomics, no host synchronisation;
 * two calls give identical bits.  V = 0 is a no-op (offsets is not written either).
 * R2_ERR_INVALID, nothing launched: V < 0; a dimension below 1; H W >= 2^31; V H W >= 2^38; k even or outside 1 .. 31;
 * V > R2_DESTRIPE_MAX_VIEWS for the sort; a NULL src, a NULL dst for the sort, dst and offsets both NULL for the mean, a NULL ws;
 * too small a workspace.  r2_proj_destripe_workspace_bytes returns 0 for arguments that the entries refuse. */
#define R2_DESTRIPE_MAX_VIEWS 4096
R2_API int r2_proj_destripe_max_views(void);   /* R2_DESTRIPE_MAX_VIEWS of the library that is loaded */
R2_API size_t r2_proj_destripe_workspace_bytes(int V, int H, int W, int method /* 0 sort, 1 mean */);
R2_API int r2_proj_destripe_sort(int V, int H, int W, const float *src, int k, float *dst /* [V][H][W] */, void *ws,
                                 size_t ws_bytes, void *stream);
R2_API int r2_proj_destripe_mean(int V, int H, int W, const float *src, int k, float *dst /* [V][H][W] or NULL */,
                                 float *offsets /* [H][W] or NULL */, void *ws, size_t ws_bytes, void *stream);

/* The forward passes order the Gaussians by depth with a bucket sort whose bucket boundaries follow the depth range seen
 * by the previous call with the same P (a per-thread hint: it saves five kernel launches and hides the num_rendered
 * read-back).  Results never depend on it -- both paths produce the exact (depth, id) order.  mode 0: never use hints,
 * 1: use them (default; the environment variable R2_DEPTH_HINT=0 also switches them off), 2: forget the history. */
R2_API void r2_depth_hint_control(int mode);

/* Tile-first binning of the rasterizer forward (csrc/raster_tilefirst.hip): single-view calls whose instance count the
 * calling thread can predict from its recent calls with the same P and detector size skip the global depth order -- instances
 * are counted and scattered per tile and every tile list is sorted on (depth, id) on its own -- and size the binning / image
 * state by that prediction (the exact count is still returned; a prediction that falls short only costs a second pass).
 * point_list, ranges, the render kernels' block masks, images and gradients are identical on both chains.  mode 0: never, 1: when applicable (default; the
 * environment variable R2_TILE_FIRST=0 also switches it off), 2: forget the calling thread's predictions (its next call of any
 * size takes the general chain). */
R2_API void r2_tile_first_control(int mode);
/* Deferred num_rendered (NEW; opt-in; SURVEY.md section 7 "kill the D2H sync", RAS/rasterizer_impl.cu:279).  mode 1 (or the
 * environment variable R2_DEFER_COUNT=1): a rasterizer forward on the tile-first chain returns WITHOUT waiting for the device --
 * the state is sized by the prediction + 50 %, every kernel is enqueued, and the value returned in place of num_rendered is a
 * TOKEN (>= 0x40000000) that the matching r2_raster_backward / _backward_batch accepts as its R: the backward reads the true count,
 * which the forward's second kernel posted to pinned host memory long before (any host thread may call it).  Images, state and
 * gradients are those of the waiting mode.  The price: a prediction that falls short cannot be repaired by a second pass any
 * more -- the backward of such a call FAILS with R2_ERR_INVALID (the forward's image is then invalid; render the view again with
 * the mode off), and callers that use the returned value as a count must not.  Forwards the chain does not take (first call of a
 * size, debug mode), and all voxelizer calls, wait as before.  mode 0: off (default). */
R2_API void r2_defer_count_control(int mode);
/* A deferred forward's token -> its true num_rendered, for callers that run no backward (evaluation under no_grad): waits for
 * the forward's control words like the backward does (stream: the forward's, for the drained-stream check).  R2_ERR_INVALID
 * with the backward's "sized for" message when the prediction fell short (the forward's image and state are invalid).  Repeat
 * calls are harmless and give the same answer: the token stays valid for its backward, until that backward has run or 64 later
 * deferred forwards have recycled its slot (then: a stale-token error).  A forward that fell short leaves nothing behind either
 * way -- the next forwards on its stream are exact whether or not anybody resolves its token. */
R2_API int r2_defer_count_resolve(int token, int *num_rendered, void *stream);
/* out[0] forwards that returned a token, [1] forwards that had to wait because 64 tokens were outstanding, [2] deferred forwards
 * whose prediction fell short -- each counted once, whether the forward thread's next forward, r2_defer_count_resolve or the
 * backward finds it.  out may be NULL (reset only). */
R2_API void r2_defer_count_stats(long long out[3], int reset);
/* process-wide counts since the last reset: out[0] forwards that took the tile-first chain, [1] forwards that did not (no
 * prediction yet, or beyond its limits), [2] chains enqueued a second time because the prediction fell short, [3] renders
 * repeated with the thin-Gaussian variant, [4] forwards whose prediction was seeded from another Gaussian count (the call after
 * a densification).  out may be NULL (reset only). */
R2_API void r2_tile_first_stats(long long out[5], int reset);

/* Stick-first binning of the voxelizer (csrc/voxel_sticks.hip): grids of more than 64 and up to 32 768 tiles (the 256^3 query of
 * test.py:105-112) are binned without a global sort -- instances are counted and scattered per STICK of up to 8 consecutive
 * tiles (per tile up to 4096 tiles) and every stick's list is sorted on (tile, z bits, id) on its own.  point_list, ranges,
 * volumes and gradients are identical on both chains; a large scene with very long lists (a list of more than 20 480 instances
 * and more than 8 Mi instances in all: the part-wise sort of such lists costs more than the general chain's radix passes;
 * r2_voxel_sticks_limits) continues on the general chain after the preprocess, and the calling thread remembers that for the
 * (P, grid).  Debug mode, larger grids
 * and P >= 2^29 always take the general chain, and so does a device that cannot give a workgroup the chain's 77.8 KB of LDS (parts
 * with a 64 KB limit; gfx950 has 160 KB per CU) -- r2_path_stats reports it as voxel.general.device_lds.  A (P, grid) that handed
 * over is remembered by the calling thread for its next 64 calls, then tried again.  mode 0: never, 1: whenever applicable
 * (default; the environment variable R2_VOXEL_STICKS=0 also switches it off), 3: forget the calling thread's notes; 4 / 5
 * (tests): lists of more than 8192 instances count as unsupported / are sorted in parts (default). */
R2_API void r2_voxel_sticks_control(int mode);
/* The two limits of that rule (process-wide; <= 0: the default).  Every thread's notes are dropped. */
R2_API void r2_voxel_sticks_limits(long long longest_list, long long instances);
/* process-wide counts since the last reset: out[0] forwards that took the chain, [1] forwards that left it after its scan for
 * the general chain, [2] forwards it declined.  out may be NULL (reset only). */
R2_API void r2_voxel_sticks_stats(long long out[3], int reset);

/* Which chain a forward took, and why the others did not (csrc/dispatch.hpp states the rules in one table): process-wide counters
 * since the last reset.  r2_path_stat_count() counters, r2_path_stat_name(i) names them ("raster.tile_first",
 * "raster.general.no_prediction", "voxel.stick_first", "voxel.general.long_lists", "raster.event.second_pass" ...), r2_path_stats
 * copies min(n, count) of them to out (may be NULL) and returns the count.  Results never depend on the chain. */
R2_API int r2_path_stat_count(void);
R2_API const char *r2_path_stat_name(int i);
R2_API int r2_path_stats(long long *out, int n, int reset);

/* Per-thread state.  The library keeps a few KB per host thread: self-resetting device counters of the tile-first rasterizer chain
 * and of the voxelizer's small-grid path and stick-first chain (one block per (device, stream) the thread has used, at most 16 of each:
 * the least recently used one is evicted), 128 bytes of pinned host memory for the num_rendered read-back, and the thread's
 * predictions and notes.
 * These -- and the convenience form r2_knn_dist2 -- are the only memory the library obtains itself; all of it is released when the
 * thread exits, or earlier by this call (waits for the device; the thread's next forward starts over). */
R2_API void r2_thread_release(void);

/* ---- introspection used by the parity tests (bit-exact tile / sort indices) ------------------- */
/* Byte offsets of the private arrays inside the state buffers of a forward call with the given sizes; lets
 * tests read the binning intermediates back without fixing the layout in the ABI.  which:
 *   0 tiles_touched u32[P]      1 point_offsets u32[P] (inclusive scan over Gaussians in depth order; with a depth hint
 *                                 only the entries of the visible Gaussians -- the first nvis -- are written)
 *   2 tiles_unsorted u32[R]     3 values_unsorted u32[R] (emission: depth-ordered Gaussians, tiles y/x-minor)
 *   4 tiles_sorted u32[R] (valid after backward, or for > 4096 tiles)   5 point_list u32[R] (== the reference's sorted point_list)
 *   6 ranges uint2[T]           7 cov3D f32[6P]
 *   8 n_contrib u32[N] (only filled when forward ran with debug != 0)
 *   9 packed render records f32[8P] (voxelizer: f32[12P])                14 {opacity, mu} f32[2P] (rasterizer)
 *  10 depth sort keys u32[P] (bits of the depth; 0xFFFFFFFF for culled Gaussians)
 *  11 first-instance index u32[P]   12 depth order u32[P] (ids sorted by (depth, id); culled ones behind, or unwritten with a hint)
 *  15 host-read words u32[8]: {num_rendered, overflow, thin flag, key extrema x4, nvis}
 *  13 inv u32[R] (sorted position of every emitted instance: the inverse permutation of the tile sort; the voxelizer only
 *     writes it for < 4096 tiles: single-pass tile sort)
 * buffer ids: 0 geometry, 1 binning, 2 image.  Returns -1 for an unknown id. */
R2_API long long r2_raster_state_offset(int which, int P, long long R, int width, int height, int *buffer_id);
R2_API long long r2_voxel_state_offset(int which, int P, long long R, int nx, int ny, int nz, int *buffer_id);

#ifdef __cplusplus
}
#endif
#endif /* R2HIP_H */
