// raster_api.hip -- extern "C" entry points of the rasterizer (see include/r2hip.h).
// Host orchestration of Rasterizer::forward / backward (RAS/rasterizer_impl.cu:196-421).
#include "raster_state.hpp"
#include "voxel_state.hpp"
#include "dispatch.hpp"
#include "chain_general.hpp"
#include "host_tables.hpp"

using namespace r2;

static EnvSwitch g_sorted_records("R2_SORTED_RECORDS", true), g_emit_hist("R2_EMIT_HIST", true);

// Forward of V views of the same Gaussians (V = 1: the reference's call).  viewmatrices / projmatrices: [V,16]; out_color
// [V,H,W]; radii [V,P].  See raster_state.hpp (tile_decode) for how the views share one pipeline.
static int raster_forward_impl(
    const char *what, r2_alloc_fn geometryBuffer, void *geometry_user, r2_alloc_fn binningBuffer, void *binning_user,
    r2_alloc_fn imageBuffer, void *image_user, int P, int V, int width, int height, const float *means3D,
    const float *opacities, const float *scales, float scale_modifier, const float *rotations,
    const float *cov3D_precomp, const float *viewmatrices, const float *projmatrices,
    float tan_fovx, float tan_fovy, int mode, float *out_color, int *radii, int debug, hipStream_t s)
{
    host_mark_forward_begin();
    if (P < 0 || V < 1 || width <= 0 || height <= 0 || !geometryBuffer || !binningBuffer || !imageBuffer || !out_color) {
        set_error("%s: invalid argument", what);
        return R2_ERR_INVALID;
    }
    const size_t N = (size_t)width * height * (size_t)V;
    const int gx = (width + TILE2D - 1) / TILE2D, gy = (height + TILE2D - 1) / TILE2D;
    const size_t T = (size_t)gx * gy * (size_t)V;
    if ((size_t)P * (size_t)V >= (size_t)1 << 31 || T >= (size_t)1 << 24) {
        set_error("%s: %d views x %d Gaussians / %zu tiles exceed the 31-bit instance / 24-bit tile range", what, V, P, T);
        return R2_ERR_INVALID;
    }
    if (P == 0) {   // the torch boundary skips the call (SUB/rasterize_points.cu:70); out_color is pre-zeroed
        R2_HIP_TRY(hipMemsetAsync(out_color, 0, N * sizeof(float), s));
        return 0;
    }
    if (!means3D || !opacities || !viewmatrices || !projmatrices || !radii ||
        (!cov3D_precomp && (!scales || !rotations))) {
        set_error("%s: NULL input (need means3D, opacities, matrices, radii and scales+rotations or cov3D_precomp)", what);
        return R2_ERR_INVALID;
    }
    if (mode != 0 && mode != 1) {
        set_error("%s: unsupported mode %d", what, mode);
        return R2_ERR_INVALID;
    }
    const int PV = P * V;   // view instances: everything between the preprocess and the render kernels works on these

    // tile-first binning (raster_tilefirst.hip): calls whose instance count this thread can predict from its recent calls (one
    // view, or V stacked views of up to 4096 tiles in all); everything else -- first call of a size, debug mode, huge grids --
    // takes the chain below
    if (!debug) {
        const int r = raster_forward_tilefirst(what, geometryBuffer, geometry_user, binningBuffer, binning_user, imageBuffer, image_user,
                                               P, V, width, height, means3D, opacities, scales, scale_modifier, rotations, cov3D_precomp,
                                               viewmatrices, projmatrices, tan_fovx, tan_fovy, mode, out_color, radii, s);
        if (r != TF_NOT_TAKEN) {
            if (r >= 0) host_mark_forward_end();
            return r;
        }
    } else {
        path_count(PS_RAS_GENERAL_DEBUG);
    }

    char *gchunk = geometryBuffer(RasterGeom::carve(nullptr, PV).bytes, geometry_user);
    if (!gchunk) {
        set_error("%s: state allocation callback returned NULL", what);
        return R2_ERR_ALLOC;
    }
    const RasterGeom geom = RasterGeom::carve(gchunk, PV);

    // Binning, first half (chain_general.hpp): view instances in (depth, id) order + their instance offsets in that order.
    // sorted records for the emission kernel: the preprocess hands each key's tile rectangle (one word) to the depth order
    uint32_t *host_words = geom.host_words;
    ChainOrder ord;
    int rc = chain_depth_order(
        CHAIN_RASTER, what, geom, PV, RASTER_STAGES,
        [&](const DepthReg &reg) {
            launch_raster_preprocess(geom, P, V, means3D, scales, scale_modifier, rotations, opacities, cov3D_precomp, viewmatrices,
                                     projmatrices, width, height, tan_fovx, tan_fovy, mode, radii, host_words + DW_USER, reg, true, s);
        },
        /*skip_preprocess=*/false, /*rects_allowed=*/g_sorted_records.on() && gx <= 256 && gy <= 256, /*reset_nvis_on_overflow=*/false, debug, s, &ord);
    if (rc) return rc;
    const size_t R = ord.num_rendered;

    RasterBinning bin{};
    RasterImage img{};
    rc = chain_state(what, binningBuffer, binning_user, imageBuffer, image_user, R,
                     [&](char *chunk) { return RasterImage::carve(chunk, T, N, R, debug != 0); }, &bin, &img);
    if (rc) return rc;

    // second half: stable sort by tile id; payloads: the emission index (-> perm, the backward's scratch row) and the Gaussian
    // id (-> point_list)
    const WorkListOut wo{img.ranges, img.chunk_base, img.work_tile, (uint32_t)T, FWD_CHUNK, debug ? nullptr : img.tile_done, 0u, 0u,
                         raster_ids_leave_room_for_masks((size_t)PV) ? 1u : 0u};
    // > 4096 tiles: general multi-pass sort, then invert its permutation (perm: the backward's scratch, free until then)
    const ChainMultiPass mp{nullptr, reinterpret_cast<uint32_t *>(bin.part), bin.vals_unsorted, bin.point_list, bin.inv};
    ChainLists lists;
    rc = chain_tile_lists(
        bin, img, R, T, RASTER_STAGES,
        [&](int bit, bool) {
            bool hist_ready = false;   // the emission kernel built the tile sort's histograms as well
            if (ord.rects && !ord.full_order) {
                TileSortPlan plan;
                if (g_emit_hist.on() && !debug && tile_sort_plan(bin.sort_temp, bin.sort_bytes, R, bit, &plan))
                    hist_ready = launch_raster_emit_hist(geom, bin, P, V, width, height, host_words + DW_NVIS, R, plan, s);
                if (!hist_ready) launch_raster_duplicate_sorted(geom, bin, P, V, width, height, host_words + DW_NVIS, s);
            } else {
                launch_raster_duplicate(geom, bin, P, V, radii, width, height, ord.full_order ? nullptr : host_words + DW_NVIS, s);
            }
            return hist_ready;
        },
        wo, mp, /*zero_ranges_in_duplicate=*/false, debug, s, &lists);
    if (rc) return rc;
    { StageScope t(ST_RAS_RENDER_FWD, s);
    // single-pass sort: the tile's last work item (or the combine kernel) also writes tiles[k] for the backward
    launch_raster_render_forward(geom, bin, img, width, height, V, out_color, debug != 0, lists.tile_counts ? bin.tiles : nullptr,
                                 /*fused_combine=*/lists.work_built && debug == 0, s, nullptr, nullptr, (size_t)PV); }
    R2_STAGE_CHECK(debug, s, "render");
    // the next call's prediction (visible keys are positive floats: their range is the P class of the host words)
    raster_tilefirst_note(P, V, width, height, ord.num_rendered, ord.hw[DW_USER] != 0, ord.hw[DW_PMAX], ~ord.hw[DW_PNMAX]);
    host_mark_forward_end();
    return (int)ord.num_rendered;
}

static int raster_backward_impl(
    const char *what, int P, int V, int R, int width, int height, const float *means3D, const float *scales, float scale_modifier,
    const float *rotations, const float *cov3D_precomp, const float *viewmatrices, const float *projmatrices,
    float tan_fovx, float tan_fovy, const int *radii, char *geom_buffer, char *binning_buffer,
    const float *dL_dpix, float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dmu,
    float *dL_dmean3D, float *dL_dcov3D, float *dL_dscale, float *dL_drot, int mode, int debug, hipStream_t s)
{
    if (P == 0) return 0;
    if (P < 0 || V < 1 || R < 0 || !means3D || !radii || !geom_buffer || (R > 0 && !binning_buffer) || !dL_dpix ||
        !viewmatrices || !projmatrices || !dL_dmean2D || !dL_dconic || !dL_dopacity || !dL_dmu || !dL_dmean3D || !dL_dcov3D ||
        (!cov3D_precomp && (!scales || !rotations || !dL_dscale || !dL_drot))) {
        set_error("%s: invalid argument", what);
        return R2_ERR_INVALID;
    }
    if (R >= DEFER_TOKEN_FLAG) {   // a deferred forward's token (r2_defer_count_control): the count is on its way, or long here
        uint32_t true_R = 0;
        const int rc = raster_resolve_deferred(what, R, s, &true_R, true);
        if (rc) return rc;
        R = (int)true_R;
    }
    const RasterGeom geom = RasterGeom::carve(geom_buffer, P * V);
    const RasterBinning bin = RasterBinning::carve(binning_buffer, (size_t)R);
    { StageScope t(ST_RAS_RENDER_BWD, s);
    launch_raster_render_backward(geom, bin, radii, width, height, V, (size_t)R, dL_dpix, s, (size_t)P * (size_t)V); }
    R2_STAGE_CHECK(debug, s, "render backward");
    const float *cov3D = cov3D_precomp ? cov3D_precomp : geom.cov3D;
    { StageScope t(ST_RAS_GEOM_BWD, s);
    launch_raster_geom_backward(P, V, means3D, radii, cov3D, scales, rotations, scale_modifier, width, height, tan_fovx,
                                tan_fovy, viewmatrices, projmatrices, dL_dconic, dL_dmu, dL_dmean2D, dL_dopacity, dL_dmean3D,
                                dL_dcov3D, dL_dscale, dL_drot, mode, geom, bin.part, s); }
    R2_STAGE_CHECK(debug, s, "geometry backward");
    return 0;
}

extern "C" int r2_raster_forward(
    r2_alloc_fn geometryBuffer, void *geometry_user, r2_alloc_fn binningBuffer, void *binning_user,
    r2_alloc_fn imageBuffer, void *image_user, int P, int width, int height, const float *means3D,
    const float *opacities, const float *scales, float scale_modifier, const float *rotations,
    const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, const float *cam_pos,
    float tan_fovx, float tan_fovy, int prefiltered, int mode, float *out_color, int *radii, int debug, void *stream)
{
    (void)cam_pos;
    (void)prefiltered;   // the reference only uses it to trap on an impossible state (RAS/auxiliary.h:160-164)
    return raster_forward_impl("r2_raster_forward", geometryBuffer, geometry_user, binningBuffer, binning_user, imageBuffer, image_user,
                               P, 1, width, height, means3D, opacities, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix,
                               projmatrix, tan_fovx, tan_fovy, mode, out_color, radii, debug, (hipStream_t)stream);
}

extern "C" int r2_raster_backward(
    int P, int R, int width, int height, const float *means3D, const float *scales, float scale_modifier,
    const float *rotations, const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix,
    const float *campos, float tan_fovx, float tan_fovy, const int *radii, char *geom_buffer, char *binning_buffer,
    char *img_buffer, const float *dL_dpix, float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dmu,
    float *dL_dmean3D, float *dL_dcov3D, float *dL_dscale, float *dL_drot, int mode, int debug, void *stream)
{
    (void)campos;
    (void)img_buffer;
    return raster_backward_impl("r2_raster_backward", P, 1, R, width, height, means3D, scales, scale_modifier, rotations, cov3D_precomp,
                                viewmatrix, projmatrix, tan_fovx, tan_fovy, radii, geom_buffer, binning_buffer, dL_dpix, dL_dmean2D,
                                dL_dconic, dL_dopacity, dL_dmu, dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot, mode, debug,
                                (hipStream_t)stream);
}

// ---- batched views (new functionality; the reference renders one view per call): see include/r2hip.h
extern "C" int r2_raster_forward_batch(
    r2_alloc_fn geometryBuffer, void *geometry_user, r2_alloc_fn binningBuffer, void *binning_user,
    r2_alloc_fn imageBuffer, void *image_user, int P, int V, int width, int height, const float *means3D,
    const float *opacities, const float *scales, float scale_modifier, const float *rotations,
    const float *cov3D_precomp, const float *viewmatrices, const float *projmatrices,
    float tan_fovx, float tan_fovy, int mode, float *out_color, int *radii, int debug, void *stream)
{
    return raster_forward_impl("r2_raster_forward_batch", geometryBuffer, geometry_user, binningBuffer, binning_user, imageBuffer,
                               image_user, P, V, width, height, means3D, opacities, scales, scale_modifier, rotations, cov3D_precomp,
                               viewmatrices, projmatrices, tan_fovx, tan_fovy, mode, out_color, radii, debug, (hipStream_t)stream);
}

extern "C" int r2_raster_backward_batch(
    int P, int V, int R, int width, int height, const float *means3D, const float *scales, float scale_modifier,
    const float *rotations, const float *cov3D_precomp, const float *viewmatrices, const float *projmatrices,
    float tan_fovx, float tan_fovy, const int *radii, char *geom_buffer, char *binning_buffer, char *img_buffer,
    const float *dL_dpix, float *dL_dmean2D, float *dL_dconic, float *dL_dopacity, float *dL_dmu,
    float *dL_dmean3D, float *dL_dcov3D, float *dL_dscale, float *dL_drot, int mode, int debug, void *stream)
{
    (void)img_buffer;
    return raster_backward_impl("r2_raster_backward_batch", P, V, R, width, height, means3D, scales, scale_modifier, rotations,
                                cov3D_precomp, viewmatrices, projmatrices, tan_fovx, tan_fovy, radii, geom_buffer, binning_buffer,
                                dL_dpix, dL_dmean2D, dL_dconic, dL_dopacity, dL_dmu, dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot, mode,
                                debug, (hipStream_t)stream);
}

extern "C" int r2_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                               uint8_t *present, void *stream)
{
    (void)projmatrix;
    if (P == 0) return 0;
    if (P < 0 || !means3D || !viewmatrix || !present) {
        set_error("r2_mark_visible: invalid argument");
        return R2_ERR_INVALID;
    }
    launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream);
    R2_STAGE_CHECK(0, (hipStream_t)stream, "markVisible");
    return 0;
}

extern "C" long long r2_raster_state_offset(int which, int P, long long R, int width, int height, int *buffer_id)
{
    char *const base = reinterpret_cast<char *>(uintptr_t(1) << 40);   // fake base: only differences are used
    const int gx = (width + TILE2D - 1) / TILE2D, gy = (height + TILE2D - 1) / TILE2D;
    const RasterGeom g = RasterGeom::carve(base, P);
    const RasterBinning b = RasterBinning::carve(base, (size_t)R);
    const RasterImage im = RasterImage::carve(base, (size_t)gx * gy, (size_t)width * height, (size_t)R, true);
    const char *p = nullptr;
    int buf = -1;
    switch (which) {
    case 0: p = (char *)g.tiles_touched; buf = 0; break;
    case 1: p = (char *)g.offsets; buf = 0; break;
    case 2: p = (char *)b.tiles_unsorted; buf = 1; break;
    case 3: p = (char *)b.vals_unsorted; buf = 1; break;
    case 4: p = (char *)b.tiles; buf = 1; break;
    case 5: p = (char *)b.point_list; buf = 1; break;
    case 6: p = (char *)im.ranges; buf = 2; break;
    case 7: p = (char *)g.cov3D; buf = 0; break;
    case 8: p = (char *)im.n_contrib; buf = 2; break;
    case 9: p = (char *)g.rec; buf = 0; break;
    case 10: p = (char *)g.depth_key; buf = 0; break;
    case 12: p = (char *)g.order; buf = 0; break;
    case 11: p = (char *)g.first; buf = 0; break;
    case 13: p = (char *)b.inv; buf = 1; break;
    case 14: p = (char *)g.op_mu; buf = 0; break;
    case 15: p = (char *)g.host_words; buf = 0; break;
    case 16: p = (char *)b.masked; buf = 1; break;
    default: return -1;
    }
    if (buffer_id) *buffer_id = buf;
    return (long long)(p - base);
}

// Everything the library keeps per host thread -- the self-resetting counter blocks of the tile-first rasterizer chain and of the
// small-grid voxelizer path (a few KB of device memory per (device, stream) the thread has used), its pinned mailbox words, its
// predictions -- is released when the thread exits; a long-lived thread can give it back earlier with this call.  Waits for
// the device (hipFree).  The next forward of the thread simply starts over.
extern "C" void r2_thread_release(void)
{
    r2::raster_tilefirst_release();
    r2::voxel_small_release();
    r2::voxel_sticks_release();
    r2::host_words_release();
}
