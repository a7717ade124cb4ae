// chain_general.hpp -- the host sequence of the GENERAL forward chain, written once for the rasterizer and the voxelizer
// (raster_api.hip / voxel_api.hip), and the two steps every chain of either operator shares: the num_rendered range check and the
// allocation of the binning and image state.  What differs between the operators comes in as flags, stage ids and small callables;
// the order in which work is enqueued on the stream is each operator's own, memsets and event records included.
#pragma once
#include "r2_common.hpp"

namespace r2 {

// also the class of the depth hint history (depth_hint_lookup / depth_hint_update)
enum ChainOperator { CHAIN_RASTER = 0, CHAIN_VOXEL = 1 };

struct ChainStages { int preprocess, scan, depthsort, duplicate, sort, ranges; };
constexpr ChainStages RASTER_STAGES{ST_RAS_PREPROCESS, ST_RAS_SCAN, ST_RAS_DEPTHSORT, ST_RAS_DUPLICATE, ST_RAS_SORT, ST_RAS_RANGES};
constexpr ChainStages VOXEL_STAGES{ST_VOX_PREPROCESS, ST_VOX_SCAN, ST_VOX_DEPTHSORT, ST_VOX_DUPLICATE, ST_VOX_SORT, ST_VOX_RANGES};

// the API returns num_rendered as a non-negative int (like the reference's int num_rendered)
inline int check_num_rendered(ChainOperator op, const char *what, uint32_t num_rendered)
{
    if (num_rendered <= 0x7FFFFFFFu) return 0;
    if (op == CHAIN_RASTER) set_error("%s: more than 2147483647 (tile, Gaussian) instances: they do not fit the 31-bit num_rendered", what);
    else set_error("%s: %u (tile, Gaussian) instances do not fit the 31-bit num_rendered", what, num_rendered);
    return R2_ERR_INVALID;
}

// The two state buffers that are sized by the instance count R: the sorted lists (+ backward scratch) and the forward work list /
// per-chunk partial images.  carve_image(chunk) is Image::carve with the call site's arguments (chunk = nullptr: sizes only).
template <class Binning, class Image, class CarveImage>
int chain_state(const char *what, r2_alloc_fn binningBuffer, void *binning_user, r2_alloc_fn imageBuffer, void *image_user, size_t R,
                CarveImage &&carve_image, Binning *bin, Image *img)
{
    char *bchunk = binningBuffer(Binning::carve(nullptr, R).bytes, binning_user);
    char *ichunk = imageBuffer(carve_image(nullptr).bytes, image_user);
    if (!bchunk || !ichunk) {
        set_error("%s: binning/image allocation callback returned NULL", what);
        return R2_ERR_ALLOC;
    }
    *bin = Binning::carve(bchunk, R);
    *img = carve_image(ichunk);
    return 0;
}

// Binning, first half: the n keys (view instances / Gaussians) in (depth, id) order + their instance offsets in that order.
//   hinted path (depth range known from the previous call with this size): preprocess registers every key in its bucket,
//   one dual scan + place + rank finish the job, and the host's read-back overlaps place + rank;
//   un-hinted path: min/max, count, scan, place, rank, then the offsets scan;
//   either may overflow a bucket (many identical depths / a stale hint): general radix sort + scan instead.
struct ChainOrder {
    uint32_t num_rendered;
    bool full_order;   // order / offsets cover all n keys (else only the visible prefix)
    bool rects;        // the depth order carried each key's tile rectangle into sorted records (rasterizer)
    uint32_t hw[DW_COUNT];
};
// geom: RasterGeom / VoxelGeom (their depth-order members carry the same names).  preprocess(reg) launches the kernel that
// produces the keys; skip_preprocess: it has run already, un-hinted (the stick chain's hand-over).  rects_allowed: a hinted call may
// ask the depth order for sorted records.  reset_nvis_on_overflow: see below -- the voxelizer's geometry backward needs it, the
// rasterizer's does not.
template <class Geom, class Preprocess>
int chain_depth_order(ChainOperator op, const char *what, const Geom &geom, int n, const ChainStages &st, Preprocess &&preprocess,
                      bool skip_preprocess, bool rects_allowed, bool reset_nvis_on_overflow, int debug, hipStream_t s, ChainOrder *out)
{
    int rc = depth_order_prepare(geom.dorder_temp, geom.dorder_bytes, (size_t)n, s);   // zeroes counters + the host-read words
    if (rc) return rc;
    uint32_t *host_words = geom.host_words;
    DepthHint hint;
    const bool hinted = !skip_preprocess && depth_hint_lookup(op, (size_t)n, &hint);
    const uint32_t pre_wgs = (uint32_t)((n + 255) / 256);
    DepthReg reg{};
    const bool rects = hinted && rects_allowed;
    if (hinted) reg = depth_order_reg(geom.dorder_temp, (size_t)n, hint, rects);
    if (!skip_preprocess) {
        StageScope t(st.preprocess, s);
        preprocess(reg);
    }
    R2_STAGE_CHECK(debug, s, "preprocess");
    uint32_t *hw = out->hw;
    for (int i = 0; i < DW_COUNT; ++i) hw[i] = 0;
    if (hinted) {
        uint32_t *mailbox = nullptr, mailbox_seq = 0;
        rc = host_mailbox_arm(&mailbox, &mailbox_seq);
        if (rc) return rc;
        { StageScope t(st.scan, s);
        rc = depth_order_fast_scan(geom.dorder_temp, (size_t)n, pre_wgs, mailbox, mailbox_seq, s); }
        if (rc) return rc;
        { StageScope t(st.depthsort, s);
        rc = depth_order_fast_finish(geom.dorder_temp, (size_t)n, geom.depth_key, geom.tiles_touched, geom.order, geom.offsets, s, rects); }
        if (rc) return rc;
        rc = host_mailbox_wait(mailbox_seq, hw, DW_COUNT, s);   // the GPU places + ranks while the host waits for the words
        if (rc) return rc;
        R2_STAGE_CHECK(debug, s, "depth order (hinted)");
    } else {
        { StageScope t(st.depthsort, s);
        rc = depth_order_buckets(geom.dorder_temp, geom.dorder_bytes, geom.depth_key, geom.order, (size_t)n, s); }
        if (rc) return rc;
        R2_STAGE_CHECK(debug, s, "depth order");
        // (fusing the scan's per-group reduction into the depth order's last kernel with per-wave atomics was measured
        // 4x slower than this separate 5 us kernel: ~5k atomics on ~75 addresses serialise at the memory side)
        { StageScope t(st.scan, s);
        rc = inclusive_scan_gather_u32(geom.scan_temp, geom.scan_bytes, geom.tiles_touched, geom.order, geom.offsets, n, s,
                                       host_words + DW_TOTAL); }
        if (rc) return rc;
        R2_STAGE_CHECK(debug, s, "scan");
        // total number of (tile, Gaussian) instances: sizes the binning state (the reference's D2H, RAS/rasterizer_impl.cu:279,
        // VOX/voxelizer_impl.cu:248)
        rc = read_host_words(host_words, hw, DW_COUNT, s);
        if (rc) return rc;
    }
    out->num_rendered = hw[DW_TOTAL];
    out->rects = rects;
    const bool overflow = hw[DW_OVERFLOW] != 0;
    out->full_order = !hinted;
    if (overflow) {   // general radix sort instead
        rc = sort_pairs_ex(geom.psort_temp, geom.psort_bytes, geom.depth_key, geom.depth_sorted, nullptr /* values = indices */, geom.order, nullptr,
                           nullptr, (size_t)n, 32, /*allow_skip=*/true, nullptr, s);
        if (!rc) rc = inclusive_scan_gather_u32(geom.scan_temp, geom.scan_bytes, geom.tiles_touched, geom.order, geom.offsets, n,
                                                s, host_words + DW_TOTAL);
        uint32_t total = 0;
        if (!rc) rc = read_host_words(host_words + DW_TOTAL, &total, 1, s);
        if (rc) return rc;
        out->num_rendered = total;
        out->full_order = true;
        // (voxelizer) `order` is now a permutation of ALL P ids (culled ones interleaved: their depth_key is bits(z), not a sentinel),
        // but the dual scan left its visible count in the device word: the geometry backward would walk only that prefix
        // and skip visible Gaussians sorted behind it.  0 = "walk all of it" (voxel_geom_backward_kernel).
        if (reset_nvis_on_overflow) R2_HIP_TRY(hipMemsetAsync(host_words + DW_NVIS, 0, sizeof(uint32_t), s));
    }
    depth_hint_update(op, (size_t)n, hw, overflow);
    return check_num_rendered(op, what, out->num_rendered);
}

// Binning, second half: one (tile, payload) pair per instance, emitted in depth order; a stable sort by tile id; tile ranges and the
// forward work list.  duplicate(bit, ranges_zeroed) launches the emission and says whether it built the tile sort's histograms
// as well.  wo: what block 0 of the single-pass sort's last kernel builds (and the chunk / min_len of the work list when the sort
// took several passes); the multi-pass sort (> 4096 tiles) writes its keys to bin.tiles and moves the payloads named here.
struct ChainMultiPass { const uint32_t *vin; uint32_t *vout; const uint32_t *win; uint32_t *wout; uint32_t *inv; };
struct ChainLists {
    const uint32_t *tile_counts = nullptr;   // single-pass sort: the per-tile counts, a by-product
    bool work_built = false;                 // ranges + work list already produced by the sort's last kernel
};
// zero_ranges_in_duplicate: ahead of a multi-pass sort the emission kernel zero-fills img.ranges for tile_ranges() (voxelizer)
template <class Binning, class Image, class Duplicate>
int chain_tile_lists(const Binning &bin, const Image &img, size_t R, size_t T, const ChainStages &st, Duplicate &&duplicate,
                     const WorkListOut &wo, const ChainMultiPass &mp, bool zero_ranges_in_duplicate, int debug, hipStream_t s,
                     ChainLists *out)
{
    int rc = 0;
    bool ranges_zeroed = false;   // img.ranges zero-filled by the duplicate kernel
    if (R > 0) {
        const int bit = (int)higher_msb((uint32_t)(T > 1 ? T - 1 : 1));   // bits of the largest tile id (the reference
                                                                     // sorts getHigherMsb(T) bits: one more for T = 2^k)
        ranges_zeroed = zero_ranges_in_duplicate && !sort_is_single_pass(bit);
        bool hist_ready = false;
        { StageScope t(st.duplicate, s);
        hist_ready = duplicate(bit, ranges_zeroed); }
        R2_STAGE_CHECK(debug, s, "duplicateWithKeys");
        { StageScope t(st.sort, s);
        if (sort_is_single_pass(bit)) {
            rc = sort_by_tile_single_pass(bin.sort_temp, bin.sort_bytes, bin.tiles_unsorted, bin.vals_unsorted, bin.point_list,
                                          debug ? bin.inv : nullptr, R, bit, &out->tile_counts, s, &wo, hist_ready);   // inv: introspection only
            out->work_built = true;
        } else {
            rc = sort_pairs_ex(bin.sort_temp, bin.sort_bytes, bin.tiles_unsorted, bin.tiles, mp.vin, mp.vout, mp.win, mp.wout, R, bit,
                               false, nullptr, s, mp.inv);
        } }
        if (rc) return rc;
        R2_STAGE_CHECK(debug, s, "sort");
    }
    { StageScope t(st.ranges, s);
    if (out->work_built) {
        // nothing to do
    } else if (out->tile_counts) {   // single-pass sort: per-tile counts are a by-product
        launch_ranges_and_work(out->tile_counts, (uint32_t)T, wo.chunk, img.ranges, img.chunk_base, img.work_tile, s, wo.min_len);
    } else {
        rc = tile_ranges(bin.tiles, nullptr, nullptr, nullptr, R, img.ranges, T, s, ranges_zeroed);
        if (rc) return rc;
        launch_build_work(img.ranges, (uint32_t)T, wo.chunk, img.chunk_base, img.work_tile, img.work_temp, s, wo.min_len);
    } }
    R2_STAGE_CHECK(debug, s, "identifyTileRanges");
    return 0;
}

}  // namespace r2
