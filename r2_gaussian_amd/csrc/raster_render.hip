// raster_render.hip -- per-tile additive line-integral render of the X-ray rasterizer and its backward.
//
// Reference: renderCUDA forward RAS/forward.cu:294-395, renderCUDA backward RAS/backward.cu:447-575.
// 256 pixel-Gaussian pairs per 32 bytes gathered: never HBM-bound; compiled with FMA contraction ON and without SLP
// packing; results are tolerance-checked, not bit-checked.  What bounds them today is in DESIGN.md section 4.
//
// Forward : a tile's depth-sorted list is cut into work items of FWD_CHUNK instances (list lengths span 0..9000 on the
//           benchmark scene, median 50: a workgroup per tile left most CUs idle behind a few dense tiles).  One
//           workgroup = one work item; its 4 waves own the tile's four 8x8 pixel blocks; records are staged through LDS
//           in 256-record batches; one LANE evaluates one record against the 64 pixels of the block (see below).  Each
//           work item produces 256 partial pixel sums; the tile's LAST work item to finish adds them IN LIST ORDER, so
//           the image is deterministic.
// Backward: one LANE owns one 8x8 block of one (tile, Gaussian) instance of the sorted list; dL/dpix of the wave's tiles
//           is staged in LDS.  The 7 gradient sums of the reference are linear in 6 moments
//           sum(w), sum(w dx), sum(w dy), sum(w dx^2), sum(w dx dy), sum(w dy^2), w = G*dL/dpix,
//           accumulated in registers: NO atomics -- each instance adds its blocks' rows in a fixed order and stores its
//           moment row to scratch at its EMISSION index (recomputed from the Gaussian's tile rectangle; contiguous per
//           Gaussian), which the geometry backward then reduces in a fixed order.  Gradients are therefore
//           bit-reproducible, unlike the reference's float atomicAdd accumulation (RAS/backward.cu:562-572).
//           One-wave workgroups walk chunks of 64 consecutive instances of the global sorted list (software-pipelined);
//           waves that straddle many sparse tiles (image borders) take their tiles three at a time.
//           The reference's n_contrib skip (RAS/backward.cu:523-525) only prunes pairs that failed the
//           forward tests; re-evaluating the tests prunes the same pairs, so n_contrib is not needed.
#include "raster_state.hpp"

R2_TS_DEFINE(render)

namespace r2 {

// ------------------------------------------------------------------------------------------------ forward
// Work item = (<= FWD_CHUNK consecutive instances of one tile list) x (one 8x8 pixel block): a workgroup's 4 waves own
// the 4 blocks of the tile and never synchronise with each other.
//
// Production kernel (item-parallel): one LANE owns one list entry and evaluates the 64 pixels of the wave's block
// into 64 register accumulators; the workgroup stages 256 entries at a time in LDS and every wave compacts the ones
// whose alpha >= 1e-5 bounding box touches its block (ballot + prefix popcount, 46 % survive on the benchmark scene)
// so that its lanes work on live entries only; at the end one 64x64 transpose-reduction (6 butterfly steps) leaves
// pixel p's sum in lane p.  Lane-per-entry makes the Gaussian separable along a pixel row: alpha(c+1) = alpha(c) * r(c),
// r(c+1) = r(c) * exp2(2 A2), i.e. TWO v_exp_f32 per 8-pixel row instead of 8 -- v_exp_f32 issues at ~1/8 the rate
// of an FMA on gfx950 and was ~40 % of the pixel-parallel kernel's issue time.  Entries that are too thin for the
// 8-step recurrence are re-anchored at pixel 4, and those too thin even for that, or whose conic is not safely positive
// definite, take the exact per-pixel path (see row_tier).
// Sums are formed in a fixed order (per lane in list order, then a fixed butterfly): the image is deterministic.
// When may a pixel row be walked with the recurrence?  The only hazard is an underflowed start: exp2(p0) = 0 for
// p0 < -126, and 0 stays 0 however large the ratios.  Along a row p(c) = -|A2| c^2 + beta c + p0 is a concave parabola
// that never exceeds 0 (positive definite conic), hence p(c) <= -(sqrt(-p0) - c sqrt|A2|)^2 (p = log2 G, without L).  The
// evaluated exponent p + L underflows for p0 < -(126 + L); with c <= 7 no later pixel of the row can then reach
// log2(alpha) >= log2(1e-5), i.e. p(c) >= log2(1e-5) - L, as long as
//     sqrt|A2| <= (sqrt(126 + L) - sqrt(L - log2(1e-5) + 1)) / 7
// (for opacity*mu = 0.01 that is |A2| <= 1.3, a conditional sigma of 0.75 px along x).  Gaussians beyond that, or
// without a finite culling box (conic not safely positive definite), are evaluated exactly, pixel by pixel.
constexpr int FWD_BATCH = 256;          // list entries staged per round: one per thread of the workgroup

// Two bodies: the 8-step row recurrence, and the exact per-pixel evaluation for entries the recurrence is not safe for (row_tier >= 1).
// (Rounds 1-5 had a third, the recurrence re-anchored at pixel 4 for row_tier == 1, compiled into a second kernel variant that the host
// chose when the previous call had seen a thin Gaussian -- and rendered AGAIN with when it had guessed wrong: 430 of 29 000 forwards of a
// bench run.  A choice made from a count over the call cannot be the same for a batch of views and for its single views, whose images
// must agree bit for bit.  Round 6: one variant; thin Gaussians -- a handful per view on the synthetic scene, none on the trained clouds
// -- take the exact path.  The backward keeps its re-anchored tier: there the choice follows the call's device-side flag.)
template <bool EXACT>
__device__ __forceinline__ void fwd_item(const float4 a, float C2, float L, float x0, float y0, float (&acc)[64])
{
    const float dx0 = a.x - x0;
    if (!EXACT) {
        const float k1 = a.z * (1.0f - 2.0f * dx0);            // log2 of alpha(1)/alpha(0), minus B2*dy
        const float rr = __builtin_amdgcn_exp2f(2.0f * a.z);   // second ratio, constant along the row
        // Round 6: a second recurrence ACROSS the rows (the voxelizer's, voxel_render.hip vfwd_item, round 4).  Until now every row
        // paid two v_exp_f32 (start value, first ratio) and the arithmetic of their arguments: 14 of a row's 54 issue slots.  The
        // row starts E(r) = log2 alpha(column 0, row r) are a parabola in r as well:
        //   rows 4..7: g(4) = 2^E(4), g(r+1) = g(r) rho(r), rho(r+1) = rho(r) kappa     rho(4) = 2^(E(5) - E(4))
        //   rows 3..0: g(3) = 2^E(3), g(r-1) = g(r) rho'(r), rho'(r-1) = rho'(r) kappa  rho'(3) = 2^(E(2) - E(3))
        //   first ratio along the row: rt(4) = 2^(k1 - B2 dy4), rt(r+1) = rt(r) chi, rt(r-1) = rt(r) / chi
        // with kappa = 2^(2 C2), chi = 2^B2: nine exponentials per entry instead of seventeen, three multiplications per row.  The
        // walks start in the middle of the block (three steps each way); item_exact (raster_state.hpp) keeps out the entries for
        // which three steps down a column and seven along a row could start from an underflowed value and climb above the cut-off.
        const float bdx = a.w * dx0, adl = dx0 * (a.z * dx0) + L;
        const float dy4 = a.y - (y0 + 4.0f), dy3 = a.y - (y0 + 3.0f);
        float gu = __builtin_amdgcn_exp2f(dy4 * (C2 * dy4 + bdx) + adl), gd = __builtin_amdgcn_exp2f(dy3 * (C2 * dy3 + bdx) + adl);
        float ru = __builtin_amdgcn_exp2f(fminf(C2 * (1.0f - 2.0f * dy4) - bdx, 100.0f));
        float rd = __builtin_amdgcn_exp2f(fminf(C2 * (1.0f + 2.0f * dy3) + bdx, 100.0f));
        const float kap = __builtin_amdgcn_exp2f(2.0f * C2);
        const float chi = __builtin_amdgcn_exp2f(a.w), chii = __builtin_amdgcn_exp2f(-a.w);
        float rtu = __builtin_amdgcn_exp2f(fminf(k1 - a.w * dy4, 120.0f));
        float rtd = rtu * chii;
        // power <= 0 holds: positive definite conic.  (The EXEC-mask form of the accumulation -- v_cmpx + add + s_mov exec, 2 VALU
        // instead of 3 -- gains 2.7 us in the backward, which is issue-bound; here it was measured twice, rounds 1 and 2: 1 us
        // SLOWER.  This kernel waits on latency, not on the VALU.)
#define R2_FWD_ROW(ROW, G0, RT0)                                                                \
        {                                                                                       \
            float g = (G0), rt = (RT0);                                                         \
            _Pragma("unroll") for (int c = 0; c < SUB2D; ++c) {                                 \
                acc[(ROW) * SUB2D + c] += (g >= ALPHA_MIN_2D) ? g : 0.f;                        \
                g *= rt;                                                                        \
                rt *= rr;                                                                       \
            }                                                                                   \
        }
#pragma unroll
        for (int j = 0; j < SUB2D / 2; ++j) {
            R2_FWD_ROW(SUB2D / 2 + j, gu, rtu)
            gu *= ru; ru *= kap; rtu *= chi;
            __builtin_amdgcn_sched_barrier(0);   // one row at a time: keeps the 64 accumulators + one row of temporaries live
        }
#pragma unroll
        for (int j = 0; j < SUB2D / 2; ++j) {
            R2_FWD_ROW(SUB2D / 2 - 1 - j, gd, rtd)
            gd *= rd; rd *= kap; rtd *= chii;
            __builtin_amdgcn_sched_barrier(0);
        }
#undef R2_FWD_ROW
        return;
    }
#pragma unroll
    for (int r = 0; r < SUB2D; ++r) {
        const float dy = a.y - (y0 + (float)r);
        const float bdy = a.w * dy;
        const float cdl = (C2 * dy) * dy + L;
#pragma unroll
        for (int c = 0; c < SUB2D; ++c) {
            const float dx = dx0 - (float)c;
            const float pl = dx * (a.z * dx + bdy) + cdl;     // log2(alpha)
            const float al = __builtin_amdgcn_exp2f(pl);
            // power <= 0 (RAS/forward.cu:369) <=> pl <= L ; alpha >= 1e-5 (RAS/forward.cu:374)
            const bool ok = (pl <= L) && (al >= ALPHA_MIN_2D);
            acc[r * SUB2D + c] += ok ? al : 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);   // one row at a time: keeps the 64 accumulators + one row of temporaries live
    }
}

// FUSED: the work item that is the LAST of its tile to finish adds the tile's partial images in list order and writes the
// image (and the backward's per-instance tile ids), instead of a separate combine launch; empty tiles are extra work items
// {tile, 0, 0, 0} that just write zeros.
template <bool FUSED, bool MV>
__global__ void __launch_bounds__(256, 4) raster_render_forward_kernel(
    const uint2 *__restrict__ ranges, const uint32_t *__restrict__ chunk_base, const uint4 *__restrict__ work_tile,
    uint32_t T, const uint32_t *__restrict__ point_list, const float4 *__restrict__ rec, int gx, int gy,
    float *__restrict__ partial, uint32_t *__restrict__ tile_done, float *__restrict__ out_color, int W, int H,
    uint32_t *__restrict__ tiles, char *tf_bin_base, const uint32_t *__restrict__ tf_words)
{
    const uint32_t w = blockIdx.x;
    R2_TS_AT(render, 0);
    // the descriptor is requested together with the count that says whether it exists (the list has a slot for every workgroup
    // of the grid): one round trip instead of two at the head of every workgroup's chain of dependent loads
    const uint4 wd = work_tile[w];   // {tile, first instance, one past the last, items of the tile}
    if (w >= chunk_base[FUSED ? T + 1 : T]) return;
    // tile-first forward: the binning buffer was carved with a PREDICTED instance count; the backward will carve it with the true
    // one, so the per-instance tile ids go where that carve puts them (raster_state.hpp)
    if (FUSED && tf_bin_base != nullptr) tiles = binning_tiles_ptr(tf_bin_base, (size_t)tf_words[DW_TOTAL]);
    const uint32_t tile = wd.x, beg = wd.y, end = wd.z;
    int tx, ty, tv;   // tile column / row inside its view, view (batched views stack their tile grids)
    tile_decode<MV>(tile, gx, gy, tx, ty, tv);
    out_color += (size_t)tv * H * W;   // this view's image
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (FUSED && wd.w == 0u) {   // empty tile
        const int px = tx * TILE2D + (tid & 15), py = ty * TILE2D + (tid >> 4);
        if (px < W && py < H) out_color[py * W + px] = 0.f;
        return;
    }
    const int bx = (wave & 1) * SUB2D, by = (wave >> 1) * SUB2D;             // this wave's block inside the tile
    const float x0 = (float)(tx * TILE2D + bx), y0 = (float)(ty * TILE2D + by);
    const unsigned long long lt_mask = (1ull << lane) - 1ull;

    // The workgroup stages FWD_BATCH list entries at a time in LDS (one entry per thread, the next batch's gathers are
    // already in flight while this one is evaluated); every wave then picks the entries that touch ITS block.
    __shared__ float4 sA[FWD_BATCH];          // {px, py, A2, B2}
    __shared__ float4 sB[FWD_BATCH];          // {C2, L, hx, hy}
    __shared__ uint16_t sQ[4][FWD_BATCH];     // per wave: indices of its live entries, in list order

    float acc[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) acc[i] = 0.f;

    float4 na, nb;   // prefetched entry of the NEXT batch
    {
        const uint32_t k = beg + (uint32_t)tid;
        const uint32_t id = point_list[k < end ? k : beg];
        na = rec[2 * id];
        nb = rec[2 * id + 1];
    }
    for (uint32_t base = beg; base < end; base += FWD_BATCH) {
        __syncthreads();                       // the previous batch has been consumed by all four waves
        sA[tid] = na;
        sB[tid] = nb;
        __syncthreads();
        if (base + FWD_BATCH < end) {          // start the next batch's gathers
            const uint32_t k = base + FWD_BATCH + (uint32_t)tid;
            const uint32_t id = point_list[k < end ? k : beg];
            na = rec[2 * id];
            nb = rec[2 * id + 1];
        }
        const int nbatch = (int)min((uint32_t)FWD_BATCH, end - base);
        // ---- this wave's live entries (ballot + prefix popcount keeps list order)
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < FWD_BATCH / 64; ++r) {
            const int e = r * 64 + lane;
            const float4 a = sA[e], b = sB[e];
            const bool keep = e < nbatch && block_live(a.x, a.y, b.z, b.w, x0, y0, (float)SUB2D);
            const unsigned long long m = __ballot(keep);
            if (keep) sQ[wave][cnt + __popcll(m & lt_mask)] = (uint16_t)e;
            cnt += __popcll(m);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // ---- 64 entries per step, one per lane
        for (int head = 0; head < cnt; head += 64) {
            float4 ea = make_float4(0.f, 0.f, 0.f, 0.f), eb = make_float4(0.f, -INFINITY, 0.f, 0.f);   // idle lane: alpha = 0
            if (head + lane < cnt) {
                const int e = sQ[wave][head + lane];
                ea = sA[e];
                eb = sB[e];
            }
            // recurrence path for the regular entries (flagged lanes contribute 0: L = -inf), then, only if the wave
            // holds any, the exact path for the flagged ones -- two in-place accumulations, no 64-register merge
            // tier 0 / 1: row recurrence over 8 pixels, or re-anchored at pixel 4 (thin Gaussians; only waves holding
            // such an entry pay for the two extra exps per row).  Tier 2 (exact) entries contribute 0
            // here (L = -inf) and are evaluated by a second in-place pass, only if the wave holds any.
            const int tier = (head + lane < cnt) ? item_tier(ea.z, ea.w, eb.x, eb.y, eb.z, eb.w) : 0;
            const bool exact = tier >= 1;   // (see fwd_item)
            const float4 ra = exact ? make_float4(0.f, 0.f, 0.f, 0.f) : ea;
            fwd_item<false>(ra, exact ? 0.f : eb.x, exact ? -INFINITY : eb.y, x0, y0, acc);
            if (__any(exact)) fwd_item<true>(ea, eb.x, exact ? eb.y : -INFINITY, x0, y0, acc);
        }
    }

    // 64x64 transpose-reduction: after the step with partner distance d, acc[0..d) hold partial sums of the d pixels
    // whose index agrees with this lane's bits >= d; after d = 1, acc[0] is the block's pixel number `lane`.
    // The two widest steps use gfx950's v_permlane32_swap / v_permlane16_swap: swapping the upper half (odd 16-lane rows)
    // of acc[i] with the lower half (even rows) of acc[d + i] leaves, in every lane, exactly the two addends that lane
    // keeps -- one instruction + one add per exchange instead of two selects, a ds_bpermute and an add.
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i]), __float_as_uint(acc[32 + i]), false, false);
        acc[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i]), __float_as_uint(acc[16 + i]), false, false);
        acc[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) {
        const bool up = (lane & d) != 0;
#pragma unroll
        for (int i = 0; i < d; ++i) {
            const float keep = up ? acc[d + i] : acc[i];
            const float send = up ? acc[i] : acc[d + i];
            acc[i] = keep + __shfl_xor(send, d);
        }
    }
    const int ly = by + (lane >> 3), lx = bx + (lane & 7);
    if (!FUSED) {
        partial[(size_t)w * 256 + (ly * TILE2D + lx)] = acc[0];
        return;
    }
    R2_TS_AT(render, 1);
    if (wd.w == 1u) {   // the tile's only work item: the image pixel itself
        const int px = tx * TILE2D + lx, py = ty * TILE2D + ly;
        if (px < W && py < H) out_color[py * W + px] = acc[0];
        if (tiles)
            for (uint32_t k = beg + (uint32_t)tid; k < end; k += 256u) tiles[k] = tile;
        return;
    }
    // The partial image travels between workgroups on different XCDs (non-coherent L2s).  A release/acquire fence pair
    // would do it, but at agent scope a release is a write-back of the XCD's whole L2 (buffer_wbl2) -- measured: the
    // kernel went from 42 to 370 us.  Instead the partials themselves are written and read with agent-scope (sc1) atomic
    // stores / loads, which go past the L2s; a store that has been acknowledged (vmcnt) is visible device-wide, so the
    // arrival counter needs no fence.
    __hip_atomic_store(&partial[(size_t)w * 256 + (ly * TILE2D + lx)], acc[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ uint32_t s_arrived;
    if (tid == 0) s_arrived = atomicAdd(&tile_done[tile], 1u);
    __syncthreads();
    if (s_arrived != wd.w - 1u) return;
    const uint32_t w0 = chunk_base[tile];
    float C = 0.f;
    for (uint32_t i = 0; i < wd.w; ++i)   // list order: deterministic image
        C += __hip_atomic_load(&partial[(size_t)(w0 + i) * 256 + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int px = tx * TILE2D + (tid & 15), py = ty * TILE2D + (tid >> 4);
    if (px < W && py < H) out_color[py * W + px] = C;
    if (tiles) {
        const uint2 rg = ranges[tile];
        for (uint32_t k = rg.x + (uint32_t)tid; k < rg.y; k += 256u) tiles[k] = tile;
    }
}

// (Measured and left out, round 4: the voxelizer's carry rows -- a batch's remainder of < 64 live entries opens the next batch's first
// step instead of being flushed as a partly filled one.  Parity green, 47.4 us either way: this kernel waits on the staging
// round trips, not on the number of steps; the voxelizer's forward, which is VALU-bound, gained 12 % from the same change.)
// (Measured and left out, round 3 -- VERDICT r2's suggestion: the same lane-per-entry scheme on HALF blocks, 8 pixels wide x 4 rows,
// 32 accumulators per lane, eight waves per workgroup, the 2-exp-per-8-pixel row recurrence kept.  Parity green.  The compiler
// needs 87-99 VGPRs for it, not ~64: 81 us at 4 waves/SIMD, 56 at 5, 52 at 6 (16 B/lane of scratch), 60 at 7, 56 at 8 (56 B of
// scratch) against 47.7 us for this kernel -- twice the (entry, block) items to compact, stage and transpose-reduce cost more than
// the finer culling and the extra waves return.)
// ---- forward, round 6: ONE-WAVE work items that gather for themselves (VERDICT r5 #2a).
// Work item = (<= FWD_CHUNK consecutive instances of one tile list) x (one 8x8 block) = one wave = one workgroup.  What the
// four-wave kernel above spends its life on, measured in round 3 (46 % of a wave's life parked at s_waitcnt, VALU issue 0.40):
// every 256-entry batch is a chain descriptor -> ids -> records -> LDS -> barrier -> four rounds of block tests -> steps, with the
// next batch's ids requested only when this batch starts, and the four waves of a tile wait for each other twice per batch.
// Here the instance list carries every entry's block mask (RasterBinning::masked, written where the list is made), so a wave
//   1. requests ALL masked ids of its chunk at once (8 coalesced loads in flight, one round trip),
//   2. compacts the ids whose mask holds its block into an LDS queue (ballot + rank: no record is gathered to be tested, dead
//      instances -- 16-19 % of a list cannot reach their tile at all -- cost one bit test),
//   3. walks the queue 64 entries per step, lane = entry as above, with the NEXT step's records (two 16-byte gathers per lane)
//      in flight while this step computes.
// No workgroup barrier, no record staging, three dependent round trips per work item whatever its length; a wave whose block is
// empty leaves at once instead of idling at its siblings' barriers.  The arithmetic (fwd_item, the transposes, the combine of a
// tile's partial sums in list order by the last arriver) is the kernel's above; the lanes that hold an entry differ (compaction over the
// whole chunk instead of per 256-entry batch), so the two kernels' images agree to float association, not bit for bit.
// blockIdx -> (work item, block): the four blocks of an item run on ONE XCD (block b of the grid runs on XCD b % 8), so its
// records are pulled into one L2.
constexpr int FWD_WAVE_OCC = 4;   // waves per SIMD the kernel is compiled for
template <bool MV>
__global__ void __launch_bounds__(64, FWD_WAVE_OCC) raster_render_forward_wave_kernel(
    const uint2 *__restrict__ ranges, const uint32_t *__restrict__ chunk_base, const uint4 *__restrict__ work_tile, uint32_t T, uint32_t NW,
    const uint32_t *__restrict__ masked, const float4 *__restrict__ rec, int gx, int gy, float *__restrict__ partial,
    uint32_t *__restrict__ tile_done, float *__restrict__ out_color, int W, int H, uint32_t *__restrict__ tiles, char *tf_bin_base,
    const uint32_t *__restrict__ tf_words)
{
    __shared__ uint32_t sQ[FWD_CHUNK];   // ids of the chunk's entries that are live for this block, in list order
    const uint32_t bi = blockIdx.x;
    const uint32_t w = (bi >> 5) * 8u + (bi & 7u);
    const int blk = (int)((bi >> 3) & 3u);
    const int lane = threadIdx.x;
    R2_TS_AT8(render, 4);
    const uint4 wd = work_tile[min(w, NW - 1u)];   // {tile, first instance, one past the last, items of the tile}
    if (w >= chunk_base[T + 1]) return;
    if (tf_bin_base != nullptr) {   // tile-first forward: the binning buffer was carved with a PREDICTED instance count (raster_state.hpp)
        const size_t Rt = (size_t)tf_words[DW_TOTAL];
        tiles = binning_tiles_ptr(tf_bin_base, Rt);
        masked = binning_masked_ptr(tf_bin_base, Rt);
    }
    const uint32_t tile = wd.x, beg = wd.y, end = wd.z;
    R2_TS_AT8(render, 5);   // the descriptor is here
    int tx, ty, tv;
    tile_decode<MV>(tile, gx, gy, tx, ty, tv);
    out_color += (size_t)tv * H * W;
    const int bx = (blk & 1) * SUB2D, by = (blk >> 1) * SUB2D;
    const int px = tx * TILE2D + bx + (lane & 7), py = ty * TILE2D + by + (lane >> 3);
    const bool inside = px < W && py < H;
    if (wd.w == 0u) {   // empty tile
        if (inside) out_color[py * W + px] = 0.f;
        return;
    }
    const float x0 = (float)(tx * TILE2D + bx), y0 = (float)(ty * TILE2D + by);
    // where this item's partial sums go: the work list is ordered longest first (WorkListOut::longest_first), the index space of
    // a tile's partial sums is the tile-order one -- chunk_base[tile] + the chunk's number inside the tile (requested now, used last)
    const uint32_t tile_beg = ranges[tile].x, w0 = chunk_base[tile];
    // the backward's per-instance tile ids
    if (tiles != nullptr && blk == 0)
        for (uint32_t k = beg + (uint32_t)lane; k < end; k += 64u) tiles[k] = tile;

    // ---- 1. the chunk's masked ids, branch-free (clamped addresses): one round trip for all of them
    constexpr int NR = (int)FWD_CHUNK / 64;
    const uint32_t n = end - beg;
    uint32_t v[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) v[r] = masked[beg + min((uint32_t)(r * 64 + lane), n - 1u)];
    // ---- 2. this block's live entries, in list order
    int cnt = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const bool keep = (uint32_t)(r * 64 + lane) < n && ((v[r] >> blk) & 1u) != 0u;
        const unsigned long long m = __ballot(keep);
        if (keep) sQ[cnt + (int)ballot_rank(m)] = v[r] >> MASK_BITS;
        cnt += __popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    R2_TS_AT8(render, 6);   // the ids are here and compacted

    float acc[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) acc[i] = 0.f;
    // ---- 3. 64 entries per step, one per lane; the next step's records are gathered while this one computes (the clamp makes the
    // last step gather an entry it does not use: cheaper than a branch around the loads, which would drain the queue)
    float4 na = make_float4(0.f, 0.f, 0.f, 0.f), nb = na;
    if (cnt > 0) {
        const uint32_t id = sQ[min(lane, cnt - 1)];
        na = rec[2 * id];
        nb = rec[2 * id + 1];
    }
    for (int head = 0; head < cnt; head += 64) {
        float4 ea = na, eb = nb;
        {
            const uint32_t id = sQ[min(head + 64 + lane, cnt - 1)];
            na = rec[2 * id];
            nb = rec[2 * id + 1];
        }
        const bool live = head + lane < cnt;
        if (!live) { ea = make_float4(0.f, 0.f, 0.f, 0.f); eb = make_float4(0.f, -INFINITY, 0.f, 0.f); }   // idle lane: alpha = 0
        const int tier = live ? item_tier(ea.z, ea.w, eb.x, eb.y, eb.z, eb.w) : 0;
        const bool exact = tier >= 1;   // (an entry the recurrences are not safe for: the exact path, see fwd_item)
        const float4 ra = exact ? make_float4(0.f, 0.f, 0.f, 0.f) : ea;
        fwd_item<false>(ra, exact ? 0.f : eb.x, exact ? -INFINITY : eb.y, x0, y0, acc);
        if (__any(exact)) fwd_item<true>(ea, eb.x, exact ? eb.y : -INFINITY, x0, y0, acc);
    }

    // 64x64 transpose-reduction (see the kernel above)
    if (cnt > 0) {
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i]), __float_as_uint(acc[32 + i]), false, false);
            acc[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i]), __float_as_uint(acc[16 + i]), false, false);
            acc[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        }
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) {
            const bool up = (lane & d) != 0;
#pragma unroll
            for (int i = 0; i < d; ++i) {
                const float keep = up ? acc[d + i] : acc[i];
                const float send = up ? acc[i] : acc[d + i];
                acc[i] = keep + __shfl_xor(send, d);
            }
        }
    }
    R2_TS_AT8(render, 7);   // steps + transposes done
    if (wd.w == 1u) {   // the tile's only work item: the image pixel itself
        if (inside) out_color[py * W + px] = acc[0];
        return;
    }
    // partial sums cross XCDs: agent-scope (sc1) stores / loads, the arrival counter bumped after they are acknowledged (see above)
    const uint32_t slot = w0 + (beg - tile_beg) / FWD_CHUNK;
    __hip_atomic_store(&partial[((size_t)slot * 4 + (size_t)blk) * 64 + (size_t)lane], acc[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t arrived = 0u;
    if (lane == 0) arrived = atomicAdd(&tile_done[tile * 4u + (uint32_t)blk], 1u);
    arrived = (uint32_t)__builtin_amdgcn_readfirstlane((int)arrived);
    R2_TS_AT8(render, 8);   // partial stored, arrival counted
    if (arrived != wd.w - 1u) return;
    float C = 0.f;
    for (uint32_t i = 0; i < wd.w; ++i)   // list order: deterministic image
        C += __hip_atomic_load(&partial[((size_t)(w0 + i) * 4 + (size_t)blk) * 64 + (size_t)lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (inside) out_color[py * W + px] = C;
}

// the masked list for chains whose sort does not carry the masks (the general chain: first call of a size, batched views):
// one workgroup per forward work item, one gather of the record's box per instance
template <bool MV>
__global__ void __launch_bounds__(256) raster_mask_fill_kernel(
    const uint32_t *__restrict__ chunk_base, const uint4 *__restrict__ work_tile, uint32_t T, const uint32_t *__restrict__ point_list,
    const float4 *__restrict__ rec, int gx, int gy, uint32_t *__restrict__ masked)
{
    const uint32_t w = blockIdx.x;
    const uint4 wd = work_tile[w];
    if (w >= chunk_base[T]) return;   // (the empty tiles' items lie behind the real ones)
    int tx, ty, tv;
    tile_decode<MV>(wd.x, gx, gy, tx, ty, tv);
    for (uint32_t k = wd.y + threadIdx.x; k < wd.z; k += 256u) {
        const uint32_t id = point_list[k];
        const float4 a = rec[2 * id], b = rec[2 * id + 1];
        masked[k] = (id << MASK_BITS) | block_mask4(a.x, a.y, b.z, b.w, tx, ty);
    }
}

// Debug-mode kernel (pixel-parallel): also tracks n_contrib (RAS/forward.cu:381,391), which only `debug` callers read
// back.  One lane per pixel, the wave's live entries are compacted per 256-entry batch and broadcast from LDS.
template <bool MV>
__global__ void __launch_bounds__(256) raster_render_forward_debug_kernel(
    const uint2 *__restrict__ ranges, const uint32_t *__restrict__ chunk_base, const uint4 *__restrict__ work_tile,
    uint32_t T, const uint32_t *__restrict__ point_list, const float4 *__restrict__ rec, int gx, int gy,
    float *__restrict__ partial, uint32_t *__restrict__ partial_last)
{
    const uint32_t w = blockIdx.x;
    if (w >= chunk_base[T]) return;
    const uint4 wd = work_tile[w];
    const uint32_t tile = wd.x, beg = wd.y, end = wd.z;
    const uint2 range = ranges[tile];
    int tx, ty, tv;
    tile_decode<MV>(tile, gx, gy, tx, ty, tv);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bx = (wave & 1) * SUB2D, by = (wave >> 1) * SUB2D;
    const int lx = bx + (lane & 7), ly = by + (lane >> 3);
    const float x0 = (float)(tx * TILE2D + bx), y0 = (float)(ty * TILE2D + by);
    const float fx = (float)(tx * TILE2D + lx), fy = (float)(ty * TILE2D + ly);
    const unsigned long long lt_mask = (1ull << lane) - 1ull;

    __shared__ float4 sA[4][256];
    __shared__ float2 sB[4][256];
    __shared__ uint32_t sK[4][256];   // 1-based list position of the kept entry
    float4 *const mA = sA[wave];
    float2 *const mB = sB[wave];

    float C = 0.f;
    uint32_t last = 0;
    for (uint32_t base = beg; base < end; base += 256) {
        float4 a[4], b[4];
        bool live[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t k = base + (uint32_t)(r * 64 + lane);
            live[r] = k < end;
            const uint32_t id = live[r] ? point_list[k] : point_list[beg];
            a[r] = rec[2 * id];
            b[r] = rec[2 * id + 1];
        }
        __builtin_amdgcn_wave_barrier();
        int n = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool keep = live[r] && block_live(a[r].x, a[r].y, b[r].z, b[r].w, x0, y0, (float)SUB2D);
            const unsigned long long m = __ballot(keep);
            if (keep) {
                const int pos = n + __popcll(m & lt_mask);
                mA[pos] = a[r];
                mB[pos] = make_float2(b[r].x, b[r].y);
                sK[wave][pos] = (base - range.x) + (uint32_t)(r * 64 + lane) + 1u;
            }
            n += __popcll(m);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int j = 0; j < n; ++j) {
            const float4 ra = mA[j];
            const float2 rb = mB[j];
            const float dx = ra.x - fx, dy = ra.y - fy;
            const float pl = dx * (ra.z * dx + ra.w * dy) + ((rb.x * dy) * dy + rb.y);
            const float alpha = __builtin_amdgcn_exp2f(pl);
            const bool ok = (pl <= rb.y) && (alpha >= ALPHA_MIN_2D);
            C += ok ? alpha : 0.f;
            last = ok ? sK[wave][j] : last;
        }
    }
    partial[(size_t)w * 256 + (ly * TILE2D + lx)] = C;
    partial_last[(size_t)w * 256 + (ly * TILE2D + lx)] = last;
}

// adds the partial sums of a tile's work items in list order and writes the image (zeros for empty tiles)
template <bool NCONTRIB, bool MV>
__global__ void __launch_bounds__(256) raster_combine_kernel(
    const uint32_t *__restrict__ chunk_base, const float *__restrict__ partial,
    const uint32_t *__restrict__ partial_last, int W, int H, int gx, int gy, float *__restrict__ out_color,
    uint32_t *__restrict__ n_contrib, const uint2 *__restrict__ ranges, uint32_t *__restrict__ tiles)
{
    const uint32_t tile = blockIdx.x;
    if (tiles) {   // tile id of every sorted instance, for the backward (the single-pass sort does not scatter its keys)
        const uint2 rg = ranges[tile];
        for (uint32_t k = rg.x + threadIdx.x; k < rg.y; k += 256) tiles[k] = tile;
    }
    int tx, ty, tv;
    tile_decode<MV>(tile, gx, gy, tx, ty, tv);
    out_color += (size_t)tv * H * W;
    if (NCONTRIB) n_contrib += (size_t)tv * H * W;
    const int tid = threadIdx.x;
    const int px = tx * TILE2D + (tid & 15), py = ty * TILE2D + (tid >> 4);
    const uint32_t w0 = chunk_base[tile], w1 = chunk_base[tile + 1];
    float C = 0.f;
    uint32_t last = 0;
    for (uint32_t w = w0; w < w1; ++w) {
        C += partial[(size_t)w * 256 + tid];
        if (NCONTRIB) {
            const uint32_t l = partial_last[(size_t)w * 256 + tid];
            last = l ? l : last;
        }
    }
    if (px < W && py < H) {
        out_color[py * W + px] = C;
        if (NCONTRIB) n_contrib[py * W + px] = last;
    }
}

// ------------------------------------------------------------------------------------------------ backward
// One LANE owns one work ITEM = one 8x8 pixel block of one (tile, Gaussian) instance of the sorted list; only
// blocks that the Gaussian's alpha >= 1e-5 bounding box touches become items (46 % on the benchmark scene).
// A wave takes 64 consecutive instances, expands them into items through a small LDS queue (wave prefix sum of
// the per-instance block counts), processes the queue 64 items at a time, and each instance then adds up the
// moment rows of its own items in a fixed order -- still no atomics, still bit-reproducible.
// dL/dpix of the tiles a wave touches is staged in LDS, three tiles per pass (97 % of the waves touch one tile).  An
// earlier version sent waves with more than three tiles through a per-lane whole-tile gather: only 0.3 % of the waves,
// but each ran for ~25 us, and they belong to the sparse tiles at the END of the list -- a third of the kernel's time
// was that tail (74 -> 50 us).
constexpr int GT_STRIDE = 20;                       // floats per staged tile row (16 + pad: the two block rows of a
constexpr int GT_TILE = TILE2D * GT_STRIDE + 4;     // tile and the tile slots land on different LDS banks)
constexpr int MAX_WAVE_TILES = 3;
// One wave per workgroup: the waves never synchronise with each other, and a wave that finishes early (few live blocks)
// frees its slot and its 8 KB of LDS at once instead of waiting for its three siblings (-3 % kernel time).  Walking the
// chunks with a grid-stride loop from a few resident workgroups per CU was measured too: no gain.
constexpr int BWD_WAVES = 1, BWD_THREADS = 64 * BWD_WAVES;
constexpr int BWD_OCC = 4;   // waves per SIMD the kernel is compiled for (121 VGPRs with the pipeline registers)

__device__ __forceinline__ void pixel_moments(float A2, float lthr, float dx, float bdy, float cdy2, float g, float &r0,
                                              float &r1, float &r3)
{
    const float p2 = dx * (A2 * dx + bdy) + cdy2;   // log2(e) * power
    const float G = __builtin_amdgcn_exp2f(p2);
    // power <= 0 and alpha >= 1e-5 (<=> p2 >= log2(1e-5) - L), RAS/backward.cu:536-543
    const bool ok = (p2 <= 0.0f) && (p2 >= lthr);
    const float w = ok ? G * g : 0.f;
    const float wdx = w * dx;
    r0 += w;
    r1 += wdx;
    r3 += wdx * dx;
}

// moments of w = G * dL/dpix over an n x n pixel block whose dL/dpix rows sit in LDS at gt (row stride GT_STRIDE).
// EXACT = false walks each row with the recurrence G(c+1) = G(c) r(c), r(c+1) = r(c) exp2(2 A2) (see the forward
// kernel): two v_exp_f32 per row instead of one per pixel.
template <int N, bool EXACT>
__device__ __forceinline__ void block_moments_lds(const float4 a, const float4 b, const float *__restrict__ gt,
                                                  float bx0, float by0, float *S)
{
    const float dx0 = a.x - bx0;
    const float lthr = LOG2_ALPHA_MIN_2D - b.y;                         // alpha >= 1e-5 <=> log2 G >= lthr
    const float gthr = EXACT ? 0.f : __builtin_amdgcn_exp2f(lthr);
    const float k1 = a.z * (1.0f - 2.0f * dx0);
    const float rr = EXACT ? 0.f : __builtin_amdgcn_exp2f(2.0f * a.z);
    // column moments t_k = sum_c (c - mid)^k w_c about the block's centre column (the (c - mid)^k are literals: one
    // FMA each), turned into moments of dx = (dx0 - mid) - (c - mid) once per row; centring halves |dx0 - mid| and
    // with it the cancellation in r3
    constexpr float mid = 0.5f * (float)(N - 1);
    const float dm = dx0 - mid;
#ifndef R2_EXP_NO_CMPX
    static_assert(N == 8, "the pixel macro below is written for 8-pixel rows");
    // the EXEC save / restore below is written for wave64 on gfx9-family ISA (64-bit exec, v_cmpx writing EXEC); the
    // plain-C++ body under R2_EXP_NO_CMPX is the portable statement of the same arithmetic (tests build and compare it)
#if defined(__AMDGCN_WAVEFRONT_SIZE) && __AMDGCN_WAVEFRONT_SIZE != 64
#error "the inline asm below assumes a 64-lane EXEC mask (wave64)"
#endif
    const unsigned long long full_exec = __builtin_amdgcn_read_exec();   // this function runs inside divergent code
    (void)full_exec;
#endif
    float U[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };   // sums over the rows of t0, t1, t2, dy t0, dy t1, dy^2 t0
    // one row of the block with the row recurrence: G = alpha / amplitude at column 0, rt = its first ratio
    auto recur_row = [&](int r, float G, float rt) {
        const float dy = a.y - (by0 + (float)r);
        float g[N];
#pragma unroll
        for (int c4 = 0; c4 < N / 4; ++c4) {
            const float4 v = *reinterpret_cast<const float4 *>(gt + r * GT_STRIDE + 4 * c4);
            g[4 * c4 + 0] = v.x; g[4 * c4 + 1] = v.y; g[4 * c4 + 2] = v.z; g[4 * c4 + 3] = v.w;
        }
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#ifndef R2_EXP_NO_CMPX
        // power <= 0 holds for a positive definite conic; the cut-off is applied as an EXEC mask: v_cmpx narrows EXEC
        // to the lanes whose pixel passes, the product and the three moment updates run under it (a masked lane keeps
        // its sums: the same as adding 0), s_mov restores EXEC on the scalar unit -- 5 VALU instead of the 6 of compare +
        // select + multiply + 3 updates (this kernel is VALU-issue-bound).  (c - mid)^k enter as literal operands.
#define R2_BWD_K(x) "n"(__builtin_bit_cast(int, (float)(x)))   /* literals: SGPR operands measured 1 us slower */
#define R2_BWD_PX(c)                                                                                                      \
        {                                                                                                                 \
            float w;                                                                                                      \
            asm volatile("v_cmpx_le_f32_e32 %[thr], %[G]\n\t"                                                             \
                         "v_mul_f32_e32 %[w], %[G], %[g]\n\t"                                                             \
                         "v_add_f32_e32 %[t0], %[t0], %[w]\n\t"                                                           \
                         "v_fmac_f32_e32 %[t1], %[k1], %[w]\n\t"                                                          \
                         "v_fmac_f32_e32 %[t2], %[k2], %[w]\n\t"                                                          \
                         "s_mov_b64 exec, %[ex]"                                                                          \
                         : [t0] "+v"(t0), [t1] "+v"(t1), [t2] "+v"(t2), [w] "=&v"(w)                                      \
                         : [thr] "v"(gthr), [G] "v"(G), [g] "v"(g[c]), [k1] R2_BWD_K((float)(c) - mid),                   \
                           [k2] R2_BWD_K(((float)(c) - mid) * ((float)(c) - mid)), [ex] "s"(full_exec)                      \
                         : "vcc");                                                                                        \
            G *= rt;                                                                                                      \
            rt *= rr;                                                                                                     \
        }
        R2_BWD_PX(0) R2_BWD_PX(1) R2_BWD_PX(2) R2_BWD_PX(3) R2_BWD_PX(4) R2_BWD_PX(5) R2_BWD_PX(6) R2_BWD_PX(7)
#undef R2_BWD_PX
#undef R2_BWD_K
#else
#pragma unroll
        for (int c = 0; c < N; ++c) {
            const float w = (G >= gthr) ? G * g[c] : 0.f;   // power <= 0 holds for a positive definite conic
            t0 += w;
            t1 = fmaf(w, (float)c - mid, t1);
            t2 = fmaf(w, ((float)c - mid) * ((float)c - mid), t2);
            G *= rt;
            rt *= rr;
        }
#endif
        // the rows' column moments are summed as they are (with the row's dy where the moment wants it) and turned into moments of
        // dx ONCE per item, below: seven instructions per row instead of twelve
        U[0] += t0; U[1] += t1; U[2] += t2;
        U[3] = fmaf(dy, t0, U[3]); U[4] = fmaf(dy, t1, U[4]); U[5] = fmaf(dy * dy, t0, U[5]);
    };
    if (!EXACT) {
        // Round 6: the row starts by a recurrence across the rows, as in the forward (fwd_item has the derivation; G carries
        // no amplitude here, the cut-off is gthr): nine exponentials per item instead of eighteen, three multiplications per row
        // instead of two exponentials and their arguments.  item_tier keeps out the entries the walks are not safe for.
        const float bdx = a.w * dx0, adx = dx0 * (a.z * dx0);
        const float dy4 = a.y - (by0 + (float)(N / 2)), dy3 = dy4 + 1.0f;
        float gu = __builtin_amdgcn_exp2f(dy4 * (b.x * dy4 + bdx) + adx), gd = __builtin_amdgcn_exp2f(dy3 * (b.x * dy3 + bdx) + adx);
        float ru = __builtin_amdgcn_exp2f(fminf(b.x * (1.0f - 2.0f * dy4) - bdx, 100.0f));
        float rd = __builtin_amdgcn_exp2f(fminf(b.x * (1.0f + 2.0f * dy3) + bdx, 100.0f));
        const float kap = __builtin_amdgcn_exp2f(2.0f * b.x);
        const float chi = __builtin_amdgcn_exp2f(a.w), chii = __builtin_amdgcn_exp2f(-a.w);
        float rtu = __builtin_amdgcn_exp2f(fminf(k1 - a.w * dy4, 120.0f));
        float rtd = rtu * chii;
        // (all four rows unrolled: with `unroll 2` -- what the loop over eight rows used until the row recurrence -- the loop-carried
        // recurrence state and the row's LDS address sat in the way of the scheduler: 53.9 -> 51.9 us, 137 -> 130 on the 331k cloud)
#pragma unroll
        for (int j = 0; j < N / 2; ++j) {
            recur_row(N / 2 + j, gu, rtu);
            gu *= ru; ru *= kap; rtu *= chi;
        }
#pragma unroll
        for (int j = 0; j < N / 2; ++j) {
            recur_row(N / 2 - 1 - j, gd, rtd);
            gd *= rd; rd *= kap; rtd *= chii;
        }
        S[0] += U[0]; S[1] += dm * U[0] - U[1]; S[3] += dm * (dm * U[0] - 2.0f * U[1]) + U[2];
        S[2] += U[3]; S[4] += dm * U[3] - U[4]; S[5] += U[5];
        return;
    }
#pragma unroll 2
    for (int r = 0; r < N; ++r) {
        const float dy = a.y - (by0 + (float)r);
        const float bdy = a.w * dy;           // B2*dy
        const float cdy2 = (b.x * dy) * dy;   // C2*dy^2
        float g[N];
#pragma unroll
        for (int c4 = 0; c4 < N / 4; ++c4) {
            const float4 v = *reinterpret_cast<const float4 *>(gt + r * GT_STRIDE + 4 * c4);
            g[4 * c4 + 0] = v.x; g[4 * c4 + 1] = v.y; g[4 * c4 + 2] = v.z; g[4 * c4 + 3] = v.w;
        }
        float r0 = 0.f, r1 = 0.f, r3 = 0.f;
#pragma unroll
        for (int c = 0; c < N; ++c) pixel_moments(a.z, lthr, dx0 - (float)c, bdy, cdy2, g[c], r0, r1, r3);
        S[0] += r0; S[1] += r1; S[3] += r3;
        S[2] += dy * r0; S[4] += dy * r1; S[5] += dy * dy * r0;
    }
}

template <bool MV>
__global__ void __launch_bounds__(BWD_THREADS, BWD_OCC) raster_render_backward_kernel(
    const uint32_t *__restrict__ tiles, const uint32_t *__restrict__ point_list, const uint32_t *__restrict__ first,
    const int *__restrict__ radii, const float4 *__restrict__ rec, uint32_t R, int W, int H, int gx, int gy,
    uint32_t nchunks, const float *__restrict__ dL_dpix, float4 *__restrict__ part, const uint32_t *__restrict__ thin_flag,
    const uint32_t *__restrict__ masked /* round 6: point_list << MASK_BITS | block mask (replaces point_list and the four
                                           block tests per instance), or null */)
{
    constexpr int NB = TILE2D / SUB2D;        // blocks per tile side (2)
    constexpr int NBLK = NB * NB;             // blocks per tile (4)
    __shared__ float s_gt[BWD_WAVES][MAX_WAVE_TILES * GT_TILE];   // dL/dpix of the wave's tiles
    __shared__ float4 s_pa[BWD_WAVES][64], s_pb[BWD_WAVES][64];           // the wave's 64 instance records
    __shared__ uint16_t s_q[BWD_WAVES][64 * NBLK];                // item queue: (owner lane << 4) | (tile slot << 2) | block
    __shared__ float4 s_r0[BWD_WAVES][64];                        // moment rows of the current round of 64 items
    __shared__ float2 s_r1[BWD_WAVES][64];
    (void)thin_flag;   // (rounds 1-5: selected the re-anchoring variant of the step; the count is still reported to the host)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *const gt = s_gt[wave];

    // ---- software pipeline over this wave's chunks (64 consecutive instances each, grid-stride).  A chunk needs two
    // dependent rounds of loads before it can compute: (1) tile + Gaussian id of its instances, (2) the gathers those ids
    // address (32-byte record, radius, first-instance index) and dL/dpix of its tiles.  With one chunk per wave those
    // round trips were ~60 % of the wave's life and the occupancy (5 waves/SIMD) could not cover them.  Here round (1) of
    // chunk i+2 and round (2) of chunk i+1 are in flight while chunk i computes; the loads are issued in the order in
    // which they are consumed, because vmcnt retires in order.
    const uint32_t nslots = ((nchunks + 7u) >> 3) << 3;
    const uint32_t G = gridDim.x;
    // All pipeline loads are BRANCH-FREE (clamped addresses; dead lanes carry valid-but-unused data and are masked where
    // the data is consumed): hipcc only emits counted s_waitcnt vmcnt(N) for loads in straight-line code -- behind a
    // per-lane branch it falls back to vmcnt(0), which would drain the whole pipeline at the first use.
    auto load1 = [&](uint32_t v, uint32_t &tile, uint32_t &id, bool &live) {
        const uint32_t chunk = v < nslots ? xcd_remap(v, nchunks) : nchunks;
        const uint32_t k = chunk * 64u + (uint32_t)lane;
        live = chunk < nchunks && k < R;
        const uint32_t kc = min(k, R - 1u);
        tile = tiles[kc];
        id = masked != nullptr ? masked[kc] : point_list[kc];   // (kernel-uniform; with the masks: id << MASK_BITS | mask)
    };
    auto load2 = [&](uint32_t idm, float4 &a, float4 &b, int &rad, uint32_t &first_row) {
        const uint32_t id = masked != nullptr ? idm >> MASK_BITS : idm;
        a = rec[2 * id];
        b = rec[2 * id + 1];
        rad = radii[id];          // only needed for the final store's address
        first_row = first[id];
    };
    // dL/dpix of one tile: lane -> (row = lane/4, 4 columns), zero outside the image
    const bool aligned = (W & 15) == 0;   // kernel-uniform: every tile column lies inside the image
    auto load_tile = [&](uint32_t t) -> float4 {
        int ttx, tty, ttv;
        tile_decode<MV>(t, gx, gy, ttx, tty, ttv);
        const int tx0 = ttx * TILE2D, ty0 = tty * TILE2D;
        const int ry = ty0 + (lane >> 2), cx = tx0 + (lane & 3) * 4;
        const float *__restrict__ img = dL_dpix + (size_t)ttv * H * W;   // this view's upstream gradient
        if (aligned)   // rows below the image are clamped here and zeroed by tile_row_ok() when the data is used
            return *reinterpret_cast<const float4 *>(img + (size_t)min(ry, H - 1) * W + cx);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ry < H) {
            const float *__restrict__ src = img + (size_t)ry * W + cx;
            if (cx + 0 < W) v.x = src[0];
            if (cx + 1 < W) v.y = src[1];
            if (cx + 2 < W) v.z = src[2];
            if (cx + 3 < W) v.w = src[3];
        }
        return v;
    };
    auto tile_row_ok = [&](uint32_t t) -> bool {
        const uint32_t tyt = t / (uint32_t)gx;
        return (int)(MV ? tyt % (uint32_t)gy : tyt) * TILE2D + (lane >> 2) < H;
    };

    uint32_t tile, id, tile1, id1;
    bool live, live1;
    float4 a, b;
    int rad;
    uint32_t first_row;
    R2_TS_AT(render, 2);
    load1(blockIdx.x, tile, id, live);
    load1(blockIdx.x + G, tile1, id1, live1);
    load2(id, a, b, rad, first_row);

    for (uint32_t v = blockIdx.x; v < nslots; v += G) {
    // distinct tiles in this chunk (the list is tile-sorted: count the run starts)
    const uint32_t prev_tile = __shfl_up(tile, 1);
    const unsigned long long heads = __ballot(live && (lane == 0 || tile != prev_tile));
    const int ntiles = __popcll(heads);
    const int my_slot = __popcll(heads & ((2ull << lane) - 1ull)) - 1;   // rank of this lane's tile among the heads
    unsigned long long hh = heads;
    // (a) dL/dpix of the first pass's tiles, into registers
    float4 stage[MAX_WAVE_TILES];
    uint32_t stage_tile[MAX_WAVE_TILES];
#pragma unroll
    for (int slot = 0; slot < MAX_WAVE_TILES; ++slot) {
        stage[slot] = make_float4(0.f, 0.f, 0.f, 0.f);
        stage_tile[slot] = 0u;
        if (slot < ntiles) {   // wave-uniform
            const int leader = __ffsll((long long)hh) - 1;
            hh &= hh - 1;
            stage_tile[slot] = __builtin_amdgcn_readfirstlane(__shfl(tile, leader));
            stage[slot] = load_tile(stage_tile[slot]);
        }
    }
    // (b) round (1) of the chunk after next, (c) round (2) of the next chunk
    uint32_t tile2, id2;
    bool live2;
    float4 a1, b1;
    int rad1;
    uint32_t first_row1;
    load1(v + 2u * G, tile2, id2, live2);
    load2(id1, a1, b1, rad1, first_row1);

    float S[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    // The chunk's tiles are handled MAX_WAVE_TILES at a time (nearly always one pass: 97 % of the waves sit inside a
    // single tile list; waves over sparse border tiles, with up to 64 different tiles, take several cheap passes).
    for (int slot0 = 0; slot0 < ntiles; slot0 += MAX_WAVE_TILES) {
        const int npass = min(MAX_WAVE_TILES, ntiles - slot0);
        const bool mine = live && my_slot >= slot0 && my_slot < slot0 + npass;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();   // the previous pass / chunk is done with the LDS buffers
        // ---- stage dL/dpix of this pass's tiles
        if (slot0 == 0) {
#pragma unroll
            for (int slot = 0; slot < MAX_WAVE_TILES; ++slot)
                if (slot < npass) {
                    const float4 tv = (!aligned || tile_row_ok(stage_tile[slot])) ? stage[slot] : make_float4(0.f, 0.f, 0.f, 0.f);
                    *reinterpret_cast<float4 *>(gt + slot * GT_TILE + (lane >> 2) * GT_STRIDE + (lane & 3) * 4) = tv;
                }
        } else {   // further passes of a chunk over sparse border tiles: loaded on demand
            for (int slot = 0; slot < npass; ++slot) {
                const int leader = __ffsll((long long)hh) - 1;
                hh &= hh - 1;
                const uint32_t t = __builtin_amdgcn_readfirstlane(__shfl(tile, leader));
                float4 tv = load_tile(t);
                if (aligned && !tile_row_ok(t)) tv = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4 *>(gt + slot * GT_TILE + (lane >> 2) * GT_STRIDE + (lane & 3) * 4) = tv;
            }
        }
        // ---- expand instances into block items
        const int slot = my_slot - slot0;
        // pixel origin of this lane's tile inside its view: one pair of integer divisions per chunk; the items below
        // fetch their owner's origin with a shuffle
        int ttx, tty, ttv;
        tile_decode<MV>(tile, gx, gy, ttx, tty, ttv);
        const float tx0 = (float)(ttx * TILE2D), ty0 = (float)(tty * TILE2D);
        uint32_t mask = 0;
        if (mine) {
            if (masked != nullptr) {
                mask = id & ((1u << MASK_BITS) - 1u);   // evaluated where the instance was emitted (block_mask4)
            } else {
#pragma unroll
                for (int q = 0; q < NBLK; ++q)
                    if (block_live(a.x, a.y, b.z, b.w, tx0 + (float)((q % NB) * SUB2D), ty0 + (float)((q / NB) * SUB2D), (float)SUB2D))
                        mask |= 1u << q;
            }
        }
        const int cnt = __popc(mask);
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const int off = incl - cnt;
        const int total = __shfl(incl, 63);
        s_pa[wave][lane] = a;
        s_pb[wave][lane] = b;
        {
            int o = off;
#pragma unroll
            for (int q = 0; q < NBLK; ++q)
                if (mask & (1u << q)) s_q[wave][o++] = (uint16_t)((lane << 4) | (slot << 2) | q);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // ---- rounds of 64 items
        for (int base = 0; base < total; base += 64) {
            const int e = base + lane;
            float M[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
            const uint32_t item = e < total ? (uint32_t)s_q[wave][e] : 0u;
            const int owner = (int)(item >> 4), sl = (int)((item >> 2) & 3u), q = (int)(item & 3u);
            const float otx0 = __shfl(tx0, owner), oty0 = __shfl(ty0, owner);   // the owner's tile origin (all lanes shuffle)
            float4 oa = make_float4(0.f, 0.f, 0.f, 0.f), ob = oa;
            if (e < total) { oa = s_pa[wave][owner]; ob = s_pb[wave][owner]; }
            const float bx0 = otx0 + (float)((q % NB) * SUB2D);
            const float by0 = oty0 + (float)((q / NB) * SUB2D);
            const float *gq = gt + sl * GT_TILE + (q / NB) * SUB2D * GT_STRIDE + (q % NB) * SUB2D;
            // exact per-pixel path for thin / not safely positive definite Gaussians, the row recurrence for the rest
            // (round 6: an item the recurrences are not safe for takes the exact path, as in the forward; rounds 1-5 re-anchored
            //  the row recurrence at pixel 4 for the in-between tier, in scenes whose preprocess had seen such a Gaussian)
            const bool exact = e < total && item_tier(oa.z, oa.w, ob.x, ob.y, ob.z, ob.w) != 0;
            if (e < total && !exact) block_moments_lds<SUB2D, false>(oa, ob, gq, bx0, by0, M);
            if (__any(e < total && exact)) {
                if (e < total && exact) block_moments_lds<SUB2D, true>(oa, ob, gq, bx0, by0, M);
            }
            __builtin_amdgcn_wave_barrier();
            s_r0[wave][lane] = make_float4(M[0], M[1], M[2], M[3]);
            s_r1[wave][lane] = make_float2(M[4], M[5]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // every instance adds the rows of its own items that were processed in this round, in item order
#pragma unroll
            for (int i = 0; i < NBLK; ++i) {
                const int e2 = off + i - base;
                if (i < cnt && e2 >= 0 && e2 < 64) {
                    const float4 m0 = s_r0[wave][e2];
                    const float2 m1 = s_r1[wave][e2];
                    S[0] += m0.x; S[1] += m0.y; S[2] += m0.z; S[3] += m0.w; S[4] += m1.x; S[5] += m1.y;
                }
            }
        }
    }
    if (live) {
        // scratch row = the instance's EMISSION index, recomputed from the Gaussian's tile rectangle (the duplicate
        // kernel emits a Gaussian's tiles y-major / x-minor from `first`): a Gaussian's rows end up contiguous, so
        // the geometry backward streams them -- no permutation has to be carried through the sort
        int rx0, ry0, rx1, ry1;
        tile_rect(a.x, a.y, rad, gx, gy, rx0, ry0, rx1, ry1);
        int ttx, tty, ttv;
        tile_decode<MV>(tile, gx, gy, ttx, tty, ttv);
        const size_t u = (size_t)first_row + (size_t)((tty - ry0) * (rx1 - rx0) + (ttx - rx0));
        // one aligned 32-byte row per instance (6 moments + 2 pad floats).  Measured, round 3: two planes (float4[R] + float2[R],
        // 24 bytes per instance) made this kernel 9 us and the geometry backward 3 us SLOWER -- the rows are scattered, and a
        // scattered row costs per 32-byte sector it touches, not per byte
        part[2 * u] = make_float4(S[0], S[1], S[2], S[3]);
        part[2 * u + 1] = make_float4(S[4], S[5], 0.f, 0.f);
    }
    // rotate the pipeline registers
    tile = tile1; id = id1; live = live1;
    tile1 = tile2; id1 = id2; live1 = live2;
    a = a1; b = b1; rad = rad1; first_row = first_row1;
    }   // chunk loop
    R2_TS_AT(render, 3);
}

// (Measured and left out, round 6 -- VERDICT r5 #2c: the backward as one-wave work items on the forward's work list, lane = entry,
// the tile's four blocks one after the other, dL/dpix of the block as SCALAR operands of the pixel sequence (s_load_dwordx8 per
// row; or broadcast from LDS), the block masks of the list instead of per-lane tests, an entry's row accumulated in LDS, no software
// pipeline: 54 VGPRs, 7 waves per SIMD, parity green on the whole suite -- and 85-89 us against this kernel's 55 (sub-chunks of 128
// and 256 entries, scalar and LDS operands alike: profiles/experiments/r06_wave_backward_ab*.txt, the patch next to them).  Its
// in-kernel stamps say why (r06_wave_kernels_stamps.txt): a step per block and sub-chunk fills 64 lanes to ~65 % where this kernel's
// queue over all blocks of 64 instances fills its rounds to ~92 %: 57 k steps instead of 36 k rounds, at ~800 issue slots each, on
// SIMDs that the seven resident waves keep 63 % busy -- the kernel was compute-bound on work it created itself.)
// ------------------------------------------------------------------------------------------------ launchers
template <bool MV>
static void launch_fwd(const RasterGeom &g, const RasterBinning &b, const RasterImage &im, int W, int H, int gx, int gy, uint32_t T,
                       float *out_color, bool write_ncontrib, uint32_t *fill_tiles, bool fused_combine, hipStream_t s,
                       char *tf_bin_base, const uint32_t *tf_words, bool ids_below_2_28)
{
    // the one-wave kernel wherever its list exists: ids carry MASK_BITS of block mask, i.e. view instances below 2^28; beyond that
    // the four-wave kernel of rounds 1-5
    // the masked list for chains whose sort did not carry the masks: the forward's wave kernel and the backward read it, so every
    // forward leaves it behind (the backward cannot ask which path ran; it chooses by the same ids_below_2_28 rule)
    if (tf_bin_base == nullptr && im.NW > 0 && ids_below_2_28)
        raster_mask_fill_kernel<MV><<<dim3((unsigned)im.NW), dim3(256), 0, s>>>(im.chunk_base, im.work_tile, T, b.point_list, g.rec,
                                                                                gx, gy, b.masked);
    if (fused_combine && !write_ncontrib && im.NW > 0 && ids_below_2_28) {
        const uint32_t *masked = b.masked;
        const unsigned grid = (unsigned)((im.NW + 7) / 8) * 32u;   // 8 work items x 4 blocks per group of 32 workgroups
        raster_render_forward_wave_kernel<MV><<<dim3(grid), dim3(64), 0, s>>>(
            im.ranges, im.chunk_base, im.work_tile, T, (uint32_t)im.NW, masked, g.rec, gx, gy, im.partial, im.tile_done, out_color, W, H,
            fill_tiles, tf_bin_base, tf_words);
        return;
    }
    if (fused_combine && !write_ncontrib && im.NW > 0) {
        // im.NW = R / FWD_CHUNK + T bounds the real work items plus one item per empty tile
        raster_render_forward_kernel<true, MV><<<dim3((unsigned)im.NW), dim3(256), 0, s>>>(
            im.ranges, im.chunk_base, im.work_tile, T, b.point_list, g.rec, gx, gy, im.partial, im.tile_done, out_color, W, H,
            fill_tiles, tf_bin_base, tf_words);
        return;
    }
    if (im.NW > 0) {
        if (write_ncontrib)
            raster_render_forward_debug_kernel<MV><<<dim3((unsigned)im.NW), dim3(256), 0, s>>>(
                im.ranges, im.chunk_base, im.work_tile, T, b.point_list, g.rec, gx, gy, im.partial, im.partial_last);
        else
            raster_render_forward_kernel<false, MV><<<dim3((unsigned)im.NW), dim3(256), 0, s>>>(
                im.ranges, im.chunk_base, im.work_tile, T, b.point_list, g.rec, gx, gy, im.partial, nullptr, nullptr, W, H, nullptr, nullptr, nullptr);
    }
    if (write_ncontrib)
        raster_combine_kernel<true, MV><<<dim3(T), dim3(256), 0, s>>>(im.chunk_base, im.partial, im.partial_last, W, H, gx, gy,
                                                                      out_color, im.n_contrib, im.ranges, fill_tiles);
    else
        raster_combine_kernel<false, MV><<<dim3(T), dim3(256), 0, s>>>(im.chunk_base, im.partial, im.partial_last, W, H, gx, gy,
                                                                       out_color, im.n_contrib, im.ranges, fill_tiles);
}

int launch_raster_render_forward(const RasterGeom &g, const RasterBinning &b, const RasterImage &im, int W, int H, int V,
                                 float *out_color, bool write_ncontrib, uint32_t *fill_tiles, bool fused_combine,
                                 hipStream_t s, char *tf_bin_base, const uint32_t *tf_words, size_t view_instances)
{
    const bool ids28 = view_instances < ((size_t)1 << (32 - MASK_BITS));
    const int gx = (W + TILE2D - 1) / TILE2D, gy = (H + TILE2D - 1) / TILE2D;
    const uint32_t T = (uint32_t)gx * gy * (uint32_t)V;   // the views' tile grids, stacked
    if (V > 1) launch_fwd<true>(g, b, im, W, H, gx, gy, T, out_color, write_ncontrib, fill_tiles, fused_combine, s, tf_bin_base, tf_words, ids28);
    else launch_fwd<false>(g, b, im, W, H, gx, gy, T, out_color, write_ncontrib, fill_tiles, fused_combine, s, tf_bin_base, tf_words, ids28);
    return 0;
}

int launch_raster_render_backward(const RasterGeom &g, const RasterBinning &b, const int *radii, int W, int H, int V, size_t R,
                                  const float *dL_dpix, hipStream_t s, size_t view_instances)
{
    if (R == 0) return 0;
    // every forward leaves the masked list behind when the ids leave room for the mask bits (launch_raster_render_forward)
    const uint32_t *masked = view_instances < ((size_t)1 << (32 - MASK_BITS)) ? b.masked : nullptr;
    const int gx = (W + TILE2D - 1) / TILE2D;
    const uint32_t nchunks = (uint32_t)((R + BWD_THREADS - 1) / BWD_THREADS);
    // Grid = a whole number of "rounds" of resident waves (CUs x 4 SIMDs x BWD_OCC); the chunks beyond it are second chunks
    // of the first waves (pipelined, see the kernel).  Chunks cost about the same, so with one wave per chunk the last,
    // partly filled round ran at low occupancy for a full wave lifetime: 18068 chunks on 4096 slots = 4.4 rounds took as
    // long as 5 (69 us); 4 full rounds + 1684 second chunks take 58 us.
    const int cus = device_cu_count();
    const uint32_t slots = (uint32_t)cus * 4u * (uint32_t)BWD_OCC;   // a multiple of 8 (XCD-aware chunk order)
    const uint32_t nslots = ((nchunks + 7u) >> 3) << 3;
    const uint32_t grid = (nslots <= slots || (slots & 7u)) ? nslots : (nslots / slots) * slots;
    const int gy = (H + TILE2D - 1) / TILE2D;
    if (V > 1)   // the view of an instance follows from its tile id
        raster_render_backward_kernel<true><<<dim3(grid), dim3(BWD_THREADS), 0, s>>>(
            b.tiles, b.point_list, g.first, radii, g.rec, (uint32_t)R, W, H, gx, gy, nchunks, dL_dpix,
            reinterpret_cast<float4 *>(b.part), g.host_words + DW_USER, masked);
    else
        raster_render_backward_kernel<false><<<dim3(grid), dim3(BWD_THREADS), 0, s>>>(
            b.tiles, b.point_list, g.first, radii, g.rec, (uint32_t)R, W, H, gx, gy, nchunks, dL_dpix,
            reinterpret_cast<float4 *>(b.part), g.host_words + DW_USER, masked);
    return 0;
}

}  // namespace r2
