// gaussian_plan.hip -- the projection plan of the exact projector: for every 16 x 16 tile of every view the ascending list of
// the Gaussians the pixel-major kernels would stage for it (include/r2hip.h: r2_project_gaussians_plan_count,
// r2_project_gaussians_plan_fill).  The planned kernels (gaussian_skeleton.hpp: list_rounds) walk a tile's list where the
// unplanned ones walk the cloud, so a cloud and a geometry that are projected many times pay the P tests per tile once.
//
// Three kernels and a scan, no atomics at all:
//   table   one thread per (view, Gaussian): gauss_radius and gauss_rect -- gaussian_rays.hpp's, the functions the kernels
//           stage with -- once, V P times where the unplanned kernels make V T P of them; the pixel rectangle is written to
//           the caller's workspace as the rectangle of TILES it meets, four 16-bit numbers (an empty one for a Gaussian
//           without radius or rectangle).  With the rectangle cut to the detector (rect_axis) and tile tx covering the
//           columns 16 tx .. min(16 tx + 16, W) - 1, tile_rounds' test c0 <= tc1 && c1 >= tc0 is c0 / 16 <= tx <= c1 / 16.
//   count   one workgroup per (view, tile) walks the view's row of the table, 256 entries per round and four compares per
//           entry, and writes the number of hits to offsets[tile + 1];
//   scan    one workgroup turns the counts into offsets in place (int64);
//   fill    the count's walk again: the hits of a round are compacted IN ORDER with gather_rounds' wave ballots and wave
//           counts and written as int32 ids from offsets[tile] on, so every list ascends.
// Where an id lands depends on the table and the offsets alone: building twice gives the same bytes, and the ids of a view's
// lists do not depend on the other views.
#include "gaussian_skeleton.hpp"

namespace r2 {

namespace {

constexpr int PB = TILE2D * TILE2D;   // threads per workgroup = table entries per round
constexpr int SCAN = 1024;            // threads of the scan's one workgroup

// The tiles a Gaussian's rectangle meets, both ends included; x0 > x1: none.
struct TileRect {
    unsigned short x0, x1, y0, y1;
};

__global__ void __launch_bounds__(PB) gaussian_plan_table_kernel(int H, int W, const float *__restrict__ rays, int cone, Cloud cl,
                                                                 TileRect *__restrict__ table)
{
    __shared__ ViewGeom vg;
    const int view = blockIdx.y;
    if (threadIdx.x == 0) vg = view_geom(rays + 12 * view, cone);
    __syncthreads();
    const int i = blockIdx.x * PB + threadIdx.x;
    if (i >= cl.P) return;
    const Gauss a = load_gauss(cl, i);
    const float radius = gauss_radius(a, cl.mod);
    TileRect e = { 1, 0, 1, 0 };
    PixRect rc;
    if (radius >= 0.0f && gauss_rect(vg, cone, a.mx, a.my, a.mz, radius, H, W, rc)) {
        e.x0 = (unsigned short)(rc.c0 / TILE2D); e.x1 = (unsigned short)(rc.c1 / TILE2D);
        e.y0 = (unsigned short)(rc.r0 / TILE2D); e.y1 = (unsigned short)(rc.r1 / TILE2D);
    }
    table[(size_t)view * cl.P + i] = e;
}

// Does entry i of the view's row meet tile (blockIdx.x, blockIdx.y)?  false beyond the row.
__device__ __forceinline__ bool meets_tile(const TileRect *__restrict__ row, int i, int P)
{
    if (i >= P) return false;
    const TileRect e = row[i];
    return e.x0 <= blockIdx.x && e.x1 >= blockIdx.x && e.y0 <= blockIdx.y && e.y1 >= blockIdx.y;
}

__device__ __forceinline__ size_t tile_index() { return ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; }

__global__ void __launch_bounds__(PB) gaussian_plan_count_kernel(int P, const TileRect *__restrict__ table, long long *__restrict__ offsets)
{
    __shared__ int wcount[PB / WAVE];
    const TileRect *row = table + (size_t)blockIdx.z * P;
    const int tid = threadIdx.x;
    int n = 0;   // wave-uniform: the hits of this wave's entries
    for (int base = 0; base < P; base += PB) n += __popcll(__ballot(meets_tile(row, base + tid, P)));
    if ((tid & (WAVE - 1)) == 0) wcount[tid / WAVE] = n;
    __syncthreads();
    if (tid == 0) {
        long long total = 0;
#pragma unroll
        for (int w = 0; w < PB / WAVE; ++w) total += wcount[w];
        offsets[tile_index() + 1] = total;
        if (tile_index() == 0) offsets[0] = 0;
    }
}

// offsets[1 .. n] hold counts; afterwards offsets[k] = the sum of the counts before list k.  One workgroup: thread t owns
// the chunk [t c, (t + 1) c) of the counts, adds it, the workgroup scans the SCAN sums, and the thread rewrites its chunk.
__global__ void __launch_bounds__(SCAN) gaussian_plan_scan_kernel(long long n, long long *__restrict__ offsets)
{
    __shared__ long long sums[SCAN];
    const int tid = threadIdx.x;
    const long long c = (n + SCAN - 1) / SCAN, lo = min((long long)tid * c, n), hi = min(lo + c, n);
    long long s = 0;
    for (long long k = lo; k < hi; ++k) s += offsets[1 + k];
    sums[tid] = s;
    __syncthreads();
    for (int d = 1; d < SCAN; d <<= 1) {   // inclusive scan of the chunk sums
        const long long v = tid >= d ? sums[tid - d] : 0;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    long long run = sums[tid] - s;
    for (long long k = lo; k < hi; ++k) {
        run += offsets[1 + k];
        offsets[1 + k] = run;
    }
}

__global__ void __launch_bounds__(PB) gaussian_plan_fill_kernel(int P, const TileRect *__restrict__ table,
                                                                const long long *__restrict__ offsets, int *__restrict__ ids,
                                                                long long capacity)
{
    __shared__ int wcount[2][PB / WAVE];   // double-buffered: one barrier per round
    const TileRect *row = table + (size_t)blockIdx.z * P;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const size_t tile = tile_index();
    long long pos = offsets[tile];                         // where the next round's first hit goes
    const long long end = min(offsets[tile + 1], capacity);   // nothing is written at or beyond either
    int buf = 0;
    for (int base = 0; base < P; base += PB, buf ^= 1) {
        const int i = base + tid;
        const bool hit = meets_tile(row, i, P);
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) wcount[buf][wave] = __popcll(mask);
        __syncthreads();
        int slot = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < PB / WAVE; ++w) {
            if (w < wave) slot += wcount[buf][w];
            total += wcount[buf][w];
        }
        if (hit && pos + slot >= 0 && pos + slot < end) ids[pos + slot] = i;
        pos += total;
    }
}

int tiles_x(int W) { return (W + TILE2D - 1) / TILE2D; }
int tiles_y(int H) { return (H + TILE2D - 1) / TILE2D; }

// The checks count and fill share; true: refuse with R2_ERR_INVALID (the error text is set).
bool plan_refused(const char *entry, int V, int H, int W, const float *rays, const Cloud &cl, const void *workspace,
                  size_t workspace_bytes)
{
    if (V <= 0 || H <= 0 || W <= 0 || cl.P < 0 || !rays || cl.missing()) {
        invalid_argument(entry);
        return true;
    }
    if (V > 65535 || tiles_y(H) > 65535 || tiles_x(W) > 65535 || cl.P > CLOUD_MAX_P) {
        set_error("%s: shape out of range (V %d, H %d, W %d, P %d)", entry, V, H, W, cl.P);
        return true;
    }
    return workspace_too_small(entry, "r2_project_gaussians_plan_workspace_bytes", workspace, workspace_bytes,
                               r2_project_gaussians_plan_workspace_bytes(V, H, W, cl.P));
}

}  // namespace

}  // namespace r2

extern "C" size_t r2_project_gaussians_plan_workspace_bytes(int V, int H, int W, int P)
{
    if (V <= 0 || H <= 0 || W <= 0 || P <= 0) return 0;
    return (size_t)V * (size_t)P * sizeof(r2::TileRect);
}

extern "C" int r2_project_gaussians_plan_count(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                               const float *density, const float *scales, float scale_modifier,
                                               const float *rotations, long long *offsets, void *workspace, size_t workspace_bytes,
                                               void *stream)
{
    using namespace r2;
    const char *entry = "r2_project_gaussians_plan_count";
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    if (!offsets) return invalid_argument(entry);
    if (plan_refused(entry, V, H, W, rays, cl, workspace, workspace_bytes)) return R2_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long lists = (long long)V * tiles_x(W) * tiles_y(H);
    if (P == 0) {
        R2_HIP_TRY(hipMemsetAsync(offsets, 0, (size_t)(lists + 1) * sizeof(long long), s));
        return 0;
    }
    TileRect *table = (TileRect *)workspace;
    gaussian_plan_table_kernel<<<dim3((P + PB - 1) / PB, V), dim3(PB), 0, s>>>(H, W, rays, cone, cl, table);
    gaussian_plan_count_kernel<<<dim3(tiles_x(W), tiles_y(H), V), dim3(PB), 0, s>>>(P, table, offsets);
    gaussian_plan_scan_kernel<<<dim3(1), dim3(SCAN), 0, s>>>(lists, offsets);
    R2_STAGE_CHECK(0, s, "project gaussians plan count");
    return 0;
}

extern "C" int r2_project_gaussians_plan_fill(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                              const float *density, const float *scales, float scale_modifier,
                                              const float *rotations, const long long *offsets, int *ids, long long ids_capacity,
                                              void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace r2;
    const char *entry = "r2_project_gaussians_plan_fill";
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    if (!offsets || ids_capacity < 0 || (ids_capacity > 0 && !ids)) return invalid_argument(entry);
    if (plan_refused(entry, V, H, W, rays, cl, workspace, workspace_bytes)) return R2_ERR_INVALID;
    if (P == 0 || ids_capacity == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    gaussian_plan_fill_kernel<<<dim3(tiles_x(W), tiles_y(H), V), dim3(PB), 0, s>>>(P, (const TileRect *)workspace, offsets, ids,
                                                                                   ids_capacity);
    R2_STAGE_CHECK(0, s, "project gaussians plan fill");
    return 0;
}
