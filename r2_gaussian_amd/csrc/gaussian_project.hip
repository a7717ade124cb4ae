// gaussian_project.hip -- the exact X-ray transform of a Gaussian cloud: out[v][r][c] = the sum over the Gaussians of the
// closed-form line integral of each along the ray of pixel (r, c) (include/r2hip.h: r2_project_gaussians; the per-pair
// arithmetic, the bounding rectangle and the cone rule are gaussian_rays.hpp's, shared with the backward).
//
// The skeleton is gaussian_skeleton.hpp's (pixel_tile, tile_rounds on gather_rounds), shared with the ray backward and the
// projection variance.  One workgroup per 16 x 16 pixel tile and view (blockIdx.z), one thread per pixel.  The workgroup
// walks the P Gaussians in index order, 256 at a time: thread i projects the bounding sphere of Gaussian base + i onto the detector (a conservative
// pixel rectangle), the ones whose rectangle meets the tile are compacted IN ORDER (wave ballots + the four wave counts) into
// an LDS batch together with their S^-1 R^T, and every pixel then adds the batch's pairs whose rectangle holds it, in batch
// order.  A pixel therefore adds its pairs in ascending Gaussian index, in one thread: no atomics, no list in memory, no
// workspace and no host synchronisation, the same bits on every call, and nothing a view computes depends on another view.
// The price is P rectangle tests per tile instead of a sorted per-tile list; DESIGN.md section 4 has what that costs.
// r2_project_gaussians_planned is the same body on the per-tile lists of a projection plan (gaussian_plan.hip; the skeleton's
// list_rounds): one staging per list entry instead of P tests per tile, the same pairs in the same order, the same bits.
#include "gaussian_skeleton.hpp"

namespace r2 {

namespace {

constexpr int GB = TILE2D * TILE2D;   // threads per workgroup = Gaussians per batch

// The kernel's body, once: src says where the tile's Gaussians come from (WholeCloud, or the TileLists of a plan).
template <typename Src>
__device__ __forceinline__ void project_tile(int H, int W, const float *__restrict__ rays, int cone, const Cloud &cl, const Src &src,
                                             float *__restrict__ out)
{
    __shared__ ViewGeom vg;
    __shared__ Staged st[GB];
    const PixelTile t = pixel_tile(rays, cone, H, W, vg);
    float acc = 0.0f;
    tile_rounds(
        src, cl, t, vg, cone, H, W, st, [&](Staged &d, const Gauss &a, int) { d.g = gauss_rec(a, cl.mod); },
        [&](const Staged &s) {
            GaussPair p;
            if (gauss_pair(s.g, t.y, cone, p)) acc += gauss_term(s.g, p, t.len);
        });
    if (t.inside) out[((size_t)t.view * H + t.r) * W + t.c] = acc;
}

__global__ void __launch_bounds__(GB) gaussian_project_kernel(int H, int W, const float *__restrict__ rays, int cone, Cloud cl,
                                                              float *__restrict__ out)
{
    project_tile(H, W, rays, cone, cl, WholeCloud{}, out);
}

// A tile without entries runs no round and writes its zeros.
__global__ void __launch_bounds__(GB) gaussian_project_planned_kernel(int H, int W, const float *__restrict__ rays, int cone, Cloud cl,
                                                                      TileLists tl, float *__restrict__ out)
{
    project_tile(H, W, rays, cone, cl, tl, out);
}

}  // namespace

}  // namespace r2

extern "C" int r2_project_gaussians(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                    const float *density, const float *scales, float scale_modifier, const float *rotations,
                                    float *out, void *stream)
{
    using namespace r2;
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays || !out || cl.missing()) return invalid_argument("r2_project_gaussians");
    if (V > 65535 || (H + TILE2D - 1) / TILE2D > 65535 || P > CLOUD_MAX_P) {
        set_error("r2_project_gaussians: shape out of range (V %d, H %d, P %d)", V, H, P);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((W + TILE2D - 1) / TILE2D, (H + TILE2D - 1) / TILE2D, V);
    gaussian_project_kernel<<<grid, dim3(GB), 0, s>>>(H, W, rays, cone, cl, out);
    R2_STAGE_CHECK(0, s, "project gaussians");
    return 0;
}

extern "C" int r2_project_gaussians_planned(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                            const float *density, const float *scales, float scale_modifier, const float *rotations,
                                            float *out, const long long *offsets, const int *ids, long long ids_capacity,
                                            void *stream)
{
    using namespace r2;
    const char *entry = "r2_project_gaussians_planned";
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    const TileLists tl = { offsets, ids, ids_capacity };
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays || !out || cl.missing() || lists_missing(P, tl)) return invalid_argument(entry);
    if (V > 65535 || (H + TILE2D - 1) / TILE2D > 65535 || P > CLOUD_MAX_P) {
        set_error("%s: shape out of range (V %d, H %d, P %d)", entry, V, H, P);
        return R2_ERR_INVALID;
    }
    if (P == 0) return r2_project_gaussians(V, H, W, rays, cone, P, means, density, scales, scale_modifier, rotations, out, stream);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((W + TILE2D - 1) / TILE2D, (H + TILE2D - 1) / TILE2D, V);
    gaussian_project_planned_kernel<<<grid, dim3(GB), 0, s>>>(H, W, rays, cone, cl, tl, out);
    R2_STAGE_CHECK(0, s, "project gaussians planned");
    return 0;
}
