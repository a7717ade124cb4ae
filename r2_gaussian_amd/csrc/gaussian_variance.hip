// gaussian_variance.hip -- the predictive variance of the exact operators under independent variances of the Gaussians'
// parameters: of the density field at caller-supplied points (r2_query_gaussians_variance) and of every pixel of the exact
// projection (r2_project_gaussians_variance), out = the sum over the point's or pixel's pairs of
// sum_t v[i][t] (d term / d theta_it)^2 (include/r2hip.h; the per-pair arithmetic is gaussian_fisher.hpp's pair_variance).
//
// Both run the forwards' rounds (gaussian_skeleton.hpp: gather_rounds) with a larger staged record (the unmodified scales,
// the quaternion and the eleven variances next to S^-1 R^T): the point kernel is gaussian_fisher.hpp's variance_points_block,
// the pixel kernel the projector's pixel_tile and tile_rounds.  A point or a pixel adds its pairs in ascending Gaussian
// index in one thread: no atomics, no list in memory, no workspace and no host synchronisation, the same bits on every call.
#include "gaussian_fisher.hpp"

namespace r2 {

namespace {

constexpr int GB = TILE2D * TILE2D;   // threads per workgroup = Gaussians per batch

// about 156 bytes, 39 kB for a batch of GB
struct StagedPixVar {
    StagedVar a;
    PixRect q;
};

__global__ void __launch_bounds__(QB) gaussian_query_variance_kernel(int N, const float *__restrict__ points, Cloud cl,
                                                                     const float *__restrict__ v_means,
                                                                     const float *__restrict__ v_density,
                                                                     const float *__restrict__ v_scales,
                                                                     const float *__restrict__ v_rotations, float *__restrict__ out)
{
    variance_points_block(N, points, cl, v_means, v_density, v_scales, v_rotations, out);
}

// One workgroup per 16 x 16 pixel tile and view (blockIdx.z), one thread per pixel: the projector's rounds (tile_rounds).
// The body, once: src says where the tile's Gaussians come from (WholeCloud, or the TileLists of a plan).
template <typename Src>
__device__ __forceinline__ void variance_tile(int H, int W, const float *__restrict__ rays, int cone, const Cloud &cl, const Src &src,
                                              const float *__restrict__ v_means, const float *__restrict__ v_density,
                                              const float *__restrict__ v_scales, const float *__restrict__ v_rotations,
                                              float *__restrict__ out)
{
    __shared__ ViewGeom vg;
    __shared__ StagedPixVar st[GB];
    const PixelTile t = pixel_tile(rays, cone, H, W, vg);
    float acc = 0.0f;
    tile_rounds(
        src, cl, t, vg, cone, H, W, st,
        [&](StagedPixVar &d, const Gauss &a, int i) { stage_var(d.a, a, cl.mod, v_means, v_density, v_scales, v_rotations, i); },
        [&](const StagedPixVar &s) {
            GaussPair p;
            if (gauss_pair(s.a.g, t.y, cone, p)) acc += staged_variance(s.a, p, t.y, t.len);
        });
    if (t.inside) out[((size_t)t.view * H + t.r) * W + t.c] = acc;
}

__global__ void __launch_bounds__(GB) gaussian_project_variance_kernel(int H, int W, const float *__restrict__ rays, int cone, Cloud cl,
                                                                       const float *__restrict__ v_means,
                                                                       const float *__restrict__ v_density,
                                                                       const float *__restrict__ v_scales,
                                                                       const float *__restrict__ v_rotations, float *__restrict__ out)
{
    variance_tile(H, W, rays, cone, cl, WholeCloud{}, v_means, v_density, v_scales, v_rotations, out);
}

__global__ void __launch_bounds__(GB) gaussian_project_variance_planned_kernel(int H, int W, const float *__restrict__ rays, int cone,
                                                                               Cloud cl, TileLists tl,
                                                                               const float *__restrict__ v_means,
                                                                               const float *__restrict__ v_density,
                                                                               const float *__restrict__ v_scales,
                                                                               const float *__restrict__ v_rotations,
                                                                               float *__restrict__ out)
{
    variance_tile(H, W, rays, cone, cl, tl, v_means, v_density, v_scales, v_rotations, out);
}

// Both entry points of the projection variance; tl: the lists of the planned one, or NULL.
int project_variance(const char *entry, const TileLists *tl, int V, int H, int W, const float *rays, int cone, const Cloud &cl,
                     const float *v_means, const float *v_density, const float *v_scales, const float *v_rotations, float *out,
                     void *stream)
{
    const int P = cl.P;
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays || !out ||
        (P > 0 && (cl.missing() || !v_means || !v_density || !v_scales || !v_rotations)) || (tl && lists_missing(P, *tl)))
        return invalid_argument(entry);
    if (V > 65535 || (H + TILE2D - 1) / TILE2D > 65535 || P > CLOUD_MAX_P) {
        set_error("%s: shape out of range (V %d, H %d, P %d)", entry, V, H, P);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((W + TILE2D - 1) / TILE2D, (H + TILE2D - 1) / TILE2D, V);
    if (tl && P > 0)   // P = 0 needs no lists: the unplanned kernel runs no round and writes the zeros
        gaussian_project_variance_planned_kernel<<<grid, dim3(GB), 0, s>>>(H, W, rays, cone, cl, *tl, v_means, v_density, v_scales,
                                                                           v_rotations, out);
    else
        gaussian_project_variance_kernel<<<grid, dim3(GB), 0, s>>>(H, W, rays, cone, cl, v_means, v_density, v_scales, v_rotations,
                                                                   out);
    R2_STAGE_CHECK(0, s, "project gaussians variance");
    return 0;
}

}  // namespace

}  // namespace r2

extern "C" int r2_query_gaussians_variance(int N, const float *points, int P, const float *means, const float *density,
                                           const float *scales, float scale_modifier, const float *rotations, const float *v_means,
                                           const float *v_density, const float *v_scales, const float *v_rotations, float *out,
                                           void *stream)
{
    using namespace r2;
    const char *entry = "r2_query_gaussians_variance";
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    if (N < 0 || P < 0 || (N > 0 && (!points || !out)) ||
        (N > 0 && P > 0 && (cl.missing() || !v_means || !v_density || !v_scales || !v_rotations)))
        return invalid_argument(entry);
    if (cloud_too_large(entry, P)) return R2_ERR_INVALID;
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    gaussian_query_variance_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, points, cl, v_means, v_density, v_scales, v_rotations,
                                                                                  out);
    R2_STAGE_CHECK(0, s, "query gaussians variance");
    return 0;
}

extern "C" int r2_project_gaussians_variance(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                             const float *density, const float *scales, float scale_modifier,
                                             const float *rotations, const float *v_means, const float *v_density,
                                             const float *v_scales, const float *v_rotations, float *out, void *stream)
{
    const r2::Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    return r2::project_variance("r2_project_gaussians_variance", nullptr, V, H, W, rays, cone, cl, v_means, v_density, v_scales,
                                v_rotations, out, stream);
}

extern "C" int r2_project_gaussians_variance_planned(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                                     const float *density, const float *scales, float scale_modifier,
                                                     const float *rotations, const float *v_means, const float *v_density,
                                                     const float *v_scales, const float *v_rotations, float *out,
                                                     const long long *offsets, const int *ids, long long ids_capacity, void *stream)
{
    const r2::Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    const r2::TileLists tl = { offsets, ids, ids_capacity };
    return r2::project_variance("r2_project_gaussians_variance_planned", &tl, V, H, W, rays, cone, cl, v_means, v_density, v_scales,
                                v_rotations, out, stream);
}
