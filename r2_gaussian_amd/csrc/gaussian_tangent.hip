// gaussian_tangent.hip -- the Jacobian of the exact projector applied forwards: J t for a tangent t of the cloud's parameters
// (r2_project_gaussians_jvp) and every pixel's derivative in its own ray (r2_project_gaussians_ray_jacobian), as
// include/r2hip.h states them; the per-pair arithmetic is gaussian_tangent.hpp's pair_tangent and gaussian_ray_grad.hpp's
// gauss_pair_ray_grad with G = 1.
//
// Both are pixel-major on the projector's skeleton (gaussian_skeleton.hpp: pixel_tile, tile_rounds): one workgroup per
// 16 x 16 pixel tile and view, one thread per pixel, which adds its pairs -- exactly those the forward sums -- in ascending
// Gaussian index.  The first is the projection variance's kernel without the square, with its staged record; the second is
// the ray backward's walk without the reduction over the pixels.  No atomics, no workspace, no host synchronisation, the same
// bits on every call, and nothing a view computes depends on another view.
#include "gaussian_ray_grad.hpp"
#include "gaussian_tangent.hpp"

namespace r2 {

namespace {

constexpr int GB = TILE2D * TILE2D;   // threads per workgroup = Gaussians per batch

// the projection variance's record: about 156 bytes, 39 kB for a batch of GB
struct StagedPixTan {
    StagedVar a;
    PixRect q;
};

// The two bodies, once each: src says where the tile's Gaussians come from (WholeCloud, or the TileLists of a plan).
template <typename Src>
__device__ __forceinline__ void jvp_tile(int H, int W, const float *__restrict__ rays, int cone, const Cloud &cl, const Src &src,
                                         const float *__restrict__ t_means, const float *__restrict__ t_density,
                                         const float *__restrict__ t_scales, const float *__restrict__ t_rotations,
                                         float *__restrict__ out)
{
    __shared__ ViewGeom vg;
    __shared__ StagedPixTan st[GB];
    const PixelTile t = pixel_tile(rays, cone, H, W, vg);
    float acc = 0.0f;
    tile_rounds(
        src, cl, t, vg, cone, H, W, st,
        [&](StagedPixTan &d, const Gauss &a, int i) { stage_var(d.a, a, cl.mod, t_means, t_density, t_scales, t_rotations, i); },
        [&](const StagedPixTan &s) {
            GaussPair p;
            if (gauss_pair(s.a.g, t.y, cone, p)) acc += staged_tangent(s.a, p, t.y, t.len);
        });
    if (t.inside) out[((size_t)t.view * H + t.r) * W + t.c] = acc;
}

// out [V,6,H,W]: planes 0..2 d pixel / d s, planes 3..5 d pixel / d d; a tile row stores 64 contiguous bytes per plane.
template <typename Src>
__device__ __forceinline__ void ray_jacobian_tile(int H, int W, const float *__restrict__ rays, int cone, const Cloud &cl,
                                                  const Src &src, float *__restrict__ out)
{
    __shared__ ViewGeom vg;
    __shared__ Staged st[GB];
    const PixelTile t = pixel_tile(rays, cone, H, W, vg);
    float gs[3] = { 0.f, 0.f, 0.f }, gd[3] = { 0.f, 0.f, 0.f };
    tile_rounds(
        src, cl, t, vg, cone, H, W, st, [&](Staged &d, const Gauss &a, int) { d.g = gauss_rec(a, cl.mod); },
        [&](const Staged &s) {
            GaussPair p;
            if (gauss_pair(s.g, t.y, cone, p)) gauss_pair_ray_grad(s.g, p, t.y, t.len, 1.0f, gs, gd);
        });
    if (t.inside) {
        const size_t plane = (size_t)H * W;
        float *dst = out + (size_t)t.view * 6 * plane + (size_t)t.r * W + t.c;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            dst[j * plane] = gs[j];
            dst[(3 + j) * plane] = gd[j];
        }
    }
}

__global__ void __launch_bounds__(GB) gaussian_project_jvp_kernel(int H, int W, const float *__restrict__ rays, int cone, Cloud cl,
                                                                  const float *__restrict__ t_means,
                                                                  const float *__restrict__ t_density,
                                                                  const float *__restrict__ t_scales,
                                                                  const float *__restrict__ t_rotations, float *__restrict__ out)
{
    jvp_tile(H, W, rays, cone, cl, WholeCloud{}, t_means, t_density, t_scales, t_rotations, out);
}

__global__ void __launch_bounds__(GB) gaussian_project_jvp_planned_kernel(int H, int W, const float *__restrict__ rays, int cone,
                                                                          Cloud cl, TileLists tl, const float *__restrict__ t_means,
                                                                          const float *__restrict__ t_density,
                                                                          const float *__restrict__ t_scales,
                                                                          const float *__restrict__ t_rotations,
                                                                          float *__restrict__ out)
{
    jvp_tile(H, W, rays, cone, cl, tl, t_means, t_density, t_scales, t_rotations, out);
}

__global__ void __launch_bounds__(GB) gaussian_project_ray_jacobian_kernel(int H, int W, const float *__restrict__ rays, int cone,
                                                                           Cloud cl, float *__restrict__ out)
{
    ray_jacobian_tile(H, W, rays, cone, cl, WholeCloud{}, out);
}

__global__ void __launch_bounds__(GB) gaussian_project_ray_jacobian_planned_kernel(int H, int W, const float *__restrict__ rays,
                                                                                   int cone, Cloud cl, TileLists tl,
                                                                                   float *__restrict__ out)
{
    ray_jacobian_tile(H, W, rays, cone, cl, tl, out);
}

bool shape_out_of_range(const char *entry, int V, int H, int P)
{
    if (V <= 65535 && (H + TILE2D - 1) / TILE2D <= 65535 && P <= CLOUD_MAX_P) return false;
    set_error("%s: shape out of range (V %d, H %d, P %d)", entry, V, H, P);
    return true;
}

// Both entry points of each operator; tl: the lists of the planned one, or NULL.  P = 0 needs no lists: the unplanned
// kernel runs no round and writes the zeros.
int project_jvp(const char *entry, const TileLists *tl, int V, int H, int W, const float *rays, int cone, const Cloud &cl,
                const float *t_means, const float *t_density, const float *t_scales, const float *t_rotations, float *out,
                void *stream)
{
    const int P = cl.P;
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays || !out ||
        (P > 0 && (cl.missing() || !t_means || !t_density || !t_scales || !t_rotations)) || (tl && lists_missing(P, *tl)))
        return invalid_argument(entry);
    if (shape_out_of_range(entry, V, H, P)) return R2_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((W + TILE2D - 1) / TILE2D, (H + TILE2D - 1) / TILE2D, V);
    if (tl && P > 0)
        gaussian_project_jvp_planned_kernel<<<grid, dim3(GB), 0, s>>>(H, W, rays, cone, cl, *tl, t_means, t_density, t_scales,
                                                                      t_rotations, out);
    else
        gaussian_project_jvp_kernel<<<grid, dim3(GB), 0, s>>>(H, W, rays, cone, cl, t_means, t_density, t_scales, t_rotations, out);
    R2_STAGE_CHECK(0, s, "project gaussians jvp");
    return 0;
}

int project_ray_jacobian(const char *entry, const TileLists *tl, int V, int H, int W, const float *rays, int cone, const Cloud &cl,
                         float *out, void *stream)
{
    const int P = cl.P;
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays || !out || cl.missing() || (tl && lists_missing(P, *tl)))
        return invalid_argument(entry);
    if (shape_out_of_range(entry, V, H, P)) return R2_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((W + TILE2D - 1) / TILE2D, (H + TILE2D - 1) / TILE2D, V);
    if (tl && P > 0)
        gaussian_project_ray_jacobian_planned_kernel<<<grid, dim3(GB), 0, s>>>(H, W, rays, cone, cl, *tl, out);
    else
        gaussian_project_ray_jacobian_kernel<<<grid, dim3(GB), 0, s>>>(H, W, rays, cone, cl, out);
    R2_STAGE_CHECK(0, s, "project gaussians ray jacobian");
    return 0;
}

}  // namespace

}  // namespace r2

extern "C" int r2_project_gaussians_jvp(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                        const float *density, const float *scales, float scale_modifier, const float *rotations,
                                        const float *t_means, const float *t_density, const float *t_scales,
                                        const float *t_rotations, float *out, void *stream)
{
    const r2::Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    return r2::project_jvp("r2_project_gaussians_jvp", nullptr, V, H, W, rays, cone, cl, t_means, t_density, t_scales, t_rotations,
                           out, stream);
}

extern "C" int r2_project_gaussians_jvp_planned(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                                const float *density, const float *scales, float scale_modifier,
                                                const float *rotations, const float *t_means, const float *t_density,
                                                const float *t_scales, const float *t_rotations, float *out,
                                                const long long *offsets, const int *ids, long long ids_capacity, void *stream)
{
    const r2::Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    const r2::TileLists tl = { offsets, ids, ids_capacity };
    return r2::project_jvp("r2_project_gaussians_jvp_planned", &tl, V, H, W, rays, cone, cl, t_means, t_density, t_scales,
                           t_rotations, out, stream);
}

extern "C" int r2_project_gaussians_ray_jacobian(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                                 const float *density, const float *scales, float scale_modifier,
                                                 const float *rotations, float *out, void *stream)
{
    const r2::Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    return r2::project_ray_jacobian("r2_project_gaussians_ray_jacobian", nullptr, V, H, W, rays, cone, cl, out, stream);
}

extern "C" int r2_project_gaussians_ray_jacobian_planned(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                                         const float *density, const float *scales, float scale_modifier,
                                                         const float *rotations, float *out, const long long *offsets,
                                                         const int *ids, long long ids_capacity, void *stream)
{
    const r2::Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    const r2::TileLists tl = { offsets, ids, ids_capacity };
    return r2::project_ray_jacobian("r2_project_gaussians_ray_jacobian_planned", &tl, V, H, W, rays, cone, cl, out, stream);
}
