// gaussian_project_rays_bwd.hip -- the gradient of r2_project_gaussians with respect to its rays [V,12], given G = dL/dout
// (include/r2hip.h: r2_project_gaussians_rays_backward; the per-pair arithmetic is gaussian_ray_grad.hpp's on top of
// gaussian_rays.hpp's pair, rectangle and cone rule, so a pair is differentiated exactly when the forward summed it).
//
// Pixel-major, on the forward's skeleton (gaussian_skeleton.hpp: tile_rounds): one workgroup per 16 x 16 pixel tile and view, one thread
// per pixel; the P Gaussians are walked 256 per round, thread i tests the rectangle of Gaussian base + i against the tile, the hits
// are compacted IN ORDER into an LDS batch, and every pixel adds the batch's pairs whose rectangle holds it to its six sums
// g_s, g_d -- in ascending Gaussian index, in one thread.  At the end a pixel forms its twelve contributions, the workgroup adds
// the 256 x 12 values in one fixed order (gaussian_ray_grad.hpp: block_sum12) and writes partial[view][tile][12] into the
// caller's workspace.  A second kernel, one workgroup per view, adds that view's tile partials -- thread t tiles t, t + 256, ...
// in ascending order, then the same fixed-order sum -- and writes dL_drays[view].  No atomics, no allocation and no host
// synchronisation, the same bits on every call, and nothing a view computes depends on another view.
#include "gaussian_ray_grad.hpp"
#include "gaussian_skeleton.hpp"

namespace r2 {

namespace {

// The first kernel's body, once: src says where the tile's Gaussians come from (WholeCloud, or the TileLists of a plan).
template <typename Src>
__device__ __forceinline__ void rays_bwd_tile(int H, int W, const float *__restrict__ rays, int cone, const Cloud &cl, const Src &src,
                                              const float *__restrict__ G, float *__restrict__ partial)
{
    static_assert(RG == TILE2D * TILE2D, "one thread per pixel of a tile");
    __shared__ ViewGeom vg;
    __shared__ Staged st[RG];
    __shared__ float wsum[RG / WAVE][12];
    const PixelTile t = pixel_tile(rays, cone, H, W, vg);
    const float Gp = t.inside ? G[((size_t)t.view * H + t.r) * W + t.c] : 0.0f;
    float gs[3] = { 0.f, 0.f, 0.f }, gd[3] = { 0.f, 0.f, 0.f };
    tile_rounds(
        src, cl, t, vg, cone, H, W, st, [&](Staged &d, const Gauss &a, int) { d.g = gauss_rec(a, cl.mod); },
        [&](const Staged &s) {
            GaussPair p;
            if (gauss_pair(s.g, t.y, cone, p)) gauss_pair_ray_grad(s.g, p, t.y, t.len, Gp, gs, gd);
        });
    float o[12];   // a thread outside the detector has added nothing: twelve zeros
    pixel_ray_grad(cone, t.r, t.c, gs, gd, o);
    block_sum12(o, wsum);
    if (threadIdx.x == 0) {
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        float *dst = partial + ((size_t)t.view * gridDim.x * gridDim.y + tile) * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) dst[k] = o[k];
    }
}

__global__ void __launch_bounds__(RG) gaussian_project_rays_bwd_kernel(int H, int W, const float *__restrict__ rays, int cone, Cloud cl,
                                                                       const float *__restrict__ G, float *__restrict__ partial)
{
    rays_bwd_tile(H, W, rays, cone, cl, WholeCloud{}, G, partial);
}

// A tile without entries runs no round and writes its zero partial.
__global__ void __launch_bounds__(RG) gaussian_project_rays_bwd_planned_kernel(int H, int W, const float *__restrict__ rays, int cone,
                                                                               Cloud cl, TileLists tl, const float *__restrict__ G,
                                                                               float *__restrict__ partial)
{
    rays_bwd_tile(H, W, rays, cone, cl, tl, G, partial);
}

__global__ void __launch_bounds__(RG) gaussian_project_rays_reduce_kernel(int tiles, const float *__restrict__ partial,
                                                                          float *__restrict__ d_rays)
{
    __shared__ float wsum[RG / WAVE][12];
    const float *src = partial + (size_t)blockIdx.x * tiles * 12;
    float o[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = 0.0f;
    for (int t = threadIdx.x; t < tiles; t += RG)
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] += src[(size_t)t * 12 + k];
    block_sum12(o, wsum);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 12; ++k) d_rays[12 * blockIdx.x + k] = o[k];
}

size_t tiles_of(int H, int W) { return (size_t)((H + TILE2D - 1) / TILE2D) * (size_t)((W + TILE2D - 1) / TILE2D); }

// Both entry points; tl: the lists of the planned one, or NULL.
int rays_backward(const char *entry, const TileLists *tl, int V, int H, int W, const float *rays, int cone, const Cloud &cl,
                  const float *dL_dout, float *dL_drays, void *workspace, size_t workspace_bytes, void *stream)
{
    const int P = cl.P;
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays || !dL_dout || !dL_drays || cl.missing() || (tl && lists_missing(P, *tl)))
        return invalid_argument(entry);
    if (V > 65535 || (H + TILE2D - 1) / TILE2D > 65535 || (long long)H * W >= (1LL << 30) || P > CLOUD_MAX_P) {
        set_error("%s: shape out of range (V %d, H %d, W %d, P %d)", entry, V, H, W, P);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) {
        R2_HIP_TRY(hipMemsetAsync(dL_drays, 0, (size_t)V * 12 * sizeof(float), s));
        return 0;
    }
    const size_t need = r2_project_gaussians_rays_backward_workspace_bytes(V, H, W);
    if (workspace_too_small(entry, "r2_project_gaussians_rays_backward_workspace_bytes", workspace, workspace_bytes, need))
        return R2_ERR_INVALID;
    const dim3 grid((W + TILE2D - 1) / TILE2D, (H + TILE2D - 1) / TILE2D, V);
    float *partial = (float *)workspace;
    if (tl)
        gaussian_project_rays_bwd_planned_kernel<<<grid, dim3(RG), 0, s>>>(H, W, rays, cone, cl, *tl, dL_dout, partial);
    else
        gaussian_project_rays_bwd_kernel<<<grid, dim3(RG), 0, s>>>(H, W, rays, cone, cl, dL_dout, partial);
    gaussian_project_rays_reduce_kernel<<<dim3(V), dim3(RG), 0, s>>>((int)tiles_of(H, W), partial, dL_drays);
    R2_STAGE_CHECK(0, s, "project gaussians rays backward");
    return 0;
}

}  // namespace

}  // namespace r2

extern "C" size_t r2_project_gaussians_rays_backward_workspace_bytes(int V, int H, int W)
{
    if (V <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)V * r2::tiles_of(H, W) * 12 * sizeof(float);
}

extern "C" int r2_project_gaussians_rays_backward(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                                  const float *density, const float *scales, float scale_modifier,
                                                  const float *rotations, const float *dL_dout, float *dL_drays, void *workspace,
                                                  size_t workspace_bytes, void *stream)
{
    const r2::Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    return r2::rays_backward("r2_project_gaussians_rays_backward", nullptr, V, H, W, rays, cone, cl, dL_dout, dL_drays, workspace,
                             workspace_bytes, stream);
}

extern "C" int r2_project_gaussians_rays_backward_planned(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                                          const float *density, const float *scales, float scale_modifier,
                                                          const float *rotations, const float *dL_dout, float *dL_drays,
                                                          void *workspace, size_t workspace_bytes, const long long *offsets,
                                                          const int *ids, long long ids_capacity, void *stream)
{
    const r2::Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    const r2::TileLists tl = { offsets, ids, ids_capacity };
    return r2::rays_backward("r2_project_gaussians_rays_backward_planned", &tl, V, H, W, rays, cone, cl, dL_dout, dL_drays, workspace,
                             workspace_bytes, stream);
}
