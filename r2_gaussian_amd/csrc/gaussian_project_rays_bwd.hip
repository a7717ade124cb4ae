// gaussian_project_rays_bwd.hip -- the gradient of r2_project_gaussians with respect to its rays [V,12], given G = dL/dout
// (include/r2hip.h: r2_project_gaussians_rays_backward; the per-pair arithmetic is gaussian_ray_grad.hpp's on top of
// gaussian_rays.hpp's pair, rectangle and cone rule, so a pair is differentiated exactly when the forward summed it).
//
// Pixel-major, on the forward's skeleton (gaussian_project.hip): one workgroup per 16 x 16 pixel tile and view, one thread per
// pixel; the P Gaussians are walked 256 per round, thread i tests the rectangle of Gaussian base + i against the tile, the hits
// are compacted IN ORDER into an LDS batch, and every pixel adds the batch's pairs whose rectangle holds it to its six sums
// g_s, g_d -- in ascending Gaussian index, in one thread.  At the end a pixel forms its twelve contributions, the workgroup adds
// the 256 x 12 values in one fixed order (gaussian_ray_grad.hpp: block_sum12) and writes partial[view][tile][12] into the
// caller's workspace.  A second kernel, one workgroup per view, adds that view's tile partials -- thread t tiles t, t + 256, ...
// in ascending order, then the same fixed-order sum -- and writes dL_drays[view].  No atomics, no allocation and no host
// synchronisation, the same bits on every call, and nothing a view computes depends on another view.
#include "gaussian_ray_grad.hpp"

namespace r2 {

namespace {

struct Staged {
    GaussRec g;
    PixRect q;
};

__global__ void __launch_bounds__(RG) gaussian_project_rays_bwd_kernel(int H, int W, const float *__restrict__ rays, int cone, int P,
                                                                       const float *__restrict__ means,
                                                                       const float *__restrict__ density,
                                                                       const float *__restrict__ scales, float mod,
                                                                       const float *__restrict__ rotations,
                                                                       const float *__restrict__ G, float *__restrict__ partial)
{
    static_assert(RG == TILE2D * TILE2D, "one thread per pixel of a tile");
    __shared__ ViewGeom vg;
    __shared__ Staged st[RG];
    __shared__ int wcount[RG / WAVE];
    __shared__ float wsum[RG / WAVE][12];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int view = blockIdx.z;
    const int tc0 = blockIdx.x * TILE2D, tr0 = blockIdx.y * TILE2D;
    const int tc1 = min(tc0 + TILE2D, W) - 1, tr1 = min(tr0 + TILE2D, H) - 1;
    const int c = tc0 + (tid & (TILE2D - 1)), r = tr0 + tid / TILE2D;
    const bool inside = c < W && r < H;
    const float *R = rays + 12 * view;
    if (tid == 0) vg = view_geom(R, cone);
    __syncthreads();
    const Ray y = pixel_ray(R, cone, r, c);
    const float len = ray_length(y);
    const float Gp = inside ? G[((size_t)view * H + r) * W + c] : 0.0f;
    float gs[3] = { 0.f, 0.f, 0.f }, gd[3] = { 0.f, 0.f, 0.f };
    for (int base = 0; base < P; base += RG) {
        const int i = base + tid;
        bool hit = false;
        float mx = 0.f, my = 0.f, mz = 0.f, rho = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        PixRect rc;
        if (i < P) {
            mx = means[3 * i]; my = means[3 * i + 1]; mz = means[3 * i + 2];
            rho = density[i];
            sx = scales[3 * i]; sy = scales[3 * i + 1]; sz = scales[3 * i + 2];
            q = make_float4(rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3]);
            const float radius = gauss_radius(mx, my, mz, rho, sx, sy, sz, mod, q);
            if (radius >= 0.0f && gauss_rect(vg, cone, mx, my, mz, radius, H, W, rc))
                hit = rc.c0 <= tc1 && rc.c1 >= tc0 && rc.r0 <= tr1 && rc.r1 >= tr0;
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) wcount[wave] = __popcll(mask);
        __syncthreads();
        int slot = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < RG / WAVE; ++w) {
            if (w < wave) slot += wcount[w];
            total += wcount[w];
        }
        if (hit) {
            st[slot].g = gauss_rec(mx, my, mz, rho, sx, sy, sz, mod, q);
            st[slot].q = rc;
        }
        __syncthreads();
        if (inside) {
            for (int j = 0; j < total; ++j) {
                const PixRect &b = st[j].q;
                if (c < b.c0 || c > b.c1 || r < b.r0 || r > b.r1) continue;
                GaussPair p;
                if (gauss_pair(st[j].g, y, cone, p)) gauss_pair_ray_grad(st[j].g, p, y, len, Gp, gs, gd);
            }
        }
        __syncthreads();   // the batch and the wave counts are rewritten by the next round
    }
    float o[12];   // a thread outside the detector has added nothing: twelve zeros
    pixel_ray_grad(cone, r, c, gs, gd, o);
    block_sum12(o, wsum);
    if (tid == 0) {
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        float *dst = partial + ((size_t)view * gridDim.x * gridDim.y + tile) * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) dst[k] = o[k];
    }
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
    using namespace r2;
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays || !dL_dout || !dL_drays ||
        (P > 0 && (!means || !density || !scales || !rotations))) {
        set_error("r2_project_gaussians_rays_backward: invalid argument");
        return R2_ERR_INVALID;
    }
    if (V > 65535 || (H + TILE2D - 1) / TILE2D > 65535 || (long long)H * W >= (1LL << 30) || P > (1 << 29)) {
        set_error("r2_project_gaussians_rays_backward: shape out of range (V %d, H %d, W %d, P %d)", V, H, W, P);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) {
        R2_HIP_TRY(hipMemsetAsync(dL_drays, 0, (size_t)V * 12 * sizeof(float), s));
        return 0;
    }
    const size_t need = r2_project_gaussians_rays_backward_workspace_bytes(V, H, W);
    if (!workspace || workspace_bytes < need) {
        set_error("r2_project_gaussians_rays_backward: workspace of %zu bytes, %zu needed "
                  "(r2_project_gaussians_rays_backward_workspace_bytes)", workspace ? workspace_bytes : (size_t)0, need);
        return R2_ERR_INVALID;
    }
    const dim3 grid((W + TILE2D - 1) / TILE2D, (H + TILE2D - 1) / TILE2D, V);
    float *partial = (float *)workspace;
    gaussian_project_rays_bwd_kernel<<<grid, dim3(RG), 0, s>>>(H, W, rays, cone, P, means, density, scales, scale_modifier,
                                                               rotations, dL_dout, partial);
    gaussian_project_rays_reduce_kernel<<<dim3(V), dim3(RG), 0, s>>>((int)tiles_of(H, W), partial, dL_drays);
    R2_STAGE_CHECK(0, s, "project gaussians rays backward");
    return 0;
}
