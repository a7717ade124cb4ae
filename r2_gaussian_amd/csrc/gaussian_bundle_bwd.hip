// gaussian_bundle_bwd.hip -- the gradients of r2_integrate_gaussians, given G = dL/dout (include/r2hip.h:
// r2_integrate_gaussians_backward): with respect to the means, densities, scales and quaternions, and to the rays.
//
// Parameters, Gaussian-major: after the cloud box (gaussian_bundle.hip) a kernel writes the box of every block of 256 rays
// (gaussian_bundle.hpp (1), (2): the forward's) into the caller's workspace; then one wave per Gaussian
// (gaussian_skeleton.hpp: gauss_wave, hit_block_walk) tests the boxes 64 at a time against the Gaussian's sphere, walks the blocks that meet it in ascending order, lane l taking rays l, l + 64,
// l + 128, l + 192 of a block, keeps the eleven sums of its own pairs in registers, and one xor butterfly over the wave adds
// the 64 partial sums in a fixed order at the end.  The rule is the forward's, so a pair is differentiated exactly when the
// forward summed it; the culling tests change no bit.  Nobody else writes a Gaussian's gradients: no atomics, the same bits on
// every call, exact zeros for a Gaussian no ray touches (or one with a non-finite parameter).
// Rays, ray-major: the forward's skeleton with six sums per thread (gaussian_bundle.hpp: integrate_rays_block<true>).
#include "gaussian_bundle.hpp"

namespace r2 {

namespace {

constexpr int PER = QB / WAVE;   // Gaussians per workgroup of the parameter kernel

__global__ void __launch_bounds__(QB) gaussian_bundle_boxes_kernel(int N, const float *__restrict__ rays, int half_line,
                                                                   const BlockBox *__restrict__ cloud, BlockBox *__restrict__ boxes)
{
    __shared__ float wbox[QB / WAVE][6];
    const long long n = (long long)blockIdx.x * QB + threadIdx.x;
    const BundleRay b = bundle_ray(rays, n, N);
    float v[6];
    bundle_ray_box(b, bundle_dir(b), half_line, cloud[0], v);
    const BlockBox box = bundle_box_reduce(v, wbox);
    if (threadIdx.x == 0) boxes[blockIdx.x] = box;
}

__global__ void __launch_bounds__(QB) gaussian_bundle_bwd_kernel(int N, const float *__restrict__ rays, int half_line, Cloud cl,
                                                                 const float *__restrict__ G, const BlockBox *__restrict__ boxes,
                                                                 CloudOut d)
{
    gauss_wave<QB>(cl, d, [&](const Gauss &a, const GaussRec &g, float radius, int lane, float *acc) {
        hit_block_walk<QB>(
            N, query_blocks(N), lane, [&](int b) { return box_meets_sphere(boxes[b], a.mx, a.my, a.mz, radius); },
            [&](long long n) {
                const BundleRay y = bundle_ray(rays, n);
                if (!y.valid || bundle_line_misses(y, bundle_dir(y), a.mx, a.my, a.mz, radius)) return;
                GaussPair p;
                if (!bundle_pair(g, y.y, half_line, p)) return;
                float o[NPAR];
                gauss_pair_grad(g, p, y.y, y.len, G[n], a.s, a.q, o);
#pragma unroll
                for (int t = 0; t < NPAR; ++t) acc[t] += o[t];
            });
    });
}

__global__ void __launch_bounds__(QB) gaussian_bundle_rays_bwd_kernel(int N, const float *__restrict__ rays, int half_line, Cloud cl,
                                                                      const float *__restrict__ G, const BlockBox *__restrict__ cloud,
                                                                      float *__restrict__ d_rays)
{
    integrate_rays_block<true>(N, rays, half_line, cl, G, cloud, d_rays);
}

}  // namespace

}  // namespace r2

extern "C" int r2_integrate_gaussians_backward(int N, const float *rays, int half_line, int P, const float *means,
                                               const float *density, const float *scales, float scale_modifier,
                                               const float *rotations, const float *dL_dout, float *dL_dmeans, float *dL_ddensity,
                                               float *dL_dscales, float *dL_drotations, float *dL_drays, void *workspace,
                                               size_t workspace_bytes, void *stream)
{
    using namespace r2;
    static_assert(sizeof(BlockBox) == 24, "the workspace is 24 bytes per box");
    const char *entry = "r2_integrate_gaussians_backward";
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    const CloudOut d = { dL_dmeans, dL_ddensity, dL_dscales, dL_drotations };
    if (N < 0 || P < 0 || (N > 0 && (!rays || !dL_dout)) || cl.missing() || d.missing(P)) return invalid_argument(entry);
    if (cloud_too_large(entry, P)) return R2_ERR_INVALID;
    const size_t need = r2_integrate_gaussians_workspace_bytes(N, P);
    if (workspace_too_small(entry, "r2_integrate_gaussians_workspace_bytes", workspace, workspace_bytes, need)) return R2_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    BlockBox *cloud = (BlockBox *)workspace;
    if (P > 0) {
        BlockBox *boxes = N > 0 ? cloud + 1 + bundle_parts(P) : nullptr;   // N = 0: no block, no workspace
        if (N > 0) {
            bundle_cloud_box(cl, cloud, s);
            gaussian_bundle_boxes_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, rays, half_line, cloud, boxes);
        }
        gaussian_bundle_bwd_kernel<<<dim3((P + PER - 1) / PER), dim3(QB), 0, s>>>(N, rays, half_line, cl, dL_dout, boxes, d);
    }
    if (N > 0 && dL_drays)
        gaussian_bundle_rays_bwd_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, rays, half_line, cl, dL_dout, cloud, dL_drays);
    R2_STAGE_CHECK(0, s, "integrate gaussians backward");
    return 0;
}
