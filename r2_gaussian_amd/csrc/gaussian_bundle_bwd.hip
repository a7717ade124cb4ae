// gaussian_bundle_bwd.hip -- the gradients of r2_integrate_gaussians, given G = dL/dout (include/r2hip.h:
// r2_integrate_gaussians_backward): with respect to the means, densities, scales and quaternions, and to the rays.
//
// Parameters, Gaussian-major: after the cloud box (gaussian_bundle.hip) a kernel writes the box of every block of 256 rays
// (gaussian_bundle.hpp (1), (2): the forward's) into the caller's workspace; then one wave per Gaussian tests the boxes 64 at
// a time against the Gaussian's sphere, walks the blocks that meet it in ascending order, lane l taking rays l, l + 64,
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
    BundleRay b;
    b.y = Ray{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    b.len = 0.0f;
    b.valid = false;
    if (n < N) b = bundle_ray(rays, n);
    float v[6];
    bundle_ray_box(b, bundle_dir(b), half_line, cloud[0], v);
    const BlockBox box = bundle_box_reduce(v, wbox);
    if (threadIdx.x == 0) boxes[blockIdx.x] = box;
}

__global__ void __launch_bounds__(QB) gaussian_bundle_bwd_kernel(int N, const float *__restrict__ rays, int half_line, int P,
                                                                 const float *__restrict__ means, const float *__restrict__ density,
                                                                 const float *__restrict__ scales, float mod,
                                                                 const float *__restrict__ rotations, const float *__restrict__ G,
                                                                 const BlockBox *__restrict__ boxes, float *__restrict__ d_means,
                                                                 float *__restrict__ d_density, float *__restrict__ d_scales,
                                                                 float *__restrict__ d_rotations)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int i = blockIdx.x * PER + threadIdx.x / WAVE;   // wave-uniform
    if (i >= P) return;
    const float mx = means[3 * i], my = means[3 * i + 1], mz = means[3 * i + 2], rho = density[i];
    const float s[3] = { scales[3 * i], scales[3 * i + 1], scales[3 * i + 2] };
    const float4 q = make_float4(rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3]);
    float acc[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) acc[k] = 0.0f;
    const float radius = gauss_radius(mx, my, mz, rho, s[0], s[1], s[2], mod, q);
    if (radius >= 0.0f) {
        const GaussRec g = gauss_rec(mx, my, mz, rho, s[0], s[1], s[2], mod, q);
        const int NB = query_blocks(N);
        for (int base = 0; base < NB; base += WAVE) {
            const int b = base + lane;
            unsigned long long mask = __ballot(b < NB && box_meets_sphere(boxes[b < NB ? b : 0], mx, my, mz, radius));
            while (mask) {   // wave-uniform: the blocks that meet the sphere, ascending
                const int hit = base + __ffsll((long long)mask) - 1;
                mask &= mask - 1ull;
#pragma unroll 1
                for (int k = 0; k < QB / WAVE; ++k) {
                    const long long n = (long long)hit * QB + k * WAVE + lane;
                    if (n >= N) continue;
                    const BundleRay y = bundle_ray(rays, n);
                    if (!y.valid || bundle_line_misses(y, bundle_dir(y), mx, my, mz, radius)) continue;
                    GaussPair p;
                    if (!bundle_pair(g, y.y, half_line, p)) continue;
                    float o[11];
                    gauss_pair_grad(g, p, y.y, y.len, G[n], s, q, o);
#pragma unroll
                    for (int t = 0; t < 11; ++t) acc[t] += o[t];
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 11; ++t)
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) acc[t] += __shfl_xor(acc[t], d);
    if (lane == 0) {
        d_means[3 * i] = acc[0]; d_means[3 * i + 1] = acc[1]; d_means[3 * i + 2] = acc[2];
        d_density[i] = acc[3];
        d_scales[3 * i] = acc[4]; d_scales[3 * i + 1] = acc[5]; d_scales[3 * i + 2] = acc[6];
        d_rotations[4 * i] = acc[7]; d_rotations[4 * i + 1] = acc[8]; d_rotations[4 * i + 2] = acc[9];
        d_rotations[4 * i + 3] = acc[10];
    }
}

__global__ void __launch_bounds__(QB) gaussian_bundle_rays_bwd_kernel(int N, const float *__restrict__ rays, int half_line, int P,
                                                                      const float *__restrict__ means,
                                                                      const float *__restrict__ density,
                                                                      const float *__restrict__ scales, float mod,
                                                                      const float *__restrict__ rotations,
                                                                      const float *__restrict__ G, const BlockBox *__restrict__ cloud,
                                                                      float *__restrict__ d_rays)
{
    integrate_rays_block<true>(N, rays, half_line, P, means, density, scales, mod, rotations, G, cloud, d_rays);
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
    if (N < 0 || P < 0 || (N > 0 && (!rays || !dL_dout)) ||
        (P > 0 && (!means || !density || !scales || !rotations || !dL_dmeans || !dL_ddensity || !dL_dscales || !dL_drotations))) {
        set_error("r2_integrate_gaussians_backward: invalid argument");
        return R2_ERR_INVALID;
    }
    if (P > (1 << 29)) {
        set_error("r2_integrate_gaussians_backward: shape out of range (P %d)", P);
        return R2_ERR_INVALID;
    }
    const size_t need = r2_integrate_gaussians_workspace_bytes(N, P);
    if (need > 0 && (!workspace || workspace_bytes < need)) {
        set_error("r2_integrate_gaussians_backward: workspace of %zu bytes, %zu needed (r2_integrate_gaussians_workspace_bytes)",
                  workspace ? workspace_bytes : (size_t)0, need);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    BlockBox *cloud = (BlockBox *)workspace;
    if (P > 0) {
        BlockBox *boxes = N > 0 ? cloud + 1 + bundle_parts(P) : nullptr;   // N = 0: no block, no workspace
        if (N > 0) {
            bundle_cloud_box(P, means, density, scales, scale_modifier, rotations, cloud, s);
            gaussian_bundle_boxes_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, rays, half_line, cloud, boxes);
        }
        gaussian_bundle_bwd_kernel<<<dim3((P + PER - 1) / PER), dim3(QB), 0, s>>>(N, rays, half_line, P, means, density, scales,
                                                                                   scale_modifier, rotations, dL_dout, boxes,
                                                                                   dL_dmeans, dL_ddensity, dL_dscales, dL_drotations);
    }
    if (N > 0 && dL_drays)
        gaussian_bundle_rays_bwd_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, rays, half_line, P, means, density, scales,
                                                                                    scale_modifier, rotations, dL_dout, cloud, dL_drays);
    R2_STAGE_CHECK(0, s, "integrate gaussians backward");
    return 0;
}
