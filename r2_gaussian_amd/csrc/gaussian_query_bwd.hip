// gaussian_query_bwd.hip -- the gradients of r2_query_gaussians, given G = dL/dout (include/r2hip.h:
// r2_query_gaussians_backward): with respect to the means, densities, scales and quaternions, and to the points.
//
// Parameters, Gaussian-major: a first kernel writes the box of every block of 256 points (gaussian_points.hpp: block_box, the
// forward's) into the caller's workspace; then one wave per Gaussian tests the boxes 64 at a time against the Gaussian's
// sphere, walks the blocks that meet it in ascending order, lane l taking points l, l + 64, l + 128, l + 192 of a block, keeps
// the eleven sums of its own pairs in registers, and one xor butterfly over the wave adds the 64 partial sums in a fixed order
// at the end.  Box, sphere and pair are the forward's, so a pair is differentiated exactly when the forward summed it.  Nobody
// else writes a Gaussian's gradients: no atomics, the same bits on every call, exact zeros for a Gaussian no point touches (or
// one with a non-finite parameter).  A Gaussian whose sphere meets every block costs its wave N pairs.
// Points, point-major: the forward's skeleton with three sums per thread (gaussian_points.hpp: query_points_block<true>).
#include "gaussian_points.hpp"

namespace r2 {

namespace {

constexpr int PER = QB / WAVE;   // Gaussians per workgroup of the parameter kernel

__global__ void __launch_bounds__(QB) gaussian_query_boxes_kernel(int N, const float *__restrict__ points, BlockBox *__restrict__ boxes)
{
    __shared__ float wbox[QB / WAVE][6];
    const long long n = (long long)blockIdx.x * QB + threadIdx.x;
    float x = 0.f, y = 0.f, z = 0.f;
    if (n < N) {
        x = points[3 * n]; y = points[3 * n + 1]; z = points[3 * n + 2];
    }
    const BlockBox b = block_box(n < N && point_finite(x, y, z), x, y, z, wbox);
    if (threadIdx.x == 0) boxes[blockIdx.x] = b;
}

__global__ void __launch_bounds__(QB) gaussian_query_bwd_kernel(int N, const float *__restrict__ points, int P,
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
        const float r2 = radius * radius;
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
                    const float x = points[3 * n], y = points[3 * n + 1], z = points[3 * n + 2];
                    GaussPair p;
                    if (!point_finite(x, y, z) || !point_pair(g, r2, x, y, z, p)) continue;
                    float o[11];
                    point_pair_grad(g, p, x, y, z, G[n], s, q, o);
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

__global__ void __launch_bounds__(QB) gaussian_query_points_bwd_kernel(int N, const float *__restrict__ points, int P,
                                                                       const float *__restrict__ means,
                                                                       const float *__restrict__ density,
                                                                       const float *__restrict__ scales, float mod,
                                                                       const float *__restrict__ rotations,
                                                                       const float *__restrict__ G, float *__restrict__ d_points)
{
    query_points_block<true>(N, points, P, means, density, scales, mod, rotations, G, d_points);
}

}  // namespace

}  // namespace r2

extern "C" size_t r2_query_gaussians_workspace_bytes(int N) { return (size_t)r2::query_blocks(N) * sizeof(r2::BlockBox); }

extern "C" int r2_query_gaussians_backward(int N, const float *points, int P, const float *means, const float *density,
                                           const float *scales, float scale_modifier, const float *rotations, const float *dL_dout,
                                           float *dL_dmeans, float *dL_ddensity, float *dL_dscales, float *dL_drotations,
                                           float *dL_dpoints, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace r2;
    static_assert(sizeof(BlockBox) == 24, "the workspace is 24 bytes per block");
    if (N < 0 || P < 0 || (N > 0 && (!points || !dL_dout)) ||
        (P > 0 && (!means || !density || !scales || !rotations || !dL_dmeans || !dL_ddensity || !dL_dscales || !dL_drotations))) {
        set_error("r2_query_gaussians_backward: invalid argument");
        return R2_ERR_INVALID;
    }
    if (P > (1 << 29)) {
        set_error("r2_query_gaussians_backward: shape out of range (P %d)", P);
        return R2_ERR_INVALID;
    }
    const size_t need = r2_query_gaussians_workspace_bytes(N);
    if (need > 0 && (!workspace || workspace_bytes < need)) {
        set_error("r2_query_gaussians_backward: workspace of %zu bytes, %zu needed (r2_query_gaussians_workspace_bytes)",
                  workspace ? workspace_bytes : (size_t)0, need);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    if (P > 0) {
        BlockBox *boxes = (BlockBox *)workspace;
        if (N > 0) gaussian_query_boxes_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, points, boxes);
        gaussian_query_bwd_kernel<<<dim3((P + PER - 1) / PER), dim3(QB), 0, s>>>(N, points, P, means, density, scales,
                                                                                  scale_modifier, rotations, dL_dout, boxes, dL_dmeans,
                                                                                  dL_ddensity, dL_dscales, dL_drotations);
    }
    if (N > 0 && dL_dpoints)
        gaussian_query_points_bwd_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, points, P, means, density, scales,
                                                                                     scale_modifier, rotations, dL_dout, dL_dpoints);
    R2_STAGE_CHECK(0, s, "query gaussians backward");
    return 0;
}
