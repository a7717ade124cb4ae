// gaussian_query_bwd.hip -- the gradients of r2_query_gaussians, given G = dL/dout (include/r2hip.h:
// r2_query_gaussians_backward): with respect to the means, densities, scales and quaternions, and to the points.
//
// Parameters, Gaussian-major: a first kernel writes the box of every block of 256 points (gaussian_points.hpp: block_box, the
// forward's) into the caller's workspace; then one wave per Gaussian (gaussian_skeleton.hpp: gauss_wave, hit_block_walk)
// tests the boxes 64 at a time against the Gaussian's sphere, walks the blocks that meet it in ascending order, lane l taking points l, l + 64, l + 128, l + 192 of a block, keeps
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

__global__ void __launch_bounds__(QB) gaussian_query_bwd_kernel(int N, const float *__restrict__ points, Cloud cl,
                                                                const float *__restrict__ G, const BlockBox *__restrict__ boxes,
                                                                CloudOut d)
{
    gauss_wave<QB>(cl, d, [&](const Gauss &a, const GaussRec &g, float radius, int lane, float *acc) {
        const float r2 = radius * radius;
        hit_block_walk<QB>(
            N, query_blocks(N), lane, [&](int b) { return box_meets_sphere(boxes[b], a.mx, a.my, a.mz, radius); },
            [&](long long n) {
                const float x = points[3 * n], y = points[3 * n + 1], z = points[3 * n + 2];
                GaussPair p;
                if (!point_finite(x, y, z) || !point_pair(g, r2, x, y, z, p)) return;
                float o[NPAR];
                point_pair_grad(g, p, x, y, z, G[n], a.s, a.q, o);
#pragma unroll
                for (int t = 0; t < NPAR; ++t) acc[t] += o[t];
            });
    });
}

__global__ void __launch_bounds__(QB) gaussian_query_points_bwd_kernel(int N, const float *__restrict__ points, Cloud cl,
                                                                       const float *__restrict__ G, float *__restrict__ d_points)
{
    query_points_block<true>(N, points, cl, G, d_points);
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
    const char *entry = "r2_query_gaussians_backward";
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    const CloudOut d = { dL_dmeans, dL_ddensity, dL_dscales, dL_drotations };
    if (N < 0 || P < 0 || (N > 0 && (!points || !dL_dout)) || cl.missing() || d.missing(P)) return invalid_argument(entry);
    if (cloud_too_large(entry, P)) return R2_ERR_INVALID;
    const size_t need = r2_query_gaussians_workspace_bytes(N);
    if (workspace_too_small(entry, "r2_query_gaussians_workspace_bytes", workspace, workspace_bytes, need)) return R2_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (P > 0) {
        BlockBox *boxes = (BlockBox *)workspace;
        if (N > 0) gaussian_query_boxes_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, points, boxes);
        gaussian_query_bwd_kernel<<<dim3((P + PER - 1) / PER), dim3(QB), 0, s>>>(N, points, cl, dL_dout, boxes, d);
    }
    if (N > 0 && dL_dpoints)
        gaussian_query_points_bwd_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, points, cl, dL_dout, dL_dpoints);
    R2_STAGE_CHECK(0, s, "query gaussians backward");
    return 0;
}
