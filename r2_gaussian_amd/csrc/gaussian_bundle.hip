// gaussian_bundle.hip -- the exact line integrals of a Gaussian cloud along caller-supplied rays: out[n] = the sum over the
// Gaussians of rho sqrt(2 pi / A) exp(-q / 2) |d| along ray n = (s, d) (include/r2hip.h: r2_integrate_gaussians; the rule, the
// culling tests with their rounding allowances and the skeleton of the kernel are gaussian_bundle.hpp's, shared with the
// backward, which runs the same skeleton with six sums for the ray gradient).
//
// Three launches on the caller's stream: the partial cloud boxes, their reduction, the rays.  No atomics, no list in memory,
// no allocation and no host synchronisation, the same bits on every call.
#include "gaussian_bundle.hpp"

namespace r2 {

// The cloud box (gaussian_bundle.hpp (0)) into boxes[0], through the partial boxes boxes[1 .. parts].  Defined here, used by
// the backward as well.
__global__ void __launch_bounds__(QB) bundle_cloud_parts_kernel(int P, const float *__restrict__ means,
                                                                const float *__restrict__ density,
                                                                const float *__restrict__ scales, float mod,
                                                                const float *__restrict__ rotations, BlockBox *__restrict__ boxes)
{
    __shared__ float wbox[QB / WAVE][6];
    float v[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    for (int i = blockIdx.x * QB + threadIdx.x; i < P; i += gridDim.x * QB) {   // i + the stride stays below 2^30
        const float m[3] = { means[3 * i], means[3 * i + 1], means[3 * i + 2] };
        const float4 q = make_float4(rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3]);
        const float radius = gauss_radius(m[0], m[1], m[2], density[i], scales[3 * i], scales[3 * i + 1], scales[3 * i + 2], mod, q);
        if (!(radius >= 0.0f)) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = fminf(v[k], m[k] - radius);
            v[3 + k] = fmaxf(v[3 + k], m[k] + radius);
        }
    }
    const BlockBox b = bundle_box_reduce(v, wbox);
    if (threadIdx.x == 0) boxes[1 + blockIdx.x] = b;
}

__global__ void __launch_bounds__(QB) bundle_cloud_box_kernel(int parts, BlockBox *__restrict__ boxes)
{
    __shared__ float wbox[QB / WAVE][6];
    float v[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    for (int i = threadIdx.x; i < parts; i += QB) {
        const BlockBox p = boxes[1 + i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = fminf(v[k], p.lo[k]);
            v[3 + k] = fmaxf(v[3 + k], p.hi[k]);
        }
    }
    const BlockBox b = bundle_box_reduce(v, wbox);
    if (threadIdx.x == 0) boxes[0] = b;
}

void bundle_cloud_box(int P, const float *means, const float *density, const float *scales, float mod, const float *rotations,
                      BlockBox *boxes, hipStream_t s)
{
    const int parts = bundle_parts(P);
    bundle_cloud_parts_kernel<<<dim3(parts), dim3(QB), 0, s>>>(P, means, density, scales, mod, rotations, boxes);
    bundle_cloud_box_kernel<<<dim3(1), dim3(QB), 0, s>>>(parts, boxes);
}

namespace {

__global__ void __launch_bounds__(QB) gaussian_bundle_kernel(int N, const float *__restrict__ rays, int half_line, int P,
                                                             const float *__restrict__ means, const float *__restrict__ density,
                                                             const float *__restrict__ scales, float mod,
                                                             const float *__restrict__ rotations,
                                                             const BlockBox *__restrict__ cloud, float *__restrict__ out)
{
    integrate_rays_block<false>(N, rays, half_line, P, means, density, scales, mod, rotations, nullptr, cloud, out);
}

}  // namespace

}  // namespace r2

extern "C" size_t r2_integrate_gaussians_workspace_bytes(int N, int P)
{
    return r2::bundle_workspace_boxes(N, P) * sizeof(r2::BlockBox);
}

extern "C" int r2_integrate_gaussians(int N, const float *rays, int half_line, int P, const float *means, const float *density,
                                      const float *scales, float scale_modifier, const float *rotations, float *out,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace r2;
    static_assert(sizeof(BlockBox) == 24, "the workspace is 24 bytes per box");
    if (N < 0 || P < 0 || (N > 0 && (!rays || !out)) || (N > 0 && P > 0 && (!means || !density || !scales || !rotations))) {
        set_error("r2_integrate_gaussians: invalid argument");
        return R2_ERR_INVALID;
    }
    if (P > (1 << 29)) {
        set_error("r2_integrate_gaussians: shape out of range (P %d)", P);
        return R2_ERR_INVALID;
    }
    if (N == 0) return 0;
    const size_t need = r2_integrate_gaussians_workspace_bytes(N, P);
    if (need > 0 && (!workspace || workspace_bytes < need)) {
        set_error("r2_integrate_gaussians: workspace of %zu bytes, %zu needed (r2_integrate_gaussians_workspace_bytes)",
                  workspace ? workspace_bytes : (size_t)0, need);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    BlockBox *boxes = (BlockBox *)workspace;
    if (P > 0) bundle_cloud_box(P, means, density, scales, scale_modifier, rotations, boxes, s);
    gaussian_bundle_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, rays, half_line, P, means, density, scales, scale_modifier,
                                                                          rotations, boxes, out);
    R2_STAGE_CHECK(0, s, "integrate gaussians");
    return 0;
}
