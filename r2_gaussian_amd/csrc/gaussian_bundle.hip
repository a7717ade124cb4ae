// gaussian_bundle.hip -- the exact line integrals of a Gaussian cloud along caller-supplied rays: out[n] = the sum over the
// Gaussians of rho sqrt(2 pi / A) exp(-q / 2) |d| along ray n = (s, d) (include/r2hip.h: r2_integrate_gaussians; the rule, the
// culling tests with their rounding allowances and the kernel's body are gaussian_bundle.hpp's, shared with the
// backward, which runs the same skeleton with six sums for the ray gradient).
//
// Three launches on the caller's stream: the partial cloud boxes, their reduction, the rays.  No atomics, no list in memory,
// no allocation and no host synchronisation, the same bits on every call.
#include "gaussian_bundle.hpp"

namespace r2 {

// The cloud box (gaussian_bundle.hpp (0)) into boxes[0], through the partial boxes boxes[1 .. parts].  Defined here, used by
// the backward as well.
__global__ void __launch_bounds__(QB) bundle_cloud_parts_kernel(Cloud cl, BlockBox *__restrict__ boxes)
{
    __shared__ float wbox[QB / WAVE][6];
    float v[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    for (int i = blockIdx.x * QB + threadIdx.x; i < cl.P; i += gridDim.x * QB) {   // i + the stride stays below 2^30
        const Gauss a = load_gauss(cl, i);
        const float m[3] = { a.mx, a.my, a.mz };
        const float radius = gauss_radius(a, cl.mod);
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

void bundle_cloud_box(const Cloud &cl, BlockBox *boxes, hipStream_t s)
{
    const int parts = bundle_parts(cl.P);
    bundle_cloud_parts_kernel<<<dim3(parts), dim3(QB), 0, s>>>(cl, boxes);
    bundle_cloud_box_kernel<<<dim3(1), dim3(QB), 0, s>>>(parts, boxes);
}

namespace {

// This kernel alone keeps the cloud as six parameters and forms its Cloud inside: by value the four pointers lose their
// __restrict__, and the same instructions, scheduled differently, ran a whole view in tile order 2 % slower on an MI355X.
__global__ void __launch_bounds__(QB) gaussian_bundle_kernel(int N, const float *__restrict__ rays, int half_line, int P,
                                                             const float *__restrict__ means, const float *__restrict__ density,
                                                             const float *__restrict__ scales, float mod,
                                                             const float *__restrict__ rotations,
                                                             const BlockBox *__restrict__ cloud, float *__restrict__ out)
{
    const Cloud cl = { P, means, density, scales, mod, rotations };
    integrate_rays_block<false>(N, rays, half_line, cl, nullptr, cloud, out);
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
    const char *entry = "r2_integrate_gaussians";
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    if (N < 0 || P < 0 || (N > 0 && (!rays || !out)) || (N > 0 && cl.missing())) return invalid_argument(entry);
    if (cloud_too_large(entry, P)) return R2_ERR_INVALID;
    if (N == 0) return 0;
    const size_t need = r2_integrate_gaussians_workspace_bytes(N, P);
    if (workspace_too_small(entry, "r2_integrate_gaussians_workspace_bytes", workspace, workspace_bytes, need)) return R2_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    BlockBox *boxes = (BlockBox *)workspace;
    if (P > 0) bundle_cloud_box(cl, boxes, s);
    gaussian_bundle_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, rays, half_line, P, means, density, scales, scale_modifier,
                                                                          rotations, boxes, out);
    R2_STAGE_CHECK(0, s, "integrate gaussians");
    return 0;
}
