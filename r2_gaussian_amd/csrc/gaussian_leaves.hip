// gaussian_leaves.hip -- the exact line integrals of a Gaussian cloud along caller-supplied rays, culled by leaves of 64
// consecutive Gaussians: out[n] = the sum over the Gaussians of rho sqrt(2 pi / A) exp(-q / 2) |d| along ray n = (s, d)
// (include/r2hip.h: r2_integrate_gaussians_leaves; the rule is gaussian_bundle.hpp's, the leaf box, the leaf test and the
// skeleton of the kernel are gaussian_leaves.hpp's, shared with the backward, which runs the same skeleton with six sums for
// the ray gradient).
//
// Two launches on the caller's stream: the prepare kernel, the rays.  No atomics, no list in memory, no allocation and no
// host synchronisation, the same bits on every call.
#include "gaussian_leaves.hpp"

namespace r2 {

namespace {

// One thread per Gaussian, one wave per leaf: the float4 {mean, radius} of the Gaussian, its record S^-1 R^T when it has a
// radius, and, by a min / max butterfly over the wave, the box of the leaf's spheres (gaussian_leaves.hpp).  min and max are
// exact, so no order matters.
__global__ void __launch_bounds__(QB) gaussian_leaves_prepare_kernel(Cloud cl, float4 *__restrict__ cent, GaussRec *__restrict__ recs,
                                                                     BlockBox *__restrict__ boxes)
{
    const int P = cl.P;
    const int lane = threadIdx.x & (WAVE - 1);
    const int leaf = blockIdx.x * LV + threadIdx.x / WAVE;   // wave-uniform
    const int i = leaf * LEAF + lane;                        // < 2^29 + 256
    float v[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    if (i < P) {
        const Gauss a = load_gauss(cl, i);
        const float m[3] = { a.mx, a.my, a.mz };
        const float r = gauss_radius(a, cl.mod);
        const bool live = r >= 0.0f;
        cent[i] = make_float4(m[0], m[1], m[2], live ? r : -1.0f);
        if (live) {
            recs[i] = gauss_rec(a, cl.mod);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v[k] = m[k] - r;
                v[3 + k] = m[k] + r;
            }
        }
    }
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = fminf(v[k], __shfl_xor(v[k], d));
            v[3 + k] = fmaxf(v[3 + k], __shfl_xor(v[3 + k], d));
        }
    if (lane == 0 && leaf < leaf_count(P)) {
        BlockBox b;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            b.lo[k] = v[k];
            b.hi[k] = v[3 + k];
        }
        boxes[leaf] = b;
    }
}

__global__ void __launch_bounds__(QB) gaussian_leaves_kernel(int N, const float *__restrict__ rays, int half_line, int P,
                                                             const float4 *__restrict__ cent, const GaussRec *__restrict__ recs,
                                                             const BlockBox *__restrict__ boxes, float *__restrict__ out)
{
    integrate_ray_wave<false>(N, rays, half_line, P, nullptr, cent, recs, boxes, out);
}

}  // namespace

void leaves_prepare(const Cloud &cl, float4 *cent, GaussRec *recs, BlockBox *boxes, hipStream_t s)
{
    gaussian_leaves_prepare_kernel<<<dim3((leaf_count(cl.P) + LV - 1) / LV), dim3(QB), 0, s>>>(cl, cent, recs, boxes);
}

}  // namespace r2

extern "C" size_t r2_integrate_gaussians_leaves_workspace_bytes(int N, int P) { return r2::leaves_workspace_bytes(N, P); }

extern "C" int r2_integrate_gaussians_leaves(int N, const float *rays, int half_line, int P, const float *means,
                                             const float *density, const float *scales, float scale_modifier,
                                             const float *rotations, float *out, void *workspace, size_t workspace_bytes,
                                             void *stream)
{
    using namespace r2;
    static_assert(sizeof(BlockBox) == 24 && sizeof(float4) == 16 && sizeof(GaussRec) == 64, "the workspace is 80 bytes per Gaussian and 24 per leaf");
    const char *entry = "r2_integrate_gaussians_leaves";
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    if (N < 0 || P < 0 || (N > 0 && (!rays || !out)) || (N > 0 && cl.missing())) return invalid_argument(entry);
    if (cloud_too_large(entry, P)) return R2_ERR_INVALID;
    if (N == 0) return 0;
    const size_t need = r2_integrate_gaussians_leaves_workspace_bytes(N, P);
    if (leaves_workspace_refused(entry, workspace, workspace_bytes, need)) return R2_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    float4 *cent = (float4 *)workspace;
    GaussRec *recs = P > 0 ? leaves_recs(workspace, P) : nullptr;
    BlockBox *boxes = P > 0 ? leaves_boxes(workspace, P) : nullptr;
    if (P > 0) leaves_prepare(cl, cent, recs, boxes, s);
    gaussian_leaves_kernel<<<dim3((unsigned)(((long long)N + LV - 1) / LV)), dim3(QB), 0, s>>>(N, rays, half_line, P, cent, recs, boxes, out);
    R2_STAGE_CHECK(0, s, "integrate gaussians leaves");
    return 0;
}
