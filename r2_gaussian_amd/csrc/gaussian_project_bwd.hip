// gaussian_project_bwd.hip -- the gradients of r2_project_gaussians with respect to the means, densities, scales and
// quaternions, given G = dL/dout (include/r2hip.h: r2_project_gaussians_backward).
//
// Gaussian-major, on gaussian_skeleton.hpp's gauss_wave and rect_walk: one wave per Gaussian.  For each view in order the
// wave takes the Gaussian's detector rectangle -- the one the forward took (gaussian_rays.hpp: gauss_radius, gauss_rect), so a pair is differentiated exactly when the forward summed
// it -- and walks its pixels row-major, lane l taking pixels l, l + 64, ...; each lane keeps the eleven sums of its own pairs
// in registers, and one xor butterfly over the wave adds the 64 partial sums in a fixed order at the end.  Nobody else
// writes a Gaussian's gradients: no atomics, no workspace, the same bits on every call, and a Gaussian no ray touches (or
// one with a non-finite parameter) gets exact zeros.  A Gaussian that covers the whole detector costs its wave V H W pairs.
#include "gaussian_skeleton.hpp"

namespace r2 {

namespace {

constexpr int BB = 256;   // threads per workgroup: four Gaussians

__global__ void __launch_bounds__(BB) gaussian_project_bwd_kernel(int V, int H, int W, const float *__restrict__ rays, int cone,
                                                                  Cloud cl, const float *__restrict__ G, CloudOut d)
{
    gauss_wave<BB>(cl, d, [&](const Gauss &a, const GaussRec &g, float radius, int lane, float *acc) {
        rect_walk(V, H, W, rays, cone, a, g, radius, lane, [&](const Ray &y, const GaussPair &p, size_t pix) {
            float o[NPAR];
            gauss_pair_grad(g, p, y, ray_length(y), G[pix], a.s, a.q, o);
#pragma unroll
            for (int t = 0; t < NPAR; ++t) acc[t] += o[t];
        });
    });
}

}  // namespace

}  // namespace r2

extern "C" int r2_project_gaussians_backward(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                             const float *density, const float *scales, float scale_modifier,
                                             const float *rotations, const float *dL_dout, float *dL_dmeans, float *dL_ddensity,
                                             float *dL_dscales, float *dL_drotations, void *stream)
{
    using namespace r2;
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    const CloudOut d = { dL_dmeans, dL_ddensity, dL_dscales, dL_drotations };
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays || !dL_dout || cl.missing() || d.missing(P))
        return invalid_argument("r2_project_gaussians_backward");
    if ((long long)H * W >= (1LL << 30) || P > CLOUD_MAX_P) {
        set_error("r2_project_gaussians_backward: shape out of range (H %d, W %d, P %d)", H, W, P);
        return R2_ERR_INVALID;
    }
    if (P == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int per = BB / WAVE;
    gaussian_project_bwd_kernel<<<dim3((P + per - 1) / per), dim3(BB), 0, s>>>(V, H, W, rays, cone, cl, dL_dout, d);
    R2_STAGE_CHECK(0, s, "project gaussians backward");
    return 0;
}
