// gaussian_fisher.hip -- the diagonal of J^T W J of the exact projector: f[i][t] = the sum over the pixels of all views of
// w (d image / d theta_it)^2, for the eleven parameters of every Gaussian (include/r2hip.h: r2_project_gaussians_fisher; the
// per-pair arithmetic is gaussian_fisher.hpp's pair_squares on gaussian_rays.hpp).
//
// The skeleton of the projector's parameter backward (gaussian_skeleton.hpp: gauss_wave, rect_walk): Gaussian-major, one wave
// per Gaussian.  For each view in order the wave takes the Gaussian's detector rectangle -- the one the forward and the backward
// take (gauss_radius, gauss_rect), so a pair is squared exactly when the backward differentiates it -- and walks its pixels
// row-major, lane l taking pixels l, l + 64, ...; each lane keeps the eleven sums of its own pairs in registers, and one xor
// butterfly over the wave adds the 64 partial sums in a fixed order at the end.  Nobody else writes a Gaussian's row: no
// atomics, no workspace, the same bits on every call, and a Gaussian no ray touches (or one with a non-finite parameter) gets
// exact zeros.  A Gaussian that covers the whole detector costs its wave V H W pairs.
#include "gaussian_fisher.hpp"

namespace r2 {

namespace {

constexpr int FB = 256;   // threads per workgroup: four Gaussians

__global__ void __launch_bounds__(FB) gaussian_fisher_kernel(int V, int H, int W, const float *__restrict__ rays, int cone, Cloud cl,
                                                             const float *__restrict__ weights, CloudOut f)
{
    gauss_wave<FB>(cl, f, [&](const Gauss &a, const GaussRec &g, float radius, int lane, float *acc) {
        rect_walk(V, H, W, rays, cone, a, g, radius, lane, [&](const Ray &y, const GaussPair &p, size_t pix) {
            float o[NPAR];
            pair_squares(g, p, y, ray_length(y), a.s, a.q, o);
            const float w = weights ? weights[pix] : 1.0f;
#pragma unroll
            for (int t = 0; t < NPAR; ++t) acc[t] += w * o[t];
        });
    });
}

}  // namespace

}  // namespace r2

extern "C" int r2_project_gaussians_fisher(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                           const float *density, const float *scales, float scale_modifier,
                                           const float *rotations, const float *weights, float *f_means, float *f_density,
                                           float *f_scales, float *f_rotations, void *stream)
{
    using namespace r2;
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    const CloudOut f = { f_means, f_density, f_scales, f_rotations };
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays || cl.missing() || f.missing(P))
        return invalid_argument("r2_project_gaussians_fisher");
    if ((long long)H * W >= (1LL << 30) || P > CLOUD_MAX_P) {
        set_error("r2_project_gaussians_fisher: shape out of range (H %d, W %d, P %d)", H, W, P);
        return R2_ERR_INVALID;
    }
    if (P == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int per = FB / WAVE;
    gaussian_fisher_kernel<<<dim3((P + per - 1) / per), dim3(FB), 0, s>>>(V, H, W, rays, cone, cl, weights, f);
    R2_STAGE_CHECK(0, s, "project gaussians fisher");
    return 0;
}
