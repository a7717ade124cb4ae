// gaussian_fisher.hip -- the diagonal of J^T W J of the exact projector: f[i][t] = the sum over the pixels of all views of
// w (d image / d theta_it)^2, for the eleven parameters of every Gaussian (include/r2hip.h: r2_project_gaussians_fisher; the
// per-pair arithmetic is gaussian_fisher.hpp's pair_squares on gaussian_rays.hpp).
//
// The skeleton of the projector's parameter backward (gaussian_project_bwd.hip), restated: Gaussian-major, one wave per
// Gaussian.  For each view in order the wave takes the Gaussian's detector rectangle -- the one the forward and the backward
// take (gauss_radius, gauss_rect), so a pair is squared exactly when the backward differentiates it -- and walks its pixels
// row-major, lane l taking pixels l, l + 64, ...; each lane keeps the eleven sums of its own pairs in registers, and one xor
// butterfly over the wave adds the 64 partial sums in a fixed order at the end.  Nobody else writes a Gaussian's row: no
// atomics, no workspace, the same bits on every call, and a Gaussian no ray touches (or one with a non-finite parameter) gets
// exact zeros.  A Gaussian that covers the whole detector costs its wave V H W pairs.
#include "gaussian_fisher.hpp"

namespace r2 {

namespace {

constexpr int FB = 256;   // threads per workgroup: four Gaussians

__global__ void __launch_bounds__(FB) gaussian_fisher_kernel(int V, int H, int W, const float *__restrict__ rays, int cone, int P,
                                                             const float *__restrict__ means, const float *__restrict__ density,
                                                             const float *__restrict__ scales, float mod,
                                                             const float *__restrict__ rotations, const float *__restrict__ weights,
                                                             float *__restrict__ f_means, float *__restrict__ f_density,
                                                             float *__restrict__ f_scales, float *__restrict__ f_rotations)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int i = blockIdx.x * (FB / WAVE) + threadIdx.x / WAVE;   // wave-uniform
    if (i >= P) return;
    const float mx = means[3 * i], my = means[3 * i + 1], mz = means[3 * i + 2], rho = density[i];
    const float s[3] = { scales[3 * i], scales[3 * i + 1], scales[3 * i + 2] };
    const float4 q = make_float4(rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3]);
    float acc[NPAR];
#pragma unroll
    for (int k = 0; k < NPAR; ++k) acc[k] = 0.0f;
    const float radius = gauss_radius(mx, my, mz, rho, s[0], s[1], s[2], mod, q);
    if (radius >= 0.0f) {
        const GaussRec g = gauss_rec(mx, my, mz, rho, s[0], s[1], s[2], mod, q);
        for (int view = 0; view < V; ++view) {
            const float *R = rays + 12 * view;
            const ViewGeom vg = view_geom(R, cone);
            PixRect rc;
            if (!gauss_rect(vg, cone, mx, my, mz, radius, H, W, rc)) continue;
            const int nw = rc.c1 - rc.c0 + 1, n = nw * (rc.r1 - rc.r0 + 1);   // <= H W < 2^30 (checked by the host)
            const float *Wv = weights ? weights + (size_t)view * H * W : nullptr;
            for (int k = lane; k < n; k += WAVE) {
                const int rr = k / nw, r = rc.r0 + rr, c = rc.c0 + (k - rr * nw);
                const Ray y = pixel_ray(R, cone, r, c);
                GaussPair p;
                if (!gauss_pair(g, y, cone, p)) continue;
                float o[NPAR];
                pair_squares(g, p, y, ray_length(y), s, q, o);
                const float w = Wv ? Wv[(size_t)r * W + c] : 1.0f;
#pragma unroll
                for (int t = 0; t < NPAR; ++t) acc[t] += w * o[t];
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NPAR; ++t)
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) acc[t] += __shfl_xor(acc[t], d);
    if (lane == 0) {
        f_means[3 * i] = acc[0]; f_means[3 * i + 1] = acc[1]; f_means[3 * i + 2] = acc[2];
        f_density[i] = acc[3];
        f_scales[3 * i] = acc[4]; f_scales[3 * i + 1] = acc[5]; f_scales[3 * i + 2] = acc[6];
        f_rotations[4 * i] = acc[7]; f_rotations[4 * i + 1] = acc[8]; f_rotations[4 * i + 2] = acc[9];
        f_rotations[4 * i + 3] = acc[10];
    }
}

}  // namespace

}  // namespace r2

extern "C" int r2_project_gaussians_fisher(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                           const float *density, const float *scales, float scale_modifier,
                                           const float *rotations, const float *weights, float *f_means, float *f_density,
                                           float *f_scales, float *f_rotations, void *stream)
{
    using namespace r2;
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays ||
        (P > 0 && (!means || !density || !scales || !rotations || !f_means || !f_density || !f_scales || !f_rotations))) {
        set_error("r2_project_gaussians_fisher: invalid argument");
        return R2_ERR_INVALID;
    }
    if ((long long)H * W >= (1LL << 30) || P > (1 << 29)) {
        set_error("r2_project_gaussians_fisher: shape out of range (H %d, W %d, P %d)", H, W, P);
        return R2_ERR_INVALID;
    }
    if (P == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int per = FB / WAVE;
    gaussian_fisher_kernel<<<dim3((P + per - 1) / per), dim3(FB), 0, s>>>(V, H, W, rays, cone, P, means, density, scales,
                                                                           scale_modifier, rotations, weights, f_means, f_density,
                                                                           f_scales, f_rotations);
    R2_STAGE_CHECK(0, s, "project gaussians fisher");
    return 0;
}
