// gaussian_project_bwd.hip -- the gradients of r2_project_gaussians with respect to the means, densities, scales and
// quaternions, given G = dL/dout (include/r2hip.h: r2_project_gaussians_backward).
//
// Gaussian-major: one wave per Gaussian.  For each view in order the wave takes the Gaussian's detector rectangle -- the one
// the forward took (gaussian_rays.hpp: gauss_radius, gauss_rect), so a pair is differentiated exactly when the forward summed
// it -- and walks its pixels row-major, lane l taking pixels l, l + 64, ...; each lane keeps the eleven sums of its own pairs
// in registers, and one xor butterfly over the wave adds the 64 partial sums in a fixed order at the end.  Nobody else
// writes a Gaussian's gradients: no atomics, no workspace, the same bits on every call, and a Gaussian no ray touches (or
// one with a non-finite parameter) gets exact zeros.  A Gaussian that covers the whole detector costs its wave V H W pairs.
#include "gaussian_rays.hpp"

namespace r2 {

namespace {

constexpr int BB = 256;   // threads per workgroup: four Gaussians

__global__ void __launch_bounds__(BB) gaussian_project_bwd_kernel(int V, int H, int W, const float *__restrict__ rays, int cone,
                                                                  int P, const float *__restrict__ means,
                                                                  const float *__restrict__ density,
                                                                  const float *__restrict__ scales, float mod,
                                                                  const float *__restrict__ rotations, const float *__restrict__ G,
                                                                  float *__restrict__ d_means, float *__restrict__ d_density,
                                                                  float *__restrict__ d_scales, float *__restrict__ d_rotations)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int i = blockIdx.x * (BB / WAVE) + threadIdx.x / WAVE;   // wave-uniform
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
        for (int view = 0; view < V; ++view) {
            const float *R = rays + 12 * view;
            const ViewGeom vg = view_geom(R, cone);
            PixRect rc;
            if (!gauss_rect(vg, cone, mx, my, mz, radius, H, W, rc)) continue;
            const int nw = rc.c1 - rc.c0 + 1, n = nw * (rc.r1 - rc.r0 + 1);   // <= H W < 2^30 (checked by the host)
            const float *Gv = G + (size_t)view * H * W;
            for (int k = lane; k < n; k += WAVE) {
                const int rr = k / nw, r = rc.r0 + rr, c = rc.c0 + (k - rr * nw);
                const Ray y = pixel_ray(R, cone, r, c);
                GaussPair p;
                if (!gauss_pair(g, y, cone, p)) continue;
                float o[11];
                gauss_pair_grad(g, p, y, ray_length(y), Gv[(size_t)r * W + c], s, q, o);
#pragma unroll
                for (int t = 0; t < 11; ++t) acc[t] += o[t];
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

}  // namespace

}  // namespace r2

extern "C" int r2_project_gaussians_backward(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                             const float *density, const float *scales, float scale_modifier,
                                             const float *rotations, const float *dL_dout, float *dL_dmeans, float *dL_ddensity,
                                             float *dL_dscales, float *dL_drotations, void *stream)
{
    using namespace r2;
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays || !dL_dout ||
        (P > 0 && (!means || !density || !scales || !rotations || !dL_dmeans || !dL_ddensity || !dL_dscales || !dL_drotations))) {
        set_error("r2_project_gaussians_backward: invalid argument");
        return R2_ERR_INVALID;
    }
    if ((long long)H * W >= (1LL << 30) || P > (1 << 29)) {
        set_error("r2_project_gaussians_backward: shape out of range (H %d, W %d, P %d)", H, W, P);
        return R2_ERR_INVALID;
    }
    if (P == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int per = BB / WAVE;
    gaussian_project_bwd_kernel<<<dim3((P + per - 1) / per), dim3(BB), 0, s>>>(V, H, W, rays, cone, P, means, density, scales,
                                                                                scale_modifier, rotations, dL_dout, dL_dmeans,
                                                                                dL_ddensity, dL_dscales, dL_drotations);
    R2_STAGE_CHECK(0, s, "project gaussians backward");
    return 0;
}
