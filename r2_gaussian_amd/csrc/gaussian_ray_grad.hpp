// gaussian_ray_grad.hpp -- the gradient of one (Gaussian, ray) pair of r2_project_gaussians in the ray itself, its start s and
// its direction d, as r2_project_gaussians_rays_backward defines it (include/r2hip.h), and the fixed-order sum of twelve
// numbers over a workgroup that both of its kernels use (gaussian_project_rays_bwd.hip).  The pair, the Gaussian's record, the
// rectangle and the cone rule are gaussian_rays.hpp's, taken as they are.  The translation unit is compiled with
// -ffp-contract=off (build.py: EXACT): every float below is one separately rounded operation in the order written, which is
// the order tests/gaussian_project_rays_ref.py restates in float32.
#pragma once
#include "gaussian_rays.hpp"

namespace r2 {

// Adds the pair's term of G d(term)/ds to gs[3] and of G d(term)/dd to gd[3].  With T, g_w, g_u as gauss_pair_grad has them
// and M = S^-1 R^T:  g_s = G |d| M^T g_w (the negative of gauss_pair_grad's d mu),  g_d = G |d| M^T g_u + G T d / |d|, the
// second term being the derivative of the factor |d|.
__device__ __forceinline__ void gauss_pair_ray_grad(const GaussRec &g, const GaussPair &p, const Ray &y, float len, float G,
                                                    float *gs, float *gd)
{
    const float T = g.rho * p.t0, gl = G * len, gt = (G * T) / len;
    float gw[3], gu[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gw[i] = -(T * p.wp[i]);
        gu[i] = T * (p.k * p.wp[i] - p.u[i] / p.A);
    }
    const float d[3] = { y.dx, y.dy, y.dz };
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        gs[j] += gl * (g.m[0][j] * gw[0] + g.m[1][j] * gw[1] + g.m[2][j] * gw[2]);
        gd[j] += gl * (g.m[0][j] * gu[0] + g.m[1][j] * gu[1] + g.m[2][j] * gu[2]) + gt * d[j];
    }
}

// What the pixel (r, c) hands to its view's twelve ray parameters {a, p00, pu, pv}, from its sums g_s and g_d: the pixel point
// is P = p00 + c pu + r pv; cone beam has s = a, d = P - a, parallel beam s = P, d = a.
__device__ __forceinline__ void pixel_ray_grad(int cone, int r, int c, const float *gs, const float *gd, float *o)
{
    const float fc = (float)c, fr = (float)r;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float gP = cone ? gd[j] : gs[j];
        o[j] = cone ? gs[j] - gd[j] : gd[j];
        o[3 + j] = gP;
        o[6 + j] = fc * gP;
        o[9 + j] = fr * gP;
    }
}

constexpr int RG = 256;   // threads per workgroup of both kernels

// v[k] summed over the RG threads of the workgroup, k < 12, in one fixed order: an xor butterfly over each wave, then the
// waves' sums in wave order through LDS.  All threads call it; thread 0 gets the sums.
__device__ __forceinline__ void block_sum12(float *v, float (*wsum)[12])
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < 12; ++k)
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) v[k] += __shfl_xor(v[k], d);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 12; ++k) wsum[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            float t = wsum[0][k];
#pragma unroll
            for (int w = 1; w < RG / WAVE; ++w) t += wsum[w][k];
            v[k] = t;
        }
}

}  // namespace r2
