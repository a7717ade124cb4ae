// gaussian_tangent.hpp -- the exact projector's per-pair derivatives applied to a tangent, unsquared: what
// r2_project_gaussians_jvp adds (include/r2hip.h).  On top of gaussian_fisher.hpp, which is taken as it is: the pair's eleven
// derivatives are gauss_pair_grad's with G = 1 (the image is a plain sum over the Gaussians, so d pixel / d theta_it IS that
// pair's number), and the staged record and its staging are the variance kernels' (StagedVar, stage_var: the slot v holds
// the Gaussian's eleven tangent components).  The translation unit is compiled with -ffp-contract=off (build.py: EXACT): every
// float below is one separately rounded operation in the order written, which is the order tests/gaussian_tangent_ref.py
// restates in float32.
#pragma once
#include "gaussian_fisher.hpp"

namespace r2 {

// sum_t tan[t] (d term / d theta_t) of one pair, added in ascending t: the pair's share of J t at the pixel.  tan may point
// into LDS: it is read component by component, as pair_variance reads its variances.
__device__ __forceinline__ float pair_tangent(const GaussRec &g, const GaussPair &p, const Ray &y, float len, const float *s,
                                              float4 q, const float *tan)
{
    float o[NPAR];
    gauss_pair_grad(g, p, y, len, 1.0f, s, q, o);
    float a = tan[0] * o[0];
#pragma unroll
    for (int t = 1; t < NPAR; ++t) a += tan[t] * o[t];
    return a;
}

// The staged Gaussian's share of J t at one ray for the pair p (a.v holds the tangent).
__device__ __forceinline__ float staged_tangent(const StagedVar &a, const GaussPair &p, const Ray &y, float len)
{
    return pair_tangent(a.g, p, y, len, a.s, make_float4(a.q[0], a.q[1], a.q[2], a.q[3]), a.v);
}

}  // namespace r2
