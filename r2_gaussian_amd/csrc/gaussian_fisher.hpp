// gaussian_fisher.hpp -- the squares of the exact operators' per-pair derivatives: what r2_project_gaussians_fisher,
// r2_query_gaussians_variance and r2_project_gaussians_variance add (include/r2hip.h).  On top of gaussian_rays.hpp and
// gaussian_points.hpp, which are taken as they are: a pair is summed exactly when the projector (rectangle, then gauss_pair)
// or the field query (sphere, then the cut at q <= GQ_CUT) sums it, and its eleven derivatives are gauss_pair_grad's with
// G = 1, so the image's Jacobian entry d pixel / d theta_it IS that pair's number (the image is a plain sum over the
// Gaussians).  The per-pair arithmetic is written once, here; the translation units that include this header are compiled
// with -ffp-contract=off (build.py: EXACT): every float below is one separately rounded operation in the order written, which
// is the order tests/gaussian_fisher_ref.py restates in float32.
#pragma once
#include "gaussian_points.hpp"

namespace r2 {

// o[t] = (d term / d theta_t)^2 of one pair: gauss_pair_grad with G = 1, squared.
__device__ __forceinline__ void pair_squares(const GaussRec &g, const GaussPair &p, const Ray &y, float len, const float *s,
                                             float4 q, float *o)
{
    gauss_pair_grad(g, p, y, len, 1.0f, s, q, o);
#pragma unroll
    for (int t = 0; t < NPAR; ++t) o[t] = o[t] * o[t];
}

// sum_t v[t] (d term / d theta_t)^2 of one pair, added in ascending t: the pair's share of the variance of the pixel (or of
// the field at the point) under independent parameter variances v.  v may point into LDS: it is read component by
// component, so the eleven variances never sit in registers next to the eleven derivatives.
__device__ __forceinline__ float pair_variance(const GaussRec &g, const GaussPair &p, const Ray &y, float len, const float *s,
                                               float4 q, const float *v)
{
    float o[NPAR];
    pair_squares(g, p, y, len, s, q, o);
    float a = v[0] * o[0];
#pragma unroll
    for (int t = 1; t < NPAR; ++t) a += v[t] * o[t];
    return a;
}

// What the two variance kernels stage of a Gaussian next to its GaussRec: the unmodified scales, the quaternion and the
// eleven variances, in gauss_pair_grad's order.
struct StagedVar {
    GaussRec g;
    float s[3];
    float q[4];
    float v[NPAR];
};

__device__ __forceinline__ void stage_var(StagedVar &d, const Gauss &a, float mod, const float *__restrict__ v_means,
                                          const float *__restrict__ v_density, const float *__restrict__ v_scales,
                                          const float *__restrict__ v_rotations, int i)
{
    d.g = gauss_rec(a, mod);
    d.s[0] = a.s[0]; d.s[1] = a.s[1]; d.s[2] = a.s[2];
    d.q[0] = a.q.x; d.q[1] = a.q.y; d.q[2] = a.q.z; d.q[3] = a.q.w;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d.v[k] = v_means[3 * i + k];
        d.v[4 + k] = v_scales[3 * i + k];
    }
    d.v[3] = v_density[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) d.v[7 + k] = v_rotations[4 * i + k];
}

// The staged Gaussian's share of the variance of one ray (or point, as point_ray) for the pair p.
__device__ __forceinline__ float staged_variance(const StagedVar &a, const GaussPair &p, const Ray &y, float len)
{
    return pair_variance(a.g, p, y, len, a.s, make_float4(a.q[0], a.q[1], a.q[2], a.q[3]), a.v);
}

// The record of the point-major variance kernel: about 140 bytes, 35 kB for a batch of QB.
struct StagedPointVar {
    StagedVar a;
    float r2;
};

// The point-major kernel of r2_query_gaussians_variance: query_points_block's rounds (gaussian_points.hpp, on
// gaussian_skeleton.hpp's gather_rounds) with the larger record.  One workgroup per block of QB points, one thread per point;
// a point adds its pairs in ascending Gaussian index, in one thread.
__device__ __forceinline__ void variance_points_block(int N, const float *__restrict__ points, const Cloud &cl,
                                                      const float *__restrict__ v_means, const float *__restrict__ v_density,
                                                      const float *__restrict__ v_scales, const float *__restrict__ v_rotations,
                                                      float *__restrict__ out)
{
    __shared__ StagedPointVar st[QB];
    __shared__ float wbox[QB / WAVE][6];
    const long long n = (long long)blockIdx.x * QB + threadIdx.x;   // < 2^31 + QB
    float x = 0.f, y = 0.f, z = 0.f;
    if (n < N) {
        x = points[3 * n]; y = points[3 * n + 1]; z = points[3 * n + 2];
    }
    const bool valid = n < N && point_finite(x, y, z);
    const BlockBox box = block_box(valid, x, y, z, wbox);
    const Ray ray = point_ray(x, y, z);
    float acc = 0.0f;
    gather_rounds<QB>(
        cl, st, valid, [&](const Gauss &a, float radius) { return box_meets_sphere(box, a.mx, a.my, a.mz, radius); },
        [&](StagedPointVar &d, const Gauss &a, float radius, int i) {
            stage_var(d.a, a, cl.mod, v_means, v_density, v_scales, v_rotations, i);
            d.r2 = radius * radius;
        },
        [&](const StagedPointVar &s) {
            GaussPair p;
            if (point_pair(s.a.g, s.r2, x, y, z, p)) acc += staged_variance(s.a, p, ray, 1.0f);
        });
    if (n < N) out[n] = acc;
}

}  // namespace r2
