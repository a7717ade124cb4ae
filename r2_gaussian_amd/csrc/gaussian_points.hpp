// gaussian_points.hpp -- the density field of a Gaussian cloud at caller-supplied points, and everything that decides whether a
// (Gaussian, point) pair is summed, as r2_query_gaussians defines them (include/r2hip.h).  Shared by the forward
// (gaussian_query.hip) and the box kernel and both backwards (gaussian_query_bwd.hip): the gradients are only those of the
// values the forward wrote if all take the same boxes, the same sphere and the same arithmetic per pair, so they are written
// once, here.  The Gaussian's record, its bounding sphere and the pair's gradient formulas are gaussian_rays.hpp's, taken as
// they are: a point x is the ray with start x and direction 0 to them (see point_pair).  Both translation units are compiled
// with -ffp-contract=off (build.py: EXACT): every float below is one separately rounded operation in the order written, which
// is the order tests/gaussian_field_ref.py restates in float32.
//
// The rule.  A pair is summed when its float32 q is at most GQ_CUT = 32.001, and only then: every pair with q <= 32 is summed
// (the 3e-5 above 32 is more than float32 loses on q), and of the pairs with q > 32, which the contract leaves free, only
// those in that sliver.  The cut is per pair on purpose.  The contract's suggested rule -- a point sums whatever Gaussian's
// sphere meets the box of its block -- makes the q > 32 tail of a point depend on its block mates, that is, on the ORDER of
// the points, and although each such term is below exp(-16) of its Gaussian's peak, their signs are mixed in every gradient
// (and in d rho through G): for a Gaussian that no point sees within q <= 32, a gradient made of an arbitrary part of its
// tail lies outside the interval between "no tail" and "all of the tail".  With the cut, values and gradients are a property
// of the pairs alone, whatever the order of the points; callers should still rely on no more than the contract states.
// Two conservative tests in front of the cut only save work and change no bit.  The points are taken in blocks of QB = 256
// consecutive ones; a block's box is the axis-aligned bounding box of its points with finite coordinates.  (1) A block skips
// a Gaussian whose gauss_radius sphere around the mean misses its box; (2) a point skips a Gaussian when it lies outside that
// sphere, |x - mu|^2 > radius^2.  q <= GQ_CUT implies |x - mu| <= sqrt(GQ_CUT) sigma_max / s_min(R) < radius (the sphere
// carries 1 %), and a point in the sphere lies in its block's box, which then meets the sphere -- in float32 as well: the
// box's distance is componentwise at most the point's, and rounding is monotone.
#pragma once
#include "gaussian_skeleton.hpp"

namespace r2 {

constexpr float GQ_CUT = 32.001f;   // a pair is summed when q <= this
constexpr int QB = 256;   // points per block = threads per workgroup = Gaussians per batch

// Blocks of N points (N + QB - 1 would overflow next to 2^31).
__host__ __device__ __forceinline__ int query_blocks(int N) { return N > 0 ? (N - 1) / QB + 1 : 0; }

// The bounding box of one block's finite points; lo = +inf, hi = -inf for a block without any.  24 bytes: the workspace of
// r2_query_gaussians_backward is an array of these.
struct BlockBox {
    float lo[3], hi[3];
};

__device__ __forceinline__ bool point_finite(float x, float y, float z)
{
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

// Squared distance from m to the box along its axes, against radius^2.  An empty box is infinitely far away; an infinite
// radius (gauss_radius: R nearly singular) meets every box.
__device__ __forceinline__ bool box_meets_sphere(const BlockBox &b, float mx, float my, float mz, float radius)
{
    const float dx = fmaxf(fmaxf(b.lo[0] - mx, mx - b.hi[0]), 0.0f);
    const float dy = fmaxf(fmaxf(b.lo[1] - my, my - b.hi[1]), 0.0f);
    const float dz = fmaxf(fmaxf(b.lo[2] - mz, mz - b.hi[2]), 0.0f);
    return dx * dx + dy * dy + dz * dz <= radius * radius;
}

// The box of the QB points of one workgroup (thread t holds point t; `valid`: it exists and is finite): a min / max butterfly
// over each wave, then over the waves through LDS.  All threads of the workgroup call it; all get the box.
__device__ __forceinline__ BlockBox block_box(bool valid, float x, float y, float z, float (*wbox)[6])
{
    float v[6] = { valid ? x : INFINITY, valid ? y : INFINITY, valid ? z : INFINITY,
                   valid ? x : -INFINITY, valid ? y : -INFINITY, valid ? z : -INFINITY };
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = fminf(v[k], __shfl_xor(v[k], d));
            v[3 + k] = fmaxf(v[3 + k], __shfl_xor(v[3 + k], d));
        }
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 6; ++k) wbox[wave][k] = v[k];
    __syncthreads();
    BlockBox b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = wbox[0][k];
        b.hi[k] = wbox[0][3 + k];
#pragma unroll
        for (int w = 1; w < QB / WAVE; ++w) {
            b.lo[k] = fminf(b.lo[k], wbox[w][k]);
            b.hi[k] = fmaxf(b.hi[k], wbox[w][3 + k]);
        }
    }
    return b;
}

// One (Gaussian, point) pair: e = x - mu, w = S^-1 R^T e, q = w.w, exp(-q / 2).  It is handed on as the GaussPair of the ray
// that starts at x and has no direction, with u = 0, A = 1, B / A = 0, wp = w and t0 = exp(-q / 2): gauss_term with |d| = 1
// is then rho exp(-q / 2), and gauss_pair_grad's sums are the point's (every term with u or d in it is an exact 0), so the
// gradient formulas and the quaternion derivative stay written once, in gaussian_rays.hpp.
// false: the pair is not summed (outside the sphere of squared radius r2, q above the cut or not a number): it contributes
// exactly 0.
__device__ __forceinline__ bool point_pair(const GaussRec &g, float r2, float x, float y, float z, GaussPair &p)
{
    p.e[0] = x - g.mx; p.e[1] = y - g.my; p.e[2] = z - g.mz;
    if (!(p.e[0] * p.e[0] + p.e[1] * p.e[1] + p.e[2] * p.e[2] <= r2)) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        p.w[i] = g.m[i][0] * p.e[0] + g.m[i][1] * p.e[1] + g.m[i][2] * p.e[2];
        p.wp[i] = p.w[i];
        p.u[i] = 0.0f;
    }
    p.A = 1.0f;
    p.k = 0.0f;
    const float q = p.w[0] * p.w[0] + p.w[1] * p.w[1] + p.w[2] * p.w[2];
    if (!(q <= GQ_CUT)) return false;
    p.t0 = expf(-0.5f * q);
    return true;
}

__device__ __forceinline__ Ray point_ray(float x, float y, float z) { return Ray{x, y, z, 0.0f, 0.0f, 0.0f}; }

// The pair's term of the field.
__device__ __forceinline__ float point_term(const GaussRec &g, const GaussPair &p) { return gauss_term(g, p, 1.0f); }

// The pair's term of the eleven parameter sums (gauss_pair_grad's layout), for the gradient G of the point's value.
__device__ __forceinline__ void point_pair_grad(const GaussRec &g, const GaussPair &p, float x, float y, float z, float G,
                                                const float *s, float4 q, float *o)
{
    gauss_pair_grad(g, p, point_ray(x, y, z), 1.0f, G, s, q, o);
}

// The pair's term of dL/dx: minus its term of dL/dmu (the field depends on x - mu alone).  The scales and the quaternion only
// enter the sums that are not used here.
__device__ __forceinline__ void point_pair_dx(const GaussRec &g, const GaussPair &p, float x, float y, float z, float G, float *o)
{
    const float s[3] = { 1.0f, 1.0f, 1.0f };
    float all[11];
    gauss_pair_grad(g, p, point_ray(x, y, z), 1.0f, G, s, make_float4(0.0f, 0.0f, 0.0f, 0.0f), all);
    o[0] = -all[0]; o[1] = -all[1]; o[2] = -all[2];
}

// What a workgroup stages of a Gaussian whose sphere meets its box.
struct StagedPoint {
    GaussRec g;
    float r2;
};

// The point-major kernel of the forward (GRAD = false: out[n] = the field at point n) and of the point gradient
// (GRAD = true: out[3 n ..] = G[n] d field / d x) on gaussian_skeleton.hpp's gather_rounds.  One workgroup per block of QB
// points, one thread per point.  A Gaussian is a hit when its sphere meets the block's box; the hits are staged with their
// S^-1 R^T, and every point adds the batch's pairs in batch order: in ascending Gaussian index, in one thread.
template <bool GRAD>
__device__ __forceinline__ void query_points_block(int N, const float *__restrict__ points, const Cloud &cl,
                                                   const float *__restrict__ G, float *__restrict__ out)
{
    __shared__ StagedPoint st[QB];
    __shared__ float wbox[QB / WAVE][6];
    const long long n = (long long)blockIdx.x * QB + threadIdx.x;   // < 2^31 + QB
    float x = 0.f, y = 0.f, z = 0.f;
    if (n < N) {
        x = points[3 * n]; y = points[3 * n + 1]; z = points[3 * n + 2];
    }
    const bool valid = n < N && point_finite(x, y, z);
    const BlockBox box = block_box(valid, x, y, z, wbox);
    const float Gn = GRAD && valid ? G[n] : 0.0f;
    float acc[3] = { 0.0f, 0.0f, 0.0f };
    gather_rounds<QB>(
        cl, st, valid, [&](const Gauss &a, float radius) { return box_meets_sphere(box, a.mx, a.my, a.mz, radius); },
        [&](StagedPoint &d, const Gauss &a, float radius, int) {
            d.g = gauss_rec(a, cl.mod);
            d.r2 = radius * radius;
        },
        [&](const StagedPoint &s) {
            GaussPair p;
            if (!point_pair(s.g, s.r2, x, y, z, p)) return;
            if (GRAD) {
                float o[3];
                point_pair_dx(s.g, p, x, y, z, Gn, o);
                acc[0] += o[0]; acc[1] += o[1]; acc[2] += o[2];
            } else {
                acc[0] += point_term(s.g, p);
            }
        });
    if (n < N) {
        if (GRAD) {
            out[3 * n] = acc[0]; out[3 * n + 1] = acc[1]; out[3 * n + 2] = acc[2];
        } else {
            out[n] = acc[0];
        }
    }
}

}  // namespace r2
