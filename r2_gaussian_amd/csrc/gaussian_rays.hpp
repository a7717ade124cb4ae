// gaussian_rays.hpp -- the exact line integral of one 3D Gaussian along one detector ray, and everything that decides
// whether a (Gaussian, ray) pair is summed, as r2_project_gaussians defines them (include/r2hip.h).  Shared by the forward
// (gaussian_project.hip) and the backward (gaussian_project_bwd.hip): the gradients are only those of the image the forward
// wrote if both take the same rectangle, the same cone rule and the same arithmetic per pair, so they are written once,
// here.  Both translation units are compiled with -ffp-contract=off (build.py: EXACT): every float below is one separately
// rounded operation in the order written, which is the order tests/gaussian_project_ref.py restates in float32.
#pragma once
#include "r2_math.hpp"
#include "ray_sampling.hpp"
#include <math.h>

namespace r2 {

constexpr float GP_TWO_PI = 6.283185307179586f;
// bounding sphere in units of sigma_max: sqrt(32), plus 1 % so that rounding never drops a pair with q <= 32
constexpr float GP_SPHERE = 5.656854249492381f * 1.01f;

// One Gaussian as a pair sees it: M = S^-1 R^T (row i = column i of R over sigma_i), 1 / sigma, the mean and the density.
struct GaussRec {
    float m[3][3];
    float is[3];
    float mx, my, mz, rho;
};

// Detector rectangle in pixels, both ends included.
struct PixRect {
    int c0, c1, r0, r1;
};

// The constants of one view for the rectangle: the rows k0, k1, k2 of [pu pv e]^-1, with e = p00 - a (cone) or a
// (parallel), and the origin o = a (cone) or p00 (parallel).  A world point X has (c t, r t, t) = K (X - o) in cone beam
// (pixel (c, r) at depth t) and (c, r, t) = K (X - o) in parallel beam.
struct ViewGeom {
    float k0[3], k1[3], k2[3], o[3];
    float n0, n1, n2, k02, k12;   // |k0|, |k1|, |k2|, k0.k2, k1.k2
};

__device__ __forceinline__ ViewGeom view_geom(const float *R, int cone)
{
    ViewGeom g;
    float e[3];
    for (int j = 0; j < 3; ++j) {
        e[j] = cone ? R[3 + j] - R[j] : R[j];
        g.o[j] = cone ? R[j] : R[3 + j];
    }
    const float *pu = R + 6, *pv = R + 9;
    const float c0[3] = { pv[1] * e[2] - pv[2] * e[1], pv[2] * e[0] - pv[0] * e[2], pv[0] * e[1] - pv[1] * e[0] };
    const float c1[3] = { e[1] * pu[2] - e[2] * pu[1], e[2] * pu[0] - e[0] * pu[2], e[0] * pu[1] - e[1] * pu[0] };
    const float c2[3] = { pu[1] * pv[2] - pu[2] * pv[1], pu[2] * pv[0] - pu[0] * pv[2], pu[0] * pv[1] - pu[1] * pv[0] };
    const float det = pu[0] * c0[0] + pu[1] * c0[1] + pu[2] * c0[2];
    for (int j = 0; j < 3; ++j) {   // a flat detector (det = 0) gives non-finite rows: every rectangle is then the whole detector
        g.k0[j] = c0[j] / det;
        g.k1[j] = c1[j] / det;
        g.k2[j] = c2[j] / det;
    }
    g.n0 = sqrtf(g.k0[0] * g.k0[0] + g.k0[1] * g.k0[1] + g.k0[2] * g.k0[2]);
    g.n1 = sqrtf(g.k1[0] * g.k1[0] + g.k1[1] * g.k1[1] + g.k1[2] * g.k1[2]);
    g.n2 = sqrtf(g.k2[0] * g.k2[0] + g.k2[1] * g.k2[1] + g.k2[2] * g.k2[2]);
    g.k02 = g.k0[0] * g.k2[0] + g.k0[1] * g.k2[1] + g.k0[2] * g.k2[2];
    g.k12 = g.k1[0] * g.k2[0] + g.k1[1] * g.k2[1] + g.k1[2] * g.k2[2];
    return g;
}

// Radius of a sphere around the mean that contains {x : |S^-1 R^T x|^2 <= 32}, or a negative value for a Gaussian that
// contributes nothing at all (a non-finite parameter, a scale <= 0).  x = R^-T S y with |y|^2 <= 32, so
// |x| <= sqrt(32) sigma_max / s_min(R).  The quaternion is used as it comes: with n2 = |q|^2, R = (1 - n2) I + n2 Rhat for the
// rotation Rhat of q / |q|, a normal matrix with the eigenvalues 1 and (1 - n2) + n2 exp(+-i theta), cos(theta) = 2 r^2 / n2 - 1:
// s_min^2 = min(1, (1 - n2)^2 + 2 (1 - n2)(2 r^2 - n2) + n2^2), which is 1 for a unit quaternion.  INFINITY when R is (nearly)
// singular: the rectangle is then the whole detector.
__device__ __forceinline__ float gauss_radius(float mx, float my, float mz, float rho, float sx, float sy, float sz, float mod,
                                              float4 q)
{
    const float all = mx + my + mz + rho + sx + sy + sz + mod + q.x + q.y + q.z + q.w;
    const float s0 = sx * mod, s1 = sy * mod, s2 = sz * mod;
    if (!(fabsf(all) < INFINITY) || !(s0 > 0.f) || !(s1 > 0.f) || !(s2 > 0.f)) return -1.0f;
    const float n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    const float om = 1.0f - n2;
    const float e2 = om * om + 2.0f * om * (2.0f * q.x * q.x - n2) + n2 * n2;
    const float smin2 = fminf(1.0f, e2);
    if (!(smin2 > 1e-6f)) return INFINITY;
    return GP_SPHERE * fmaxf(s0, fmaxf(s1, s2)) / sqrtf(smin2);
}

__device__ __forceinline__ GaussRec gauss_rec(float mx, float my, float mz, float rho, float sx, float sy, float sz, float mod,
                                              float4 q)
{
    GaussRec g;
    const M3 R = quat_to_rot(q.x, q.y, q.z, q.w);   // R.m[j][i] = R_ji of the standard rotation (quat_to_rot lists it by rows)
    g.is[0] = 1.0f / (sx * mod);
    g.is[1] = 1.0f / (sy * mod);
    g.is[2] = 1.0f / (sz * mod);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) g.m[i][j] = R.m[j][i] * g.is[i];
    g.mx = mx; g.my = my; g.mz = mz; g.rho = rho;
    return g;
}

// One detector axis of the rectangle: the pixel interval [lo, hi] widened by one pixel plus the rounding of the tangent
// computation (see gauss_rect), cut to [0, n - 1].  Returns false when nothing is left.
__device__ __forceinline__ bool rect_axis(float lo, float hi, int n, int &i0, int &i1)
{
    if (!(fabsf(lo) < INFINITY) || !(fabsf(hi) < INFINITY)) {
        i0 = 0; i1 = n - 1;
        return true;
    }
    const float pad = 1.0f + 1e-3f * fmaxf(fabsf(lo), fabsf(hi));
    const float a = floorf(lo - pad), b = ceilf(hi + pad);
    if (b < 0.0f || a > (float)(n - 1)) return false;
    i0 = (int)fmaxf(a, 0.0f);
    i1 = (int)fminf(b, (float)(n - 1));
    return true;
}

// The pixels whose ray can pass within `radius` of the mean: a conservative rectangle.  Parallel beam: the planes c = const
// tangent to the sphere lie at k0.(mu - o) +- radius |k0|.  Cone beam: the plane through the source with pixel column c has
// the normal k0 - c k2, and it touches the sphere when (y0 - c y2)^2 = radius^2 |k0 - c k2|^2 (y = K (mu - a)), a quadratic
// in c whose two roots bound the columns when the sphere lies wholly in front of the source plane (y2 > radius |k2|); a
// sphere that contains the source or straddles that plane takes the whole detector.  The discriminant cancels to about
// sqrt(eps) |c| pixels, which rect_axis' pad covers.
__device__ __forceinline__ bool gauss_rect(const ViewGeom &v, int cone, float mx, float my, float mz, float radius, int H, int W,
                                           PixRect &q)
{
    q.c0 = 0; q.c1 = W - 1; q.r0 = 0; q.r1 = H - 1;
    if (!(radius < INFINITY)) return true;
    const float dx = mx - v.o[0], dy = my - v.o[1], dz = mz - v.o[2];
    const float y0 = v.k0[0] * dx + v.k0[1] * dy + v.k0[2] * dz;
    const float y1 = v.k1[0] * dx + v.k1[1] * dy + v.k1[2] * dz;
    const float y2 = v.k2[0] * dx + v.k2[1] * dy + v.k2[2] * dz;
    float clo, chi, rlo, rhi;
    if (cone) {
        if (!(y2 > 1.05f * radius * v.n2)) return true;
        const float r2 = radius * radius;
        const float a = y2 * y2 - r2 * v.n2 * v.n2;
        const float bc = y0 * y2 - r2 * v.k02, cc = y0 * y0 - r2 * v.n0 * v.n0;
        const float br = y1 * y2 - r2 * v.k12, cr = y1 * y1 - r2 * v.n1 * v.n1;
        const float sc = sqrtf(fmaxf(bc * bc - a * cc, 0.0f)), sr = sqrtf(fmaxf(br * br - a * cr, 0.0f));
        clo = (bc - sc) / a; chi = (bc + sc) / a;
        rlo = (br - sr) / a; rhi = (br + sr) / a;
    } else {
        clo = y0 - radius * v.n0; chi = y0 + radius * v.n0;
        rlo = y1 - radius * v.n1; rhi = y1 + radius * v.n1;
    }
    return rect_axis(clo, chi, W, q.c0, q.c1) && rect_axis(rlo, rhi, H, q.r0, q.r1);
}

// What a pair computes before the density comes in.
struct GaussPair {
    float e[3], u[3], w[3], wp[3];   // s - mu, S^-1 R^T d, S^-1 R^T (s - mu), w - (B / A) u
    float A, k, t0;                  // u.u, B / A, sqrt(2 pi / A) exp(-q / 2)
};

// false: the pair contributes exactly 0 (A = 0 or not finite: a ray without direction; cone beam: closest approach t* = -B / A
// at or behind the source; a non-finite result).
__device__ __forceinline__ bool gauss_pair(const GaussRec &g, const Ray &y, int cone, GaussPair &p)
{
    p.e[0] = y.sx - g.mx; p.e[1] = y.sy - g.my; p.e[2] = y.sz - g.mz;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        p.u[i] = g.m[i][0] * y.dx + g.m[i][1] * y.dy + g.m[i][2] * y.dz;
        p.w[i] = g.m[i][0] * p.e[0] + g.m[i][1] * p.e[1] + g.m[i][2] * p.e[2];
    }
    p.A = p.u[0] * p.u[0] + p.u[1] * p.u[1] + p.u[2] * p.u[2];
    const float B = p.u[0] * p.w[0] + p.u[1] * p.w[1] + p.u[2] * p.w[2];
    if (!(p.A > 0.0f)) return false;
    p.k = B / p.A;
    if (cone && !(p.k < 0.0f)) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) p.wp[i] = p.w[i] - p.k * p.u[i];
    const float q = p.wp[0] * p.wp[0] + p.wp[1] * p.wp[1] + p.wp[2] * p.wp[2];   // never w.w - B^2 / A: that cancels
    p.t0 = sqrtf(GP_TWO_PI / p.A) * expf(-0.5f * q);
    return fabsf(p.t0) < INFINITY;
}

// |d| of a ray.
__device__ __forceinline__ float ray_length(const Ray &y) { return sqrtf(y.dx * y.dx + y.dy * y.dy + y.dz * y.dz); }

// The pair's term of the image: rho sqrt(2 pi / A) exp(-q / 2) |d|.
__device__ __forceinline__ float gauss_term(const GaussRec &g, const GaussPair &p, float len) { return g.rho * p.t0 * len; }

// The pair's term of the eleven gradient sums, for the pixel gradient G: o[0..2] d mu, o[3] d rho, o[4..6] d scale (the
// unmodified one: sigma_i = mod s_i, so d / d s_i = -(...) / s_i), o[7..10] d quaternion (r, x, y, z; as given, no
// normalisation Jacobian).  s[3]: the unmodified scales; q: the quaternion.
__device__ __forceinline__ void gauss_pair_grad(const GaussRec &g, const GaussPair &p, const Ray &y, float len, float G,
                                                const float *s, float4 q, float *o)
{
    const float T = g.rho * p.t0, gl = G * len;
    float gw[3], gu[3], hu[3], hw[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gw[i] = -(T * p.wp[i]);
        gu[i] = T * (p.k * p.wp[i] - p.u[i] / p.A);
        hu[i] = gu[i] * g.is[i];
        hw[i] = gw[i] * g.is[i];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = -(gl * (g.m[0][j] * gw[0] + g.m[1][j] * gw[1] + g.m[2][j] * gw[2]));
    o[3] = G * (p.t0 * len);
#pragma unroll
    for (int i = 0; i < 3; ++i) o[4 + i] = -(gl * ((gu[i] * p.u[i] + gw[i] * p.w[i]) / s[i]));
    // dL/dR_ji = G |d| (d_j (S^-1 g_u)_i + e_j (S^-1 g_w)_i), then the derivative of quat_to_rot's entries
    const float d[3] = { y.dx, y.dy, y.dz };
    float D[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) D[j][i] = gl * (d[j] * hu[i] + p.e[j] * hw[i]);
    const float r = q.x, x = q.y, yy = q.z, z = q.w;
    o[7] = 2.0f * (z * (D[1][0] - D[0][1]) + yy * (D[0][2] - D[2][0]) + x * (D[2][1] - D[1][2]));
    o[8] = 2.0f * (yy * (D[0][1] + D[1][0]) + z * (D[0][2] + D[2][0]) + r * (D[2][1] - D[1][2])) - 4.0f * (x * (D[1][1] + D[2][2]));
    o[9] = 2.0f * (x * (D[0][1] + D[1][0]) + r * (D[0][2] - D[2][0]) + z * (D[1][2] + D[2][1])) - 4.0f * (yy * (D[0][0] + D[2][2]));
    o[10] = 2.0f * (r * (D[1][0] - D[0][1]) + x * (D[0][2] + D[2][0]) + yy * (D[1][2] + D[2][1])) - 4.0f * (z * (D[0][0] + D[1][1]));
}

}  // namespace r2
