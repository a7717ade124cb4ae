// gaussian_bundle.hpp -- the exact line integral of a Gaussian cloud along caller-supplied rays, one start and one direction
// per ray, and everything that decides whether a (Gaussian, ray) pair is summed, as r2_integrate_gaussians defines them
// (include/r2hip.h).  Shared by the forward (gaussian_bundle.hip) and the cloud-box, block-box and both backward kernels
// (gaussian_bundle_bwd.hip).  The pair is gaussian_rays.hpp's gauss_pair, its gradients gauss_pair_grad and
// gaussian_ray_grad.hpp's gauss_pair_ray_grad, the cut and the box test gaussian_points.hpp's, all taken as they are.  The
// translation units are compiled with -ffp-contract=off (build.py: EXACT): every float below is one separately rounded
// operation in the order written, which is the order tests/gaussian_bundle_ref.py restates in float32.
//
// The rule.  A ray is valid when its six numbers are finite and its float32 length len = sqrt(dx dx + dy dy + dz dz) is
// positive and finite.  A pair of a valid ray and a Gaussian with gauss_radius >= 0 is summed when gauss_pair accepts it and
// its float32 q = wp.wp, recomputed from the pair's wp (the same bits gauss_pair put into the exponent), is at most GQ_CUT,
// and only then.  That is a property of the pair alone (gaussian_points.hpp has the reason), so a ray's value and its ray
// gradient do not depend on which other rays are in the call or on their order, bit for bit.
//
// Culling comes in front of the rule, saves work and changes no bit; each test is conservative for the INFINITE line, so the
// cone rule needs no case of its own.  A summed pair has q <= GQ_CUT at the line's Mahalanobis-closest point x*, hence
// |x* - mu| <= sqrt(GQ_CUT) sigma_max / s_min(R) = 0.9901 radius for gauss_radius' sphere: the line enters the sphere.  The
// sphere's 1 % stays what it is for the siblings, the room for the rounding of q itself; the tests below do not draw on it
// for their own arithmetic but carry explicit allowances in units of GB_EPS = 2^-20 = 16 float32 unit roundoffs (eps = 2^-24).
// The inputs are float32 numbers and define the geometry exactly; a difference of two of them is rounded relative to the
// RESULT, so e = s - mu carries eps |e| however far from the origin the scene lies.
//
// (0) The cloud box: the bounding box of the spheres mu +- radius of all Gaussians with radius >= 0 (an infinite radius makes
//     it infinite, no such Gaussian leaves it empty: lo > hi).  mu -+ radius is rounded once: eps |bound|.
// (1) The ray's segment.  With the unit direction dh = d / len (each component within 3 eps of the true one) the ray is clipped
//     to the cloud box by the slab method, in world length t along dh.  Each bound is first moved outwards by
//     GB_EPS |bound| (16 x the rounding in (0)); (bound - s_k) / dh_k then has 2 eps from its two operations and 3 eps from dh_k,
//     relative to t itself, and every t is moved outwards by GB_EPS |t|.  An axis with dh_k = 0 clips nothing and misses when
//     s_k lies outside the moved bounds.  half_line rays start at t = 0: a summed pair has its float32 t* > 0, and where the
//     true t* is negative it is so by the rounding of B / A, at most some 3 eps cond(S) |w| / |u| <= 200 eps |x* - mu| in
//     length for the 50 : 1 Gaussians the tests hold, against the 0.0099 radius the point s keeps to the sphere's surface.
//     A ray that misses the box (t0 > t1) sums nothing: every point of its line in a sphere would lie in the box.  Rays whose
//     len^2 is outside [1e-30, 1e30] are not clipped and not culled: their segment is all of space.
// (2) The ray's box: the bounding box of the end points p = s + t dh of the segment, each component moved outwards by
//     GB_EPS (|s_k| + |t|): the product and the sum round by 2 eps (|s_k| + |t dh_k|) and the direction moves the point by
//     3 eps |t dh_k|.  Any point of the true line inside the cloud box lies on the true segment, hence between the true end
//     points in every component, hence in the ray's box.  A block's box is the bounding box of the boxes of its QB
//     consecutive rays (invalid and missing rays stay out), and a block skips a Gaussian through box_meets_sphere, whose own
//     rounding (differences relative to their result, three squares and two sums: 4 eps of the distance) is the kind the
//     sphere's 1 % was made for and does not grow with the distance from the origin.
// (3) A ray skips a Gaussian whose sphere its line misses: c = e x dh, |c|^2 > (radius + a)^2 (1 + 1e-5).  Each component of c
//     is a difference of two rounded products of the rounded e and dh: |c - true| <= sum_k 5 eps (|e_i dh_j| + |e_j dh_i|)
//     <= 10 eps |e|_1, and a = GB_EPS |e|_1 covers it.  This is the term a fixed 1 % cannot: the products cancel down
//     from |e| to the line's distance, so the error is relative to |e|, not to radius -- for sigma = 5e-4 seen from six units
//     away 10 eps |e| is 0.1 % of the radius already, and it grows with the distance of the start while the radius does not.
//     The factor 1 + 1e-5 covers the three squares, two sums and the square on the right (10 eps).
#pragma once
#include "gaussian_points.hpp"
#include "gaussian_ray_grad.hpp"

namespace r2 {

constexpr float GB_EPS = 9.5367431640625e-07f;   // 2^-20
constexpr int GB_PARTS = 1024;                   // at most this many workgroups build the cloud box

// Workgroups of the cloud-box kernel for P Gaussians.
__host__ __device__ __forceinline__ int bundle_parts(int P)
{
    const int g = P > 0 ? (P - 1) / QB + 1 : 0;
    return g < GB_PARTS ? g : GB_PARTS;
}

// The workspace: [0] the cloud box, [1 .. parts] its partial boxes, then one box per block of QB rays.
__host__ __device__ __forceinline__ size_t bundle_workspace_boxes(int N, int P)
{
    return N > 0 && P > 0 ? (size_t)1 + (size_t)bundle_parts(P) + (size_t)query_blocks(N) : (size_t)0;
}

// Launches the two kernels that write the cloud box (0) into boxes[0] (gaussian_bundle.hip); P > 0.
void bundle_cloud_box(const Cloud &cl, BlockBox *boxes, hipStream_t s);

// What the kernels keep of a ray: the ray itself, its length and whether it is valid.
struct BundleRay {
    Ray y;
    float len;
    bool valid;
};

__device__ __forceinline__ BundleRay bundle_ray(const float *__restrict__ rays, long long n)
{
    BundleRay b;
    b.y = Ray{rays[6 * n], rays[6 * n + 1], rays[6 * n + 2], rays[6 * n + 3], rays[6 * n + 4], rays[6 * n + 5]};
    b.len = ray_length(b.y);
    b.valid = point_finite(b.y.sx, b.y.sy, b.y.sz) && point_finite(b.y.dx, b.y.dy, b.y.dz) && b.len > 0.0f && b.len < INFINITY;
    return b;
}

// Ray n of N; n >= N: the ray that is not there, invalid.
__device__ __forceinline__ BundleRay bundle_ray(const float *__restrict__ rays, long long n, long long N)
{
    BundleRay b;
    b.y = Ray{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    b.len = 0.0f;
    b.valid = false;
    if (n < N) b = bundle_ray(rays, n);
    return b;
}

// The unit direction of a valid ray for the culling tests; tame = false: the ray is neither clipped nor culled.
struct BundleDir {
    float h[3];
    bool tame;
};

__device__ __forceinline__ BundleDir bundle_dir(const BundleRay &b)
{
    BundleDir u;
    const float l2 = b.len * b.len;
    u.tame = b.valid && l2 >= 1e-30f && l2 <= 1e30f;
    u.h[0] = u.tame ? b.y.dx / b.len : 0.0f;
    u.h[1] = u.tame ? b.y.dy / b.len : 0.0f;
    u.h[2] = u.tame ? b.y.dz / b.len : 0.0f;
    return u;
}

// v[0..2] = min, v[3..5] = max over the QB threads of the workgroup: a butterfly over each wave, then over the waves through
// LDS.  All threads call it; all get the result.  (min and max are exact, so the order is immaterial.)
__device__ __forceinline__ BlockBox bundle_box_reduce(float *v, float (*wbox)[6])
{
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

// (1) and (2): the box of the ray's segment in the cloud box, written to v (min, max); false: the ray is invalid or misses
// the cloud box, v is then the empty box.
__device__ __forceinline__ bool bundle_ray_box(const BundleRay &b, const BundleDir &u, int half_line, const BlockBox &cloud, float *v)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = INFINITY;
        v[3 + k] = -INFINITY;
    }
    if (!b.valid || !(cloud.lo[0] <= cloud.hi[0])) return false;
    const float s[3] = { b.y.sx, b.y.sy, b.y.sz };
    float t0 = half_line ? 0.0f : -INFINITY, t1 = INFINITY;
    bool whole = !u.tame;
    if (u.tame) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float lo = cloud.lo[k] - GB_EPS * fabsf(cloud.lo[k]), hi = cloud.hi[k] + GB_EPS * fabsf(cloud.hi[k]);
            if (u.h[k] == 0.0f) {
                if (s[k] < lo || s[k] > hi) return false;
                continue;
            }
            const float ta = (lo - s[k]) / u.h[k], tb = (hi - s[k]) / u.h[k];
            const float a = fminf(ta, tb), c = fmaxf(ta, tb);
            t0 = fmaxf(t0, a - GB_EPS * fabsf(a));
            t1 = fminf(t1, c + GB_EPS * fabsf(c));
        }
        if (!(t0 <= t1)) return false;
        whole = !(fabsf(t0) < INFINITY && fabsf(t1) < INFINITY);
    }
    if (whole) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = -INFINITY;
            v[3 + k] = INFINITY;
        }
        return true;
    }
    const float tm = fmaxf(fabsf(t0), fabsf(t1));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p0 = s[k] + t0 * u.h[k], p1 = s[k] + t1 * u.h[k];
        const float pad = GB_EPS * (fabsf(s[k]) + tm);
        v[k] = fminf(p0, p1) - pad;
        v[3 + k] = fmaxf(p0, p1) + pad;
    }
    return true;
}

// (3): true when the line of the ray misses the sphere of `radius` around the Gaussian's mean.
__device__ __forceinline__ bool bundle_line_misses(const BundleRay &b, const BundleDir &u, float mx, float my, float mz, float radius)
{
    if (!u.tame) return false;
    const float ex = b.y.sx - mx, ey = b.y.sy - my, ez = b.y.sz - mz;
    const float cx = ey * u.h[2] - ez * u.h[1], cy = ez * u.h[0] - ex * u.h[2], cz = ex * u.h[1] - ey * u.h[0];
    const float lim = radius + GB_EPS * (fabsf(ex) + fabsf(ey) + fabsf(ez));
    return cx * cx + cy * cy + cz * cz > (lim * lim) * 1.00001f;
}

// One (Gaussian, ray) pair of a valid ray by the rule: gauss_pair, then the cut on q recomputed from its wp.
__device__ __forceinline__ bool bundle_pair(const GaussRec &g, const Ray &y, int half_line, GaussPair &p)
{
    if (!gauss_pair(g, y, half_line, p)) return false;
    const float q = p.wp[0] * p.wp[0] + p.wp[1] * p.wp[1] + p.wp[2] * p.wp[2];
    return q <= GQ_CUT;
}

// What a workgroup stages of a Gaussian whose sphere meets its box.
struct StagedRayGauss {
    GaussRec g;
    float radius;
};

// The ray-major kernel of the forward (GRAD = false: out[n] = the integral along ray n) and of the ray gradient
// (GRAD = true: out[6 n ..] = G[n] d integral / d (s, d)) on gaussian_skeleton.hpp's gather_rounds.  One workgroup per block of
// QB rays, one thread per ray.  A Gaussian is a hit when its sphere meets the block's box; the hits are staged with their
// S^-1 R^T, and every ray adds the batch's pairs in batch order: in ascending Gaussian index, in one thread.
template <bool GRAD>
__device__ __forceinline__ void integrate_rays_block(int N, const float *__restrict__ rays, int half_line, const Cloud &cl,
                                                     const float *__restrict__ G, const BlockBox *__restrict__ cloud,
                                                     float *__restrict__ out)
{
    __shared__ StagedRayGauss st[QB];
    __shared__ float wbox[QB / WAVE][6];
    const long long n = (long long)blockIdx.x * QB + threadIdx.x;   // < 2^31 + QB
    const BundleRay b = bundle_ray(rays, n, N);
    const BundleDir u = bundle_dir(b);
    float acc[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    if (cl.P > 0) {   // uniform; the cloud box is only there when there is a cloud
        float v[6];
        const bool live = bundle_ray_box(b, u, half_line, cloud[0], v);
        const BlockBox box = bundle_box_reduce(v, wbox);
        const float Gn = GRAD && live ? G[n] : 0.0f;
        gather_rounds<QB>(
            cl, st, live, [&](const Gauss &a, float radius) { return box_meets_sphere(box, a.mx, a.my, a.mz, radius); },
            [&](StagedRayGauss &d, const Gauss &a, float radius, int) {
                d.g = gauss_rec(a, cl.mod);
                d.radius = radius;
            },
            [&](const StagedRayGauss &s) {
                if (bundle_line_misses(b, u, s.g.mx, s.g.my, s.g.mz, s.radius)) return;
                GaussPair p;
                if (!bundle_pair(s.g, b.y, half_line, p)) return;
                if (GRAD)
                    gauss_pair_ray_grad(s.g, p, b.y, b.len, Gn, acc, acc + 3);
                else
                    acc[0] += gauss_term(s.g, p, b.len);
            });
    }
    if (n < N) {
        if (GRAD) {
#pragma unroll
            for (int k = 0; k < 6; ++k) out[6 * n + k] = acc[k];
        } else {
            out[n] = acc[0];
        }
    }
}

}  // namespace r2
