// siddon_ray.hpp -- the ray of one detector pixel against the piecewise-constant voxel grid, as r2_project_volume_siddon
// defines it (include/r2hip.h).  Shared by the Siddon forward projector (projector_siddon.hip) and its exact transpose
// (backprojector_siddon.hip): a matrix entry is the same bits in both only if both take the same plane parameters and the
// same clip, so they are written once, here.  Both translation units are compiled with -ffp-contract=off (build.py: EXACT):
// every float below is the same separately rounded operation in both.
//
// The ray itself (pixel_ray, the 12 ray parameters) is ray_sampling.hpp's, unchanged.  The voxel model is not: voxel
// (i,j,k) is the index-space cube [i - 1/2, i + 1/2]^3 with the constant value vol[i][j][k]; the volume is
// [-1/2, n_a - 1/2] on each axis and zero outside.
#pragma once
#include "ray_sampling.hpp"

namespace r2 {

// One axis of a ray: start s, reciprocal direction rd = 1 / d (one correctly rounded division), and `flat`: d is 0, or so
// small that 1 / d overflows -- the ray does not cross this axis's planes, it lies in one slab of it (or in none).
struct SiddonAxis {
    float s, rd;
    bool flat;
};

__device__ __forceinline__ SiddonAxis siddon_axis(float s, float d)
{
    SiddonAxis a;
    a.s = s;
    a.rd = 1.0f / d;
    a.flat = !(fabsf(a.rd) < INFINITY);
    return a;
}

// The ray parameter of plane m (m = 0..n_a, at q = m - 1/2) of a non-flat axis, from the integer m: (float)m - 1/2 is
// exact, then one rounded subtraction and one rounded product.  Every step is monotone, so plane_t is monotone in m
// (non-decreasing for d > 0, non-increasing for d < 0) and carries no drift along the ray: it is never accumulated.
__device__ __forceinline__ float plane_t(const SiddonAxis &a, int m) { return (((float)m - 0.5f) - a.s) * a.rd; }

// Does voxel slab m (q in [m - 1/2, m + 1/2)) of a flat axis hold the ray?  Exact comparisons on exact floats.
__device__ __forceinline__ bool flat_in_slab(const SiddonAxis &a, int m)
{
    return a.s >= (float)m - 0.5f && a.s < (float)m + 0.5f;
}

// The slab of a flat axis that holds the ray, or -1 when the ray passes the volume by on this axis.
__device__ __forceinline__ int flat_slab(const SiddonAxis &a, int n)
{
    if (!(a.s >= -0.5f && a.s < (float)n - 0.5f)) return -1;
    int m = (int)floorf(fminf(fmaxf(a.s + 0.5f, 0.0f), (float)(n - 1)));
    // s + 1/2 is rounded: settle the index with the exact comparisons flat_in_slab makes
    if (m > 0 && a.s < (float)m - 0.5f) --m;
    else if (m < n - 1 && a.s >= (float)m + 0.5f) ++m;
    return m;
}

struct SiddonRay {
    SiddonAxis x, y, z;
    float t0, t1;     // the clip to the volume
    float wlen;       // |d (.) dVoxel|: world length per unit t
    bool hit;         // false: the ray contributes nothing (misses, t1 <= t0, no direction, or non-finite parameters)
};

__device__ __forceinline__ bool siddon_clip_axis(const SiddonAxis &a, int n, float &t0, float &t1)
{
    if (a.flat) return a.s >= -0.5f && a.s < (float)n - 0.5f;
    const float ta = plane_t(a, 0), tb = plane_t(a, n);
    t0 = fmaxf(t0, fminf(ta, tb));
    t1 = fminf(t1, fmaxf(ta, tb));
    return true;
}

// Set the ray up against the volume: the three axes, [t0, t1] built from plane_t(., 0) and plane_t(., n_a) (t0 >= 0 for a
// cone ray), and wlen as ray_sampling computes it.
__device__ __forceinline__ SiddonRay siddon_ray(const Ray &y, int cone, int nx, int ny, int nz, float3 dv)
{
    SiddonRay q;
    q.x = siddon_axis(y.sx, y.dx);
    q.y = siddon_axis(y.sy, y.dy);
    q.z = siddon_axis(y.sz, y.dz);
    q.t0 = cone ? 0.0f : -INFINITY;
    q.t1 = INFINITY;
    const bool inside = siddon_clip_axis(q.x, nx, q.t0, q.t1) & siddon_clip_axis(q.y, ny, q.t0, q.t1) &
                        siddon_clip_axis(q.z, nz, q.t0, q.t1);
    const bool finite = fabsf(y.sx) + fabsf(y.sy) + fabsf(y.sz) + fabsf(y.dx) + fabsf(y.dy) + fabsf(y.dz) < INFINITY;
    const bool moves = !(q.x.flat & q.y.flat & q.z.flat);
    q.hit = inside && finite && moves && q.t1 > q.t0;
    const float wx = y.dx * dv.x, wy = y.dy * dv.y, wz = y.dz * dv.z;
    q.wlen = sqrtf(wx * wx + wy * wy + wz * wz);
    return q;
}

// The interval of t one axis allows voxel slab m: [lo, hi] between plane_t(m) and plane_t(m + 1); a flat axis allows all t
// when the ray lies in the slab and none otherwise (returns false).
__device__ __forceinline__ bool siddon_slab(const SiddonAxis &a, int m, float &lo, float &hi)
{
    if (a.flat) return flat_in_slab(a, m);
    const float ta = plane_t(a, m), tb = plane_t(a, m + 1);
    lo = fmaxf(lo, fminf(ta, tb));
    hi = fminf(hi, fmaxf(ta, tb));
    return true;
}

// The matrix entry A[rho, v] of a ray that hits, for voxel v = (i, j, k): wlen max(0, min(t1, min_a hi_a) - max(t0, max_a
// lo_a)).
__device__ __forceinline__ float siddon_entry(const SiddonRay &q, int i, int j, int k)
{
    float lo = q.t0, hi = q.t1;
    const bool in = siddon_slab(q.x, i, lo, hi) & siddon_slab(q.y, j, lo, hi) & siddon_slab(q.z, k, lo, hi);
    if (!in || !(hi > lo)) return 0.0f;
    return q.wlen * (hi - lo);
}

}  // namespace r2
