// ray_sampling.hpp -- the ray of one detector pixel and its midpoint samples, as r2_project_volume defines them
// (include/r2hip.h).  Shared by the forward projector (projector.hip) and its exact transpose (backprojector.hip): the
// adjoint is only exact if both take the same clip points, sample count, sample positions and trilinear weights, so they
// are written once, here.  Both translation units are compiled with -ffp-contract=off (build.py: EXACT), so every float
// below is the same separately rounded operation in both.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace r2 {

// Clip the line s + t d to the slab -1 <= q <= n of one axis.  Returns false when the line misses it.
__device__ __forceinline__ bool clip_axis(float s, float d, int n, float &t0, float &t1)
{
    const float lo = -1.0f, hi = (float)n;
    if (d == 0.0f) return s > lo && s < hi;
    const float ta = (lo - s) / d, tb = (hi - s) / d;
    t0 = fmaxf(t0, fminf(ta, tb));
    t1 = fminf(t1, fmaxf(ta, tb));
    return true;
}

// One axis of the trilinear footprint: the two neighbour indices clamped into the volume, and their weights, zero for a
// neighbour outside it.
struct Axis {
    int i0, i1;
    float w0, w1;
};

__device__ __forceinline__ Axis axis_of(float q, int n)
{
    // q lies in [-1, n] up to rounding; clamp before the int conversion so that no rounding can overflow it
    const float f = floorf(fminf(fmaxf(q, -2.0f), (float)n + 1.0f));
    const int i = (int)f;
    const float w = q - f;
    Axis a;
    a.w0 = (unsigned)i < (unsigned)n ? 1.0f - w : 0.0f;
    a.w1 = (unsigned)(i + 1) < (unsigned)n ? w : 0.0f;
    a.i0 = min(max(i, 0), n - 1);
    a.i1 = min(max(i + 1, 0), n - 1);
    return a;
}

// The start s and direction d of the ray of pixel (r, c) of the view whose 12 ray parameters are R (include/r2hip.h).
struct Ray {
    float sx, sy, sz, dx, dy, dz;
};

__device__ __forceinline__ Ray pixel_ray(const float *R, int cone, int r, int c)
{
    const float fc = (float)c, fr = (float)r;
    const float px = R[3] + fc * R[6] + fr * R[9];
    const float py = R[4] + fc * R[7] + fr * R[10];
    const float pz = R[5] + fc * R[8] + fr * R[11];
    float sx, sy, sz, dx, dy, dz;
    if (cone) {
        sx = R[0]; sy = R[1]; sz = R[2];
        dx = px - sx; dy = py - sy; dz = pz - sz;
    } else {
        sx = px; sy = py; sz = pz;
        dx = R[0]; dy = R[1]; dz = R[2];
    }
    return Ray{sx, sy, sz, dx, dy, dz};
}

// Clip the ray to the support [-1, n_a] of the trilinear interpolant: [t0, t1].  Returns false when it misses.
__device__ __forceinline__ bool clip_ray(const Ray &y, int cone, int nx, int ny, int nz, float &t0, float &t1)
{
    t0 = cone ? 0.0f : -INFINITY;
    t1 = INFINITY;
    const bool inside = clip_axis(y.sx, y.dx, nx, t0, t1) & clip_axis(y.sy, y.dy, ny, t0, t1) & clip_axis(y.sz, y.dz, nz, t0, t1);
    return inside && t1 > t0;
}

// The sampling of a ray that hits: n = max(1, ceil(L / accuracy)) pieces of length dt in t, and |d_world|, the world
// length per unit t (the direction scaled back from index units by the voxel size).
struct Sampling {
    int n;
    float dt, wlen;
};

__device__ __forceinline__ Sampling ray_sampling(const Ray &y, float t0, float t1, float3 dv, float accuracy)
{
    const float span = t1 - t0;
    const float len = sqrtf(y.dx * y.dx + y.dy * y.dy + y.dz * y.dz);
    const float nf = ceilf(span * len / accuracy);
    Sampling m;
    m.n = max(1, (int)fminf(nf, 1073741824.0f));
    m.dt = span / (float)m.n;
    const float wx = y.dx * dv.x, wy = y.dy * dv.y, wz = y.dz * dv.z;
    m.wlen = sqrtf(wx * wx + wy * wy + wz * wz);
    return m;
}

// Sample k of the ray: its parameter t_k = t0 + (k + 1/2) dt, contracted by hand as the contract states.
__device__ __forceinline__ float sample_t(int k, float dt, float t0) { return fmaf((float)k + 0.5f, dt, t0); }

}  // namespace r2
