// voxel_gather.hpp -- the voxel-driven gather of the exact adjoints (backprojector.hip, backprojector_siddon.hip):
// vol = A^T projs for a projector model whose matrix entry A[rho, v] can be evaluated for one (ray, voxel) pair.
//
// One thread per voxel, no atomics.  A model is a struct with
//   static constexpr float HALF                     the half width of a voxel's support, in index units, and
//   float entry(y, cone, nx, ny, nz, dv, i, j, k, lo, hi) const
//                                                   A[rho, v] for the ray y of a pixel and the voxel v = (i, j, k), from
//                                                   the forward's own arithmetic; [lo, hi] is the filter's interval of t.
// For each view (in order) the thread
//   1. projects the 8 corners of the voxel's support [i - HALF, i + HALF]^3 onto the detector and takes their bounding
//      box in pixels, widened by one pixel on every side (the view's 3x3 matrix B^-1 maps index space to detector
//      coordinates: a projective map for cone beams, affine for parallel ones, so the box of a convex support is the box
//      of its corners); when a corner lies on or behind the source plane (a cone source inside or beside the support)
//      the box is the whole detector;
//   2. for each pixel of the box, clips the pixel's ray to the support widened by 1/16 voxel (approximate reciprocals:
//      only a filter) and drops the pixels whose rays pass it by;
//   3. for the rest, asks the model for the entry.
// The box and the filter only decide which pixels are looked at, and must never drop one that carries weight; each
// model's file says why its support makes them safe.  The entries are the forward's.  Each voxel's sum runs in a fixed
// order (views, pixel rows, columns, then whatever the model sums) in one thread, so the result is bit-reproducible and
// does not depend on what `vol` held before.
#pragma once
#include "ray_sampling.hpp"
#include "volume_entry.hpp"
#include <math.h>

namespace r2 {

constexpr int BZ = 16, BY = 4, BX = 4;   // a block: 16 z x 4 y voxels per wave, 4 waves along x
constexpr int NT = BZ * BY * BX;
constexpr float WIDEN = 0.0625f;         // support widening of the pixel filter (step 2), index units

__device__ __forceinline__ float cross_dot(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                                           float cz)
{
    // (a x b) . c
    return (ay * bz - az * by) * cx + (az * bx - ax * bz) * cy + (ax * by - ay * bx) * cz;
}

// A view's map from index space to the detector: B = [pu pv e] with e = p00 - a (cone: B^-1 (q - a) = lambda (c, r, 1))
// or e = a (parallel: B^-1 (q - p00) = (c, r, t)); B^-1 = adj(B) / det, rows (pv x e, e x pu, pu x pv) / det.
struct DetectorMap {
    float m00, m01, m02, m10, m11, m12, m20, m21, m22;   // rows of B^-1
    float ox, oy, oz;                                    // the origin q is taken from: a (cone) or p00 (parallel)
};

__device__ __forceinline__ DetectorMap detector_map(const float *R, int cone)
{
    const float pux = R[6], puy = R[7], puz = R[8], pvx = R[9], pvy = R[10], pvz = R[11];
    const float ex = cone ? R[3] - R[0] : R[0], ey = cone ? R[4] - R[1] : R[1], ez = cone ? R[5] - R[2] : R[2];
    DetectorMap B;
    B.ox = cone ? R[0] : R[3]; B.oy = cone ? R[1] : R[4]; B.oz = cone ? R[2] : R[5];
    const float rdet = 1.0f / cross_dot(pvx, pvy, pvz, ex, ey, ez, pux, puy, puz);
    B.m00 = (pvy * ez - pvz * ey) * rdet; B.m01 = (pvz * ex - pvx * ez) * rdet; B.m02 = (pvx * ey - pvy * ex) * rdet;
    B.m10 = (ey * puz - ez * puy) * rdet; B.m11 = (ez * pux - ex * puz) * rdet; B.m12 = (ex * puy - ey * pux) * rdet;
    B.m20 = (puy * pvz - puz * pvy) * rdet; B.m21 = (puz * pvx - pux * pvz) * rdet; B.m22 = (pux * pvy - puy * pvx) * rdet;
    return B;
}

// Step 1: the pixels [r0, r1] x [c0, c1] that the support of half width HALF around (fi, fj, fk) can reach.
struct PixelBox {
    int r0, r1, c0, c1;
};

template <typename Model>
__device__ __forceinline__ PixelBox footprint_box(const DetectorMap &B, int cone, float fi, float fj, float fk, int H, int W)
{
    constexpr float HALF = Model::HALF;
    const float qx = fi - B.ox, qy = fj - B.oy, qz = fk - B.oz;
    const float cx = B.m00 * qx + B.m01 * qy + B.m02 * qz, cy = B.m10 * qx + B.m11 * qy + B.m12 * qz,
                cz = B.m20 * qx + B.m21 * qy + B.m22 * qz;
    float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY, zmin = INFINITY;
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const float sa = (corner & 1) ? HALF : -HALF, sb = (corner & 2) ? HALF : -HALF, sc = (corner & 4) ? HALF : -HALF;
        const float X = cx + sa * B.m00 + sb * B.m01 + sc * B.m02;
        const float Y = cy + sa * B.m10 + sb * B.m11 + sc * B.m12;
        const float Z = cz + sa * B.m20 + sb * B.m21 + sc * B.m22;
        const float rz = cone ? __builtin_amdgcn_rcpf(Z) : 1.0f;
        umin = fminf(umin, X * rz); umax = fmaxf(umax, X * rz);
        vmin = fminf(vmin, Y * rz); vmax = fmaxf(vmax, Y * rz);
        zmin = fminf(zmin, Z);
    }
    PixelBox b{0, H - 1, 0, W - 1};
    // a support that reaches the source plane, or any non-finite coordinate, takes the whole detector
    const bool bounded = (!cone || zmin > 0.0f) && umin >= -1e30f && umax <= 1e30f && vmin >= -1e30f && vmax <= 1e30f;
    if (bounded) {
        // clamped on both sides in float before the conversion: a box off the detector comes out empty (c0 > c1)
        b.c0 = (int)fminf(fmaxf(floorf(umin) - 1.0f, 0.0f), (float)W);
        b.c1 = (int)fmaxf(fminf(ceilf(umax) + 1.0f, (float)(W - 1)), -1.0f);
        b.r0 = (int)fminf(fmaxf(floorf(vmin) - 1.0f, 0.0f), (float)H);
        b.r1 = (int)fmaxf(fminf(ceilf(vmax) + 1.0f, (float)(H - 1)), -1.0f);
    }
    return b;
}

// Step 2, one axis: clip t to the slab |s + t d - i| <= HALF + WIDEN, with an approximate reciprocal of d.  false: the
// line misses.
template <typename Model>
__device__ __forceinline__ bool widened_slab(float s, float d, int i, float &lo, float &hi)
{
    const float a = (float)i - (Model::HALF + WIDEN) - s, b = (float)i + (Model::HALF + WIDEN) - s;
    if (d == 0.0f) return a <= 0.0f && b >= 0.0f;
    const float rd = __builtin_amdgcn_rcpf(d);
    const float ta = a * rd, tb = b * rd;
    lo = fmaxf(lo, fminf(ta, tb));
    hi = fminf(hi, fmaxf(ta, tb));
    return true;
}

template <typename Model>
__global__ void __launch_bounds__(NT) gather_kernel(int V, int H, int W, const float *__restrict__ rays, int cone, int nx,
                                                    int ny, int nz, float3 dv, Model model,
                                                    const float *__restrict__ projs, float *__restrict__ vol)
{
    const int k = blockIdx.x * BZ + (threadIdx.x & (BZ - 1));
    const int j = blockIdx.y * BY + ((threadIdx.x / BZ) & (BY - 1));
    const int i = blockIdx.z * BX + threadIdx.x / (BZ * BY);
    if (i >= nx || j >= ny || k >= nz) return;
    const float fi = (float)i, fj = (float)j, fk = (float)k;
    float total = 0.0f;
    for (int view = 0; view < V; ++view) {
        const float *R = rays + 12 * view;
        const PixelBox box = footprint_box<Model>(detector_map(R, cone), cone, fi, fj, fk, H, W);
        const float *P = projs + (size_t)view * H * W;
        float vsum = 0.0f;
        for (int r = box.r0; r <= box.r1; ++r) {
            for (int c = box.c0; c <= box.c1; ++c) {
                const Ray y = pixel_ray(R, cone, r, c);
                float lo = cone ? 0.0f : -INFINITY, hi = INFINITY;
                const bool near = widened_slab<Model>(y.sx, y.dx, i, lo, hi) & widened_slab<Model>(y.sy, y.dy, j, lo, hi) &
                                  widened_slab<Model>(y.sz, y.dz, k, lo, hi);
                if (!near || !(hi >= lo)) continue;
                const float entry = model.entry(y, cone, nx, ny, nz, dv, i, j, k, lo, hi);
                if (entry != 0.0f) vsum += entry * P[(size_t)r * W + c];
            }
        }
        total += vsum;
    }
    vol[((size_t)i * ny + j) * nz + k] = total;
}

// The entry point of an adjoint: `fn` names it in error texts, `stage` in a failed launch's; `accuracy` as in
// volume_args_valid.  The forward's shape limits, plus the voxel grid's.
template <typename Model>
int launch_gather(const char *fn, const char *stage, Model model, const float *accuracy, int V, int H, int W,
                  const float *rays, int cone, int nx, int ny, int nz, float dx, float dy, float dz, const float *projs,
                  float *vol, void *stream)
{
    if (!volume_args_valid(fn, V, H, W, rays, nx, ny, nz, dx, dy, dz, accuracy, projs, vol)) return R2_ERR_INVALID;
    if (!forward_shape_in_range(V, H, ny, nz) || (ny + BY - 1) / BY > 65535 || (nx + BX - 1) / BX > 65535) {
        set_error("%s: shape out of range (V %d, H %d, nx %d, ny %d, ny*nz %lld)", fn, V, H, nx, ny, (long long)ny * nz);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((nz + BZ - 1) / BZ, (ny + BY - 1) / BY, (nx + BX - 1) / BX);
    gather_kernel<Model><<<grid, dim3(NT), 0, s>>>(V, H, W, rays, cone, nx, ny, nz, make_float3(dx, dy, dz), model, projs, vol);
    R2_STAGE_CHECK(0, s, stage);
    return 0;
}

}  // namespace r2
