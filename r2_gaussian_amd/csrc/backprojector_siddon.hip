// backprojector_siddon.hip -- the exact transpose of the Siddon forward projector (projector_siddon.hip): vol = A^T projs
// with A[rho, v] = |d_world| * (the length of t the ray rho spends in voxel v), the entry include/r2hip.h states for
// r2_project_volume_siddon.
//
// Voxel-driven gather, one thread per voxel, no atomics.  An entry is one clip of the ray against the voxel's cube: no
// sample loop and no 8-corner footprint, which is what makes this adjoint cheap next to backprojector.hip's.  For each view
// (in order) the thread
//   1. projects the 8 corners of the voxel's cube [i - 1/2, i + 1/2]^3 onto the detector and takes their bounding box in
//      pixels, widened by one pixel on every side (the view's 3x3 matrix B^-1 as in backprojector.hip); when a corner lies on
//      or behind the source plane (a cone source inside or beside the cube) the box is the whole detector;
//   2. for each pixel of the box, clips the pixel's ray to the cube widened by 1/16 voxel with approximate reciprocals (only
//      a filter) and drops the pixels whose rays pass it by;
//   3. for the rest, sets the ray up exactly as the forward does (siddon_ray.hpp: the three axes, the clip to the volume,
//      |d_world|) and evaluates the entry from plane_t of the voxel's six planes.
// The box and the filter only decide which pixels are looked at; the entries are the forward's, bit for bit.  Each voxel's
// sum runs in a fixed order (views, pixel rows, columns) in one thread, so the result is bit-reproducible and does not
// depend on what `vol` held before.
//
// Compiled with -ffp-contract=off (build.py: EXACT) like projector_siddon.hip.
#include "r2_common.hpp"
#include "siddon_ray.hpp"
#include <math.h>

namespace r2 {

namespace {

constexpr int BZ = 16, BY = 4, BX = 4;   // a block: 16 z x 4 y voxels per wave, 4 waves along x
constexpr int NT = BZ * BY * BX;
constexpr float HALF = 0.5f;             // the cube's half width, index units
constexpr float WIDEN = 0.0625f;         // cube widening of the pixel filter (step 2), index units

__device__ __forceinline__ float cross_dot(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                                           float cz)
{
    // (a x b) . c
    return (ay * bz - az * by) * cx + (az * bx - ax * bz) * cy + (ax * by - ay * bx) * cz;
}

// Clip t to the slab |s + t d - i| <= 1/2 + WIDEN of one axis, with an approximate reciprocal of d.  false: the line misses.
__device__ __forceinline__ bool widened_slab(float s, float d, int i, float &lo, float &hi)
{
    const float a = (float)i - (HALF + WIDEN) - s, b = (float)i + (HALF + WIDEN) - s;
    if (d == 0.0f) return a <= 0.0f && b >= 0.0f;
    const float rd = __builtin_amdgcn_rcpf(d);
    const float ta = a * rd, tb = b * rd;
    lo = fmaxf(lo, fminf(ta, tb));
    hi = fminf(hi, fmaxf(ta, tb));
    return true;
}

__global__ void __launch_bounds__(NT) backproject_siddon_kernel(int V, int H, int W, const float *__restrict__ rays,
                                                                int cone, int nx, int ny, int nz, float3 dv,
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
        // B = [pu pv e] with e = p00 - a (cone: B^-1 (q - a) = lambda (c, r, 1)) or e = a (parallel: B^-1 (q - p00) =
        // (c, r, t)); B^-1 = adj(B) / det, rows (pv x e, e x pu, pu x pv) / det
        const float pux = R[6], puy = R[7], puz = R[8], pvx = R[9], pvy = R[10], pvz = R[11];
        const float ex = cone ? R[3] - R[0] : R[0], ey = cone ? R[4] - R[1] : R[1], ez = cone ? R[5] - R[2] : R[2];
        const float ox = cone ? R[0] : R[3], oy = cone ? R[1] : R[4], oz = cone ? R[2] : R[5];
        const float rdet = 1.0f / cross_dot(pvx, pvy, pvz, ex, ey, ez, pux, puy, puz);
        // rows of B^-1
        const float m00 = (pvy * ez - pvz * ey) * rdet, m01 = (pvz * ex - pvx * ez) * rdet, m02 = (pvx * ey - pvy * ex) * rdet;
        const float m10 = (ey * puz - ez * puy) * rdet, m11 = (ez * pux - ex * puz) * rdet, m12 = (ex * puy - ey * pux) * rdet;
        const float m20 = (puy * pvz - puz * pvy) * rdet, m21 = (puz * pvx - pux * pvz) * rdet, m22 = (pux * pvy - puy * pvx) * rdet;
        const float qx = fi - ox, qy = fj - oy, qz = fk - oz;
        const float cx = m00 * qx + m01 * qy + m02 * qz, cy = m10 * qx + m11 * qy + m12 * qz, cz = m20 * qx + m21 * qy + m22 * qz;
        float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY, zmin = INFINITY;
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            const float sa = (corner & 1) ? HALF : -HALF, sb = (corner & 2) ? HALF : -HALF, sc = (corner & 4) ? HALF : -HALF;
            const float X = cx + sa * m00 + sb * m01 + sc * m02;
            const float Y = cy + sa * m10 + sb * m11 + sc * m12;
            const float Z = cz + sa * m20 + sb * m21 + sc * m22;
            const float rz = cone ? __builtin_amdgcn_rcpf(Z) : 1.0f;
            umin = fminf(umin, X * rz); umax = fmaxf(umax, X * rz);
            vmin = fminf(vmin, Y * rz); vmax = fmaxf(vmax, Y * rz);
            zmin = fminf(zmin, Z);
        }
        int c0 = 0, c1 = W - 1, r0 = 0, r1 = H - 1;
        // a cube that reaches the source plane, or any non-finite coordinate, takes the whole detector
        const bool bounded = (!cone || zmin > 0.0f) && umin >= -1e30f && umax <= 1e30f && vmin >= -1e30f && vmax <= 1e30f;
        if (bounded) {
            // clamped on both sides in float before the conversion: a box off the detector comes out empty (c0 > c1)
            c0 = (int)fminf(fmaxf(floorf(umin) - 1.0f, 0.0f), (float)W);
            c1 = (int)fmaxf(fminf(ceilf(umax) + 1.0f, (float)(W - 1)), -1.0f);
            r0 = (int)fminf(fmaxf(floorf(vmin) - 1.0f, 0.0f), (float)H);
            r1 = (int)fmaxf(fminf(ceilf(vmax) + 1.0f, (float)(H - 1)), -1.0f);
        }
        const float *P = projs + (size_t)view * H * W;
        float vsum = 0.0f;
        for (int r = r0; r <= r1; ++r) {
            for (int c = c0; c <= c1; ++c) {
                const Ray y = pixel_ray(R, cone, r, c);
                float lo = cone ? 0.0f : -INFINITY, hi = INFINITY;
                const bool near = widened_slab(y.sx, y.dx, i, lo, hi) & widened_slab(y.sy, y.dy, j, lo, hi) &
                                  widened_slab(y.sz, y.dz, k, lo, hi);
                if (!near || !(hi >= lo)) continue;
                const SiddonRay q = siddon_ray(y, cone, nx, ny, nz, dv);
                if (!q.hit) continue;
                const float entry = siddon_entry(q, i, j, k);
                if (entry != 0.0f) vsum += entry * P[(size_t)r * W + c];
            }
        }
        total += vsum;
    }
    vol[((size_t)i * ny + j) * nz + k] = total;
}

}  // namespace

}  // namespace r2

extern "C" int r2_backproject_volume_siddon(int V, int H, int W, const float *rays, int cone, int nx, int ny, int nz,
                                            float dVoxel_x, float dVoxel_y, float dVoxel_z, const float *projs, float *vol,
                                            void *stream)
{
    using namespace r2;
    if (V <= 0 || H <= 0 || W <= 0 || nx <= 0 || ny <= 0 || nz <= 0 || !rays || !projs || !vol || !(dVoxel_x > 0.f) ||
        !(dVoxel_y > 0.f) || !(dVoxel_z > 0.f)) {
        set_error("r2_backproject_volume_siddon: invalid argument");
        return R2_ERR_INVALID;
    }
    // the forward's limits, plus the voxel grid's
    if ((long long)ny * nz >= (1LL << 32) || V > 65535 || (H + 15) / 16 > 65535 || (ny + BY - 1) / BY > 65535 ||
        (nx + BX - 1) / BX > 65535) {
        set_error("r2_backproject_volume_siddon: shape out of range (V %d, H %d, nx %d, ny %d, ny*nz %lld)", V, H, nx, ny,
                  (long long)ny * nz);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((nz + BZ - 1) / BZ, (ny + BY - 1) / BY, (nx + BX - 1) / BX);
    backproject_siddon_kernel<<<grid, dim3(NT), 0, s>>>(V, H, W, rays, cone, nx, ny, nz,
                                                        make_float3(dVoxel_x, dVoxel_y, dVoxel_z), projs, vol);
    R2_STAGE_CHECK(0, s, "backproject volume siddon");
    return 0;
}
