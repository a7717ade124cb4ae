// projector_siddon.hip -- ray-driven forward projection of a voxel volume with the Siddon (ray-voxel intersection) model:
// the exact radiological path through a piecewise-constant voxel grid.  projector.hip is the interpolated model; the rays,
// coordinates and ray parameters are the same (ray_sampling.hpp: pixel_ray), the voxel model is siddon_ray.hpp's.
//
// One thread per detector pixel.  The ray is clipped to the volume ([t0, t1]; a ray that misses writes 0) and walked cell by
// cell (Amanatides-Woo / Jacobs): each axis keeps an integer counter m_a of the next plane it will cross and that plane's
// parameter plane_t(m_a), recomputed from the integer every time; the axis with the smallest one advances, ties in the
// fixed order x, y, z, and the cell index moves by that axis's integer step.  Each segment adds (t_next - t_cur) vol[cell]
// in order in one thread, and the sum is scaled by |d_world| once: no atomics, and each pixel's bits depend only on its own
// ray.  Because plane_t is monotone in m, the interval the walk spends in a cell is exactly the intersection of the
// per-axis intervals that include/r2hip.h states as the matrix entry, which is what backprojector_siddon.hip gathers.
//
// The walk stays inside the volume by construction: an axis only advances while its next plane lies strictly before
// t1 <= plane_t(last plane of that axis), so by monotonicity the plane crossed is never the volume's last one.  A NaN never
// compares smaller, so it neither advances an axis nor keeps the loop alive.
//
// The gather of a cell does not depend on the value of the one before, only on the plane parameters: the loop loads the
// next cell's value before it adds the current segment, so one gather is in flight while the next step is computed.
//
// Work order as in projector.hip: blockIdx.z is the view, each wave covers an 8 x 8 pixel tile.
#include "siddon_ray.hpp"
#include "volume_entry.hpp"
#include <math.h>

namespace r2 {

namespace {

// The walk's state on one axis: the cell index, its step (+1, -1, or 0 on a flat axis), the next plane m and plane_t(m).
struct Walk {
    int i, step, m;
    float t;
};

// The cell of the ray at t0 on one axis and the first plane after it.  The estimate from the position at t0 is settled
// with plane_t itself: plane_t(entry plane of i) <= t0 < plane_t(exit plane of i), the order the walk then keeps.
__device__ __forceinline__ Walk walk_start(const SiddonAxis &a, float d, int n, float t0)
{
    Walk w;
    if (a.flat) {
        w.i = max(flat_slab(a, n), 0);   // a hit ray lies in a slab
        w.step = 0;
        w.m = 0;
        w.t = INFINITY;
        return w;
    }
    int i = (int)floorf(fminf(fmaxf(a.s + t0 * d + 0.5f, 0.0f), (float)(n - 1)));
    if (d > 0.0f) {
        while (i > 0 && plane_t(a, i) > t0) --i;
        while (i < n - 1 && plane_t(a, i + 1) <= t0) ++i;
        w.step = 1;
        w.m = i + 1;
    } else {
        while (i < n - 1 && plane_t(a, i + 1) > t0) ++i;
        while (i > 0 && plane_t(a, i) <= t0) --i;
        w.step = -1;
        w.m = i;
    }
    w.i = i;
    w.t = plane_t(a, w.m);
    return w;
}

template <typename OFF>
__global__ void __launch_bounds__(PB) project_siddon_kernel(int H, int W, const float *__restrict__ rays, int cone, int nx,
                                                            int ny, int nz, float3 dv, const float *__restrict__ vol,
                                                            float *__restrict__ out)
{
    int r, c;
    if (!thread_pixel(H, W, r, c)) return;
    const int view = blockIdx.z;
    const Ray y = pixel_ray(rays + 12 * view, cone, r, c);
    const SiddonRay q = siddon_ray(y, cone, nx, ny, nz, dv);
    float *o = out + ((size_t)view * H + r) * W + c;
    if (!q.hit) {
        *o = 0.0f;
        return;
    }
    const float t1 = q.t1;
    Walk X = walk_start(q.x, y.dx, nx, q.t0), Y = walk_start(q.y, y.dy, ny, q.t0), Z = walk_start(q.z, y.dz, nz, q.t0);
    // voxel offsets: unsigned 32-bit when the volume has fewer than 2^32 voxels (OFF = unsigned), 64-bit otherwise; the
    // steps are added modulo 2^width, so a negative step is its two's complement
    const OFF sx = (OFF)ny * (OFF)nz * (OFF)X.step, sy = (OFF)nz * (OFF)Y.step, sz = (OFF)Z.step;
    OFF off = ((OFF)X.i * (OFF)ny + (OFF)Y.i) * (OFF)nz + (OFF)Z.i;
    float t = q.t0, acc = 0.0f;
    float v = vol[off];
    for (;;) {
        const float tyz = fminf(Y.t, Z.t);
        const float tn = fminf(X.t, tyz);
        if (!(tn < t1)) break;
        if (X.t <= tyz) {
            X.m += X.step;
            X.t = plane_t(q.x, X.m);
            off += sx;
        } else if (Y.t <= Z.t) {
            Y.m += Y.step;
            Y.t = plane_t(q.y, Y.m);
            off += sy;
        } else {
            Z.m += Z.step;
            Z.t = plane_t(q.z, Z.m);
            off += sz;
        }
        const float vn = vol[off];
        acc += (tn - t) * v;
        t = tn;
        v = vn;
    }
    acc += (t1 - t) * v;
    *o = acc * q.wlen;
}

}  // namespace

}  // namespace r2

extern "C" int r2_project_volume_siddon(int V, int H, int W, const float *rays, int cone, int nx, int ny, int nz,
                                        float dVoxel_x, float dVoxel_y, float dVoxel_z, const float *vol, float *out,
                                        void *stream)
{
    using namespace r2;
    if (const int rc = check_forward_args("r2_project_volume_siddon", V, H, W, rays, nx, ny, nz, dVoxel_x, dVoxel_y,
                                          dVoxel_z, nullptr, vol, out))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid = volume_pixel_grid(V, H, W);
    const float3 d = make_float3(dVoxel_x, dVoxel_y, dVoxel_z);
    if ((unsigned long long)nx * ny * nz < (1ULL << 32))
        project_siddon_kernel<unsigned><<<grid, dim3(PB), 0, s>>>(H, W, rays, cone, nx, ny, nz, d, vol, out);
    else
        project_siddon_kernel<size_t><<<grid, dim3(PB), 0, s>>>(H, W, rays, cone, nx, ny, nz, d, vol, out);
    R2_STAGE_CHECK(0, s, "project volume siddon");
    return 0;
}
