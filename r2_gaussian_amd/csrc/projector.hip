// projector.hip -- ray-driven forward projection of a voxel volume: the counterpart of tigre.Ax, which the reference's data
// generator calls to turn a CT volume into its training and test projections
// (data_generator/synthetic_dataset/generate_data.py:47-69).  fdk.hip is the back-projection half of the pair.
//
// One thread per detector pixel.  The ray of pixel (r, c) is P(r, c) = p00 + c pu + r pv, in voxel-index coordinates
// (voxel (i,j,k) at integer q): a cone ray runs from the source s through P for t >= 0, a parallel ray through P along the
// direction a for all t.  The host derives those 12 floats per view from the rasterizer's camera (projector.py), so the
// projections are registered to rendered images by construction.
//
// The integrand is the trilinear interpolant of the volume with zero outside [0, n_a - 1], whose support is [-1, n_a].  The
// ray is clipped to that box analytically ([t0, t1]; a ray that misses writes 0 and costs nothing), and the chord is cut into
// n = max(1, ceil(L / accuracy)) equal pieces (L: chord length in index units) sampled at their midpoints:
//     out = (t1 - t0)/n * |d|_world * sum_k f(q(t0 + (k + 1/2)(t1 - t0)/n)).
// The sum runs over k in order in one thread: no atomics, and each pixel's bits depend only on its own ray.
//
// Work order: blockIdx.z is the view, so the grid walks the views one after the other and the volume stays in the Infinity
// Cache while a view's rays traverse it; each wave covers an 8 x 8 pixel tile, so its 64 rays walk neighbouring voxels.
// Hardware-filtered texture sampling is not used: its interpolation weights are fixed-point with 8 fractional bits
// (an error of up to 2^-9 of the local voxel difference per sample), far beyond the float32 explicit gathers' error.
//
// This TU is compiled with -ffp-contract=off (build.py: EXACT): the clip points and n are separately rounded float32
// operations, so the float64 restatement (tests/projector_ref.py) can tell which pixels sit on a decision boundary.  The
// sampling loop contracts by hand (fmaf), where the restatement's bound covers it.
#include "trilinear.hpp"
#include "volume_entry.hpp"
#include <math.h>

namespace r2 {

namespace {

template <typename OFF>
__global__ void __launch_bounds__(PB) project_kernel(int H, int W, const float *__restrict__ rays, int cone, int nx, int ny,
                                                     int nz, float3 dv, float accuracy, const float *__restrict__ vol,
                                                     float *__restrict__ out)
{
    int r, c;
    if (!thread_pixel(H, W, r, c)) return;
    const int view = blockIdx.z;
    const Ray y = pixel_ray(rays + 12 * view, cone, r, c);
    float t0, t1;
    const bool hit = clip_ray(y, cone, nx, ny, nz, t0, t1);
    float *o = out + ((size_t)view * H + r) * W + c;
    if (!hit) {
        *o = 0.0f;
        return;
    }
    const Sampling m = ray_sampling(y, t0, t1, dv, accuracy);
    const float sx = y.sx, sy = y.sy, sz = y.sz, dx = y.dx, dy = y.dy, dz = y.dz;
    const int ns = m.n;
    const float dt = m.dt, wlen = m.wlen;
    // voxel offsets: unsigned 32-bit when the volume has fewer than 2^32 voxels (OFF = unsigned), 64-bit otherwise
    const OFF sxy = (OFF)ny * (OFF)nz;
    float acc = 0.0f;
    for (int k = 0; k < ns; ++k) {
        const float t = sample_t(k, dt, t0);
        const Axis X = axis_of(fmaf(t, dx, sx), nx), Y = axis_of(fmaf(t, dy, sy), ny), Z = axis_of(fmaf(t, dz, sz), nz);
        acc += trilinear<OFF>(vol, X, Y, Z, sxy, nz);
    }
    *o = acc * (dt * wlen);
}

}  // namespace

}  // namespace r2

extern "C" int r2_project_volume(int V, int H, int W, const float *rays, int cone, int nx, int ny, int nz, float dVoxel_x,
                                 float dVoxel_y, float dVoxel_z, float accuracy, const float *vol, float *out, void *stream)
{
    using namespace r2;
    if (const int rc = check_forward_args("r2_project_volume", V, H, W, rays, nx, ny, nz, dVoxel_x, dVoxel_y, dVoxel_z,
                                          &accuracy, vol, out))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid = volume_pixel_grid(V, H, W);
    const float3 d = make_float3(dVoxel_x, dVoxel_y, dVoxel_z);
    if ((unsigned long long)nx * ny * nz < (1ULL << 32))
        project_kernel<unsigned><<<grid, dim3(PB), 0, s>>>(H, W, rays, cone, nx, ny, nz, d, accuracy, vol, out);
    else
        project_kernel<size_t><<<grid, dim3(PB), 0, s>>>(H, W, rays, cone, nx, ny, nz, d, accuracy, vol, out);
    R2_STAGE_CHECK(0, s, "project volume");
    return 0;
}
