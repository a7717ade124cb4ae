// backprojector_siddon.hip -- the exact transpose of the Siddon forward projector (projector_siddon.hip): vol = A^T projs
// with A[rho, v] = |d_world| * (the length of t the ray rho spends in voxel v), the entry include/r2hip.h states for
// r2_project_volume_siddon.
//
// Voxel-driven gather, one thread per voxel, no atomics (voxel_gather.hpp).  An entry is one clip of the ray against the
// voxel's cube: no sample loop, which is what makes this adjoint cheap next to backprojector.hip's.  The model below gives
// the gather
//   * the support of a voxel, its cube [i - 1/2, i + 1/2]^3: an entry is non-zero only where the ray spends t inside the
//     cube, so its pixel lies inside the box of the cube's corners, and the filter (the cube widened by 1/16 voxel, far more
//     than the error of its approximate reciprocals against plane_t's exact ones) keeps it;
//   * the entry of a (ray, voxel) pair: the ray is set up exactly as the forward does (siddon_ray.hpp: the three axes, the
//     clip to the volume, |d_world|) and the entry comes from plane_t of the voxel's six planes.
// The box and the filter only decide which pixels are looked at; the entries are the forward's, bit for bit.  Each voxel's
// sum runs in a fixed order (views, pixel rows, columns).
//
// Compiled with -ffp-contract=off (build.py: EXACT) like projector_siddon.hip.
#include "siddon_ray.hpp"
#include "voxel_gather.hpp"

namespace r2 {

namespace {

struct SiddonModel {
    static constexpr float HALF = 0.5f;   // the cube's half width

    __device__ __forceinline__ float entry(const Ray &y, int cone, int nx, int ny, int nz, float3 dv, int i, int j, int k,
                                           float, float) const
    {
        const SiddonRay q = siddon_ray(y, cone, nx, ny, nz, dv);
        if (!q.hit) return 0.0f;
        return siddon_entry(q, i, j, k);
    }
};

}  // namespace

}  // namespace r2

extern "C" int r2_backproject_volume_siddon(int V, int H, int W, const float *rays, int cone, int nx, int ny, int nz,
                                            float dVoxel_x, float dVoxel_y, float dVoxel_z, const float *projs, float *vol,
                                            void *stream)
{
    return r2::launch_gather("r2_backproject_volume_siddon", "backproject volume siddon", r2::SiddonModel{}, nullptr, V, H, W,
                             rays, cone, nx, ny, nz, dVoxel_x, dVoxel_y, dVoxel_z, projs, vol, stream);
}
