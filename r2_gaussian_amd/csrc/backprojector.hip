// backprojector.hip -- the exact transpose of the volume forward projector (projector.hip): vol = A^T projs, the `Atb` the
// iterative reconstructions (recon.py: CGLS, SART, OS-SART, ASD-POCS) need alongside r2_project_volume's `Ax`.
//
// A[rho, v] = dt |d_world| sum_k X_k(v_x) Y_k(v_y) Z_k(v_z) for the ray rho of a detector pixel, with the forward's own
// float32 clip points, sample count, sample positions and trilinear weights (ray_sampling.hpp, shared with projector.hip).
//
// Voxel-driven gather, one thread per voxel, no atomics (voxel_gather.hpp): a ray-driven scatter would need 8 float atomics
// per sample at scattered addresses and its sums would depend on their arrival order.  The model below gives the gather
//   * the support of a voxel's trilinear weight, [i-1, i+1]^3: a sample carries weight for voxel i on an axis only where its
//     floor index is i or i - 1, i.e. where its coordinate lies in (i-1, i+1), so a ray with a weighted sample passes
//     through the support, its pixel lies inside the box of the support's corners, and the filter (the support widened by
//     1/16 voxel, far more than the error of its approximate reciprocals) keeps it;
//   * the entry of a (ray, voxel) pair: the ray is set up exactly as the forward does, the filter's interval becomes a range
//     of sample indices with one more sample of margin on each side, axis_of is evaluated at those samples exactly as the
//     forward does and each axis's weight is kept only where its index is the voxel's.
// The filter and the margins only decide which samples are looked at; the samples that carry weight and their weights
// are the forward's, bit for bit.  Each voxel's sum runs in a fixed order (views, pixel rows, columns, samples).
//
// Compiled with -ffp-contract=off (build.py: EXACT) like projector.hip, so that the shared ray set-up is the same
// sequence of separately rounded operations in both translation units.
#include "voxel_gather.hpp"

namespace r2 {

namespace {

// The weight of voxel index i on one axis at a sample: w0 where the floor index is i, w1 where it is i - 1.  The clamped
// indices of axis_of coincide only where the other weight is 0, so the sum adds an exact zero.
__device__ __forceinline__ float axis_weight(const Axis &a, int i)
{
    return (a.i0 == i ? a.w0 : 0.0f) + (a.i1 == i ? a.w1 : 0.0f);
}

struct InterpolatedModel {
    static constexpr float HALF = 1.0f;   // the trilinear interpolant's support around a voxel
    float accuracy;

    __device__ __forceinline__ float entry(const Ray &y, int cone, int nx, int ny, int nz, float3 dv, int i, int j, int k,
                                           float lo, float hi) const
    {
        float t0, t1;
        if (!clip_ray(y, cone, nx, ny, nz, t0, t1)) return 0.0f;
        const Sampling m = ray_sampling(y, t0, t1, dv, accuracy);
        if (!(m.dt > 0.0f)) return 0.0f;   // every sample at t0 with weight dt |d| = 0: the forward's entry is 0 too
        // sample index range of the widened interval, one sample of margin on each side, clamped in float
        const float rdt = __builtin_amdgcn_rcpf(m.dt);
        const float klo = fmaxf(floorf((lo - t0) * rdt - 0.5f) - 1.0f, 0.0f);
        const float khi = fminf(ceilf((hi - t0) * rdt - 0.5f) + 1.0f, (float)(m.n - 1));
        if (!(khi >= klo)) return 0.0f;
        float acc = 0.0f;
        for (int s = (int)klo, se = (int)khi; s <= se; ++s) {
            const float t = sample_t(s, m.dt, t0);
            const float wx = axis_weight(axis_of(fmaf(t, y.dx, y.sx), nx), i);
            const float wy = axis_weight(axis_of(fmaf(t, y.dy, y.sy), ny), j);
            const float wz = axis_weight(axis_of(fmaf(t, y.dz, y.sz), nz), k);
            acc += wx * wy * wz;
        }
        return acc * (m.dt * m.wlen);
    }
};

}  // namespace

}  // namespace r2

extern "C" int r2_backproject_volume(int V, int H, int W, const float *rays, int cone, int nx, int ny, int nz,
                                     float dVoxel_x, float dVoxel_y, float dVoxel_z, float accuracy, const float *projs,
                                     float *vol, void *stream)
{
    return r2::launch_gather("r2_backproject_volume", "backproject volume", r2::InterpolatedModel{accuracy}, &accuracy, V, H,
                             W, rays, cone, nx, ny, nz, dVoxel_x, dVoxel_y, dVoxel_z, projs, vol, stream);
}
