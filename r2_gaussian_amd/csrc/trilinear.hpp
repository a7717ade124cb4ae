// trilinear.hpp -- the trilinear value of a volume at one sample of a ray, as r2_project_volume defines it
// (include/r2hip.h): the eight clamped neighbours of the three Axis footprints (ray_sampling.hpp), gathered
// unconditionally, and three levels of weighted pairs, z first, each a product and an fmaf.  Shared by the forward
// projector (projector.hip) and the volume renderer (volume_render.hip), which classify and composite the very values the
// projector sums; tests/projector_ref.py bounds this expression by 8 u M (M: the largest |voxel| of the cell).
#pragma once
#include "ray_sampling.hpp"

namespace r2 {

// OFF: the type of a voxel offset, unsigned 32-bit when the volume has fewer than 2^32 voxels, 64-bit otherwise;
// sxy = ny * nz in it.
template <typename OFF>
__device__ __forceinline__ float trilinear(const float *__restrict__ vol, const Axis &X, const Axis &Y, const Axis &Z, OFF sxy,
                                           int nz)
{
    const OFF x0 = (OFF)X.i0 * sxy, x1 = X.i1 != X.i0 ? x0 + sxy : x0;
    const unsigned y0 = (unsigned)Y.i0 * (unsigned)nz, y1 = Y.i1 != Y.i0 ? y0 + (unsigned)nz : y0;
    const unsigned z0 = (unsigned)Z.i0, z1 = (unsigned)Z.i1;
    // the clamped neighbours are always inside the volume: load all eight unconditionally (no branches around the
    // gathers); a neighbour outside it has weight 0
    const float v000 = vol[x0 + (y0 + z0)], v001 = vol[x0 + (y0 + z1)], v010 = vol[x0 + (y1 + z0)], v011 = vol[x0 + (y1 + z1)];
    const float v100 = vol[x1 + (y0 + z0)], v101 = vol[x1 + (y0 + z1)], v110 = vol[x1 + (y1 + z0)], v111 = vol[x1 + (y1 + z1)];
    const float c00 = fmaf(Z.w1, v001, Z.w0 * v000), c01 = fmaf(Z.w1, v011, Z.w0 * v010);
    const float c10 = fmaf(Z.w1, v101, Z.w0 * v100), c11 = fmaf(Z.w1, v111, Z.w0 * v110);
    const float c0 = fmaf(Y.w1, c01, Y.w0 * c00), c1 = fmaf(Y.w1, c11, Y.w0 * c10);
    return fmaf(X.w1, c1, X.w0 * c0);
}

}  // namespace r2
