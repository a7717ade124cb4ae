// volume_entry.hpp -- what the four volume operators' entry points share (r2_project_volume, r2_backproject_volume and
// their _siddon pair; include/r2hip.h): the validation of their common arguments, the limits a forward launch puts on
// the shapes, and the forward kernels' mapping of threads to detector pixels.
#pragma once
#include "r2_common.hpp"

namespace r2 {

constexpr int PT = 8;          // wave tile: PT x PT pixels, so a wave's 64 rays walk neighbouring voxels
constexpr int PB = 256;        // threads per block: 2 x 2 wave tiles
constexpr int BW = 2 * PT, BH = 2 * PT;

// The pixel of this thread in a forward launch of volume_pixel_grid(): false when it lies off the detector.
__device__ __forceinline__ bool thread_pixel(int H, int W, int &r, int &c)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    c = blockIdx.x * BW + (wave & 1) * PT + (lane & (PT - 1));
    r = blockIdx.y * BH + (wave >> 1) * PT + (lane / PT);
    return c < W && r < H;
}

inline dim3 volume_pixel_grid(int V, int H, int W) { return dim3((W + BW - 1) / BW, (H + BH - 1) / BH, V); }

// The arguments every entry point takes: sizes, pointers, voxel sizes, and `accuracy` where the operator has one
// (nullptr where it has none).  false: the error text is set in the name of `fn`.
inline bool volume_args_valid(const char *fn, int V, int H, int W, const float *rays, int nx, int ny, int nz, float dx,
                              float dy, float dz, const float *accuracy, const float *in, const float *out)
{
    if (V <= 0 || H <= 0 || W <= 0 || nx <= 0 || ny <= 0 || nz <= 0 || !rays || !in || !out ||
        (accuracy && !(*accuracy > 0.f)) || !(dx > 0.f) || !(dy > 0.f) || !(dz > 0.f)) {
        set_error("%s: invalid argument", fn);
        return false;
    }
    return true;
}

// The shapes a forward launch can take: ny * nz in the forward's 32-bit in-slab offsets, V and the rows of pixel tiles in
// a grid dimension.  The adjoints keep to them too, so that every operator pair accepts the same shapes.
inline bool forward_shape_in_range(int V, int H, int ny, int nz)
{
    return (long long)ny * nz < (1LL << 32) && V <= 65535 && (H + BH - 1) / BH <= 65535;
}

// Both checks of a forward entry point.  0, or R2_ERR_INVALID with the error text set.
inline int check_forward_args(const char *fn, int V, int H, int W, const float *rays, int nx, int ny, int nz, float dx,
                              float dy, float dz, const float *accuracy, const float *vol, const float *out)
{
    if (!volume_args_valid(fn, V, H, W, rays, nx, ny, nz, dx, dy, dz, accuracy, vol, out)) return R2_ERR_INVALID;
    if (!forward_shape_in_range(V, H, ny, nz)) {
        set_error("%s: shape out of range (V %d, H %d, ny*nz %lld)", fn, V, H, (long long)ny * nz);
        return R2_ERR_INVALID;
    }
    return 0;
}

}  // namespace r2
