// tv_descent.hip -- normalised steepest descent on the smoothed isotropic total variation, the TV half of ASD-POCS
// (recon.py).  The discretisation is stated in include/r2hip.h (r2_tv_descent).  loss_ops.hip's tv3d_kernel is the training
// loss on a patch and is unrelated.
//
// One iteration is three launches on the caller's stream, none of which the host waits for:
//   tv_grad:   g = grad TV_eps(x) into the scratch, and per block the sum of g^2 in double, in a fixed tree order;
//   tv_norm:   one block sums the block sums in a fixed order: |g|_2;
//   tv_update: x <- x - (step / |g|) g, skipped where |g| = 0 (a constant volume).
// Each voxel's gradient reads at most ten neighbours of x (its own forward differences and those of its three backward
// neighbours); nothing depends on the launch order of blocks, so the result is bit-reproducible.
#include "r2_common.hpp"
#include <math.h>

namespace r2 {

namespace {

constexpr int TB = 256;           // threads per block
constexpr int PER = 4;            // voxels per thread: a block covers TB * PER consecutive voxels
constexpr int CHUNK = TB * PER;
constexpr float EPS = 1e-8f;

struct Grid {
    int nx, ny, nz;
    size_t sx, sy;   // strides of x and y (z is contiguous)
};

// The forward differences of x at (i, j, k), zero past the last index, and 1 / sqrt(dx^2 + dy^2 + dz^2 + eps).
__device__ __forceinline__ float inv_norm_at(const float *__restrict__ x, const Grid &g, int i, int j, int k, size_t o,
                                             float &dx, float &dy, float &dz)
{
    const float v = x[o];
    dx = i + 1 < g.nx ? x[o + g.sx] - v : 0.0f;
    dy = j + 1 < g.ny ? x[o + g.sy] - v : 0.0f;
    dz = k + 1 < g.nz ? x[o + 1] - v : 0.0f;
    return 1.0f / sqrtf(dx * dx + dy * dy + dz * dz + EPS);
}

__device__ __forceinline__ double block_sum(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = TB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

__global__ void __launch_bounds__(TB) tv_grad(Grid g, size_t N, const float *__restrict__ x, float *__restrict__ grad,
                                              double *__restrict__ partial)
{
    __shared__ double sh[TB];
    double sq = 0.0;
    for (int p = 0; p < PER; ++p) {
        const size_t o = (size_t)blockIdx.x * CHUNK + (size_t)p * TB + threadIdx.x;
        if (o >= N) break;
        const int k = (int)(o % (size_t)g.nz);
        const int j = (int)((o / (size_t)g.nz) % (size_t)g.ny);
        const int i = (int)(o / g.sx);
        float dx, dy, dz;
        const float inv = inv_norm_at(x, g, i, j, k, o, dx, dy, dz);
        float gv = -(dx + dy + dz) * inv;
        // the terms of the backward neighbours, whose forward difference along that axis ends at this voxel
        float ex, ey, ez;
        if (i > 0) gv += (x[o] - x[o - g.sx]) * inv_norm_at(x, g, i - 1, j, k, o - g.sx, ex, ey, ez);
        if (j > 0) gv += (x[o] - x[o - g.sy]) * inv_norm_at(x, g, i, j - 1, k, o - g.sy, ex, ey, ez);
        if (k > 0) gv += (x[o] - x[o - 1]) * inv_norm_at(x, g, i, j, k - 1, o - 1, ex, ey, ez);
        grad[o] = gv;
        sq += (double)gv * (double)gv;
    }
    const double s = block_sum(sq, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(TB) tv_norm(int nblocks, const double *__restrict__ partial, float *__restrict__ norm)
{
    __shared__ double sh[TB];
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += TB) s += partial[b];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) *norm = (float)sqrt(s);
}

__global__ void __launch_bounds__(TB) tv_update(size_t N, float *__restrict__ x, const float *__restrict__ grad,
                                                const float *__restrict__ norm, const float *__restrict__ step)
{
    const float n = *norm;
    if (!(n > 0.0f)) return;   // a zero gradient: no update, no division
    const float f = *step / n;
    for (int p = 0; p < PER; ++p) {
        const size_t o = (size_t)blockIdx.x * CHUNK + (size_t)p * TB + threadIdx.x;
        if (o >= N) break;
        x[o] = x[o] - f * grad[o];
    }
}

size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace

}  // namespace r2

extern "C" size_t r2_tv_descent_scratch_bytes(int nx, int ny, int nz)
{
    using namespace r2;
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
    const size_t N = (size_t)nx * ny * nz, nb = (N + CHUNK - 1) / CHUNK;
    return align8(N * sizeof(float)) + nb * sizeof(double) + sizeof(double);
}

extern "C" int r2_tv_descent(int nx, int ny, int nz, float *vol, const float *step, int n_iter, void *scratch,
                             size_t scratch_bytes, void *stream)
{
    using namespace r2;
    if (nx <= 0 || ny <= 0 || nz <= 0 || !vol || !step || n_iter < 0 || !scratch) {
        set_error("r2_tv_descent: invalid argument");
        return R2_ERR_INVALID;
    }
    const size_t N = (size_t)nx * ny * nz, nb = (N + CHUNK - 1) / CHUNK;
    if (scratch_bytes < r2_tv_descent_scratch_bytes(nx, ny, nz) || nb > 0x7fffffffULL) {
        set_error("r2_tv_descent: scratch of %zu bytes, %zu needed (or volume too large)", scratch_bytes,
                  r2_tv_descent_scratch_bytes(nx, ny, nz));
        return R2_ERR_INVALID;
    }
    float *grad = (float *)scratch;
    double *partial = (double *)((char *)scratch + align8(N * sizeof(float)));
    float *norm = (float *)(partial + nb);
    const Grid g{nx, ny, nz, (size_t)ny * nz, (size_t)nz};
    hipStream_t s = (hipStream_t)stream;
    for (int it = 0; it < n_iter; ++it) {
        tv_grad<<<dim3((unsigned)nb), dim3(TB), 0, s>>>(g, N, vol, grad, partial);
        tv_norm<<<dim3(1), dim3(TB), 0, s>>>((int)nb, partial, norm);
        tv_update<<<dim3((unsigned)nb), dim3(TB), 0, s>>>(N, vol, grad, norm, step);
    }
    R2_STAGE_CHECK(0, s, "tv descent");
    return 0;
}
