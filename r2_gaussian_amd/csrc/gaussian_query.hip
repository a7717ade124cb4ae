// gaussian_query.hip -- the density field of a Gaussian cloud at caller-supplied points: out[n] = the sum over the Gaussians
// of rho exp(-(x_n - mu)^T Sigma^-1 (x_n - mu) / 2) (include/r2hip.h: r2_query_gaussians; the per-pair arithmetic, the block
// boxes and the sphere rule are gaussian_points.hpp's, shared with the backward, and so is the skeleton of this kernel, which
// the point gradient runs with three sums instead of one).
//
// No atomics, no list in memory, no workspace and no host synchronisation, the same bits on every call.  The price is P
// sphere / box tests per block of 256 points instead of a per-block list; DESIGN.md section 4 has what that costs.
#include "gaussian_points.hpp"

namespace r2 {

namespace {

__global__ void __launch_bounds__(QB) gaussian_query_kernel(int N, const float *__restrict__ points, Cloud cl, float *__restrict__ out)
{
    query_points_block<false>(N, points, cl, nullptr, out);
}

}  // namespace

}  // namespace r2

extern "C" int r2_query_gaussians(int N, const float *points, int P, const float *means, const float *density, const float *scales,
                                  float scale_modifier, const float *rotations, float *out, void *stream)
{
    using namespace r2;
    const char *entry = "r2_query_gaussians";
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    if (N < 0 || P < 0 || (N > 0 && (!points || !out)) || (N > 0 && cl.missing())) return invalid_argument(entry);
    if (cloud_too_large(entry, P)) return R2_ERR_INVALID;
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    gaussian_query_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, points, cl, out);
    R2_STAGE_CHECK(0, s, "query gaussians");
    return 0;
}
