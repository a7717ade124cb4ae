// gaussian_variance.hip -- the predictive variance of the exact operators under independent variances of the Gaussians'
// parameters: of the density field at caller-supplied points (r2_query_gaussians_variance) and of every pixel of the exact
// projection (r2_project_gaussians_variance), out = the sum over the point's or pixel's pairs of
// sum_t v[i][t] (d term / d theta_it)^2 (include/r2hip.h; the per-pair arithmetic is gaussian_fisher.hpp's pair_variance).
//
// Both are the forwards' skeletons with a larger staged record (the unmodified scales, the quaternion and the eleven
// variances next to S^-1 R^T): the point kernel is gaussian_fisher.hpp's variance_points_block, the pixel kernel restates
// gaussian_project.hip's.  A point or a pixel adds its pairs in ascending Gaussian index in one thread: no atomics, no list
// in memory, no workspace and no host synchronisation, the same bits on every call.
#include "gaussian_fisher.hpp"

namespace r2 {

namespace {

constexpr int GB = TILE2D * TILE2D;   // threads per workgroup = Gaussians per batch

// about 156 bytes, 39 kB for a batch of GB
struct StagedPixVar {
    StagedVar a;
    PixRect q;
};

__global__ void __launch_bounds__(QB) gaussian_query_variance_kernel(int N, const float *__restrict__ points, int P,
                                                                     const float *__restrict__ means,
                                                                     const float *__restrict__ density,
                                                                     const float *__restrict__ scales, float mod,
                                                                     const float *__restrict__ rotations,
                                                                     const float *__restrict__ v_means,
                                                                     const float *__restrict__ v_density,
                                                                     const float *__restrict__ v_scales,
                                                                     const float *__restrict__ v_rotations, float *__restrict__ out)
{
    variance_points_block(N, points, P, means, density, scales, mod, rotations, v_means, v_density, v_scales, v_rotations, out);
}

// One workgroup per 16 x 16 pixel tile and view (blockIdx.z), one thread per pixel; the P Gaussians in index order, GB at a
// time: rectangle test, in-order compaction into LDS, and every pixel adds the batch's pairs whose rectangle holds it.
__global__ void __launch_bounds__(GB) gaussian_project_variance_kernel(int H, int W, const float *__restrict__ rays, int cone, int P,
                                                                       const float *__restrict__ means,
                                                                       const float *__restrict__ density,
                                                                       const float *__restrict__ scales, float mod,
                                                                       const float *__restrict__ rotations,
                                                                       const float *__restrict__ v_means,
                                                                       const float *__restrict__ v_density,
                                                                       const float *__restrict__ v_scales,
                                                                       const float *__restrict__ v_rotations, float *__restrict__ out)
{
    __shared__ ViewGeom vg;
    __shared__ StagedPixVar st[GB];
    __shared__ int wcount[GB / WAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int view = blockIdx.z;
    const int tc0 = blockIdx.x * TILE2D, tr0 = blockIdx.y * TILE2D;
    const int tc1 = min(tc0 + TILE2D, W) - 1, tr1 = min(tr0 + TILE2D, H) - 1;
    const int c = tc0 + (tid & (TILE2D - 1)), r = tr0 + tid / TILE2D;
    const bool inside = c < W && r < H;
    const float *R = rays + 12 * view;
    if (tid == 0) vg = view_geom(R, cone);
    __syncthreads();
    const Ray y = pixel_ray(R, cone, r, c);
    const float len = ray_length(y);
    float acc = 0.0f;
    for (int base = 0; base < P; base += GB) {
        const int i = base + tid;
        bool hit = false;
        float mx = 0.f, my = 0.f, mz = 0.f, rho = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        PixRect rc;
        if (i < P) {
            mx = means[3 * i]; my = means[3 * i + 1]; mz = means[3 * i + 2];
            rho = density[i];
            sx = scales[3 * i]; sy = scales[3 * i + 1]; sz = scales[3 * i + 2];
            q = make_float4(rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3]);
            const float radius = gauss_radius(mx, my, mz, rho, sx, sy, sz, mod, q);
            if (radius >= 0.0f && gauss_rect(vg, cone, mx, my, mz, radius, H, W, rc))
                hit = rc.c0 <= tc1 && rc.c1 >= tc0 && rc.r0 <= tr1 && rc.r1 >= tr0;
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) wcount[wave] = __popcll(mask);
        __syncthreads();
        int slot = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < GB / WAVE; ++w) {
            if (w < wave) slot += wcount[w];
            total += wcount[w];
        }
        if (hit) {
            stage_var(st[slot].a, mx, my, mz, rho, sx, sy, sz, mod, q, v_means, v_density, v_scales, v_rotations, i);
            st[slot].q = rc;
        }
        __syncthreads();
        if (inside) {
            for (int j = 0; j < total; ++j) {
                const PixRect &b = st[j].q;
                if (c < b.c0 || c > b.c1 || r < b.r0 || r > b.r1) continue;
                const StagedVar &a = st[j].a;
                GaussPair p;
                if (gauss_pair(a.g, y, cone, p))
                    acc += pair_variance(a.g, p, y, len, a.s, make_float4(a.q[0], a.q[1], a.q[2], a.q[3]), a.v);
            }
        }
        __syncthreads();   // the batch and the wave counts are rewritten by the next round
    }
    if (inside) out[((size_t)view * H + r) * W + c] = acc;
}

}  // namespace

}  // namespace r2

extern "C" int r2_query_gaussians_variance(int N, const float *points, int P, const float *means, const float *density,
                                           const float *scales, float scale_modifier, const float *rotations, const float *v_means,
                                           const float *v_density, const float *v_scales, const float *v_rotations, float *out,
                                           void *stream)
{
    using namespace r2;
    if (N < 0 || P < 0 || (N > 0 && (!points || !out)) ||
        (N > 0 && P > 0 && (!means || !density || !scales || !rotations || !v_means || !v_density || !v_scales || !v_rotations))) {
        set_error("r2_query_gaussians_variance: invalid argument");
        return R2_ERR_INVALID;
    }
    if (P > (1 << 29)) {
        set_error("r2_query_gaussians_variance: shape out of range (P %d)", P);
        return R2_ERR_INVALID;
    }
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    gaussian_query_variance_kernel<<<dim3(query_blocks(N)), dim3(QB), 0, s>>>(N, points, P, means, density, scales, scale_modifier,
                                                                                  rotations, v_means, v_density, v_scales, v_rotations,
                                                                                  out);
    R2_STAGE_CHECK(0, s, "query gaussians variance");
    return 0;
}

extern "C" int r2_project_gaussians_variance(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                             const float *density, const float *scales, float scale_modifier,
                                             const float *rotations, const float *v_means, const float *v_density,
                                             const float *v_scales, const float *v_rotations, float *out, void *stream)
{
    using namespace r2;
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays || !out ||
        (P > 0 && (!means || !density || !scales || !rotations || !v_means || !v_density || !v_scales || !v_rotations))) {
        set_error("r2_project_gaussians_variance: invalid argument");
        return R2_ERR_INVALID;
    }
    if (V > 65535 || (H + TILE2D - 1) / TILE2D > 65535 || P > (1 << 29)) {
        set_error("r2_project_gaussians_variance: shape out of range (V %d, H %d, P %d)", V, H, P);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((W + TILE2D - 1) / TILE2D, (H + TILE2D - 1) / TILE2D, V);
    gaussian_project_variance_kernel<<<grid, dim3(GB), 0, s>>>(H, W, rays, cone, P, means, density, scales, scale_modifier, rotations,
                                                               v_means, v_density, v_scales, v_rotations, out);
    R2_STAGE_CHECK(0, s, "project gaussians variance");
    return 0;
}
