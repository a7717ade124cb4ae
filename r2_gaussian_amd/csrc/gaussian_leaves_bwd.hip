// gaussian_leaves_bwd.hip -- the gradients of r2_integrate_gaussians_leaves, given G = dL/dout (include/r2hip.h:
// r2_integrate_gaussians_leaves_backward): with respect to the means, densities, scales and quaternions, and to the rays.
//
// Parameters, leaf-major, the mirror of the forward: after the prepare kernel (gaussian_leaves.hip) one wave per leaf, one
// lane per Gaussian, the lane holding its GaussRec, scales, quaternion and eleven sums in registers.  The wave takes the N
// rays 64 at a time: lane l tests the line of ray base + l against the leaf's box (gaussian_leaves.hpp: the leaf test), the
// hits are compacted IN RAY ORDER (ballot + popcount) into the wave's own LDS slice, and every lane walks the slice:
// bundle_line_misses, bundle_pair, gauss_pair_grad, eleven adds.  A Gaussian's gradient is summed by one lane in ascending
// ray index: no butterfly, no atomics, the same bits on every call, exact zeros for a Gaussian no ray touches (or one with a
// non-finite parameter).  The rule is the forward's, so a pair is differentiated exactly when the forward summed it.
// Rays, ray-major: the forward's skeleton with six sums per lane (gaussian_leaves.hpp: integrate_ray_wave<true>).
#include "gaussian_leaves.hpp"

namespace r2 {

namespace {

// What the slice keeps of a ray whose line meets the leaf's box: s, d, |d|, the unit direction, tame, G[n].
constexpr int SLICE = 12;

__global__ void __launch_bounds__(QB) gaussian_leaves_bwd_kernel(int N, const float *__restrict__ rays, int half_line, int P,
                                                                 const float *__restrict__ means, const float *__restrict__ density,
                                                                 const float *__restrict__ scales, float mod,
                                                                 const float *__restrict__ rotations, const float *__restrict__ G,
                                                                 const BlockBox *__restrict__ boxes, float *__restrict__ d_means,
                                                                 float *__restrict__ d_density, float *__restrict__ d_scales,
                                                                 float *__restrict__ d_rotations)
{
    __shared__ float slice[LV][SLICE][WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int leaf = blockIdx.x * LV + wave;   // wave-uniform
    const int i = leaf * LEAF + lane;          // < 2^29 + 256
    // A wave whose leaf does not exist (the tail workgroup) runs the rounds with no hit: the barriers below are the
    // workgroup's, and the round count is the same for every wave.
    const bool exists = leaf < leaf_count(P) && N > 0;
    float s[3] = { 1.0f, 1.0f, 1.0f }, acc[11];
    float4 q = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    GaussRec g = {};
    float radius = -1.0f;
    BlockBox box = { { INFINITY, INFINITY, INFINITY }, { -INFINITY, -INFINITY, -INFINITY } };
#pragma unroll
    for (int k = 0; k < 11; ++k) acc[k] = 0.0f;
    if (exists) box = boxes[leaf];
    if (i < P) {
        const float mx = means[3 * i], my = means[3 * i + 1], mz = means[3 * i + 2], rho = density[i];
        s[0] = scales[3 * i]; s[1] = scales[3 * i + 1]; s[2] = scales[3 * i + 2];
        q = make_float4(rotations[4 * i], rotations[4 * i + 1], rotations[4 * i + 2], rotations[4 * i + 3]);
        radius = gauss_radius(mx, my, mz, rho, s[0], s[1], s[2], mod, q);
        if (radius >= 0.0f) g = gauss_rec(mx, my, mz, rho, s[0], s[1], s[2], mod, q);
    }
    const bool live = radius >= 0.0f;
    float (*sl)[WAVE] = slice[wave];
    for (long long base = 0; base < N; base += WAVE) {
        const long long n = base + lane;
        BundleRay y;
        y.y = Ray{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        y.len = 0.0f;
        y.valid = false;
        if (exists && n < N) y = bundle_ray(rays, n);
        const BundleDir u = bundle_dir(y);
        float v[6];
        const bool hit = exists && bundle_ray_box(y, u, half_line, box, v);
        const unsigned long long mask = __ballot(hit);
        const int total = __popcll(mask);
        if (hit) {
            const int slot = __popcll(mask & ((1ull << lane) - 1ull));
            sl[0][slot] = y.y.sx; sl[1][slot] = y.y.sy; sl[2][slot] = y.y.sz;
            sl[3][slot] = y.y.dx; sl[4][slot] = y.y.dy; sl[5][slot] = y.y.dz;
            sl[6][slot] = y.len;
            sl[7][slot] = u.h[0]; sl[8][slot] = u.h[1]; sl[9][slot] = u.h[2];
            sl[10][slot] = u.tame ? 1.0f : 0.0f;
            sl[11][slot] = G[n];
        }
        __syncthreads();
        if (live) {
            for (int j = 0; j < total; ++j) {
                BundleRay r;
                r.y = Ray{sl[0][j], sl[1][j], sl[2][j], sl[3][j], sl[4][j], sl[5][j]};
                r.len = sl[6][j];
                r.valid = true;
                BundleDir w;
                w.h[0] = sl[7][j]; w.h[1] = sl[8][j]; w.h[2] = sl[9][j];
                w.tame = sl[10][j] != 0.0f;
                if (bundle_line_misses(r, w, g.mx, g.my, g.mz, radius)) continue;
                GaussPair p;
                if (!bundle_pair(g, r.y, half_line, p)) continue;
                float o[11];
                gauss_pair_grad(g, p, r.y, r.len, sl[11][j], s, q, o);
#pragma unroll
                for (int t = 0; t < 11; ++t) acc[t] += o[t];
            }
        }
        __syncthreads();   // the slice is rewritten by the next round
    }
    if (i < P) {
        d_means[3 * i] = acc[0]; d_means[3 * i + 1] = acc[1]; d_means[3 * i + 2] = acc[2];
        d_density[i] = acc[3];
        d_scales[3 * i] = acc[4]; d_scales[3 * i + 1] = acc[5]; d_scales[3 * i + 2] = acc[6];
        d_rotations[4 * i] = acc[7]; d_rotations[4 * i + 1] = acc[8]; d_rotations[4 * i + 2] = acc[9];
        d_rotations[4 * i + 3] = acc[10];
    }
}

__global__ void __launch_bounds__(QB) gaussian_leaves_rays_bwd_kernel(int N, const float *__restrict__ rays, int half_line, int P,
                                                                      const float *__restrict__ G, const float4 *__restrict__ cent,
                                                                      const GaussRec *__restrict__ recs,
                                                                      const BlockBox *__restrict__ boxes, float *__restrict__ d_rays)
{
    integrate_ray_wave<true>(N, rays, half_line, P, G, cent, recs, boxes, d_rays);
}

}  // namespace

}  // namespace r2

extern "C" int r2_integrate_gaussians_leaves_backward(int N, const float *rays, int half_line, int P, const float *means,
                                                      const float *density, const float *scales, float scale_modifier,
                                                      const float *rotations, const float *dL_dout, float *dL_dmeans,
                                                      float *dL_ddensity, float *dL_dscales, float *dL_drotations, float *dL_drays,
                                                      void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace r2;
    static_assert(sizeof(BlockBox) == 24 && sizeof(float4) == 16 && sizeof(GaussRec) == 64, "the workspace is 80 bytes per Gaussian and 24 per leaf");
    if (N < 0 || P < 0 || (N > 0 && (!rays || !dL_dout)) ||
        (P > 0 && (!means || !density || !scales || !rotations || !dL_dmeans || !dL_ddensity || !dL_dscales || !dL_drotations))) {
        set_error("r2_integrate_gaussians_leaves_backward: invalid argument");
        return R2_ERR_INVALID;
    }
    if (P > (1 << 29)) {
        set_error("r2_integrate_gaussians_leaves_backward: shape out of range (P %d)", P);
        return R2_ERR_INVALID;
    }
    const size_t need = r2_integrate_gaussians_leaves_workspace_bytes(N, P);
    if (need > 0 && (!workspace || workspace_bytes < need)) {
        set_error("r2_integrate_gaussians_leaves_backward: workspace of %zu bytes, %zu needed "
                  "(r2_integrate_gaussians_leaves_workspace_bytes)", workspace ? workspace_bytes : (size_t)0, need);
        return R2_ERR_INVALID;
    }
    if (need > 0 && ((size_t)workspace & 15) != 0) {
        set_error("r2_integrate_gaussians_leaves_backward: the workspace must be aligned to 16 bytes");
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    float4 *cent = (float4 *)workspace;
    GaussRec *recs = need > 0 ? leaves_recs(workspace, P) : nullptr;     // N = 0 or P = 0: no workspace
    BlockBox *boxes = need > 0 ? leaves_boxes(workspace, P) : nullptr;
    if (P > 0) {
        if (N > 0) leaves_prepare(P, means, density, scales, scale_modifier, rotations, cent, recs, boxes, s);
        gaussian_leaves_bwd_kernel<<<dim3((leaf_count(P) + LV - 1) / LV), dim3(QB), 0, s>>>(N, rays, half_line, P, means, density, scales,
                                                                                           scale_modifier, rotations, dL_dout, boxes,
                                                                                           dL_dmeans, dL_ddensity, dL_dscales,
                                                                                           dL_drotations);
    }
    if (N > 0 && dL_drays)
        gaussian_leaves_rays_bwd_kernel<<<dim3((unsigned)(((long long)N + LV - 1) / LV)), dim3(QB), 0, s>>>(
            N, rays, half_line, P, dL_dout, cent, recs, boxes, dL_drays);
    R2_STAGE_CHECK(0, s, "integrate gaussians leaves backward");
    return 0;
}
