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

__global__ void __launch_bounds__(QB) gaussian_leaves_bwd_kernel(int N, const float *__restrict__ rays, int half_line, Cloud cl,
                                                                 const float *__restrict__ G, const BlockBox *__restrict__ boxes,
                                                                 CloudOut d)
{
    __shared__ float slice[LV][SLICE][WAVE];
    const int P = cl.P;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int leaf = blockIdx.x * LV + wave;   // wave-uniform
    const int i = leaf * LEAF + lane;          // < 2^29 + 256
    // A wave whose leaf does not exist (the tail workgroup) runs the rounds with no hit: the barriers below are the
    // workgroup's, and the round count is the same for every wave.
    const bool exists = leaf < leaf_count(P) && N > 0;
    float acc[NPAR];
    Gauss a = { 0.0f, 0.0f, 0.0f, 0.0f, { 1.0f, 1.0f, 1.0f }, make_float4(1.0f, 0.0f, 0.0f, 0.0f) };
    GaussRec g = {};
    float radius = -1.0f;
    BlockBox box = { { INFINITY, INFINITY, INFINITY }, { -INFINITY, -INFINITY, -INFINITY } };
#pragma unroll
    for (int k = 0; k < NPAR; ++k) acc[k] = 0.0f;
    if (exists) box = boxes[leaf];
    if (i < P) {
        a = load_gauss(cl, i);
        radius = gauss_radius(a, cl.mod);
        if (radius >= 0.0f) g = gauss_rec(a, cl.mod);
    }
    const bool live = radius >= 0.0f;
    float (*sl)[WAVE] = slice[wave];
    for (long long base = 0; base < N; base += WAVE) {
        const long long n = base + lane;
        const BundleRay y = bundle_ray(rays, n, exists ? N : 0);
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
                float o[NPAR];
                gauss_pair_grad(g, p, r.y, r.len, sl[11][j], a.s, a.q, o);
#pragma unroll
                for (int t = 0; t < NPAR; ++t) acc[t] += o[t];
            }
        }
        __syncthreads();   // the slice is rewritten by the next round
    }
    if (i < P) store_gauss(d, i, acc);
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
    const char *entry = "r2_integrate_gaussians_leaves_backward";
    const Cloud cl = { P, means, density, scales, scale_modifier, rotations };
    const CloudOut d = { dL_dmeans, dL_ddensity, dL_dscales, dL_drotations };
    if (N < 0 || P < 0 || (N > 0 && (!rays || !dL_dout)) || cl.missing() || d.missing(P)) return invalid_argument(entry);
    if (cloud_too_large(entry, P)) return R2_ERR_INVALID;
    const size_t need = r2_integrate_gaussians_leaves_workspace_bytes(N, P);
    if (leaves_workspace_refused(entry, workspace, workspace_bytes, need)) return R2_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    float4 *cent = (float4 *)workspace;
    GaussRec *recs = need > 0 ? leaves_recs(workspace, P) : nullptr;     // N = 0 or P = 0: no workspace
    BlockBox *boxes = need > 0 ? leaves_boxes(workspace, P) : nullptr;
    if (P > 0) {
        if (N > 0) leaves_prepare(cl, cent, recs, boxes, s);
        gaussian_leaves_bwd_kernel<<<dim3((leaf_count(P) + LV - 1) / LV), dim3(QB), 0, s>>>(N, rays, half_line, cl, dL_dout, boxes, d);
    }
    if (N > 0 && dL_drays)
        gaussian_leaves_rays_bwd_kernel<<<dim3((unsigned)(((long long)N + LV - 1) / LV)), dim3(QB), 0, s>>>(
            N, rays, half_line, P, dL_dout, cent, recs, boxes, dL_drays);
    R2_STAGE_CHECK(0, s, "integrate gaussians leaves backward");
    return 0;
}
