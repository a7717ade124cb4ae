// gaussian_project.hip -- the exact X-ray transform of a Gaussian cloud: out[v][r][c] = the sum over the Gaussians of the
// closed-form line integral of each along the ray of pixel (r, c) (include/r2hip.h: r2_project_gaussians; the per-pair
// arithmetic, the bounding rectangle and the cone rule are gaussian_rays.hpp's, shared with the backward).
//
// One workgroup per 16 x 16 pixel tile and view (blockIdx.z), one thread per pixel.  The workgroup walks the P Gaussians in
// index order, 256 at a time: thread i projects the bounding sphere of Gaussian base + i onto the detector (a conservative
// pixel rectangle), the ones whose rectangle meets the tile are compacted IN ORDER (wave ballots + the four wave counts) into
// an LDS batch together with their S^-1 R^T, and every pixel then adds the batch's pairs whose rectangle holds it, in batch
// order.  A pixel therefore adds its pairs in ascending Gaussian index, in one thread: no atomics, no list in memory, no
// workspace and no host synchronisation, the same bits on every call, and nothing a view computes depends on another view.
// The price is P rectangle tests per tile instead of a sorted per-tile list; DESIGN.md section 4 has what that costs.
#include "gaussian_rays.hpp"

namespace r2 {

namespace {

constexpr int GB = TILE2D * TILE2D;   // threads per workgroup = Gaussians per batch

struct Staged {
    GaussRec g;
    PixRect q;
};

__global__ void __launch_bounds__(GB) gaussian_project_kernel(int H, int W, const float *__restrict__ rays, int cone, int P,
                                                              const float *__restrict__ means, const float *__restrict__ density,
                                                              const float *__restrict__ scales, float mod,
                                                              const float *__restrict__ rotations, float *__restrict__ out)
{
    __shared__ ViewGeom vg;
    __shared__ Staged st[GB];
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
            st[slot].g = gauss_rec(mx, my, mz, rho, sx, sy, sz, mod, q);
            st[slot].q = rc;
        }
        __syncthreads();
        if (inside) {
            for (int j = 0; j < total; ++j) {
                const PixRect &b = st[j].q;
                if (c < b.c0 || c > b.c1 || r < b.r0 || r > b.r1) continue;
                GaussPair p;
                if (gauss_pair(st[j].g, y, cone, p)) acc += gauss_term(st[j].g, p, len);
            }
        }
        __syncthreads();   // the batch and the wave counts are rewritten by the next round
    }
    if (inside) out[((size_t)view * H + r) * W + c] = acc;
}

}  // namespace

}  // namespace r2

extern "C" int r2_project_gaussians(int V, int H, int W, const float *rays, int cone, int P, const float *means,
                                    const float *density, const float *scales, float scale_modifier, const float *rotations,
                                    float *out, void *stream)
{
    using namespace r2;
    if (V <= 0 || H <= 0 || W <= 0 || P < 0 || !rays || !out || (P > 0 && (!means || !density || !scales || !rotations))) {
        set_error("r2_project_gaussians: invalid argument");
        return R2_ERR_INVALID;
    }
    if (V > 65535 || (H + TILE2D - 1) / TILE2D > 65535 || P > (1 << 29)) {
        set_error("r2_project_gaussians: shape out of range (V %d, H %d, P %d)", V, H, P);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((W + TILE2D - 1) / TILE2D, (H + TILE2D - 1) / TILE2D, V);
    gaussian_project_kernel<<<grid, dim3(GB), 0, s>>>(H, W, rays, cone, P, means, density, scales, scale_modifier, rotations, out);
    R2_STAGE_CHECK(0, s, "project gaussians");
    return 0;
}
