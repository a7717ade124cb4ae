// gaussian_leaves.hpp -- the exact line integral of a Gaussian cloud along caller-supplied rays, culled from the Gaussians'
// side: by leaves of LEAF = 64 consecutive Gaussians, one per lane of a wave, each with the bounding box of its spheres, as
// r2_integrate_gaussians_leaves defines it (include/r2hip.h).  Shared by the prepare kernel, the forward
// (gaussian_leaves.hip) and both backward kernels (gaussian_leaves_bwd.hip).  The rule, the ray, its unit direction, the
// slab test, the sphere test and the pair are gaussian_bundle.hpp's, taken as they are; the translation units are compiled
// with -ffp-contract=off (build.py: EXACT), and tests/gaussian_leaves_ref.py restates the prepare kernel and the leaf test
// in float32 in the order written here.
//
// The rule is gaussian_bundle.hpp's, unchanged: a valid ray and a Gaussian with gauss_radius >= 0 are summed exactly when
// bundle_pair accepts them.  Leaf culling comes in front of it, is conservative for the INFINITE line and changes which
// pairs are summed by nothing.
//
// The leaf box: the bounding box of the spheres mu -+ radius of the leaf's members with radius >= 0 (an infinite radius makes
// it infinite, no such member leaves it empty: lo > hi); each bound is rounded once, eps |bound|, as the cloud box of
// gaussian_bundle.hpp (0) is.  The last leaf may be partial.
// The leaf test: a ray meets a leaf when bundle_ray_box clips it to a non-empty segment in the leaf's box, that is,
// gaussian_bundle.hpp (1) with the leaf's box in the place of the cloud box: bounds moved outwards by GB_EPS |bound|, every t
// by GB_EPS |t|, a half-line ray clipped to t >= 0, an axis with no direction deciding by the start alone, an untame ray
// meeting every leaf that has a box.  The argument is (1)'s own, for one leaf: a summed pair has q <= GQ_CUT at the line's
// Mahalanobis-closest point x*, x* lies in the Gaussian's sphere (0.9901 radius), the sphere lies in its leaf's box, so the
// true line has a point in the true box and the slab test, whose allowances cover the rounding of its own arithmetic, keeps
// the leaf; with half_line, x* has its float32 t* > 0 and a true t* that is negative only by the rounding (1) bounds against
// the 0.0099 radius the start then keeps to the sphere's surface: the start itself lies in the box, at t = 0.  Only the return
// value is used; the segment's box that bundle_ray_box also forms is dead code here.
// (3), bundle_line_misses, then skips the members of a met leaf whose sphere the line misses, with (3)'s allowance.
#pragma once
#include "gaussian_bundle.hpp"

namespace r2 {

constexpr int LEAF = WAVE;        // Gaussians per leaf: one per lane
constexpr int LV = QB / WAVE;     // waves per workgroup: rays per workgroup of the forward, leaves of the other kernels

// Leaves of P Gaussians.
__host__ __device__ __forceinline__ int leaf_count(int P) { return P > 0 ? (P - 1) / LEAF + 1 : 0; }

// The workspace: P float4 {mx, my, mz, radius} (radius = -1: the Gaussian contributes nothing), then the P GaussRec of the
// Gaussians with radius >= 0 (64 bytes each; the others' are not written and not read), then one BlockBox per leaf.  The
// float4 is all the culling reads; a pair that passes test (3) loads its record.  Recomputing the record per accepted pair from
// the 44 bytes of parameters instead (gauss_rec gives the same bits wherever it is formed) measured 1.17 x to 1.4 x slower in
// the forward on an MI355X, so it is stored.
__host__ __device__ __forceinline__ size_t leaves_workspace_bytes(int N, int P)
{
    return N > 0 && P > 0 ? (size_t)P * (sizeof(float4) + sizeof(GaussRec)) + (size_t)leaf_count(P) * sizeof(BlockBox) : (size_t)0;
}

__host__ __device__ __forceinline__ GaussRec *leaves_recs(void *workspace, int P)
{
    return (GaussRec *)((char *)workspace + (size_t)P * sizeof(float4));
}

__host__ __device__ __forceinline__ BlockBox *leaves_boxes(void *workspace, int P)
{
    return (BlockBox *)((char *)workspace + (size_t)P * (sizeof(float4) + sizeof(GaussRec)));
}

// host: the workspace is absent, too small or not aligned to 16 bytes (the float4 loads); sets the error text.
inline bool leaves_workspace_refused(const char *entry, const void *workspace, size_t workspace_bytes, size_t need)
{
    if (workspace_too_small(entry, "r2_integrate_gaussians_leaves_workspace_bytes", workspace, workspace_bytes, need)) return true;
    if (need == 0 || ((size_t)workspace & 15) == 0) return false;
    set_error("%s: the workspace must be aligned to 16 bytes", entry);
    return true;
}

// Launches the prepare kernel (gaussian_leaves.hip): the float4 and the record of every Gaussian, the box of every leaf; P > 0.
void leaves_prepare(const Cloud &cl, float4 *cent, GaussRec *recs, BlockBox *boxes, hipStream_t s);

// The ray-major skeleton of the forward (GRAD = false: out[n] = the integral along ray n) and of the ray gradient
// (GRAD = true: out[6 n ..] = G[n] d integral / d (s, d)).  One wave per ray, LV rays per workgroup, no LDS, no barrier.  The
// wave takes the leaves 64 at a time: lane l tests the box of leaf base + l, the wave ballots and walks the met leaves in
// ascending order, lane l taking Gaussian 64 leaf + l.  A lane adds its pairs in ascending leaf; one fixed xor butterfly adds
// the 64 lanes at the end and lane 0 writes.  The same bits on every call, whatever the other rays are.
template <bool GRAD>
__device__ __forceinline__ void integrate_ray_wave(int N, const float *__restrict__ rays, int half_line, int P,
                                                   const float *__restrict__ G, const float4 *__restrict__ cent,
                                                   const GaussRec *__restrict__ recs, const BlockBox *__restrict__ boxes,
                                                   float *__restrict__ out)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long n = (long long)blockIdx.x * LV + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);   // wave-uniform
    if (n >= N) return;   // no barrier below
    const BundleRay b = bundle_ray(rays, n);
    const BundleDir u = bundle_dir(b);
    float acc[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    if (b.valid) {   // wave-uniform; an invalid ray writes exact zeros
        const float Gn = GRAD ? G[n] : 0.0f;
        const int L = leaf_count(P);
        for (int base = 0; base < L; base += WAVE) {
            const int l = base + lane;
            float v[6];
            unsigned long long mask = __ballot(l < L && bundle_ray_box(b, u, half_line, boxes[l < L ? l : 0], v));
            while (mask) {   // wave-uniform: the leaves the line meets, ascending
                const int leaf = base + __ffsll((long long)mask) - 1;
                mask &= mask - 1ull;
                const int i = leaf * LEAF + lane;   // < 2^29 + 64
                if (i >= P) continue;
                const float4 m = cent[i];
                if (!(m.w >= 0.0f) || bundle_line_misses(b, u, m.x, m.y, m.z, m.w)) continue;
                const GaussRec g = recs[i];
                GaussPair p;
                if (!bundle_pair(g, b.y, half_line, p)) continue;
                if (GRAD)
                    gauss_pair_ray_grad(g, p, b.y, b.len, Gn, acc, acc + 3);
                else
                    acc[0] += gauss_term(g, p, b.len);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < (GRAD ? 6 : 1); ++k)
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) acc[k] += __shfl_xor(acc[k], d);
    if (lane == 0) {
        if (GRAD) {
#pragma unroll
            for (int k = 0; k < 6; ++k) out[6 * n + k] = acc[k];
        } else {
            out[n] = acc[0];
        }
    }
}

}  // namespace r2
