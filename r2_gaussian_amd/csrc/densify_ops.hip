// densify_ops.hip -- adaptive density control on the device: the densification statistics of a view, and
// densify (clone / split) + prune with the optimizer-state surgery, as a handful of kernels and ONE host read instead of
// ~30 torch ops with boolean-mask indexing (each a device synchronisation) and two full passes of optimizer-state
// re-allocation.  Reference: r2_gaussian/gaussian/gaussian_model.py:320-556 (densify_and_clone, densify_and_split,
// prune_points, cat_tensors_to_optimizer, _prune_optimizer, add_densification_stats), train.py:151-168.
//
// Result layout = the reference's, element for element: [surviving originals in order | surviving clones | surviving first
// split children | surviving second split children] (densification_postfix appends clones, then the 2 x selected children as
// two repeated blocks; the split parents and the pruned rows are then removed by stable masks).
#include "r2_common.hpp"
#include "cloud_model.hpp"

namespace r2 {
namespace {

struct DensifyCfg {
    float grad_thr, scale_thr, density_min;
    float lo[3], hi[3];          // bounding box
    bool bounded;                // scale_lo < scale_hi: the bounded-sigmoid scaling activation; else exp (cloud_model.hpp)
    float s_range, s_lo;         // scale_hi - scale_lo subtracted in float, scale_lo
    int do_densify;
    float max_screen, max_scale; // optional prune thresholds (gaussian_model.py:540-545); <= 0: off (the reference's None)
};

__device__ __forceinline__ bool outside(const float *p, const DensifyCfg &c)
{
    return p[0] < c.lo[0] || p[0] > c.hi[0] || p[1] < c.lo[1] || p[1] > c.hi[1] || p[2] < c.lo[2] || p[2] > c.hi[2];
}

struct Decision {
    bool clone, split, keep_orig, keep_clone, keep_child[2];
    float density_raw_orig;       // raw density of the original after the clone step (halved if cloned)
    float child_xyz[2][3], child_density_raw, child_scaling_raw[3];
};

// everything densify_and_prune decides about Gaussian i (gaussian_model.py:430-550), recomputed by both passes; of r it reads the
// four parameters and stat = max_radii2D, grad_accum, denom
__device__ __forceinline__ Decision decide(int i, int P, const CloudRows &r, const float *__restrict__ normals, const DensifyCfg &c)
{
    Decision d;
    const float *xyz = r.p[0], *density = r.p[1], *scaling = r.p[2], *rotation = r.p[3], *max_radii = r.stat[0];
    const float p[3] = { xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] };
    auto act = [&](float x) { return scale_act(x, c.bounded, c.s_range, c.s_lo); };
    const float s[3] = { act(scaling[3 * i]), act(scaling[3 * i + 1]), act(scaling[3 * i + 2]) };
    const float smax = fmaxf(fmaxf(s[0], s[1]), s[2]);
    const float dens = softplus_f(density[i]);
    float g = r.stat[1][i] / r.stat[2][i];
    if (g != g) g = 0.f;                                   // grads[grads.isnan()] = 0
    const bool hot = c.do_densify && g >= c.grad_thr;
    d.clone = hot && smax <= c.scale_thr;                  // :474-483
    d.split = hot && smax > c.scale_thr;                   // :430-441
    d.density_raw_orig = d.clone ? inv_softplus_reference_f(dens * 0.5f) : density[i];   // :486-493: both copies get half the density
    // the prune mask is evaluated AFTER clone / split on all rows (:524-546); a clone shares its original's scale and
    // max_radii2D, split children inherit the parent's max_radii2D (:468) and get scale / 1.6
    const bool big_screen = c.max_screen > 0.f && max_radii[i] > c.max_screen;   // :540-542
    const bool pruned = softplus_f(d.density_raw_orig) < c.density_min || outside(p, c) || big_screen ||
                        (c.max_scale > 0.f && smax > c.max_scale);               // :543-545
    d.keep_orig = !d.split && !pruned;
    d.keep_clone = d.clone && !pruned;
    d.keep_child[0] = d.keep_child[1] = false;
    if (d.split) {
        // rotation matrix of the normalised quaternion (utils/gaussian_utils.py:49-84)
        const float q0 = rotation[4 * i], q1 = rotation[4 * i + 1], q2 = rotation[4 * i + 2], q3 = rotation[4 * i + 3];
        const float n = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
        float R[3][3];
        quat_rot(q0 / n, q1 / n, q2 / n, q3 / n, R);
        d.child_density_raw = inv_softplus_reference_f(dens * 0.5f);
        for (int k = 0; k < 3; ++k) d.child_scaling_raw[k] = scale_inv(s[k] / 1.6f, c.bounded, c.s_range, c.s_lo);   // / (0.8 N), N = 2
        bool low = softplus_f(d.child_density_raw) < c.density_min || big_screen;
        if (c.max_scale > 0.f)
            low = low || fmaxf(fmaxf(act(d.child_scaling_raw[0]), act(d.child_scaling_raw[1])), act(d.child_scaling_raw[2])) > c.max_scale;
        for (int ch = 0; ch < 2; ++ch) {
            const float *nn = normals + ((size_t)ch * P + i) * 3;
            const float v[3] = { nn[0] * s[0], nn[1] * s[1], nn[2] * s[2] };   // N(0, scale) in the local frame
            for (int j = 0; j < 3; ++j) d.child_xyz[ch][j] = R[j][0] * v[0] + R[j][1] * v[1] + R[j][2] * v[2] + p[j];
            d.keep_child[ch] = !low && !outside(d.child_xyz[ch], c);
        }
    }
    return d;
}

__global__ void __launch_bounds__(256) densify_classify_kernel(int P, CloudRows r, const float *__restrict__ normals, DensifyCfg c,
                                                               uint32_t *__restrict__ keep /* [4][P] */)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const Decision d = decide(i, P, r, normals, c);
    keep[i] = d.keep_orig;
    keep[(size_t)P + i] = d.keep_clone;
    keep[2 * (size_t)P + i] = d.keep_child[0];
    keep[3 * (size_t)P + i] = d.keep_child[1];
}

__global__ void __launch_bounds__(256) densify_emit_kernel(int P, CloudRows r, const float *__restrict__ normals, DensifyCfg c,
                                                           const uint32_t *__restrict__ pos /* [4][P] inclusive scans */)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const Decision d = decide(i, P, r, normals, c);
    const uint32_t n0 = pos[P - 1], n1 = pos[2 * (size_t)P - 1], n2 = pos[3 * (size_t)P - 1];
    // row o from Gaussian i with another raw density; fresh rows (zero moments) of a split also get their own xyz and scaling
    auto write = [&](size_t o, bool fresh, float dens_raw, const float *xyz_new, const float *scal_raw) {
        cloud_copy_row(r, (size_t)i, o, fresh);
        r.po[1][o] = dens_raw;
        if (xyz_new)
            for (int k = 0; k < 3; ++k) { r.po[0][o * 3 + k] = xyz_new[k]; r.po[2][o * 3 + k] = scal_raw[k]; }
        r.stat_out[0][o] = r.stat[0][i];
        // densification_postfix resets the statistics (:423-425); a prune-only call (P >= max_num_gaussians) keeps them
        r.stat_out[1][o] = c.do_densify ? 0.f : r.stat[1][i];
        r.stat_out[2][o] = c.do_densify ? 0.f : r.stat[2][i];
    };
    if (d.keep_orig) write(pos[i] - 1u, false, d.density_raw_orig, nullptr, nullptr);   // parameters and Adam moments move with it
    if (d.keep_clone) write((size_t)n0 + pos[(size_t)P + i] - 1u, true, d.density_raw_orig, nullptr, nullptr);
    if (d.keep_child[0]) write((size_t)n0 + n1 + pos[2 * (size_t)P + i] - 1u, true, d.child_density_raw, d.child_xyz[0], d.child_scaling_raw);
    if (d.keep_child[1])
        write((size_t)n0 + n1 + n2 + pos[3 * (size_t)P + i] - 1u, true, d.child_density_raw, d.child_xyz[1], d.child_scaling_raw);
}

// train.py:151-154 + add_densification_stats (gaussian_model.py:552-556) of ONE view for ONE Gaussian, on the three statistics
// in registers.  The single-view and the batched kernel both are this function.
__device__ __forceinline__ void densify_stats_view(int rad, const float *__restrict__ g /* dL_dmeans2D row */, float grad_scale,
                                                   float &max_radius, float &accum, float &count)
{
    if (!(rad > 0)) return;
    max_radius = fmaxf(max_radius, (float)rad);
    const float gx = g[0], gy = g[1];
    accum += grad_scale * sqrtf(gx * gx + gy * gy);
    count += 1.0f;
}

// one launch, no boolean-mask indexing
__global__ void __launch_bounds__(256) densify_stats_kernel(int P, const int *__restrict__ radii, const float *__restrict__ g2d,
                                                            float *__restrict__ max_radii, float *__restrict__ grad_accum,
                                                            float *__restrict__ denom)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int rad = radii[i];
    if (!(rad > 0)) return;
    float mr = max_radii[i], ga = grad_accum[i], dn = denom[i];
    densify_stats_view(rad, g2d + 3 * (size_t)i, 1.0f, mr, ga, dn);
    max_radii[i] = mr; grad_accum[i] = ga; denom[i] = dn;
}

// V views of the same Gaussians (radii [V,P], g2d [V,P,3]): every thread owns a Gaussian and walks the views in order
__global__ void __launch_bounds__(256) densify_stats_batch_kernel(int P, int V, const int *__restrict__ radii,
                                                                  const float *__restrict__ g2d, float grad_scale,
                                                                  float *__restrict__ max_radii, float *__restrict__ grad_accum,
                                                                  float *__restrict__ denom)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    float mr = max_radii[i], ga = grad_accum[i], dn = denom[i];
    bool seen = false;
    for (int v = 0; v < V; ++v) {
        const size_t o = (size_t)v * P + i;
        const int rad = radii[o];
        seen = seen || rad > 0;
        densify_stats_view(rad, g2d + 3 * o, grad_scale, mr, ga, dn);
    }
    if (seen) { max_radii[i] = mr; grad_accum[i] = ga; denom[i] = dn; }
}

}  // namespace
}  // namespace r2

extern "C" int r2_densify_stats(int P, const int *radii, const float *dL_dmeans2D, float *max_radii2D, float *grad_accum,
                                float *denom, void *stream)
{
    if (P == 0) return 0;
    if (P < 0 || !radii || !dL_dmeans2D || !max_radii2D || !grad_accum || !denom) {
        r2::set_error("r2_densify_stats: invalid argument");
        return R2_ERR_INVALID;
    }
    r2::densify_stats_kernel<<<dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(P, radii, dL_dmeans2D, max_radii2D,
                                                                                          grad_accum, denom);
    R2_STAGE_CHECK(0, (hipStream_t)stream, "densification statistics");
    return 0;
}

extern "C" int r2_densify_stats_batch(int P, int V, const int *radii, const float *dL_dmeans2D, float grad_scale, float *max_radii2D,
                                      float *grad_accum, float *denom, void *stream)
{
    if (P < 0 || V < 1) {
        r2::set_error("r2_densify_stats_batch: invalid argument (P < 0 or V < 1)");
        return R2_ERR_INVALID;
    }
    if (P == 0) return 0;
    if (!radii || !dL_dmeans2D || !max_radii2D || !grad_accum || !denom) {
        r2::set_error("r2_densify_stats_batch: invalid argument (NULL array)");
        return R2_ERR_INVALID;
    }
    r2::densify_stats_batch_kernel<<<dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(P, V, radii, dL_dmeans2D, grad_scale,
                                                                                                max_radii2D, grad_accum, denom);
    R2_STAGE_CHECK(0, (hipStream_t)stream, "batched densification statistics");
    return 0;
}

extern "C" size_t r2_densify_scratch_bytes(int P)
{
    return 2 * 4 * (size_t)P * sizeof(uint32_t) + r2::scan_temp_bytes(4 * P) + 1024;
}

static r2::DensifyCfg make_cfg(float grad_thr, float scale_thr, float density_min, const float *bbox, float scale_lo, float scale_hi,
                               int do_densify, float max_screen_size, float max_scale)
{
    r2::DensifyCfg c;
    c.grad_thr = grad_thr; c.scale_thr = scale_thr; c.density_min = density_min;
    for (int k = 0; k < 3; ++k) { c.lo[k] = bbox[k]; c.hi[k] = bbox[3 + k]; }
    c.bounded = scale_lo < scale_hi; c.s_range = scale_hi - scale_lo; c.s_lo = scale_lo; c.do_densify = do_densify;
    c.max_screen = max_screen_size; c.max_scale = max_scale;
    return c;
}

// pass 1: decide and count.  counts_host[4] = surviving {originals, clones, first children, second children}; the call
// synchronises the stream once to read them (the caller sizes the outputs with them).
extern "C" int r2_densify_classify(int P, const float *xyz, const float *density, const float *scaling, const float *rotation,
                                   const float *max_radii2D, const float *grad_accum, const float *denom, const float *normals,
                                   float grad_thr, float scale_thr, float density_min, const float *bbox_host, float scale_lo,
                                   float scale_hi, int do_densify, float max_screen_size, float max_scale, void *scratch,
                                   unsigned int *counts_host, void *stream)
{
    using namespace r2;
    if (P <= 0 || !xyz || !density || !scaling || !rotation || !max_radii2D || !grad_accum || !denom || !normals || !bbox_host ||
        !scratch || !counts_host) {
        set_error("r2_densify_classify: invalid argument");
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const DensifyCfg c = make_cfg(grad_thr, scale_thr, density_min, bbox_host, scale_lo, scale_hi, do_densify, max_screen_size, max_scale);
    uint32_t *keep = reinterpret_cast<uint32_t *>(scratch), *pos = keep + 4 * (size_t)P;
    char *scan_temp = reinterpret_cast<char *>(pos + 4 * (size_t)P);
    const float *const params[4] = { xyz, density, scaling, rotation };
    CloudRows r;
    cloud_rows(r, params, nullptr, nullptr, max_radii2D, grad_accum, denom);
    densify_classify_kernel<<<dim3((P + 255) / 256), dim3(256), 0, s>>>(P, r, normals, c, keep);
    for (int a = 0; a < 4; ++a) {
        const int rc = inclusive_scan_u32(scan_temp, scan_temp_bytes(4 * P), keep + (size_t)a * P, pos + (size_t)a * P, P, s);
        if (rc) return rc;
    }
    uint32_t h[4];
    for (int a = 0; a < 4; ++a)
        R2_HIP_TRY(hipMemcpyAsync(&h[a], pos + (size_t)(a + 1) * P - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    R2_HIP_TRY(hipStreamSynchronize(s));
    for (int a = 0; a < 4; ++a) counts_host[a] = h[a];
    return 0;
}

// pass 2: write the new parameter / Adam-moment / statistics arrays (sized sum(counts) rows) from the decisions of pass 1
// (recomputed: same inputs, same code).  params / exp_avg / exp_avg_sq: 4 pointers each in the order xyz, density, scaling,
// rotation; the moment arrays may be all NULL (no optimizer state yet).
extern "C" int r2_densify_emit(int P, const float *const *params, const float *const *exp_avg, const float *const *exp_avg_sq,
                               const float *max_radii2D, const float *grad_accum, const float *denom, const float *normals,
                               float grad_thr, float scale_thr, float density_min, const float *bbox_host, float scale_lo,
                               float scale_hi, int do_densify, float max_screen_size, float max_scale, const void *scratch,
                               float *const *params_out,
                               float *const *exp_avg_out, float *const *exp_avg_sq_out, float *max_radii2D_out,
                               float *grad_accum_out, float *denom_out, void *stream)
{
    using namespace r2;
    // decide() reads grad_accum, denom and normals on the device and make_cfg reads bbox_host here: as in r2_densify_classify
    if (P <= 0 || !params || !params_out || !max_radii2D || !grad_accum || !denom || !normals || !bbox_host || !max_radii2D_out ||
        !grad_accum_out || !denom_out || !scratch) {
        set_error("r2_densify_emit: invalid argument");
        return R2_ERR_INVALID;
    }
    CloudRows r;
    const CloudGiven g = cloud_rows(r, params, exp_avg, exp_avg_sq, max_radii2D, grad_accum, denom, params_out, exp_avg_out,
                                     exp_avg_sq_out, max_radii2D_out, grad_accum_out, denom_out);
    bool ok = g.params && g.params_out;
    for (int a = 0; a < 4; ++a) {   // an array's moments move when all four of its moment arrays are there; none, or nothing moves
        const int n = (r.m[a] != nullptr) + (r.v[a] != nullptr) + (r.mo[a] != nullptr) + (r.vo[a] != nullptr);
        ok = ok && (n == 0 || n == 4);   // exp_avg without exp_avg_sq, or an input without its output, would drop state silently
    }
    if (!ok) {
        set_error("r2_densify_emit: NULL parameter array / inconsistent moment arrays");
        return R2_ERR_INVALID;
    }
    const DensifyCfg c = make_cfg(grad_thr, scale_thr, density_min, bbox_host, scale_lo, scale_hi, do_densify, max_screen_size, max_scale);
    const uint32_t *pos = reinterpret_cast<const uint32_t *>(scratch) + 4 * (size_t)P;
    densify_emit_kernel<<<dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(P, r, normals, c, pos);
    R2_STAGE_CHECK(0, (hipStream_t)stream, "densify emit");
    return 0;
}
