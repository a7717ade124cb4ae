// cloud_model.hpp -- what the model-side translation units (gaussian_step.hip, densify_ops.hip, gaussian_mcmc.hip,
// gaussian_merge.hip) know about a Gaussian cloud, stated once.  All four are built with -ffp-contract=off and state their
// results bit for bit, so every expression here is written in the one order they all round in.
//   1. The arithmetic of one Gaussian: the activations of GaussianModel (r2_gaussian/gaussian/gaussian_model.py:38-64) with
//      their inverses, and the rotation matrix of a quaternion.  Host-compilable, as philox.hpp is: plain g++ builds it without
//      HIP (tests/cloud_model_main.cpp).
//   2. Under hipcc, the row model of the kernels that add, move and remove rows: four raw parameter arrays (xyz, density,
//      scaling, rotation), two Adam moments each, three per-row statistics (max_radii2D, grad_accum, denom), in and out.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define R2_CLOUD_HD __host__ __device__ __forceinline__
#else
#define R2_CLOUD_HD inline
#endif

namespace r2 {

R2_CLOUD_HD float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // torch.nn.Softplus(beta=1, threshold=20)
R2_CLOUD_HD float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// Two inverses of the softplus, on purpose.  The reference's float formula (utils/gaussian_utils.py:5-6), which the threshold
// densification reproduces element for element ...
R2_CLOUD_HD float inv_softplus_reference_f(float y) { return logf(expf(y) - 1.0f); }
// ... and the inverse taken in double and rounded once, with softplus_f's threshold, for the relocation: it has no reference to
// follow, and the n + 1 copies of a density rho / (n + 1) should sum back to rho as closely as float allows.
R2_CLOUD_HD float inv_softplus_rounded(float x) { return x > 20.f ? x : (float)log(expm1((double)x)); }

// the scaling activation: sigmoid(x) * range + lo under a scale bound (lo, lo + range), exp(x) without.  `range` is the caller's:
// gaussian_step.hip rounds hi - lo once from double, densify_ops.hip subtracts two floats ("The cloud's row model").
R2_CLOUD_HD float scale_act(float x, bool bounded, float range, float lo) { return bounded ? sigmoid_f(x) * range + lo : expf(x); }
// its inverse as the reference's split forms it: inverse_sigmoid(relu((y - lo) / range)), or log(y)
R2_CLOUD_HD float scale_inv(float y, bool bounded, float range, float lo)
{
    if (!bounded) return logf(y);
    const float t = fmaxf((y - lo) / range, 0.f);
    return logf(t / (1.0f - t));
}

// The rotation matrix of the quaternion (r, x, y, z) as it comes (not normalised), R[j][i] = row j, column i: the same matrix as
// r2_math.hpp's quat_to_rot, which the render and geometry kernels keep for themselves.
template <class T>
R2_CLOUD_HD void quat_rot(T r, T x, T y, T z, T (&R)[3][3])
{
    R[0][0] = T(1) - T(2) * (y * y + z * z); R[0][1] = T(2) * (x * y - r * z); R[0][2] = T(2) * (x * z + r * y);
    R[1][0] = T(2) * (x * y + r * z); R[1][1] = T(1) - T(2) * (x * x + z * z); R[1][2] = T(2) * (y * z - r * x);
    R[2][0] = T(2) * (x * z - r * y); R[2][1] = T(2) * (y * z + r * x); R[2][2] = T(1) - T(2) * (x * x + y * y);
}

#ifdef __HIPCC__
__device__ const int CLOUD_W[4] = { 3, 1, 3, 4 };   // floats per row of xyz, density, scaling, rotation

struct CloudRows {
    const float *p[4], *m[4], *v[4];   // raw parameters, exp_avg, exp_avg_sq; a NULL moment: nothing to move for that array
    float *po[4], *mo[4], *vo[4];
    const float *stat[3];              // max_radii2D, grad_accum, denom
    float *stat_out[3];
};

// what an entry point was handed; the entry decides what it accepts
enum { CLOUD_NONE, CLOUD_ALL, CLOUD_PART };
struct CloudGiven {
    bool params, params_out;   // the table and its four arrays
    int moments, stats;        // CLOUD_NONE: every table / pointer NULL; CLOUD_ALL: every array there; CLOUD_PART: anything else
};

// r from the ABI's pointer tables (each NULL or four pointers) and statistics pointers; an absent table leaves NULLs
inline CloudGiven cloud_rows(CloudRows &r, const float *const *params, const float *const *exp_avg = nullptr,
                             const float *const *exp_avg_sq = nullptr, const float *max_radii2D = nullptr,
                             const float *grad_accum = nullptr, const float *denom = nullptr, float *const *params_out = nullptr,
                             float *const *exp_avg_out = nullptr, float *const *exp_avg_sq_out = nullptr,
                             float *max_radii2D_out = nullptr, float *grad_accum_out = nullptr, float *denom_out = nullptr)
{
    int np = 0, npo = 0, nm = 0, ns = 0;
    for (int a = 0; a < 4; ++a) {
        r.p[a] = params ? params[a] : nullptr; r.po[a] = params_out ? params_out[a] : nullptr;
        r.m[a] = exp_avg ? exp_avg[a] : nullptr; r.mo[a] = exp_avg_out ? exp_avg_out[a] : nullptr;
        r.v[a] = exp_avg_sq ? exp_avg_sq[a] : nullptr; r.vo[a] = exp_avg_sq_out ? exp_avg_sq_out[a] : nullptr;
        np += r.p[a] != nullptr; npo += r.po[a] != nullptr;
        nm += (r.m[a] != nullptr) + (r.v[a] != nullptr) + (r.mo[a] != nullptr) + (r.vo[a] != nullptr);
    }
    r.stat[0] = max_radii2D; r.stat[1] = grad_accum; r.stat[2] = denom;
    r.stat_out[0] = max_radii2D_out; r.stat_out[1] = grad_accum_out; r.stat_out[2] = denom_out;
    for (int k = 0; k < 3; ++k) ns += (r.stat[k] != nullptr) + (r.stat_out[k] != nullptr);
    const bool tables = exp_avg || exp_avg_sq || exp_avg_out || exp_avg_sq_out;
    return CloudGiven{ np == 4, npo == 4, nm == 16 ? CLOUD_ALL : tables ? CLOUD_PART : CLOUD_NONE,
                       ns == 6 ? CLOUD_ALL : ns ? CLOUD_PART : CLOUD_NONE };
}

// output row dst = input row src: the four parameters, and for every array whose moments move (mo[a] != NULL) the source's
// moments, or zeros for a fresh row.  The statistics and whatever a kernel changes in the row are the caller's to write after.
__device__ __forceinline__ void cloud_copy_row(const CloudRows &r, size_t src, size_t dst, bool fresh)
{
    for (int a = 0; a < 4; ++a)
        for (int k = 0; k < CLOUD_W[a]; ++k) {
            const size_t from = src * CLOUD_W[a] + k, to = dst * CLOUD_W[a] + k;
            r.po[a][to] = r.p[a][from];
            if (r.mo[a]) {
                r.mo[a][to] = fresh ? 0.f : r.m[a][from];
                r.vo[a][to] = fresh ? 0.f : r.v[a][from];
            }
        }
}
#endif

}  // namespace r2
