// gaussian_mcmc.hip -- the fixed-budget density control of "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et
// al., NeurIPS 2024) for a cloud whose field is a plain sum: covariance-shaped Langevin noise on the positions of near-dead
// Gaussians (r2_gaussian_noise), and the relocation of dead rows onto live ones drawn in proportion to their weight, with a
// fixed number of appended rows and the Adam state carried along (r2_relocate_plan, r2_relocate_emit); contract in
// include/r2hip.h.  No counterpart in the reference, whose density control is the threshold clone / split / prune.
//
// Randomness is philox.hpp's: a value is a function of (seed, call, purpose, index) alone.  The sampler works in integers -- the
// weights become 64-bit integers, their prefix sum and the draws are exact -- so the sources and their counts depend on nothing
// but the inputs, whatever order the device adds in; the only atomics are integer ones (the largest weight as its bit pattern,
// the counts).  Compiled with -ffp-contract=off: the float arithmetic is, operation for operation, what tests/mcmc_ref.py
// restates.  The inverse softplus of a split density is taken in double and rounded once (cloud_model.hpp).
#include "r2_common.hpp"
#include "cloud_model.hpp"
#include "philox.hpp"

#include <cmath>

namespace r2 {
namespace {

constexpr int MC_THREADS = 256;
constexpr int RL_SCAN_THREADS = 1024, RL_SCAN_IPT = 4;
constexpr int RL_SCAN_TILE = R2_RELOCATE_SCAN_TILE;   // elements per workgroup of the 64-bit scan
static_assert(RL_SCAN_TILE == RL_SCAN_THREADS * RL_SCAN_IPT, "r2hip.h states the tile of the 64-bit scan");
constexpr long long RL_MAX_ROWS = 1ll << 29;          // P + n_new: keeps the prefix sum of the integer weights below 2^62

inline unsigned mc_blocks(size_t n) { return (unsigned)((n + MC_THREADS - 1) / MC_THREADS); }

__device__ __forceinline__ bool mc_finite(float v) { return fabsf(v) < INFINITY; }

// ---- r2_gaussian_noise: one thread per Gaussian
__global__ void __launch_bounds__(MC_THREADS) gaussian_noise_kernel(int P, float *__restrict__ xyz, const float *__restrict__ density,
                                                                    const float *__restrict__ scaling,
                                                                    const float *__restrict__ rotation, double lr, float tau,
                                                                    float kappa, uint64_t seed, uint64_t call)
{
    const int i = blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= P) return;
    const float rho = density[i];
    const float s[3] = { scaling[3 * (size_t)i], scaling[3 * (size_t)i + 1], scaling[3 * (size_t)i + 2] };
    const float q[4] = { rotation[4 * (size_t)i], rotation[4 * (size_t)i + 1], rotation[4 * (size_t)i + 2], rotation[4 * (size_t)i + 3] };
    if (!(mc_finite(rho) && mc_finite(s[0]) && mc_finite(s[1]) && mc_finite(s[2]) && mc_finite(q[0]) && mc_finite(q[1]) &&
          mc_finite(q[2]) && mc_finite(q[3])))
        return;
    float e[3];
    philox_normal3(seed, call, PHILOX_NOISE, (uint32_t)i, e);
    const float gate = 1.0f / (1.0f + expf(kappa * (rho / tau - 1.0f)));
    const float lg = (float)(lr * (double)gate);
    float R[3][3], b[3];   // Sigma = R S^2 R^T
    quat_rot(q[0], q[1], q[2], q[3], R);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = (R[0][k] * e[0] + R[1][k] * e[1]) + R[2][k] * e[2];   // a = R^T eps
        b[k] = (s[k] * s[k]) * a;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float d = (R[j][0] * b[0] + R[j][1] * b[1]) + R[j][2] * b[2];   // R b
        xyz[3 * (size_t)i + j] = xyz[3 * (size_t)i + j] + lg * d;
    }
}

// ---- relocation.  The workspace: w [P] | dead [P] | deadpos [P] | q [P] | cdf [P] | words | 32-bit scan temp | 64-bit partials
enum { RW_WMAX = 0, RW_DRAWABLE, RW_COUNT = 8 };
struct RlSpace {
    float *w;                // the weight of a drawable row, 0 for every other
    uint32_t *dead, *deadpos;   // 1 for a dead row; its inclusive scan
    uint64_t *q, *cdf;       // the integer weights; their inclusive scan
    uint32_t *words;         // RW_*
    char *scan32;
    uint64_t *partial;
    size_t bytes;
};
inline RlSpace rl_space(void *workspace, int P)
{
    Bump b(static_cast<char *>(workspace));
    RlSpace s;
    s.q = b.take<uint64_t>((size_t)P);
    s.cdf = b.take<uint64_t>((size_t)P);
    s.partial = b.take<uint64_t>(((size_t)P + RL_SCAN_TILE - 1) / RL_SCAN_TILE + 1);
    s.w = b.take<float>((size_t)P);
    s.dead = b.take<uint32_t>((size_t)P);
    s.deadpos = b.take<uint32_t>((size_t)P);
    s.words = b.take<uint32_t>(RW_COUNT);
    s.scan32 = b.take<char>(scan_temp_bytes(P));
    s.bytes = b.total();
    return s;
}

// weights: nullable (the activated density)
__global__ void __launch_bounds__(MC_THREADS) relocate_classify_kernel(int P, CloudRows r, const float *density_act,
                                                                       const float *weights, float dead_density,
                                                                       float *__restrict__ w, uint32_t *__restrict__ dead,
                                                                       uint32_t *__restrict__ words)
{
    const int i = blockIdx.x * MC_THREADS + threadIdx.x;
    float wv = 0.f;
    if (i < P) {
        bool fin = true;
        for (int a = 0; a < 4; ++a)
            for (int k = 0; k < CLOUD_W[a]; ++k) fin = fin && mc_finite(r.p[a][(size_t)i * CLOUD_W[a] + k]);
        const float rho = density_act[i];
        const bool alive = fin && rho > dead_density && rho < INFINITY;   // (a NaN fails both)
        const float wi = weights ? weights[i] : rho;
        if (alive && wi > 0.f && wi < INFINITY) wv = wi;
        w[i] = wv;
        dead[i] = alive ? 0u : 1u;
    }
    // positive floats order as their bit patterns: an integer maximum, the same in any order
    uint32_t m = __float_as_uint(wv), n = wv > 0.f ? 1u : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        m = max(m, (uint32_t)__shfl_xor(m, d));
        n += __shfl_xor(n, d);
    }
    if ((threadIdx.x & 63) == 0 && n) {
        atomicMax(&words[RW_WMAX], m);
        atomicAdd(&words[RW_DRAWABLE], n);
    }
}

__global__ void __launch_bounds__(MC_THREADS) relocate_weight_kernel(int P, const float *__restrict__ w,
                                                                     const uint32_t *__restrict__ words, uint64_t *__restrict__ q)
{
    const int i = blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= P) return;
    const float wi = w[i], wmax = __uint_as_float(words[RW_WMAX]);
    uint64_t v = 0;
    if (wi > 0.f) {
        const float ratio = wi / wmax;                                  // in (0, 1], one rounding
        v = (uint64_t)((double)ratio * 4294967296.0);                   // exact: a 24-bit significand times 2^32, truncated
        if (v == 0) v = 1;
    }
    q[i] = v;
}

// the 64-bit inclusive scan: inclusive_scan_u32's two kernels (binning.hip) on 64-bit words
__device__ __forceinline__ uint64_t rl_block_sum(uint64_t v, uint64_t *sh /* [16] */)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    uint64_t t = 0;
#pragma unroll
    for (int k = 0; k < RL_SCAN_THREADS / 64; ++k) t += sh[k];
    __syncthreads();
    return t;
}

__global__ void __launch_bounds__(RL_SCAN_THREADS) scan64_reduce_kernel(const uint64_t *__restrict__ in, uint32_t n,
                                                                        uint64_t *__restrict__ partial)
{
    __shared__ uint64_t sh[RL_SCAN_THREADS / 64];
    const size_t base = (size_t)blockIdx.x * RL_SCAN_TILE + (size_t)threadIdx.x * RL_SCAN_IPT;
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < RL_SCAN_IPT; ++k)
        if (base + k < n) v += in[base + k];
    const uint64_t t = rl_block_sum(v, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ void __launch_bounds__(RL_SCAN_THREADS) scan64_apply_kernel(const uint64_t *__restrict__ in, uint32_t n,
                                                                       const uint64_t *__restrict__ partial,
                                                                       uint64_t *__restrict__ out)
{
    __shared__ uint64_t sh[RL_SCAN_THREADS / 64];
    __shared__ uint64_t wsum[RL_SCAN_THREADS / 64];
    uint64_t pre = 0;
    for (uint32_t g = threadIdx.x; g < blockIdx.x; g += RL_SCAN_THREADS) pre += partial[g];
    const uint64_t tile_base = rl_block_sum(pre, sh);
    const size_t base = (size_t)blockIdx.x * RL_SCAN_TILE + (size_t)threadIdx.x * RL_SCAN_IPT;
    uint64_t x[RL_SCAN_IPT], sum = 0;
#pragma unroll
    for (int k = 0; k < RL_SCAN_IPT; ++k) {
        x[k] = base + k < n ? in[base + k] : 0;
        sum += x[k];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((unsigned long long)incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint64_t run = tile_base + incl - sum;
    for (int k = 0; k < wave; ++k) run += wsum[k];
#pragma unroll
    for (int k = 0; k < RL_SCAN_IPT; ++k) {
        run += x[k];
        if (base + k < n) out[base + k] = run;
    }
}

// one thread per possible slot: slot k < D is the k-th dead row, slot D + j the appended row P + j
__global__ void __launch_bounds__(MC_THREADS) relocate_draw_kernel(int P, int n_new, const uint64_t *__restrict__ cdf,
                                                                   const uint32_t *__restrict__ deadpos, uint64_t seed,
                                                                   uint64_t call, int *__restrict__ sources,
                                                                   uint32_t *__restrict__ draws)
{
    const size_t k = (size_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (k >= (size_t)P + (size_t)n_new) return;
    const size_t slots = (size_t)deadpos[P - 1] + (size_t)n_new;
    const uint64_t T = cdf[P - 1];
    if (k >= slots || T == 0) {
        sources[k] = -1;
        return;
    }
    const Philox4 p = philox_words(seed, call, PHILOX_DRAW, (uint32_t)k);
    const uint64_t r = ((uint64_t)p.w[0] << 32) | (uint64_t)p.w[1];
    const uint64_t t = __umul64hi(r, T);          // in [0, T)
    int lo = 0, hi = P - 1;                       // the first i with cdf[i] > t; cdf[P - 1] = T > t
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    sources[k] = lo;
    atomicAdd(&draws[lo], 1u);
}

// one thread per OUTPUT row: every word of the outputs has one writer.  Moments and statistics: all there or all NULL
__global__ void __launch_bounds__(MC_THREADS) relocate_emit_kernel(int P, int n_new, CloudRows r, const float *density_act,
                                                                   const float *scaling_act,
                                                                   const float *rotation_act, float spread,
                                                                   uint64_t seed, uint64_t call, const uint32_t *__restrict__ dead,
                                                                   const uint32_t *__restrict__ deadpos,
                                                                   const uint64_t *__restrict__ cdf, const int *__restrict__ sources,
                                                                   const uint32_t *__restrict__ draws)
{
    const size_t o = (size_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (o >= (size_t)P + (size_t)n_new) return;
    const uint32_t D = deadpos[P - 1];
    const bool drawable = cdf[P - 1] != 0;
    // what row o becomes: a slot filled from `src` (slot >= 0), a source that keeps its place, or a copy of row `src`
    long long slot = -1;
    size_t src = o;
    bool fresh = false, parked = false;
    if (o < (size_t)P) {
        if (dead[o]) {
            if (drawable) slot = (long long)deadpos[o] - 1;
        } else if (draws[o] >= 1u) {
            fresh = true;
        }
    } else if (drawable) {
        slot = (long long)D + (long long)(o - (size_t)P);
    } else {
        src = (o - (size_t)P) % (size_t)P;   // nothing to draw from: a finite row that is dead, relocated next time
        fresh = parked = true;
    }
    if (slot >= 0) {
        // (arrays that are not r2_relocate_plan's on these inputs: nothing outside the inputs is read, nothing outside the outputs written)
        if ((size_t)slot >= (size_t)P + (size_t)n_new) return;
        const int sidx = sources[slot];
        if (sidx < 0 || sidx >= P) return;
        src = (size_t)sidx;
        fresh = true;
    }
    cloud_copy_row(r, src, o, fresh);
    for (int k = 0; k < 3; ++k)
        if (r.stat_out[k]) r.stat_out[k][o] = fresh ? 0.f : r.stat[k][src];
    if (!fresh) return;
    if (parked) {
        r.po[1][o] = -100.f;
        return;
    }
    const uint32_t n = min(draws[src], 0x7ffffffeu);
    r.po[1][o] = inv_softplus_rounded(density_act[src] / (float)(n + 1u));
    if (slot >= 0 && spread > 0.f) {
        float e[3], R[3][3], v[3];
        philox_normal3(seed, call, PHILOX_SPREAD, (uint32_t)slot, e);
        const float *q = rotation_act + 4 * src;
        quat_rot(q[0], q[1], q[2], q[3], R);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = scaling_act[3 * src + k] * e[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float d = (R[j][0] * v[0] + R[j][1] * v[1]) + R[j][2] * v[2];   // R S eps
            r.po[0][3 * o + j] = r.p[0][3 * src + j] + spread * d;
        }
    }
}

int scan64(const uint64_t *in, uint64_t *out, uint64_t *partial, int P, hipStream_t s)
{
    const unsigned tiles = (unsigned)(((size_t)P + RL_SCAN_TILE - 1) / RL_SCAN_TILE);
    scan64_reduce_kernel<<<dim3(tiles), dim3(RL_SCAN_THREADS), 0, s>>>(in, (uint32_t)P, partial);
    scan64_apply_kernel<<<dim3(tiles), dim3(RL_SCAN_THREADS), 0, s>>>(in, (uint32_t)P, partial, out);
    R2_HIP_TRY(hipGetLastError());
    return 0;
}

bool rl_shape_ok(int P, int n_new) { return P >= 0 && n_new >= 0 && (long long)P + n_new <= RL_MAX_ROWS && !(P == 0 && n_new > 0); }

}  // namespace
}  // namespace r2

extern "C" int r2_gaussian_noise(int P, float *xyz, const float *density, const float *scaling, const float *rotation, double lr,
                                 float density_threshold, float sharpness, unsigned long long seed, unsigned long long call,
                                 void *stream)
{
    using namespace r2;
    if (P < 0 || !(lr >= 0.0) || !(lr < (double)INFINITY) || !(density_threshold > 0.f) || !(density_threshold < INFINITY) ||
        !(sharpness >= 0.f) || !(sharpness < INFINITY) || (P > 0 && (!xyz || !density || !scaling || !rotation))) {
        set_error("r2_gaussian_noise: invalid argument (P < 0, a NULL array, lr or sharpness not in [0, inf), "
                  "density_threshold not in (0, inf))");
        return R2_ERR_INVALID;
    }
    if (P == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    gaussian_noise_kernel<<<dim3(mc_blocks((size_t)P)), dim3(MC_THREADS), 0, s>>>(P, xyz, density, scaling, rotation, lr,
                                                                                 density_threshold, sharpness, (uint64_t)seed,
                                                                                 (uint64_t)call);
    R2_STAGE_CHECK(0, s, "gaussian noise");
    return 0;
}

extern "C" size_t r2_relocate_workspace_bytes(int P, int n_new)
{
    if (!r2::rl_shape_ok(P, n_new) || P == 0) return 0;
    return r2::rl_space(nullptr, P).bytes;
}

extern "C" int r2_relocate_plan(int P, int n_new, const float *const *params, const float *density_act, const float *weights,
                                float dead_density, unsigned long long seed, unsigned long long call, int *sources,
                                unsigned int *draws, void *workspace, size_t workspace_bytes, unsigned int *counts_host,
                                void *stream)
{
    using namespace r2;
    if (!rl_shape_ok(P, n_new)) {
        set_error("r2_relocate_plan: invalid shape (P < 0, n_new < 0, P + n_new > 2^29, or P = 0 with n_new > 0)");
        return R2_ERR_INVALID;
    }
    if (counts_host) counts_host[0] = counts_host[1] = counts_host[2] = 0u;
    if (P == 0) return 0;
    CloudRows r;
    if (!cloud_rows(r, params).params || !density_act || !sources || !draws || !(dead_density == dead_density)) {
        set_error("r2_relocate_plan: a NULL array, or a NaN dead_density");
        return R2_ERR_INVALID;
    }
    if (!workspace || workspace_bytes < r2_relocate_workspace_bytes(P, n_new)) {
        set_error("r2_relocate_plan: the workspace must hold %zu bytes", r2_relocate_workspace_bytes(P, n_new));
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const RlSpace w = rl_space(workspace, P);
    const size_t rows = (size_t)P + (size_t)n_new;
    R2_HIP_TRY(hipMemsetAsync(w.words, 0, RW_COUNT * sizeof(uint32_t), s));
    R2_HIP_TRY(hipMemsetAsync(draws, 0, (size_t)P * sizeof(uint32_t), s));
    relocate_classify_kernel<<<dim3(mc_blocks((size_t)P)), dim3(MC_THREADS), 0, s>>>(P, r, density_act, weights, dead_density, w.w, w.dead,
                                                                                     w.words);
    relocate_weight_kernel<<<dim3(mc_blocks((size_t)P)), dim3(MC_THREADS), 0, s>>>(P, w.w, w.words, w.q);
    int rc = scan64(w.q, w.cdf, w.partial, P, s);
    if (rc) return rc;
    rc = inclusive_scan_u32(w.scan32, scan_temp_bytes(P), w.dead, w.deadpos, P, s);
    if (rc) return rc;
    relocate_draw_kernel<<<dim3(mc_blocks(rows)), dim3(MC_THREADS), 0, s>>>(P, n_new, w.cdf, w.deadpos, (uint64_t)seed, (uint64_t)call,
                                                                           sources, draws);
    R2_STAGE_CHECK(0, s, "relocate plan");
    if (counts_host) {
        uint32_t h[2];
        R2_HIP_TRY(hipMemcpyAsync(&h[0], w.deadpos + (P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        R2_HIP_TRY(hipMemcpyAsync(&h[1], w.words + RW_DRAWABLE, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        R2_HIP_TRY(hipStreamSynchronize(s));
        counts_host[0] = h[0];
        counts_host[1] = (uint32_t)P - h[0];
        counts_host[2] = h[1];
    }
    return 0;
}

extern "C" int r2_relocate_emit(int P, int n_new, const float *const *params, const float *const *exp_avg,
                                const float *const *exp_avg_sq, const float *density_act, const float *scaling_act,
                                const float *rotation_act, const float *max_radii2D, const float *grad_accum, const float *denom,
                                float spread, unsigned long long seed, unsigned long long call, const int *sources,
                                const unsigned int *draws, const void *workspace, size_t workspace_bytes, float *const *params_out,
                                float *const *exp_avg_out, float *const *exp_avg_sq_out, float *max_radii2D_out,
                                float *grad_accum_out, float *denom_out, void *stream)
{
    using namespace r2;
    if (!rl_shape_ok(P, n_new)) {
        set_error("r2_relocate_emit: invalid shape (P < 0, n_new < 0, P + n_new > 2^29, or P = 0 with n_new > 0)");
        return R2_ERR_INVALID;
    }
    if (P == 0) return 0;
    CloudRows r;
    const CloudGiven g = cloud_rows(r, params, exp_avg, exp_avg_sq, max_radii2D, grad_accum, denom, params_out, exp_avg_out,
                                     exp_avg_sq_out, max_radii2D_out, grad_accum_out, denom_out);
    if (!g.params || !g.params_out || g.moments == CLOUD_PART || g.stats == CLOUD_PART || !density_act || !sources || !draws ||
        !(spread >= 0.f && spread < INFINITY) || (spread != 0.f && !(scaling_act && rotation_act))) {
        set_error("r2_relocate_emit: a NULL array, moment or statistics arrays given in part, spread not in [0, inf), or "
                  "spread > 0 without the activated scaling and rotation");
        return R2_ERR_INVALID;
    }
    if (!workspace || workspace_bytes < r2_relocate_workspace_bytes(P, n_new)) {
        set_error("r2_relocate_emit: the workspace must hold %zu bytes", r2_relocate_workspace_bytes(P, n_new));
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const RlSpace w = rl_space(const_cast<void *>(workspace), P);
    relocate_emit_kernel<<<dim3(mc_blocks((size_t)P + (size_t)n_new)), dim3(MC_THREADS), 0, s>>>(
        P, n_new, r, density_act, scaling_act, rotation_act, spread, (uint64_t)seed, (uint64_t)call, w.dead, w.deadpos, w.cdf, sources,
        draws);
    R2_STAGE_CHECK(0, s, "relocate emit");
    return 0;
}
