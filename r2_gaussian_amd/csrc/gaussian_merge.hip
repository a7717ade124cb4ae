// gaussian_merge.hip -- moment-preserving merging of neighbouring Gaussians: Runnalls' Kullback-Leibler bound on the edges of a
// neighbour graph (r2_merge_cost), a locally-dominant-edge matching of any graph (r2_graph_match), and the replacement of every
// matched pair by the single Gaussian of the same mass, mean and second moment (r2_merge_count, r2_merge_emit); contract in
// include/r2hip.h.  No counterpart in the reference.
//
// All per-pair arithmetic is double, rounded to float once at the store: a determinant or an eigen-decomposition of a 100:1
// anisotropic covariance loses 3-4 digits in float32, and the edges are few (P * K).  Compiled with -ffp-contract=off.  No
// atomics: every output word has one writer and every reduction a fixed order, so two calls give the same bits.
#include "r2_common.hpp"
#include "cloud_model.hpp"

#include <climits>
#include <cmath>

namespace r2 {
namespace {

constexpr int MG_THREADS = 256;
constexpr int MG_HUB = R2_MERGE_HUB;          // longer incoming lists are walked by the whole wave
constexpr int MG_SWEEPS = R2_MERGE_JACOBI_SWEEPS;

// ---- one Gaussian in double: mean, covariance (xx, xy, xz, yy, yz, zz), mass = density * s1 s2 s3
struct MgGauss {
    double mu[3], cov[6], mass;
    bool ok;   // every parameter finite, density > 0, scales > 0
};

__device__ __forceinline__ double mg_mass(int i, const float *__restrict__ density, const float *__restrict__ scaling)
{
    return (double)density[i] * (double)scaling[3 * (size_t)i] * (double)scaling[3 * (size_t)i + 1] * (double)scaling[3 * (size_t)i + 2];
}
__device__ __forceinline__ bool mg_mass_ok(double m) { return m > 0.0 && m < INFINITY; }

__device__ __forceinline__ MgGauss mg_load(int i, const float *__restrict__ means, const float *__restrict__ density,
                                           const float *__restrict__ scaling, const float *__restrict__ rotation)
{
    MgGauss g;
    const float rho = density[i];
    const float s[3] = { scaling[3 * (size_t)i], scaling[3 * (size_t)i + 1], scaling[3 * (size_t)i + 2] };
    const float q[4] = { rotation[4 * (size_t)i], rotation[4 * (size_t)i + 1], rotation[4 * (size_t)i + 2], rotation[4 * (size_t)i + 3] };
    bool fin = isfinite(rho);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float m = means[3 * (size_t)i + k];
        g.mu[k] = (double)m;
        fin = fin && isfinite(m) && isfinite(s[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) fin = fin && isfinite(q[k]);
    g.ok = fin && rho > 0.f && s[0] > 0.f && s[1] > 0.f && s[2] > 0.f;
    g.mass = (double)rho * (double)s[0] * (double)s[1] * (double)s[2];
    double R[3][3];   // Sigma = R^T diag(s^2) R of the quaternion as given (r2_math.hpp: cov3d_from_scale_rot, mod = 1)
    quat_rot((double)q[0], (double)q[1], (double)q[2], (double)q[3], R);
    const double v[3] = { (double)s[0] * (double)s[0], (double)s[1] * (double)s[1], (double)s[2] * (double)s[2] };
    g.cov[0] = (v[0] * R[0][0] * R[0][0] + v[1] * R[1][0] * R[1][0]) + v[2] * R[2][0] * R[2][0];
    g.cov[1] = (v[0] * R[0][0] * R[0][1] + v[1] * R[1][0] * R[1][1]) + v[2] * R[2][0] * R[2][1];
    g.cov[2] = (v[0] * R[0][0] * R[0][2] + v[1] * R[1][0] * R[1][2]) + v[2] * R[2][0] * R[2][2];
    g.cov[3] = (v[0] * R[0][1] * R[0][1] + v[1] * R[1][1] * R[1][1]) + v[2] * R[2][1] * R[2][1];
    g.cov[4] = (v[0] * R[0][1] * R[0][2] + v[1] * R[1][1] * R[1][2]) + v[2] * R[2][1] * R[2][2];
    g.cov[5] = (v[0] * R[0][2] * R[0][2] + v[1] * R[1][2] * R[1][2]) + v[2] * R[2][2] * R[2][2];
    return g;
}

// the moment-matched Gaussian of the pair (a, b): alpha = m_a / (m_a + m_b), Sigma_ab = alpha Sigma_a + (1 - alpha) Sigma_b +
// alpha (1 - alpha) d d^T with d = mu_a - mu_b
__device__ __forceinline__ void mg_pair(const MgGauss &a, const MgGauss &b, double &alpha, double cov[6])
{
    alpha = a.mass / (a.mass + b.mass);
    const double beta = 1.0 - alpha, w = alpha * beta;
    const double d[3] = { a.mu[0] - b.mu[0], a.mu[1] - b.mu[1], a.mu[2] - b.mu[2] };
    cov[0] = (alpha * a.cov[0] + beta * b.cov[0]) + w * (d[0] * d[0]);
    cov[1] = (alpha * a.cov[1] + beta * b.cov[1]) + w * (d[0] * d[1]);
    cov[2] = (alpha * a.cov[2] + beta * b.cov[2]) + w * (d[0] * d[2]);
    cov[3] = (alpha * a.cov[3] + beta * b.cov[3]) + w * (d[1] * d[1]);
    cov[4] = (alpha * a.cov[4] + beta * b.cov[4]) + w * (d[1] * d[2]);
    cov[5] = (alpha * a.cov[5] + beta * b.cov[5]) + w * (d[2] * d[2]);
}

// log det of a symmetric positive definite 3 x 3 by its L D L^T pivots (backward stable: the relative error of the determinant
// grows with the condition number, not with its square as the cofactor expansion's does); NaN when a pivot is not positive
__device__ __forceinline__ double mg_logdet(const double c[6])
{
    const double d1 = c[0];
    const double l10 = c[1] / d1, l20 = c[2] / d1;
    const double d2 = c[3] - l10 * c[1];
    const double t = c[4] - l20 * c[1];
    const double d3 = (c[5] - l20 * c[2]) - (t / d2) * t;
    if (!(d1 > 0.0 && d2 > 0.0 && d3 > 0.0)) return NAN;
    return (log(d1) + log(d2)) + log(d3);
}

// ---- r2_merge_cost: one thread per directed edge
__global__ void __launch_bounds__(MG_THREADS) merge_cost_kernel(int P, int K, uint32_t n, const int *__restrict__ idx,
                                                                const float *__restrict__ means, const float *__restrict__ density,
                                                                const float *__restrict__ scaling, const float *__restrict__ rotation,
                                                                float max_trace, float *__restrict__ cost)
{
    const uint32_t e = blockIdx.x * (uint32_t)MG_THREADS + threadIdx.x;
    if (e >= n) return;
    const int i = (int)(e / (uint32_t)K), j = idx[e];
    float out = INFINITY;
    if (j >= 0 && j < P && j != i) {
        // the pair in index order: both directions of an edge run the same operations on the same operands
        const MgGauss a = mg_load(min(i, j), means, density, scaling, rotation);
        const MgGauss b = mg_load(max(i, j), means, density, scaling, rotation);
        if (a.ok && b.ok) {
            double alpha, cov[6];
            mg_pair(a, b, alpha, cov);
            const double c = 0.5 * ((mg_logdet(cov) - alpha * mg_logdet(a.cov)) - (1.0 - alpha) * mg_logdet(b.cov));
            const bool wide = max_trace > 0.f && (cov[0] + cov[3]) + cov[5] > (double)max_trace;
            if (!wide && c < INFINITY) out = (float)fmax(c, 0.0);   // (a NaN fails the comparison)
        }
    }
    cost[e] = out;
}

// ---- r2_graph_match.  The key of a directed edge between i and j: (cost, min(i, j), max(i, j)), lexicographic.
struct MgKey {
    float c;
    int lo, hi;
};
__device__ __forceinline__ MgKey mg_none() { return MgKey{ INFINITY, INT_MAX, INT_MAX }; }
__device__ __forceinline__ bool mg_less(const MgKey &a, const MgKey &b)
{
    if (a.c < b.c) return true;
    if (a.c > b.c) return false;
    if (a.lo != b.lo) return a.lo < b.lo;
    return a.hi < b.hi;
}

// edge between node i and `other` with cost c: eligible when other is a node, not i, c <= max_cost (a NaN never is) and other is
// unmatched (i is, or the caller would not ask)
__device__ __forceinline__ void mg_consider(MgKey &best, int P, int i, int other, float c, float max_cost, const int *__restrict__ mate)
{
    if (other < 0 || other >= P || other == i) return;
    if (!(c <= max_cost)) return;
    if (mate[other] != -1) return;
    const MgKey k{ c, min(i, other), max(i, other) };
    if (mg_less(k, best)) best = k;
}

// entry m of an incoming list of node i: the edge in_edges[m] = s * K + k, checked against idx (a list not made by
// r2_graph_transpose on this idx: nothing outside the inputs is read, an entry that is no edge to i is skipped)
__device__ __forceinline__ void mg_incoming(MgKey &best, int P, int K, uint32_t n, int i, int e, const int *__restrict__ idx,
                                            const float *__restrict__ cost, float max_cost, const int *__restrict__ mate)
{
    if ((uint32_t)e >= n) return;
    if (idx[e] != i) return;
    mg_consider(best, P, i, (int)((uint32_t)e / (uint32_t)K), cost[e], max_cost, mate);
}

// The partner of node i's smallest-key eligible edge among its own row and its incoming list, or -1.  Called by every thread of
// the workgroup (active = false: no node, or a matched one): a node with more than MG_HUB incoming edges has its list walked by
// its wave, hub after hub in ascending lane, lane l taking entries l, l + 64, ...; the 64 minima fold by xor butterfly.  The key
// is a total order over pairs, so the minimum does not depend on the order the edges are visited in.
__device__ __forceinline__ int mg_best(int P, int K, uint32_t n, int i, bool active, const int *__restrict__ idx,
                                       const int *__restrict__ in_offsets, const int *__restrict__ in_edges,
                                       const float *__restrict__ cost, float max_cost, const int *__restrict__ mate)
{
    const int lane = threadIdx.x & 63;
    MgKey best = mg_none();
    int o0 = 0, o1 = 0;
    if (active) {
        for (int k = 0; k < K; ++k) {
            const size_t e = (size_t)i * K + k;
            mg_consider(best, P, i, idx[e], cost[e], max_cost, mate);
        }
        o0 = min(max(in_offsets[i], 0), (int)n);
        o1 = min(max(in_offsets[i + 1], o0), (int)n);
    }
    const bool hub = o1 - o0 > MG_HUB;
    if (!hub)
        for (int m = o0; m < o1; ++m) mg_incoming(best, P, K, n, i, in_edges[m], idx, cost, max_cost, mate);
    unsigned long long hubs = __ballot(hub);
    while (hubs) {
        const int l = __ffsll((long long)hubs) - 1;
        hubs &= hubs - 1;
        const int h0 = __shfl(o0, l), h1 = __shfl(o1, l), hi = __shfl(i, l);
        MgKey p = mg_none();
        for (int m = h0 + lane; m < h1; m += 64) mg_incoming(p, P, K, n, hi, in_edges[m], idx, cost, max_cost, mate);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const MgKey o{ __shfl_xor(p.c, d), __shfl_xor(p.lo, d), __shfl_xor(p.hi, d) };
            if (mg_less(o, p)) p = o;
        }
        if (lane == l && mg_less(p, best)) best = p;
    }
    if (best.lo == INT_MAX) return -1;
    return best.lo == i ? best.hi : best.lo;
}

__global__ void __launch_bounds__(MG_THREADS) match_point_kernel(int P, int K, uint32_t n, const int *__restrict__ idx,
                                                                 const int *__restrict__ in_offsets, const int *__restrict__ in_edges,
                                                                 const float *__restrict__ cost, float max_cost,
                                                                 const int *__restrict__ mate, int *__restrict__ ptr)
{
    const int i = blockIdx.x * MG_THREADS + threadIdx.x;
    const bool live = i < P;
    const bool active = live && mate[i] == -1;
    const int b = mg_best(P, K, n, i, active, idx, in_offsets, in_edges, cost, max_cost, mate);
    if (live) ptr[i] = b;
}

// i and j are matched when they point at each other; thread i writes mate[i] alone
__global__ void __launch_bounds__(MG_THREADS) match_pair_kernel(int P, const int *__restrict__ ptr, int *__restrict__ mate)
{
    const int i = blockIdx.x * MG_THREADS + threadIdx.x;
    if (i >= P) return;
    const int j = ptr[i];
    if (j >= 0 && ptr[j] == i) mate[i] = j;
}

// ---- r2_merge_count.  vmate: the validated mate; keep: 0 for the higher index of a pair
__global__ void __launch_bounds__(MG_THREADS) merge_validate_kernel(int P, const int *__restrict__ mate, const float *__restrict__ density,
                                                                    const float *__restrict__ scaling, int *__restrict__ vmate,
                                                                    uint32_t *__restrict__ keep)
{
    const int i = blockIdx.x * MG_THREADS + threadIdx.x;
    if (i >= P) return;
    const int j = mate[i];
    int v = -1;
    if (j >= 0 && j < P && j != i && mate[j] == i && mg_mass_ok(mg_mass(i, density, scaling)) && mg_mass_ok(mg_mass(j, density, scaling)))
        v = j;
    vmate[i] = v;
    keep[i] = (v >= 0 && v < i) ? 0u : 1u;
}

__global__ void __launch_bounds__(MG_THREADS) merge_open_kernel(int P, int K, uint32_t n, const int *__restrict__ idx,
                                                                const int *__restrict__ in_offsets, const int *__restrict__ in_edges,
                                                                const float *__restrict__ cost, float max_cost,
                                                                const int *__restrict__ vmate, uint32_t *__restrict__ open)
{
    const int i = blockIdx.x * MG_THREADS + threadIdx.x;
    const bool live = i < P;
    const bool active = live && vmate[i] == -1;
    const int b = mg_best(P, K, n, i, active, idx, in_offsets, in_edges, cost, max_cost, vmate);
    if (live) open[i] = b >= 0 ? 1u : 0u;
}

// ---- r2_merge_emit.  One cyclic Jacobi rotation of the symmetric A (full storage) in the (p, q) plane, r the third index;
// V's columns collect the eigenvectors.  Indices are template arguments: everything stays in registers.
template <int p, int q, int r>
__device__ __forceinline__ void mg_jacobi_rotate(double A[3][3], double V[3][3])
{
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));   // (theta^2 = inf: t = 0)
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[p][p] = A[p][p] - t * apq;
    A[q][q] = A[q][q] + t * apq;
    A[p][q] = A[q][p] = 0.0;
    const double arp = A[r][p], arq = A[r][q];
    A[r][p] = A[p][r] = c * arp - s * arq;
    A[r][q] = A[q][r] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
    }
}

template <int a, int b>
__device__ __forceinline__ void mg_order(double lam[3], double V[3][3])   // lam[a] >= lam[b] afterwards, the columns following
{
    if (lam[a] < lam[b]) {
        const double t = lam[a]; lam[a] = lam[b]; lam[b] = t;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double u = V[k][a]; V[k][a] = V[k][b]; V[k][b] = u; }
    }
}

__global__ void __launch_bounds__(MG_THREADS) merge_emit_kernel(int P, int Pn, const float *__restrict__ means,
                                                                const float *__restrict__ density, const float *__restrict__ scaling,
                                                                const float *__restrict__ rotation, const int *__restrict__ vmate,
                                                                const uint32_t *__restrict__ pos /* inclusive scan of keep */,
                                                                float *__restrict__ means_out, float *__restrict__ density_out,
                                                                float *__restrict__ scaling_out, float *__restrict__ rotation_out,
                                                                int *__restrict__ src)
{
    const int i = blockIdx.x * MG_THREADS + threadIdx.x;
    if (i >= P) return;
    const int j = vmate[i];
    if (j >= 0 && j < i) return;                       // the higher index of a pair: its row is the lower one's
    const size_t o = (size_t)pos[i] - 1u;
    if (pos[i] == 0u || o >= (size_t)Pn) return;       // (a scratch that is not r2_merge_count's on these inputs: nothing outside the outputs)
    src[2 * o] = i;
    src[2 * o + 1] = (j >= 0 && j < P) ? j : -1;
    if (j < 0 || j >= P) {                             // unmerged: the bits of the input row
#pragma unroll
        for (int k = 0; k < 3; ++k) means_out[3 * o + k] = means[3 * (size_t)i + k];
        density_out[o] = density[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) scaling_out[3 * o + k] = scaling[3 * (size_t)i + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) rotation_out[4 * o + k] = rotation[4 * (size_t)i + k];
        return;
    }
    const MgGauss a = mg_load(i, means, density, scaling, rotation);
    const MgGauss b = mg_load(j, means, density, scaling, rotation);
    double alpha, cov[6];
    mg_pair(a, b, alpha, cov);
#pragma unroll
    for (int k = 0; k < 3; ++k) means_out[3 * o + k] = (float)(alpha * a.mu[k] + (1.0 - alpha) * b.mu[k]);
    double A[3][3] = { { cov[0], cov[1], cov[2] }, { cov[1], cov[3], cov[4] }, { cov[2], cov[4], cov[5] } };
    double V[3][3] = { { 1.0, 0.0, 0.0 }, { 0.0, 1.0, 0.0 }, { 0.0, 0.0, 1.0 } };
    for (int sweep = 0; sweep < MG_SWEEPS; ++sweep) {
        mg_jacobi_rotate<0, 1, 2>(A, V);
        mg_jacobi_rotate<0, 2, 1>(A, V);
        mg_jacobi_rotate<1, 2, 0>(A, V);
    }
    double lam[3] = { A[0][0], A[1][1], A[2][2] };
    mg_order<0, 1>(lam, V);
    mg_order<1, 2>(lam, V);
    mg_order<0, 1>(lam, V);
    // rows of R = the eigenvectors (Sigma = R^T diag(s^2) R), right-handed by flipping the third
    double R[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[k][c] = V[c][k];
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    if (det < 0.0) { R[2][0] = -R[2][0]; R[2][1] = -R[2][1]; R[2][2] = -R[2][2]; }
    // the quaternion of R (the inverse of quat_rot), from the largest of 4 r^2, 4 x^2, 4 y^2, 4 z^2
    const double tr = R[0][0] + R[1][1] + R[2][2];
    const double fr = 1.0 + tr, fx = 1.0 + R[0][0] - R[1][1] - R[2][2], fy = 1.0 - R[0][0] + R[1][1] - R[2][2],
                 fz = 1.0 - R[0][0] - R[1][1] + R[2][2];
    double q[4];
    if (fr >= fx && fr >= fy && fr >= fz) {
        const double h = 0.5 * sqrt(fr), w = 0.25 / h;
        q[0] = h; q[1] = (R[2][1] - R[1][2]) * w; q[2] = (R[0][2] - R[2][0]) * w; q[3] = (R[1][0] - R[0][1]) * w;
    } else if (fx >= fy && fx >= fz) {
        const double h = 0.5 * sqrt(fx), w = 0.25 / h;
        q[1] = h; q[0] = (R[2][1] - R[1][2]) * w; q[2] = (R[0][1] + R[1][0]) * w; q[3] = (R[0][2] + R[2][0]) * w;
    } else if (fy >= fz) {
        const double h = 0.5 * sqrt(fy), w = 0.25 / h;
        q[2] = h; q[0] = (R[0][2] - R[2][0]) * w; q[1] = (R[0][1] + R[1][0]) * w; q[3] = (R[1][2] + R[2][1]) * w;
    } else {
        const double h = 0.5 * sqrt(fz), w = 0.25 / h;
        q[3] = h; q[0] = (R[1][0] - R[0][1]) * w; q[1] = (R[0][2] + R[2][0]) * w; q[2] = (R[1][2] + R[2][1]) * w;
    }
    const double qn = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    float qf[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) qf[k] = (float)(q[k] / qn);
    // r >= 0, and the first non-zero component positive when r = 0: decided on the rounded values (negation is exact)
    const float lead = qf[0] != 0.f ? qf[0] : (qf[1] != 0.f ? qf[1] : (qf[2] != 0.f ? qf[2] : qf[3]));
    const float sgn = lead < 0.f ? -1.f : 1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) rotation_out[4 * o + k] = qf[k] == 0.f ? 0.f : sgn * qf[k];
    const float sf[3] = { (float)sqrt(lam[0]), (float)sqrt(lam[1]), (float)sqrt(lam[2]) };
#pragma unroll
    for (int k = 0; k < 3; ++k) scaling_out[3 * o + k] = sf[k];
    // the density that restores the pair's mass with the scales as stored: one rounding between the mass and its float product
    density_out[o] = (float)((a.mass + b.mass) / (((double)sf[0] * (double)sf[1]) * (double)sf[2]));
}

inline size_t mg_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline bool mg_shape_ok(int P, int K) { return P >= 0 && K >= 1 && (size_t)P * (size_t)K <= 0x7fffffffu; }
inline unsigned mg_blocks(size_t n) { return (unsigned)((n + MG_THREADS - 1) / MG_THREADS); }

// r2_merge_count's scratch: vmate [P] | keep [P] | pos [P] | open [P] | open scan [P] | scan temp
struct MgScratch {
    int *vmate;
    uint32_t *keep, *pos, *open, *opos;
    char *scan_temp;
};
inline MgScratch mg_scratch(void *scratch, int P)
{
    char *b = static_cast<char *>(scratch);
    const size_t row = mg_align((size_t)P * sizeof(uint32_t));
    MgScratch s;
    s.vmate = reinterpret_cast<int *>(b);
    s.keep = reinterpret_cast<uint32_t *>(b + row);
    s.pos = reinterpret_cast<uint32_t *>(b + 2 * row);
    s.open = reinterpret_cast<uint32_t *>(b + 3 * row);
    s.opos = reinterpret_cast<uint32_t *>(b + 4 * row);
    s.scan_temp = b + 5 * row;
    return s;
}

}  // namespace
}  // namespace r2

extern "C" int r2_merge_cost(int P, int K, const int *idx, const float *means, const float *density, const float *scaling,
                             const float *rotation, float max_trace, float *cost, void *stream)
{
    using namespace r2;
    if (!mg_shape_ok(P, K) || (P > 0 && (!idx || !means || !density || !scaling || !rotation || !cost))) {
        set_error("r2_merge_cost: invalid argument");
        return R2_ERR_INVALID;
    }
    if (P == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)((size_t)P * (size_t)K);
    merge_cost_kernel<<<dim3(mg_blocks(n)), dim3(MG_THREADS), 0, s>>>(P, K, n, idx, means, density, scaling, rotation, max_trace, cost);
    R2_STAGE_CHECK(0, s, "merge cost");
    return 0;
}

extern "C" size_t r2_graph_match_workspace_bytes(int P)
{
    return P > 0 ? r2::mg_align((size_t)P * sizeof(int)) : 0;
}

extern "C" int r2_graph_match(int P, int K, const int *idx, const int *in_offsets, const int *in_edges, const float *cost,
                              float max_cost, int rounds, int *mate, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace r2;
    if (!mg_shape_ok(P, K) || rounds < 0 || (P > 0 && (!idx || !in_offsets || !in_edges || !cost || !mate))) {
        set_error("r2_graph_match: invalid argument");
        return R2_ERR_INVALID;
    }
    if (P == 0) return 0;
    if (!workspace || workspace_bytes < r2_graph_match_workspace_bytes(P)) {
        set_error("r2_graph_match: the workspace must hold %zu bytes", r2_graph_match_workspace_bytes(P));
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)((size_t)P * (size_t)K);
    int *ptr = static_cast<int *>(workspace);
    const dim3 grid(mg_blocks((size_t)P)), block(MG_THREADS);
    R2_HIP_TRY(hipMemsetAsync(mate, 0xFF, (size_t)P * sizeof(int), s));   // -1: nobody is matched
    for (int r = 0; r < rounds; ++r) {
        match_point_kernel<<<grid, block, 0, s>>>(P, K, n, idx, in_offsets, in_edges, cost, max_cost, mate, ptr);
        match_pair_kernel<<<grid, block, 0, s>>>(P, ptr, mate);
    }
    R2_STAGE_CHECK(0, s, "graph match");
    return 0;
}

extern "C" size_t r2_merge_scratch_bytes(int P)
{
    if (P <= 0) return 0;
    return 5 * r2::mg_align((size_t)P * sizeof(uint32_t)) + r2::mg_align(r2::scan_temp_bytes(P)) + 256;
}

extern "C" int r2_merge_count(int P, int K, const int *idx, const int *in_offsets, const int *in_edges, const float *cost,
                              float max_cost, const int *mate, const float *density, const float *scaling, void *scratch,
                              unsigned int *counts_host, void *stream)
{
    using namespace r2;
    if (!mg_shape_ok(P, K) || !counts_host ||
        (P > 0 && (!idx || !in_offsets || !in_edges || !cost || !mate || !density || !scaling || !scratch))) {
        set_error("r2_merge_count: invalid argument");
        return R2_ERR_INVALID;
    }
    counts_host[0] = counts_host[1] = 0u;
    if (P == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)((size_t)P * (size_t)K);
    const MgScratch w = mg_scratch(scratch, P);
    const dim3 grid(mg_blocks((size_t)P)), block(MG_THREADS);
    merge_validate_kernel<<<grid, block, 0, s>>>(P, mate, density, scaling, w.vmate, w.keep);
    merge_open_kernel<<<grid, block, 0, s>>>(P, K, n, idx, in_offsets, in_edges, cost, max_cost, w.vmate, w.open);
    int rc = inclusive_scan_u32(w.scan_temp, scan_temp_bytes(P), w.keep, w.pos, P, s);
    if (rc) return rc;
    rc = inclusive_scan_u32(w.scan_temp, scan_temp_bytes(P), w.open, w.opos, P, s);
    if (rc) return rc;
    uint32_t h[2];
    R2_HIP_TRY(hipMemcpyAsync(&h[0], w.pos + (P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    R2_HIP_TRY(hipMemcpyAsync(&h[1], w.opos + (P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    R2_HIP_TRY(hipStreamSynchronize(s));
    counts_host[0] = (uint32_t)P - h[0];
    counts_host[1] = h[1];
    return 0;
}

extern "C" int r2_merge_emit(int P, const float *means, const float *density, const float *scaling, const float *rotation,
                             const void *scratch, int Pn, float *means_out, float *density_out, float *scaling_out,
                             float *rotation_out, int *src, void *stream)
{
    using namespace r2;
    if (P < 0 || Pn < 0 || Pn > P ||
        (P > 0 && (!means || !density || !scaling || !rotation || !scratch)) ||
        (Pn > 0 && (!means_out || !density_out || !scaling_out || !rotation_out || !src))) {
        set_error("r2_merge_emit: invalid argument");
        return R2_ERR_INVALID;
    }
    if (P == 0 || Pn == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const MgScratch w = mg_scratch(const_cast<void *>(scratch), P);
    merge_emit_kernel<<<dim3(mg_blocks((size_t)P)), dim3(MG_THREADS), 0, s>>>(P, Pn, means, density, scaling, rotation, w.vmate, w.pos,
                                                                            means_out, density_out, scaling_out, rotation_out, src);
    R2_STAGE_CHECK(0, s, "merge emit");
    return 0;
}
