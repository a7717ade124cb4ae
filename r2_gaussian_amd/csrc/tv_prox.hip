// tv_prox.hip -- the proximal operator of the isotropic, unsmoothed total variation with a box constraint (ROF denoising),
//     x = argmin 1/2 |x - y|^2 + lambda TV(x),  lo <= x <= hi,
// by Beck and Teboulle's fast gradient projection on the dual (recon.py: tv_prox, tv_denoise, fista_tv).  The iteration, the
// discretisation and the per-voxel operation order are stated in include/r2hip.h (r2_tv_prox); tests/tv_prox_ref.py restates
// them in float32 operation for operation, which is why this file is compiled without FMA contraction.
//
// One iteration is ONE launch (tv_prox_brick): a workgroup owns a brick of BRICK_X x BRICK_Y x BRICK_Z voxels, forms the
// primal iterate x_k = P_C(y - lambda D^T r_k) on the brick and on its one-voxel upper faces in LDS (x_k never goes to
// memory), and then updates the dual of its own voxels from the forward differences of that LDS image.  A voxel's x_k reads
// r_k at the voxel and at its three lower neighbours, which may belong to another workgroup: r is therefore kept twice and
// the launches alternate between the copies; p is read and written at the own voxel only and is updated in place.  A face
// voxel's x_k is computed by two workgroups with the same operations on the same operands, so nothing depends on the brick
// or on the launch order.  The last launch (tv_prox_primal) writes x = P_C(y - lambda D^T p_n); it reads y at its own voxel
// only, so x may be y.
//
// -DR2_TV_PROX_TWO_LAUNCH (experiment builds: build.py --out=) replaces the brick kernel by two flat launches per iteration,
// x_k written to memory by the first and read back with its upper neighbours by the second; the per-voxel arithmetic is the
// same functions, so the bits are the same.  DESIGN.md section 4 has both timings.
#include "r2_common.hpp"
#include <math.h>

namespace r2 {

namespace {

constexpr int TB = 256;                                   // threads per workgroup
constexpr int BRICK_X = 8, BRICK_Y = 8, BRICK_Z = 64;     // voxels a workgroup owns; z is the contiguous axis
constexpr int HX = BRICK_X + 1, HY = BRICK_Y + 1, HZ = BRICK_Z + 1;   // ... plus the upper faces: the LDS image of x_k
constexpr int PER = 4;                                    // flat kernels: voxels per thread
constexpr int CHUNK = TB * PER;

struct Grid {
    int nx, ny, nz;
    size_t sx, sy, N;   // strides of x and y (z is contiguous) and the voxel count: the stride of a dual component
};

// tau = 1 / (12 lambda), and whether lambda asks for any iteration at all (r2hip.h: otherwise x = P_C(y))
__device__ __forceinline__ bool lambda_active(float lam, float &tau)
{
    tau = 1.0f / (12.0f * lam);
    return lam > 0.0f && tau > 0.0f && tau < INFINITY;
}

__device__ __forceinline__ float clamp_to(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// P_C(y - lambda (D^T d)(v)) for the dual field d (three planes of N floats); ZERO: d = 0.  The seven loads are
// unconditional (a lower neighbour that does not exist is read at the voxel itself and discarded), so that the compiler can
// issue them together and an unrolled caller keeps several voxels' loads in flight.
template <bool ZERO>
__device__ __forceinline__ float primal_at(const Grid &g, const float *__restrict__ y, const float *__restrict__ d, float lam,
                                           float lo, float hi, int i, int j, int k, size_t o)
{
    float v = y[o];
    if (!ZERO) {
        const float *dx = d, *dy = d + g.N, *dz = d + 2 * g.N;
        const float ux = dx[i > 0 ? o - g.sx : o], uy = dy[j > 0 ? o - g.sy : o], uz = dz[k > 0 ? o - 1 : o];
        const float wx = dx[o], wy = dy[o], wz = dz[o];
        const float tx = (i > 0 ? ux : 0.0f) - (i + 1 < g.nx ? wx : 0.0f);
        const float ty = (j > 0 ? uy : 0.0f) - (j + 1 < g.ny ? wy : 0.0f);
        const float tz = (k > 0 ? uz : 0.0f) - (k + 1 < g.nz ? wz : 0.0f);
        const float div = (tx + ty) + tz;
        v = v - lam * div;
    }
    return clamp_to(v, lo, hi);
}

// The dual step at voxel o from the forward differences of x_k there.  ZERO: r_k = p_{k-1} = 0 (the first iteration: nothing
// is read from the scratch).  store: false for a thread whose voxel lies outside the volume (o is then some voxel inside,
// so that the loads stay unconditional; nothing is written).
template <bool ZERO>
__device__ __forceinline__ void dual_at(const Grid &g, size_t o, float dx, float dy, float dz, float tau, float mom,
                                        const float *r_in, float *r_out /* may be r_in */, float *__restrict__ p,
                                        bool write_r, bool store)
{
    const float rx = ZERO ? 0.0f : r_in[o], ry = ZERO ? 0.0f : r_in[o + g.N], rz = ZERO ? 0.0f : r_in[o + 2 * g.N];
    const float ox = ZERO ? 0.0f : p[o], oy = ZERO ? 0.0f : p[o + g.N], oz = ZERO ? 0.0f : p[o + 2 * g.N];
    const float qx = rx + tau * dx, qy = ry + tau * dy, qz = rz + tau * dz;
    const float n2 = (qx * qx + qy * qy) + qz * qz;
    const float n = sqrtf(n2);
    const float m = n > 1.0f ? n : 1.0f;
    const float px = qx / m, py = qy / m, pz = qz / m;
    if (!store) return;
    if (write_r) {
        r_out[o] = px + mom * (px - ox);
        r_out[o + g.N] = py + mom * (py - oy);
        r_out[o + 2 * g.N] = pz + mom * (pz - oz);
    }
    p[o] = px;
    p[o + g.N] = py;
    p[o + 2 * g.N] = pz;
}

// One iteration in one launch.  bny, bnz: bricks along y and z (blockIdx.x = (bx * bny + by) * bnz + bz).  A point of the LDS
// image that lies outside the volume is computed at the nearest voxel inside (min(i, nx - 1) ...): no owned voxel reads it,
// and the loops carry no data-dependent branch.
template <bool ZERO>
__global__ void __launch_bounds__(TB) tv_prox_brick(Grid g, int bny, int bnz, const float *__restrict__ y,
                                                    const float *__restrict__ lam_p, float lo, float hi, float mom,
                                                    const float *__restrict__ r_in, float *__restrict__ r_out,
                                                    float *__restrict__ p, int write_r)
{
    __shared__ float xs[HX * HY * HZ];
    float tau;
    const float lam = *lam_p;
    if (!lambda_active(lam, tau)) return;   // kernel-uniform
    const int bz = (int)(blockIdx.x % (unsigned)bnz), by = (int)((blockIdx.x / (unsigned)bnz) % (unsigned)bny);
    const int bx = (int)(blockIdx.x / ((unsigned)bnz * (unsigned)bny));
    const int i0 = bx * BRICK_X, j0 = by * BRICK_Y, k0 = bz * BRICK_Z;
    auto primal_to_lds = [&](int lx, int ly, int lz) {
        const int i = min(i0 + lx, g.nx - 1), j = min(j0 + ly, g.ny - 1), k = min(k0 + lz, g.nz - 1);
        const size_t o = (size_t)i * g.sx + (size_t)j * g.sy + (size_t)k;
        xs[(lx * HY + ly) * HZ + lz] = primal_at<ZERO>(g, y, r_in, lam, lo, hi, i, j, k, o);
    };
    // the brick itself: a wave takes a row of BRICK_Z voxels
    static_assert(BRICK_Z == 64 && BRICK_Y == 8 && (BRICK_X * BRICK_Y * BRICK_Z) % TB == 0, "the index arithmetic below");
#pragma unroll 4
    for (int it = 0; it < BRICK_X * BRICK_Y * BRICK_Z / TB; ++it) {
        const int e = it * TB + (int)threadIdx.x;
        primal_to_lds(e >> 9, (e >> 6) & 7, e & 63);
    }
    // its three upper faces (their edges and corners are the neighbours of no owned voxel)
    constexpr int FACE_X = BRICK_Y * BRICK_Z, FACE_Y = BRICK_X * BRICK_Z, FACE_Z = BRICK_X * BRICK_Y;
#pragma unroll
    for (int it = 0; it < (FACE_X + FACE_Y + FACE_Z + TB - 1) / TB; ++it) {
        const int f = it * TB + (int)threadIdx.x;
        if (f >= FACE_X + FACE_Y + FACE_Z) break;
        if (f < FACE_X) primal_to_lds(BRICK_X, f >> 6, f & 63);
        else if (f < FACE_X + FACE_Y) primal_to_lds((f - FACE_X) >> 6, BRICK_Y, f & 63);
        else primal_to_lds((f - FACE_X - FACE_Y) >> 3, (f - FACE_X - FACE_Y) & 7, BRICK_Z);
    }
    __syncthreads();
#pragma unroll 4
    for (int it = 0; it < BRICK_X * BRICK_Y * BRICK_Z / TB; ++it) {
        const int e = it * TB + (int)threadIdx.x;
        const int lz = e & 63, ly = (e >> 6) & 7, lx = e >> 9;
        const int i = i0 + lx, j = j0 + ly, k = k0 + lz;
        const bool in = i < g.nx && j < g.ny && k < g.nz;
        const size_t o = (size_t)min(i, g.nx - 1) * g.sx + (size_t)min(j, g.ny - 1) * g.sy + (size_t)min(k, g.nz - 1);
        const int s = (lx * HY + ly) * HZ + lz;
        const float xc = xs[s];
        const float dx = i + 1 < g.nx ? xs[s + HY * HZ] - xc : 0.0f;
        const float dy = j + 1 < g.ny ? xs[s + HZ] - xc : 0.0f;
        const float dz = k + 1 < g.nz ? xs[s + 1] - xc : 0.0f;
        dual_at<ZERO>(g, o, dx, dy, dz, tau, mom, r_in, r_out, p, write_r != 0, in);
    }
}

__device__ __forceinline__ void unflatten(const Grid &g, size_t o, int &i, int &j, int &k)
{
    k = (int)(o % (size_t)g.nz);
    j = (int)((o / (size_t)g.nz) % (size_t)g.ny);
    i = (int)(o / g.sx);
}

// x = P_C(y - lambda D^T d) over the whole volume.  final: the output pass, which also serves a lambda that asks for no
// iteration (x = P_C(y)); otherwise the first launch of the two-launch iteration, skipped for such a lambda.
template <bool ZERO>
__global__ void __launch_bounds__(TB) tv_prox_primal(Grid g, const float *y, const float *__restrict__ lam_p, float lo, float hi,
                                                     const float *__restrict__ d, float *x, int final)
{
    float tau;
    const float lam = *lam_p;
    const bool active = lambda_active(lam, tau);
    if (!active && !final) return;
    for (int q = 0; q < PER; ++q) {
        const size_t o = (size_t)blockIdx.x * CHUNK + (size_t)q * TB + threadIdx.x;
        if (o >= g.N) break;
        int i, j, k;
        unflatten(g, o, i, j, k);
        x[o] = (ZERO || !active) ? clamp_to(y[o], lo, hi) : primal_at<false>(g, y, d, lam, lo, hi, i, j, k, o);
    }
}

#ifdef R2_TV_PROX_TWO_LAUNCH
// the second launch of the two-launch iteration: the dual step from x_k in memory; r and p at the own voxel, in place
template <bool ZERO>
__global__ void __launch_bounds__(TB) tv_prox_dual(Grid g, const float *__restrict__ x, const float *__restrict__ lam_p,
                                                   float mom, float *r, float *__restrict__ p, int write_r)
{
    float tau;
    if (!lambda_active(*lam_p, tau)) return;
    for (int q = 0; q < PER; ++q) {
        const size_t o = (size_t)blockIdx.x * CHUNK + (size_t)q * TB + threadIdx.x;
        if (o >= g.N) break;
        int i, j, k;
        unflatten(g, o, i, j, k);
        const float xc = x[o];
        const float dx = i + 1 < g.nx ? x[o + g.sx] - xc : 0.0f;
        const float dy = j + 1 < g.ny ? x[o + g.sy] - xc : 0.0f;
        const float dz = k + 1 < g.nz ? x[o + 1] - xc : 0.0f;
        dual_at<ZERO>(g, o, dx, dy, dz, tau, mom, r, r, p, write_r != 0, true);
    }
}
#endif

}  // namespace

}  // namespace r2

extern "C" size_t r2_tv_prox_scratch_bytes(int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
    return (size_t)9 * ((size_t)nx * ny * nz) * sizeof(float);   // r twice and p, three components each
}

extern "C" int r2_tv_prox(int nx, int ny, int nz, const float *y, float *x, const float *lambda, int n_iter, float lo, float hi,
                          void *scratch, size_t scratch_bytes, void *stream)
{
    using namespace r2;
    if (nx <= 0 || ny <= 0 || nz <= 0 || !y || !x || !lambda || n_iter < 0 || !scratch) {
        set_error("r2_tv_prox: invalid argument");
        return R2_ERR_INVALID;
    }
    if (!(lo <= hi)) {
        set_error("r2_tv_prox: the bounds must satisfy lo <= hi, got %g and %g", (double)lo, (double)hi);
        return R2_ERR_INVALID;
    }
    const size_t N = (size_t)nx * ny * nz, nb = (N + CHUNK - 1) / CHUNK;
    const size_t bnx = (nx + BRICK_X - 1) / BRICK_X, bny = (ny + BRICK_Y - 1) / BRICK_Y, bnz = (nz + BRICK_Z - 1) / BRICK_Z;
    const size_t bricks = bnx * bny * bnz;
    if (scratch_bytes < r2_tv_prox_scratch_bytes(nx, ny, nz) || nb > 0x7fffffffULL || bricks > 0x7fffffffULL) {
        set_error("r2_tv_prox: scratch of %zu bytes, %zu needed (or volume too large)", scratch_bytes,
                  r2_tv_prox_scratch_bytes(nx, ny, nz));
        return R2_ERR_INVALID;
    }
    float *rbuf[2] = {(float *)scratch, (float *)scratch + 3 * N};
    float *p = (float *)scratch + 6 * N;
    const Grid g{nx, ny, nz, (size_t)ny * nz, (size_t)nz, N};
    hipStream_t s = (hipStream_t)stream;
    double t = 1.0;
    for (int k = 1; k <= n_iter; ++k) {
        // the momentum of r_{k+1}: data-independent, in double on the host
        const double t_next = 0.5 * (1.0 + sqrt(1.0 + 4.0 * t * t));
        const float mom = (float)((t - 1.0) / t_next);
        t = t_next;
        const int write_r = k < n_iter;   // nobody reads r_{n+1}
#ifdef R2_TV_PROX_TWO_LAUNCH
        float *xk = rbuf[1], *r = rbuf[0];
        if (k == 1) {
            tv_prox_primal<true><<<dim3((unsigned)nb), dim3(TB), 0, s>>>(g, y, lambda, lo, hi, r, xk, 0);
            tv_prox_dual<true><<<dim3((unsigned)nb), dim3(TB), 0, s>>>(g, xk, lambda, mom, r, p, write_r);
        } else {
            tv_prox_primal<false><<<dim3((unsigned)nb), dim3(TB), 0, s>>>(g, y, lambda, lo, hi, r, xk, 0);
            tv_prox_dual<false><<<dim3((unsigned)nb), dim3(TB), 0, s>>>(g, xk, lambda, mom, r, p, write_r);
        }
#else
        const float *r_in = rbuf[(k - 1) & 1];
        float *r_out = rbuf[k & 1];
        if (k == 1)
            tv_prox_brick<true><<<dim3((unsigned)bricks), dim3(TB), 0, s>>>(g, (int)bny, (int)bnz, y, lambda, lo, hi, mom, r_in,
                                                                            r_out, p, write_r);
        else
            tv_prox_brick<false><<<dim3((unsigned)bricks), dim3(TB), 0, s>>>(g, (int)bny, (int)bnz, y, lambda, lo, hi, mom,
                                                                             r_in, r_out, p, write_r);
#endif
    }
    if (n_iter == 0)
        tv_prox_primal<true><<<dim3((unsigned)nb), dim3(TB), 0, s>>>(g, y, lambda, lo, hi, p, x, 1);
    else
        tv_prox_primal<false><<<dim3((unsigned)nb), dim3(TB), 0, s>>>(g, y, lambda, lo, hi, p, x, 1);
    R2_STAGE_CHECK(0, s, "tv prox");
    return 0;
}
