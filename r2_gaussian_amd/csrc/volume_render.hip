// volume_render.hip -- direct volume rendering of a voxel volume: the counterpart of pyvista's plotter.add_volume as the
// reference's scripts/plot_volume.py and data_generator/check_volume.py call it to look at a result, for machines without a
// monitor.  r2_volume_bricks, r2_render_volume, r2_render_volume_mip (include/r2hip.h states the contract).
//
// The walk is the forward projector's (projector.hip): one thread per detector pixel, a wave per 8 x 8 pixel tile, the view
// in blockIdx.z; the ray, its clip, the sample count, the sample positions and the trilinear value come from the headers
// the projector is written on (ray_sampling.hpp, trilinear.hpp, volume_entry.hpp), so a renderer sample IS a projector
// sample.  In place of the projector's sum a sample is classified by a transfer function (a table of K rows (r, g, b,
// extinction), kept in LDS, linear between its rows) and composited front to back, or the maximum is kept (MIP).
//
// Two things end a ray's work early:
// * early termination: the compositing loop stops after the first sample that leaves the transmittance below t_stop;
// * empty-space skipping: a table of the min and max of every 8^3 brick of cells (r2_volume_bricks) tells whether any value
//   the interpolant can take inside a brick reaches a table row with extinction > 0 (compositing) or exceeds the running
//   maximum (MIP).  If not, the samples of that brick contribute exactly nothing (expf(-0) = 1, T * 1 = T, T * 0 * c = 0) and
//   are passed over.  The output is the same bits with and without the table.
//
// How a ray passes an empty brick: it estimates the parameter at which it leaves the brick, turns that into a sample index
// ke, and evaluates sample ke's position with the walk's own arithmetic.  sample_t and the three fmaf of a position are
// monotone in k, and so are floor, the clamp and the shift that make a brick index of a position; hence if samples k and ke
// lie in the same brick, so does every sample between them, and k jumps to ke + 1.  If they do not, only sample k is passed
// over.  The estimate therefore needs no margin and can never skip a sample of another brick.
//
// This TU is compiled with -ffp-contract=off (build.py: EXACT): the per-sample operations are the separately rounded ones
// the header states and tests/volume_render_ref.py restates; only the explicit fmaf calls of the shared headers are fused.
#include "trilinear.hpp"
#include "volume_entry.hpp"
#include <math.h>

namespace r2 {

namespace {

constexpr int BRICK = R2_RENDER_BRICK;
constexpr int BRICK_SHIFT = 3;
static_assert((1 << BRICK_SHIFT) == BRICK, "a brick index is a shift of the clamped floor index");
constexpr int MAX_K = 1024;
constexpr float PAD = 4.76837158203125e-07f;   // 8 u = 2^-21: the interpolant's rounding, relative to the brick's largest |value|

inline int brick_count(int n) { return (n + BRICK - 1) / BRICK; }

// ---- the brick table -------------------------------------------------------------------------------------------------------
// One wave per brick: the lanes share the (x, y) rows of its up to 9 x 9 x 9 voxels and fold min and max through the wave;
// min and max do not depend on the order, so the table is bit-reproducible without atomics.
__global__ void __launch_bounds__(64) bricks_kernel(int nx, int ny, int nz, int nby, int nbz, const float *__restrict__ vol,
                                                    float2 *__restrict__ bricks)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int bk = b % nbz, bj = (b / nbz) % nby, bi = b / (nbz * nby);
    const int x0 = bi * BRICK, y0 = bj * BRICK, z0 = bk * BRICK;
    const int x1 = min(x0 + BRICK, nx - 1), y1 = min(y0 + BRICK, ny - 1), z1 = min(z0 + BRICK, nz - 1);
    const int ey = y1 - y0 + 1, rows = (x1 - x0 + 1) * ey;
    float mn = INFINITY, mx = -INFINITY;
    for (int row = lane; row < rows; row += 64) {
        const float *p = vol + ((size_t)(x0 + row / ey) * ny + (size_t)(y0 + row % ey)) * nz;
        for (int z = z0; z <= z1; ++z) {
            const float v = p[z];
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    // a cell on a face of the volume mixes in the zero outside
    if (bi == 0 || x0 + BRICK > nx - 1 || bj == 0 || y0 + BRICK > ny - 1 || bk == 0 || z0 + BRICK > nz - 1) {
        mn = fminf(mn, 0.0f);
        mx = fmaxf(mx, 0.0f);
    }
    // + 0: a zero is stored as +0 whichever of -0 and +0 the min or max picked
    if (lane == 0) bricks[b] = make_float2(mn + 0.0f, mx + 0.0f);
}

// ---- the walk both renderers share -------------------------------------------------------------------------------------------
struct Walk {
    float sx, sy, sz, dx, dy, dz;
    float rdx, rdy, rdz, rdt;     // reciprocals for the exit estimate only
    float t0, dt;
    int ns, nx, ny, nz, nby, nbz;
};

__device__ __forceinline__ int brick_index(const Walk &w, const Axis &X, const Axis &Y, const Axis &Z)
{
    // Axis::i0 is the floor index clamped into the volume
    return ((X.i0 >> BRICK_SHIFT) * w.nby + (Y.i0 >> BRICK_SHIFT)) * w.nbz + (Z.i0 >> BRICK_SHIFT);
}

// The parameter at which the line s + t d leaves the cells of brick b = i0 >> 3 on one axis, estimated; the first and the
// last brick of an axis reach to the ends of the support.
__device__ __forceinline__ float axis_exit(float s, float d, float rd, int i0, int n)
{
    if (d == 0.0f) return INFINITY;
    const int b = i0 >> BRICK_SHIFT;
    const float face = d > 0.0f ? ((b + 1) * BRICK > n - 1 ? INFINITY : (float)((b + 1) * BRICK))
                                : (b == 0 ? -INFINITY : (float)(b * BRICK));
    return (face - s) * rd;
}

// The last sample ke >= k for which samples k .. ke are known to share sample k's brick `bi` (see the head of the file).
__device__ __forceinline__ int brick_run_end(const Walk &w, int k, int bi, const Axis &X, const Axis &Y, const Axis &Z)
{
    const float te = fminf(fminf(axis_exit(w.sx, w.dx, w.rdx, X.i0, w.nx), axis_exit(w.sy, w.dy, w.rdy, Y.i0, w.ny)),
                           axis_exit(w.sz, w.dz, w.rdz, Z.i0, w.nz));
    // t_k = t0 + (k + 1/2) dt: the last sample before te, clamped in float before the conversion (a NaN lands on k)
    const float kf = floorf((te - w.t0) * w.rdt - 0.5f);
    const int ke = min((int)fminf(fmaxf(kf, (float)k), 1073741824.0f), w.ns - 1);
    if (ke <= k) return k;
    const float t = sample_t(ke, w.dt, w.t0);
    const Axis Xe = axis_of(fmaf(t, w.dx, w.sx), w.nx), Ye = axis_of(fmaf(t, w.dy, w.sy), w.ny),
               Ze = axis_of(fmaf(t, w.dz, w.sz), w.nz);
    return brick_index(w, Xe, Ye, Ze) == bi ? ke : k;
}

// The range of values the float32 interpolant can take in a brick whose voxels span [mm.x, mm.y]: widened by 8 u M and,
// where M > 0, rounded outwards by one more float32 (nextafterf(h, h) is h: a brick of exact zeros keeps [0, 0]).
__device__ __forceinline__ float2 brick_range(float2 mm)
{
    const float pad = fmaxf(fabsf(mm.x), fabsf(mm.y)) * PAD;
    const float l = mm.x - pad, h = mm.y + pad;
    return make_float2(nextafterf(l, l - pad), nextafterf(h, h + pad));
}

// Position of a value in the table: x = clamp((f - lo) * scale, 0, K - 1), a NaN landing on 0, and its cell i <= K - 2.
__device__ __forceinline__ int lut_cell(float f, float lo, float scale, int K, float &x)
{
    x = fminf(fmaxf((f - lo) * scale, 0.0f), (float)(K - 1));
    return min((int)floorf(x), K - 2);
}

// The ray of pixel (r, c) of the block's view: false when it misses the volume.  dl: the world length of one sample.
__device__ __forceinline__ bool walk_begin(Walk &w, const float *rays, int cone, int nx, int ny, int nz, float3 dv, float accuracy,
                                           int r, int c, float &dl)
{
    const Ray y = pixel_ray(rays + 12 * blockIdx.z, cone, r, c);
    float t0, t1;
    if (!clip_ray(y, cone, nx, ny, nz, t0, t1)) return false;
    const Sampling m = ray_sampling(y, t0, t1, dv, accuracy);
    w.sx = y.sx; w.sy = y.sy; w.sz = y.sz; w.dx = y.dx; w.dy = y.dy; w.dz = y.dz;
    w.rdx = 1.0f / y.dx; w.rdy = 1.0f / y.dy; w.rdz = 1.0f / y.dz; w.rdt = 1.0f / m.dt;
    w.t0 = t0; w.dt = m.dt; w.ns = m.n;
    w.nx = nx; w.ny = ny; w.nz = nz;
    w.nby = (ny + BRICK - 1) / BRICK; w.nbz = (nz + BRICK - 1) / BRICK;
    dl = m.dt * m.wlen;
    return true;
}

// ---- compositing ---------------------------------------------------------------------------------------------------------------
// Dynamic LDS: the table, K float4, then nzp[K + 1] 16-bit counts, nzp[j] = the number of rows below j with extinction != 0.
// A brick whose values reach the table positions xa <= xb, in the cells ia <= ib, reads the rows ia .. last, last = ib + 1 if
// xb > ib (a weight on the upper row) and ib otherwise; it is empty iff nzp[last + 1] == nzp[ia].
// waves_per_eu(8): 64 registers, so that eight waves per SIMD stay resident (the loop fits them without scratch)
template <typename OFF>
__global__ void __launch_bounds__(PB) __attribute__((amdgpu_waves_per_eu(8, 8))) render_kernel(int H, int W, const float *__restrict__ rays, int cone, int nx, int ny, int nz,
                                                    float3 dv, float accuracy, const float *__restrict__ vol,
                                                    const float2 *__restrict__ bricks, int K, const float4 *__restrict__ lut,
                                                    float lo, float scale, float t_stop, float4 *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4 *s_lut = reinterpret_cast<float4 *>(smem);
    unsigned short *nzp = reinterpret_cast<unsigned short *>(smem + (size_t)K * sizeof(float4));
    const int tid = threadIdx.x;
    for (int j = tid; j < K; j += PB) {
        const float4 e = lut[j];
        s_lut[j] = e;
        nzp[j + 1] = e.w != 0.0f;
    }
    if (tid == 0) nzp[0] = 0;
    __syncthreads();
    if (bricks) {   // inclusive scan of the flags in place, MAX_K / PB = 4 entries per thread (wave-uniform branch)
        for (int off = 1; off < K; off <<= 1) {
            unsigned short v[MAX_K / PB];
#pragma unroll
            for (int m = 0; m < MAX_K / PB; ++m) {
                const int j = tid + m * PB + 1;
                v[m] = j <= K ? (unsigned short)(nzp[j] + (j - off >= 1 ? nzp[j - off] : 0)) : (unsigned short)0;
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < MAX_K / PB; ++m) {
                const int j = tid + m * PB + 1;
                if (j <= K) nzp[j] = v[m];
            }
            __syncthreads();
        }
    }
    int r, c;
    if (!thread_pixel(H, W, r, c)) return;
    float4 *o = out + ((size_t)blockIdx.z * H + r) * W + c;
    Walk w;
    float dl;
    if (!walk_begin(w, rays, cone, nx, ny, nz, dv, accuracy, r, c, dl)) {
        *o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const OFF sxy = (OFF)ny * (OFF)nz;
    float Cr = 0.0f, Cg = 0.0f, Cb = 0.0f, T = 1.0f;
    int seen = -1;   // the brick last found not empty: not tested again while the ray stays in it
    for (int k = 0; k < w.ns; ++k) {
        const float t = sample_t(k, w.dt, w.t0);
        const Axis X = axis_of(fmaf(t, w.dx, w.sx), nx), Y = axis_of(fmaf(t, w.dy, w.sy), ny), Z = axis_of(fmaf(t, w.dz, w.sz), nz);
        if (bricks) {
            const int bi = brick_index(w, X, Y, Z);
            if (bi != seen) {
                const float2 range = brick_range(bricks[bi]);
                float xa, xb;
                const int ia = lut_cell(range.x, lo, scale, K, xa), ib = lut_cell(range.y, lo, scale, K, xb);
                const int last = xb > (float)ib ? ib + 1 : ib;
                if (nzp[last + 1] == nzp[ia]) {
                    k = brick_run_end(w, k, bi, X, Y, Z);
                    continue;
                }
                seen = bi;
            }
        }
        const float f = trilinear<OFF>(vol, X, Y, Z, sxy, nz);
        float x;
        const int i = lut_cell(f, lo, scale, K, x);
        const float wt = x - (float)i;
        const float4 a = s_lut[i], b = s_lut[i + 1];
        const float cr = a.x + wt * (b.x - a.x), cg = a.y + wt * (b.y - a.y), cb = a.z + wt * (b.z - a.z);
        const float ext = a.w + wt * (b.w - a.w);
        const float e = expf(-(ext * dl));
        const float wgt = T * (1.0f - e);
        Cr = Cr + wgt * cr;
        Cg = Cg + wgt * cg;
        Cb = Cb + wgt * cb;
        T = T * e;
        if (T < t_stop) break;
    }
    *o = make_float4(Cr, Cg, Cb, 1.0f - T);
}

// ---- maximum intensity ---------------------------------------------------------------------------------------------------------
template <typename OFF>
__global__ void __launch_bounds__(PB) mip_kernel(int H, int W, const float *__restrict__ rays, int cone, int nx, int ny, int nz,
                                                 float3 dv, float accuracy, const float *__restrict__ vol,
                                                 const float2 *__restrict__ bricks, float *__restrict__ out)
{
    int r, c;
    if (!thread_pixel(H, W, r, c)) return;
    float *o = out + ((size_t)blockIdx.z * H + r) * W + c;
    Walk w;
    float dl;
    if (!walk_begin(w, rays, cone, nx, ny, nz, dv, accuracy, r, c, dl)) {
        *o = 0.0f;
        return;
    }
    const OFF sxy = (OFF)ny * (OFF)nz;
    float best = -INFINITY, seen_hi = INFINITY;
    int seen = -1;   // the brick whose upper end seen_hi is
    for (int k = 0; k < w.ns; ++k) {
        const float t = sample_t(k, w.dt, w.t0);
        const Axis X = axis_of(fmaf(t, w.dx, w.sx), nx), Y = axis_of(fmaf(t, w.dy, w.sy), ny), Z = axis_of(fmaf(t, w.dz, w.sz), nz);
        if (bricks) {
            const int bi = brick_index(w, X, Y, Z);
            if (bi != seen) {
                seen = bi;
                seen_hi = brick_range(bricks[bi]).y;
            }
            if (seen_hi <= best) {   // nothing in the brick can raise the maximum
                k = brick_run_end(w, k, bi, X, Y, Z);
                continue;
            }
        }
        best = fmaxf(best, trilinear<OFF>(vol, X, Y, Z, sxy, nz));
    }
    *o = best;
}

inline bool bricks_fit(int nx, int ny, int nz)
{
    return (long long)brick_count(nx) * brick_count(ny) * brick_count(nz) <= 2147483647LL;
}

inline bool aligned_to(const void *p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

}  // namespace

}  // namespace r2

extern "C" int r2_volume_bricks(int nx, int ny, int nz, const float *vol, float *bricks, void *stream)
{
    using namespace r2;
    if (nx <= 0 || ny <= 0 || nz <= 0 || !vol || !bricks || !aligned_to(bricks, 8)) {
        set_error("r2_volume_bricks: invalid argument");
        return R2_ERR_INVALID;
    }
    if (!bricks_fit(nx, ny, nz)) {
        set_error("r2_volume_bricks: more than 2^31 - 1 bricks");
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const int nbx = brick_count(nx), nby = brick_count(ny), nbz = brick_count(nz);
    bricks_kernel<<<dim3(nbx * nby * nbz), dim3(64), 0, s>>>(nx, ny, nz, nby, nbz, vol, reinterpret_cast<float2 *>(bricks));
    R2_STAGE_CHECK(0, s, "volume bricks");
    return 0;
}

extern "C" int r2_render_volume(int V, int H, int W, const float *rays, int cone, int nx, int ny, int nz, float dVoxel_x,
                                float dVoxel_y, float dVoxel_z, float accuracy, const float *vol, const float *bricks, int K,
                                const float *lut, float lo, float hi, float t_stop, float *out, void *stream)
{
    using namespace r2;
    if (const int rc = check_forward_args("r2_render_volume", V, H, W, rays, nx, ny, nz, dVoxel_x, dVoxel_y, dVoxel_z, &accuracy,
                                          vol, out))
        return rc;
    if (K < 2 || K > MAX_K || !lut || !(hi > lo) || !(fabsf(lo) < INFINITY) || !(fabsf(hi) < INFINITY) || !(t_stop >= 0.0f) ||
        !(t_stop < 1.0f) || (bricks && !bricks_fit(nx, ny, nz)) || !aligned_to(lut, 16) || !aligned_to(out, 16) ||
        !aligned_to(bricks, 8)) {
        set_error("r2_render_volume: invalid argument (K %d in [2, %d], finite lo %g < hi %g, t_stop %g in [0, 1), lut and out "
                  "16-byte aligned, bricks 8-byte)", K, MAX_K, (double)lo, (double)hi, (double)t_stop);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid = volume_pixel_grid(V, H, W);
    const float3 d = make_float3(dVoxel_x, dVoxel_y, dVoxel_z);
    const float scale = (float)(K - 1) / (hi - lo);
    // the table and the K + 1 counts, the counts' start 16-byte aligned by the float4 rows before them
    const size_t lds = (size_t)K * sizeof(float4) + (((size_t)K + 1) * sizeof(unsigned short) + 15) / 16 * 16;
    const float2 *bt = reinterpret_cast<const float2 *>(bricks);
    const float4 *lt = reinterpret_cast<const float4 *>(lut);
    float4 *o = reinterpret_cast<float4 *>(out);
    if ((unsigned long long)nx * ny * nz < (1ULL << 32))
        render_kernel<unsigned><<<grid, dim3(PB), lds, s>>>(H, W, rays, cone, nx, ny, nz, d, accuracy, vol, bt, K, lt, lo, scale,
                                                            t_stop, o);
    else
        render_kernel<size_t><<<grid, dim3(PB), lds, s>>>(H, W, rays, cone, nx, ny, nz, d, accuracy, vol, bt, K, lt, lo, scale,
                                                          t_stop, o);
    R2_STAGE_CHECK(0, s, "render volume");
    return 0;
}

extern "C" int r2_render_volume_mip(int V, int H, int W, const float *rays, int cone, int nx, int ny, int nz, float dVoxel_x,
                                    float dVoxel_y, float dVoxel_z, float accuracy, const float *vol, const float *bricks,
                                    float *out, void *stream)
{
    using namespace r2;
    if (const int rc = check_forward_args("r2_render_volume_mip", V, H, W, rays, nx, ny, nz, dVoxel_x, dVoxel_y, dVoxel_z,
                                          &accuracy, vol, out))
        return rc;
    if (bricks && (!bricks_fit(nx, ny, nz) || !aligned_to(bricks, 8))) {
        set_error("r2_render_volume_mip: more than 2^31 - 1 bricks, or a table that is not 8-byte aligned");
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid = volume_pixel_grid(V, H, W);
    const float3 d = make_float3(dVoxel_x, dVoxel_y, dVoxel_z);
    const float2 *bt = reinterpret_cast<const float2 *>(bricks);
    if ((unsigned long long)nx * ny * nz < (1ULL << 32))
        mip_kernel<unsigned><<<grid, dim3(PB), 0, s>>>(H, W, rays, cone, nx, ny, nz, d, accuracy, vol, bt, out);
    else
        mip_kernel<size_t><<<grid, dim3(PB), 0, s>>>(H, W, rays, cone, nx, ny, nz, d, accuracy, vol, bt, out);
    R2_STAGE_CHECK(0, s, "render volume mip");
    return 0;
}
