// loss_ops.hip -- the training loop's loss stack as three kernels: L1 + lambda (1 - SSIM) of a rendered
// projection against its measurement, forward AND gradient in two launches, and the 3D total-variation regulariser of the
// 32^3 query volume in one.  Reference: r2_gaussian/utils/loss_utils.py:19-104 (tv_3d_loss, l1_loss, ssim: 11x11 Gaussian
// window, sigma 1.5, zero padding, mean of the SSIM map), train.py:118-147.
//
// In the reference these are ~60 torch kernels per iteration (five conv2d through the vendor DNN library, their backward,
// and two dozen elementwise ops) -- more GPU time than the rasterizer at these sizes (measured: 440 us forward + their share
// of a 790 us backward vs 215 us for render forward + backward) -- and the vendor convolution reads past the end of its
// 484-byte weight tensor on this stack (scripts/miopen_overread_probe.py: a pure-torch loop faults when the window sits at the
// end of an allocator segment).  Here: separable 11-tap blurs staged in LDS, analytic SSIM derivative, deterministic sums.
//
//   S = (2 m1 m2 + C1)(2 s12 + C2) / ((m1^2 + m2^2 + C1)(s1 + s2 + C2)),  m = W*x, s1 = W*x^2 - m1^2, s12 = W*xy - m1 m2
//   dL/dx(p) = -lambda/N sum_q W(q-p) [ D1(q) + 2 x(p) D2(q) + y(p) D3(q) ] + sign(x - y)/N,
//   D1 = dS/dm1 (with s1, s12 depending on m1), D2 = dS/d(W*x^2), D3 = dS/d(W*xy).
#include "ssim_window.hpp"

namespace r2 {

namespace {

constexpr int LT = SSIM_LT, WIN = SSIM_WIN, HALO = SSIM_HALO, LR = SSIM_LR;
using Window = SsimWindow;

__device__ __forceinline__ float load_or_zero(const float *__restrict__ p, int x, int y, int W, int H)
{
    return (x >= 0 && x < W && y >= 0 && y < H) ? p[(size_t)y * W + x] : 0.f;
}

// pass 1 of ONE view, by the block (blockIdx.x, blockIdx.y) of its tile grid: SSIM map value + its three partial derivatives
// per pixel; per-block sums of S and |x - y|.  The single-view and the batched kernel both are this function.
__device__ __forceinline__ void ssim_forward_view(int W, int H, const float *__restrict__ x, const float *__restrict__ y,
                                                  const Window &win, float *__restrict__ D /* [3][H][W] */,
                                                  float2 *__restrict__ partial /* per block {sum S, sum |x-y|} */)
{
    __shared__ float sx[LR][LR + 1], sy[LR][LR + 1];
    __shared__ float hb[5][LR][LT + 1];   // horizontally blurred x, y, x^2, y^2, xy
    __shared__ float2 red[LT * LT / 64];
    const int tid = threadIdx.x, tx = tid % LT, ty = tid / LT;
    const int ox = blockIdx.x * LT, oy = blockIdx.y * LT;
    for (int i = tid; i < LR * LR; i += LT * LT) {
        const int ry = i / LR, rx = i % LR;
        sx[ry][rx] = load_or_zero(x, ox + rx - HALO, oy + ry - HALO, W, H);
        sy[ry][rx] = load_or_zero(y, ox + rx - HALO, oy + ry - HALO, W, H);
    }
    __syncthreads();
    for (int i = tid; i < LR * LT; i += LT * LT) {
        const int ry = i / LT, cx = i % LT;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float u = sx[ry][cx + k], v = sy[ry][cx + k], w = win.w[k];
            a += w * u; b += w * v; aa += w * (u * u); bb += w * (v * v); ab += w * (u * v);
        }
        hb[0][ry][cx] = a; hb[1][ry][cx] = b; hb[2][ry][cx] = aa; hb[3][ry][cx] = bb; hb[4][ry][cx] = ab;
    }
    __syncthreads();
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < WIN; ++k) {
        const float w = win.w[k];
        m1 += w * hb[0][ty + k][tx]; m2 += w * hb[1][ty + k][tx]; e11 += w * hb[2][ty + k][tx];
        e22 += w * hb[3][ty + k][tx]; e12 += w * hb[4][ty + k][tx];
    }
    const int px = ox + tx, py = oy + ty;
    const bool in = px < W && py < H;
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float s1 = e11 - m1 * m1, s2 = e22 - m2 * m2, s12 = e12 - m1 * m2;
    const float A1 = 2.f * m1 * m2 + C1, A2 = 2.f * s12 + C2, B1 = m1 * m1 + m2 * m2 + C1, B2 = s1 + s2 + C2;
    const float inv = 1.0f / (B1 * B2);
    const float S = A1 * A2 * inv;
    float2 acc = make_float2(0.f, 0.f);
    if (in) {
        // m1 enters A1 (2 m2), B1 (2 m1), s1 (-2 m1 -> B2) and s12 (-m2 -> A2: -2 m2)
        const float d1 = (2.f * m2 * A2 - 2.f * m2 * A1) * inv - S * (2.f * m1 / B1 - 2.f * m1 / B2);
        const float d2 = -S / B2;
        const float d3 = 2.f * A1 * inv;
        const size_t o = (size_t)py * W + px, N = (size_t)W * H;
        D[o] = d1; D[N + o] = d2; D[2 * N + o] = d3;
        acc = make_float2(S, fabsf(sx[ty + HALO][tx + HALO] - sy[ty + HALO][tx + HALO]));
    }
    // deterministic block sum
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { acc.x += __shfl_xor(acc.x, d); acc.y += __shfl_xor(acc.y, d); }
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        float2 t = red[0];
        for (int w = 1; w < LT * LT / 64; ++w) { t.x += red[w].x; t.y += red[w].y; }
        partial[blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
}

// pass 2 of ONE view: blur the three derivative maps, combine with x, y -> dL/dx with the weights (w_l1, w_ssim)
__device__ __forceinline__ void ssim_backward_view(int W, int H, const float *__restrict__ x, const float *__restrict__ y,
                                                   const Window &win, const float *__restrict__ D, float w_l1, float w_ssim,
                                                   float *__restrict__ dL_dx)
{
    __shared__ float sd[3][LR][LR + 1];
    __shared__ float hb[3][LR][LT + 1];
    const int tid = threadIdx.x, tx = tid % LT, ty = tid / LT;
    const int ox = blockIdx.x * LT, oy = blockIdx.y * LT;
    const size_t N = (size_t)W * H;
    for (int i = tid; i < LR * LR; i += LT * LT) {
        const int ry = i / LR, rx = i % LR;
#pragma unroll
        for (int c = 0; c < 3; ++c) sd[c][ry][rx] = load_or_zero(D + c * N, ox + rx - HALO, oy + ry - HALO, W, H);
    }
    __syncthreads();
    for (int i = tid; i < LR * LT; i += LT * LT) {
        const int ry = i / LT, cx = i % LT;
        float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float w = win.w[k];
            a += w * sd[0][ry][cx + k]; b += w * sd[1][ry][cx + k]; c += w * sd[2][ry][cx + k];
        }
        hb[0][ry][cx] = a; hb[1][ry][cx] = b; hb[2][ry][cx] = c;
    }
    __syncthreads();
    float b1 = 0.f, b2 = 0.f, b3 = 0.f;
#pragma unroll
    for (int k = 0; k < WIN; ++k) {
        const float w = win.w[k];
        b1 += w * hb[0][ty + k][tx]; b2 += w * hb[1][ty + k][tx]; b3 += w * hb[2][ty + k][tx];
    }
    const int px = ox + tx, py = oy + ty;
    if (px < W && py < H) {
        const size_t o = (size_t)py * W + px;
        const float xv = x[o], yv = y[o], df = xv - yv;
        const float sgn = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
        const float invN = 1.0f / (float)N;
        dL_dx[o] = -w_ssim * invN * (b1 + 2.f * xv * b2 + yv * b3) + w_l1 * invN * sgn;
    }
}

// fixed-order reduction of ONE view's per-block sums in double, by a whole block: deterministic scalars {l1 mean, ssim mean,
// loss}, returned to thread 0 (the other threads' return value is not meaningful).  A block that calls this more than once
// puts a __syncthreads() between the calls (`red` is reused).
__device__ __forceinline__ float3 ssim_fold_view(const float2 *__restrict__ partial, int nblocks, size_t N, float w_l1, float w_ssim)
{
    __shared__ double red[LT * LT / 64][2];
    const int tid = threadIdx.x;
    float3 out = make_float3(0.f, 0.f, 0.f);
    double sS = 0.0, sA = 0.0;
    for (int i = tid; i < nblocks; i += LT * LT) { const float2 q = partial[i]; sS += q.x; sA += q.y; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { sS += __shfl_xor(sS, d); sA += __shfl_xor(sA, d); }
    if ((tid & 63) == 0) { red[tid >> 6][0] = sS; red[tid >> 6][1] = sA; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < LT * LT / 64; ++w) { red[0][0] += red[w][0]; red[0][1] += red[w][1]; }
        const double l1 = red[0][1] / (double)N, ssim = red[0][0] / (double)N;
        out = make_float3((float)l1, (float)ssim, (float)((double)w_l1 * l1 + (double)w_ssim * (1.0 - ssim)));
    }
    return out;
}

__global__ void __launch_bounds__(LT * LT) ssim_forward_kernel(int W, int H, const float *__restrict__ x, const float *__restrict__ y,
                                                                Window win, float *__restrict__ D, float2 *__restrict__ partial)
{
    ssim_forward_view(W, H, x, y, win, D, partial);
}

// block 0 also folds the partial sums into the scalars
__global__ void __launch_bounds__(LT * LT) ssim_backward_kernel(int W, int H, const float *__restrict__ x, const float *__restrict__ y,
                                                                 Window win, const float *__restrict__ D,
                                                                 const float2 *__restrict__ partial, int nblocks, float w_l1,
                                                                 float w_ssim, float *__restrict__ dL_dx,
                                                                 float *__restrict__ scalars /* {l1 mean, ssim mean, loss} */)
{
    ssim_backward_view(W, H, x, y, win, D, w_l1, w_ssim, dL_dx);
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        const float3 r = ssim_fold_view(partial, nblocks, (size_t)W * H, w_l1, w_ssim);
        if (threadIdx.x == 0) { scalars[0] = r.x; scalars[1] = r.y; scalars[2] = r.z; }
    }
}

// ---- V views per launch: the view is the third grid dimension, every block runs the single-view code on its view.  The
// images, derivative maps, partial sums, gradients and scalar rows of a launch's views are contiguous; the ground truths are
// not, so their pointers travel by value, R2_LOSS_BATCH_CHUNK views per launch.
struct GtChunk { const float *gt[R2_LOSS_BATCH_CHUNK]; };

__global__ void __launch_bounds__(LT * LT) ssim_forward_batch_kernel(int W, int H, const float *__restrict__ x, GtChunk gts, Window win,
                                                                      float *__restrict__ D, float2 *__restrict__ partial)
{
    const size_t v = blockIdx.z, N = (size_t)W * H;
    ssim_forward_view(W, H, x + v * N, gts.gt[v], win, D + 3 * v * N, partial + v * (gridDim.x * gridDim.y));
}

// (w_l1, w_ssim) weigh the scalars' loss, (gw_l1, gw_ssim) the gradient.  n_all > 0 (the LAST launch of a call, whose views
// complete the batch): block (0, 0, 0) then folds every view of the batch again, in view order, and writes the batch row:
// the means of the float rows, summed in double.
__global__ void __launch_bounds__(LT * LT) ssim_backward_batch_kernel(int W, int H, const float *__restrict__ x, GtChunk gts, Window win,
                                                                       const float *__restrict__ D, const float2 *__restrict__ partial,
                                                                       float w_l1, float w_ssim, float gw_l1, float gw_ssim,
                                                                       float *__restrict__ dL_dx, float *__restrict__ scalars,
                                                                       int n_all, const float2 *partial_all /* view 0's */,
                                                                       float *batch_row /* scalars row n_all */)
{
    const size_t v = blockIdx.z, N = (size_t)W * H;
    const int nblocks = gridDim.x * gridDim.y;
    ssim_backward_view(W, H, x + v * N, gts.gt[v], win, D + 3 * v * N, gw_l1, gw_ssim, dL_dx + v * N);
    if (blockIdx.x != 0 || blockIdx.y != 0) return;
    const float3 mine = ssim_fold_view(partial + v * nblocks, nblocks, N, w_l1, w_ssim);
    if (threadIdx.x == 0) { scalars[3 * v] = mine.x; scalars[3 * v + 1] = mine.y; scalars[3 * v + 2] = mine.z; }
    if (n_all > 0 && v == 0) {
        double l1 = 0.0, ssim = 0.0, loss = 0.0;
        for (int u = 0; u < n_all; ++u) {
            __syncthreads();
            const float3 r = ssim_fold_view(partial_all + (size_t)u * nblocks, nblocks, N, w_l1, w_ssim);
            l1 += (double)r.x; ssim += (double)r.y; loss += (double)r.z;
        }
        if (threadIdx.x == 0) {
            batch_row[0] = (float)(l1 / n_all); batch_row[1] = (float)(ssim / n_all); batch_row[2] = (float)(loss / n_all);
        }
    }
}

// tv_3d_loss(vol, "mean") and its gradient: one thread per voxel
__global__ void __launch_bounds__(256) tv3d_kernel(int nx, int ny, int nz, const float *__restrict__ v, float weight,
                                                   float *__restrict__ dL_dv, float *__restrict__ partial)
{
    __shared__ float red[4];
    const size_t n = (size_t)nx * ny * nz;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const float cnt = (float)((size_t)(nx - 1) * ny * nz + (size_t)nx * (ny - 1) * nz + (size_t)nx * ny * (nz - 1));
    float sum = 0.f;
    if (i < n) {
        const int z = (int)(i % nz), yy = (int)((i / nz) % ny), xx = (int)(i / ((size_t)nz * ny));
        const float c = v[i];
        auto sgn = [](float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); };
        float g = 0.f;
        const size_t sxs = (size_t)ny * nz, sys = (size_t)nz;
        if (xx > 0) { const float d = c - v[i - sxs]; g += sgn(d); }
        if (xx + 1 < nx) { const float d = v[i + sxs] - c; g -= sgn(d); sum += fabsf(d); }
        if (yy > 0) { const float d = c - v[i - sys]; g += sgn(d); }
        if (yy + 1 < ny) { const float d = v[i + sys] - c; g -= sgn(d); sum += fabsf(d); }
        if (z > 0) { const float d = c - v[i - 1]; g += sgn(d); }
        if (z + 1 < nz) { const float d = v[i + 1] - c; g -= sgn(d); sum += fabsf(d); }
        dL_dv[i] = cnt > 0.f ? weight * g / cnt : 0.f;   // no neighbour pairs: the reference's 0/0 value has a zero gradient
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// fixed-order fold of the per-block sums in double; cnt == 0 (no neighbour pairs) gives 0 / 0 = NaN like the reference
__global__ void __launch_bounds__(256) tv3d_finish_kernel(const float *__restrict__ partial, int nblocks, double cnt, float weight,
                                                          float *__restrict__ scalars)
{
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) s += partial[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tv = (red[0] + red[1] + red[2] + red[3]) / cnt;
        scalars[0] = (float)tv;
        scalars[1] = (float)((double)weight * tv);
    }
}

}  // namespace
}  // namespace r2

namespace {
// the float2 partials follow the three derivative maps, rounded up to an even float offset (8-byte aligned for odd W * H)
size_t ssim_partial_offset(int width, int height) { return (3 * (size_t)width * height + 1) & ~(size_t)1; }
}  // namespace

extern "C" size_t r2_loss_l1_ssim_scratch_floats(int width, int height)
{
    const size_t nb = (size_t)((width + r2::LT - 1) / r2::LT) * ((height + r2::LT - 1) / r2::LT);
    return ssim_partial_offset(width, height) + 2 * nb;
}

extern "C" int r2_loss_l1_ssim(int width, int height, const float *img, const float *gt, float w_l1, float w_ssim,
                               float *dL_dimg, float *scratch, float *scalars, void *stream)
{
    using namespace r2;
    if (width <= 0 || height <= 0 || !img || !gt || !dL_dimg || !scratch || !scalars) {
        set_error("r2_loss_l1_ssim: invalid argument");
        return R2_ERR_INVALID;
    }
    const dim3 grid((width + LT - 1) / LT, (height + LT - 1) / LT);
    const int nb = (int)(grid.x * grid.y);
    float *D = scratch;
    float2 *partial = reinterpret_cast<float2 *>(scratch + ssim_partial_offset(width, height));
    const Window win = make_ssim_window();
    hipStream_t s = (hipStream_t)stream;
    ssim_forward_kernel<<<grid, dim3(LT * LT), 0, s>>>(width, height, img, gt, win, D, partial);
    ssim_backward_kernel<<<grid, dim3(LT * LT), 0, s>>>(width, height, img, gt, win, D, partial, nb, w_l1, w_ssim, dL_dimg, scalars);
    R2_STAGE_CHECK(0, s, "l1 + ssim loss");
    return 0;
}

namespace {
size_t ssim_blocks(int width, int height) { return (size_t)((width + r2::LT - 1) / r2::LT) * ((height + r2::LT - 1) / r2::LT); }
// batched scratch: [V][3][H][W] derivative maps, then (8-byte aligned) [V][blocks] float2 partial sums
size_t ssim_batch_partial_offset(int V, int width, int height) { return (3 * (size_t)V * width * height + 1) & ~(size_t)1; }
}  // namespace

extern "C" size_t r2_loss_l1_ssim_batch_scratch_floats(int V, int width, int height)
{
    if (V < 1 || width <= 0 || height <= 0) return 0;
    return ssim_batch_partial_offset(V, width, height) + 2 * (size_t)V * ssim_blocks(width, height);
}

extern "C" int r2_loss_l1_ssim_batch(int V, int width, int height, const float *imgs, const float *const *gts_host, float w_l1,
                                     float w_ssim, float *dL_dimg, float *scratch, float *scalars, void *stream)
{
    using namespace r2;
    if (V < 1 || width <= 0 || height <= 0 || !imgs || !gts_host || !dL_dimg || !scratch || !scalars) {
        set_error("r2_loss_l1_ssim_batch: invalid argument");
        return R2_ERR_INVALID;
    }
    for (int v = 0; v < V; ++v)
        if (!gts_host[v]) {
            set_error("r2_loss_l1_ssim_batch: ground truth %d is NULL", v);
            return R2_ERR_INVALID;
        }
    const size_t N = (size_t)width * height, nb = ssim_blocks(width, height);
    const dim3 tiles((width + LT - 1) / LT, (height + LT - 1) / LT);
    if (tiles.y > 65535u || nb > 0x7fffffffu || (size_t)V * nb > 0x7fffffffu) {   // grid limits; block counts are ints on the device
        set_error("r2_loss_l1_ssim_batch: %d views of %d x %d exceed the grid", V, width, height);
        return R2_ERR_INVALID;
    }
    float2 *partial = reinterpret_cast<float2 *>(scratch + ssim_batch_partial_offset(V, width, height));
    const Window win = make_ssim_window();
    const float gw_l1 = w_l1 / (float)V, gw_ssim = w_ssim / (float)V;
    hipStream_t s = (hipStream_t)stream;
    for (int v0 = 0; v0 < V; v0 += R2_LOSS_BATCH_CHUNK) {
        const int nv = V - v0 < R2_LOSS_BATCH_CHUNK ? V - v0 : R2_LOSS_BATCH_CHUNK;
        GtChunk gts;
        for (int k = 0; k < R2_LOSS_BATCH_CHUNK; ++k) gts.gt[k] = k < nv ? gts_host[v0 + k] : nullptr;
        const dim3 grid(tiles.x, tiles.y, nv);
        const float *x = imgs + (size_t)v0 * N;
        float *D = scratch + 3 * (size_t)v0 * N;
        ssim_forward_batch_kernel<<<grid, dim3(LT * LT), 0, s>>>(width, height, x, gts, win, D, partial + (size_t)v0 * nb);
        ssim_backward_batch_kernel<<<grid, dim3(LT * LT), 0, s>>>(width, height, x, gts, win, D, partial + (size_t)v0 * nb, w_l1, w_ssim,
                                                                 gw_l1, gw_ssim, dL_dimg + (size_t)v0 * N, scalars + 3 * (size_t)v0,
                                                                 v0 + nv == V ? V : 0, partial, scalars + 3 * (size_t)V);
    }
    R2_STAGE_CHECK(0, s, "batched l1 + ssim loss");
    return 0;
}

extern "C" size_t r2_loss_tv3d_scratch_floats(int nx, int ny, int nz)
{
    return ((size_t)nx * ny * nz + 255) / 256;
}

extern "C" int r2_loss_tv3d(int nx, int ny, int nz, const float *vol, float weight, float *dL_dvol, float *scratch,
                            float *scalars, void *stream)
{
    using namespace r2;
    if (nx <= 0 || ny <= 0 || nz <= 0 || !vol || !dL_dvol || !scratch || !scalars) {
        set_error("r2_loss_tv3d: invalid argument");
        return R2_ERR_INVALID;
    }
    const size_t n = (size_t)nx * ny * nz;
    const int nb = (int)((n + 255) / 256);
    const double cnt = (double)(nx - 1) * ny * nz + (double)nx * (ny - 1) * nz + (double)nx * ny * (nz - 1);
    hipStream_t s = (hipStream_t)stream;
    tv3d_kernel<<<dim3(nb), dim3(256), 0, s>>>(nx, ny, nz, vol, weight, dL_dvol, scratch);
    tv3d_finish_kernel<<<dim3(1), dim3(256), 0, s>>>(scratch, nb, cnt, weight, scalars);
    R2_STAGE_CHECK(0, s, "tv3d loss");
    return 0;
}
