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
//
// With per-pixel weights w (r2_loss_l1_ssim_weighted*, a second instantiation of the same device functions plus a fold launch
// between the passes): y -> y' = w > 0 ? y : x (held constant), 1/N -> 1/sum w, D_i -> w D_i, sign -> w sign; include/r2hip.h.
#include "ssim_window.hpp"

namespace r2 {

namespace {

constexpr int LT = SSIM_LT, WIN = SSIM_WIN, HALO = SSIM_HALO, LR = SSIM_LR;
using Window = SsimWindow;

__device__ __forceinline__ float load_or_zero(const float *__restrict__ p, int x, int y, int W, int H)
{
    return (x >= 0 && x < W && y >= 0 && y < H) ? p[(size_t)y * W + x] : 0.f;
}

// a weight as the weighted loss counts it: negative, zero and NaN weights are 0
__device__ __forceinline__ float counted_weight(float w) { return w > 0.f ? w : 0.f; }

// pass 1 of ONE view, by the block (blockIdx.x, blockIdx.y) of its tile grid: SSIM map value + its three partial derivatives
// per pixel; per-block sums of S and |x - y|.  The single-view and the batched kernel both are this function.
// WEIGHTED: wt [H][W] (nullptr = all ones) weighs every pixel.  The measurement is y' = y where the weight counts and the
// image's own value elsewhere, selected while the tile is staged (an unmeasured y may be NaN: it is loaded, never used); the
// derivative maps are stored times the weight, the sums become {sum w S, sum w |x - y'|} and, in wpartial, sum w.  A product
// with a weight of exactly 1 is exact, fused or not, so an all-ones wt gives the bits of the unweighted instantiation.
template <bool WEIGHTED>
__device__ __forceinline__ void ssim_forward_view(int W, int H, const float *__restrict__ x, const float *__restrict__ y,
                                                  const float *__restrict__ wt, const Window &win,
                                                  float *__restrict__ D /* [3][H][W] */,
                                                  float2 *__restrict__ partial /* per block {sum S, sum |x-y|} */,
                                                  float *__restrict__ wpartial /* per block sum w */)
{
    __shared__ float sx[LR][LR + 1], sy[LR][LR + 1];
    __shared__ float hb[5][LR][LT + 1];   // horizontally blurred x, y, x^2, y^2, xy
    __shared__ float2 red[LT * LT / 64];
    const int tid = threadIdx.x, tx = tid % LT, ty = tid / LT;
    const int ox = blockIdx.x * LT, oy = blockIdx.y * LT;
    for (int i = tid; i < LR * LR; i += LT * LT) {
        const int ry = i / LR, rx = i % LR;
        if constexpr (WEIGHTED) {
            const int gx = ox + rx - HALO, gy = oy + ry - HALO;
            float xv = 0.f, yv = 0.f;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t o = (size_t)gy * W + gx;
                xv = x[o];
                const float yl = y[o], wv = wt ? wt[o] : 1.f;
                yv = wv > 0.f ? yl : xv;
            }
            sx[ry][rx] = xv;
            sy[ry][rx] = yv;
        } else {
            sx[ry][rx] = load_or_zero(x, ox + rx - HALO, oy + ry - HALO, W, H);
            sy[ry][rx] = load_or_zero(y, ox + rx - HALO, oy + ry - HALO, W, H);
        }
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
    // a sum of two products can contract either way round, and does so differently from one instantiation to the other: the
    // weighted one spells those out (B1, d1, pass 2's last line) in the operations the unweighted one's plain expressions
    // compile to, which is what makes unit weights give the unweighted bits (tests/test_weighted_loss_gpu.py compares them)
    const float A1 = 2.f * m1 * m2 + C1, A2 = 2.f * s12 + C2, B2 = s1 + s2 + C2;
    const float B1 = WEIGHTED ? fmaf(m2, m2, m1 * m1) + C1 : m1 * m1 + m2 * m2 + C1;
    const float inv = 1.0f / (B1 * B2);
    const float S = A1 * A2 * inv;
    float2 acc = make_float2(0.f, 0.f);
    [[maybe_unused]] float accw = 0.f;
    if (in) {
        // m1 enters A1 (2 m2), B1 (2 m1), s1 (-2 m1 -> B2) and s12 (-m2 -> A2: -2 m2)
        const float d1 = WEIGHTED ? fmaf(fmaf(2.f * m2, A2, -(2.f * m2 * A1)), inv, -(S * (2.f * m1 / B1 - 2.f * m1 / B2)))
                                  : (2.f * m2 * A2 - 2.f * m2 * A1) * inv - S * (2.f * m1 / B1 - 2.f * m1 / B2);
        const float d2 = -S / B2;
        const float d3 = 2.f * A1 * inv;
        const size_t o = (size_t)py * W + px, N = (size_t)W * H;
        if constexpr (WEIGHTED) {
            const float wq = wt ? counted_weight(wt[o]) : 1.f;
            D[o] = wq * d1; D[N + o] = wq * d2; D[2 * N + o] = wq * d3;
            acc = make_float2(wq * S, wq * fabsf(sx[ty + HALO][tx + HALO] - sy[ty + HALO][tx + HALO]));
            accw = wq;
        } else {
            D[o] = d1; D[N + o] = d2; D[2 * N + o] = d3;
            acc = make_float2(S, fabsf(sx[ty + HALO][tx + HALO] - sy[ty + HALO][tx + HALO]));
        }
    }
    // deterministic block sum
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { acc.x += __shfl_xor(acc.x, d); acc.y += __shfl_xor(acc.y, d); }
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    if constexpr (WEIGHTED) {
        __shared__ float redw[LT * LT / 64];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) accw += __shfl_xor(accw, d);
        if ((tid & 63) == 0) redw[tid >> 6] = accw;
        __syncthreads();
        if (tid == 0) {
            float t = redw[0];
            for (int w = 1; w < LT * LT / 64; ++w) t += redw[w];
            wpartial[blockIdx.y * gridDim.x + blockIdx.x] = t;
        }
    } else {
        __syncthreads();
    }
    if (tid == 0) {
        float2 t = red[0];
        for (int w = 1; w < LT * LT / 64; ++w) { t.x += red[w].x; t.y += red[w].y; }
        partial[blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
}

// pass 2 of ONE view: blur the three derivative maps, combine with x, y -> dL/dx with the weights (w_l1, w_ssim)
// WEIGHTED: D holds the maps times the pixel weights, sum_w is the view's folded weight sum (ssim_fold_view) and takes the
// place of N (a sum of 0, no measured pixel, gives a zero gradient); the L1 term carries the pixel's own weight and y is y'.
// The combination is spelled out in the operations the unweighted expression contracts to, so that unit weights give its bits.
template <bool WEIGHTED>
__device__ __forceinline__ void ssim_backward_view(int W, int H, const float *__restrict__ x, const float *__restrict__ y,
                                                   const float *__restrict__ wt, float sum_w, const Window &win,
                                                   const float *__restrict__ D, float w_l1, float w_ssim,
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
        if constexpr (WEIGHTED) {
            const float xv = x[o], yl = y[o], wp = wt ? counted_weight(wt[o]) : 1.f;
            const float yv = wp > 0.f ? yl : xv, df = xv - yv;
            const float sgn = df > 0.f ? wp : (df < 0.f ? -wp : 0.f);
            const float inv = sum_w > 0.f ? 1.0f / sum_w : 0.f;
            const float g = fmaf(b3, yv, fmaf(b2, xv + xv, b1));
            const float s = (w_ssim * inv) * g;
            dL_dx[o] = fmaf(w_l1 * inv, sgn, -s);
        } else {
            const float xv = x[o], yv = y[o], df = xv - yv;
            const float sgn = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
            const float invN = 1.0f / (float)N;
            dL_dx[o] = -w_ssim * invN * (b1 + 2.f * xv * b2 + yv * b3) + w_l1 * invN * sgn;
        }
    }
}

// fixed-order reduction of ONE view's per-block sums in double, by a whole block: deterministic scalars {l1 mean, ssim mean,
// loss}, returned to thread 0 (the other threads' return value is not meaningful).  A block that calls this more than once
// puts a __syncthreads() between the calls (`red` is reused).
// WEIGHTED: the per-block weight sums wpartial are folded the same way and their sum takes the place of N: scalars {sum w
// |x - y'| / sum w, sum w S / sum w, loss} and, in .w, sum w rounded to float once; no measured pixel (sum w = 0): {0, 1, 0, 0}.
template <bool WEIGHTED>
__device__ __forceinline__ float4 ssim_fold_view(const float2 *__restrict__ partial, const float *__restrict__ wpartial,
                                                 int nblocks, size_t N, float w_l1, float w_ssim)
{
    __shared__ double red[LT * LT / 64][WEIGHTED ? 3 : 2];
    const int tid = threadIdx.x;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    double sS = 0.0, sA = 0.0;
    [[maybe_unused]] double sW = 0.0;
    for (int i = tid; i < nblocks; i += LT * LT) {
        const float2 q = partial[i]; sS += q.x; sA += q.y;
        if constexpr (WEIGHTED) sW += wpartial[i];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sS += __shfl_xor(sS, d); sA += __shfl_xor(sA, d);
        if constexpr (WEIGHTED) sW += __shfl_xor(sW, d);
    }
    if ((tid & 63) == 0) {
        red[tid >> 6][0] = sS; red[tid >> 6][1] = sA;
        if constexpr (WEIGHTED) red[tid >> 6][2] = sW;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < LT * LT / 64; ++w) {
            red[0][0] += red[w][0]; red[0][1] += red[w][1];
            if constexpr (WEIGHTED) red[0][2] += red[w][2];
        }
        if constexpr (WEIGHTED) {
            const double sw = red[0][2];
            const double l1 = sw > 0.0 ? red[0][1] / sw : 0.0, ssim = sw > 0.0 ? red[0][0] / sw : 1.0;
            out = make_float4((float)l1, (float)ssim, (float)((double)w_l1 * l1 + (double)w_ssim * (1.0 - ssim)), (float)sw);
        } else {
            const double l1 = red[0][1] / (double)N, ssim = red[0][0] / (double)N;
            out = make_float4((float)l1, (float)ssim, (float)((double)w_l1 * l1 + (double)w_ssim * (1.0 - ssim)), 0.f);
        }
    }
    return out;
}

__global__ void __launch_bounds__(LT * LT) ssim_forward_kernel(int W, int H, const float *__restrict__ x, const float *__restrict__ y,
                                                                Window win, float *__restrict__ D, float2 *__restrict__ partial)
{
    ssim_forward_view<false>(W, H, x, y, nullptr, win, D, partial, nullptr);
}

// block 0 also folds the partial sums into the scalars
__global__ void __launch_bounds__(LT * LT) ssim_backward_kernel(int W, int H, const float *__restrict__ x, const float *__restrict__ y,
                                                                 Window win, const float *__restrict__ D,
                                                                 const float2 *__restrict__ partial, int nblocks, float w_l1,
                                                                 float w_ssim, float *__restrict__ dL_dx,
                                                                 float *__restrict__ scalars /* {l1 mean, ssim mean, loss} */)
{
    ssim_backward_view<false>(W, H, x, y, nullptr, 0.f, win, D, w_l1, w_ssim, dL_dx);
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        const float4 r = ssim_fold_view<false>(partial, nullptr, nblocks, (size_t)W * H, w_l1, w_ssim);
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
    ssim_forward_view<false>(W, H, x + v * N, gts.gt[v], nullptr, win, D + 3 * v * N, partial + v * (gridDim.x * gridDim.y), nullptr);
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
    ssim_backward_view<false>(W, H, x + v * N, gts.gt[v], nullptr, 0.f, win, D + 3 * v * N, gw_l1, gw_ssim, dL_dx + v * N);
    if (blockIdx.x != 0 || blockIdx.y != 0) return;
    const float4 mine = ssim_fold_view<false>(partial + v * nblocks, nullptr, nblocks, N, w_l1, w_ssim);
    if (threadIdx.x == 0) { scalars[3 * v] = mine.x; scalars[3 * v + 1] = mine.y; scalars[3 * v + 2] = mine.z; }
    if (n_all > 0 && v == 0) {
        double l1 = 0.0, ssim = 0.0, loss = 0.0;
        for (int u = 0; u < n_all; ++u) {
            __syncthreads();
            const float4 r = ssim_fold_view<false>(partial_all + (size_t)u * nblocks, nullptr, nblocks, N, w_l1, w_ssim);
            l1 += (double)r.x; ssim += (double)r.y; loss += (double)r.z;
        }
        if (threadIdx.x == 0) {
            batch_row[0] = (float)(l1 / n_all); batch_row[1] = (float)(ssim / n_all); batch_row[2] = (float)(loss / n_all);
        }
    }
}

// ---- the weighted loss: three launches for up to R2_LOSS_BATCH_CHUNK views (one view is a chunk of one).  Between the two
// passes one block per view folds that view's partial sums: the backward needs 1 / sum w in every block, and a fold by every
// block for itself would read all per-block sums once per block.  wt[v] == nullptr: view v has unit weights.
struct WeightedChunk { const float *gt[R2_LOSS_BATCH_CHUNK]; const float *wt[R2_LOSS_BATCH_CHUNK]; };

__global__ void __launch_bounds__(LT * LT) ssim_forward_weighted_kernel(int W, int H, const float *__restrict__ x, WeightedChunk views,
                                                                         Window win, float *__restrict__ D, float2 *__restrict__ partial,
                                                                         float *__restrict__ wpartial)
{
    const size_t v = blockIdx.z, N = (size_t)W * H, nblocks = (size_t)gridDim.x * gridDim.y;
    ssim_forward_view<true>(W, H, x + v * N, views.gt[v], views.wt[v], win, D + 3 * v * N, partial + v * nblocks, wpartial + v * nblocks);
}

// block v: the scalar row {l1, ssim, loss, sum w} of the launch's view v, and its sum w again in sum_w[v] for the backward
__global__ void __launch_bounds__(LT * LT) ssim_fold_weighted_kernel(const float2 *__restrict__ partial, const float *__restrict__ wpartial,
                                                                      int nblocks, size_t N, float w_l1, float w_ssim,
                                                                      float *__restrict__ scalars, float *__restrict__ sum_w)
{
    const size_t v = blockIdx.x;
    const float4 mine = ssim_fold_view<true>(partial + v * nblocks, wpartial + v * nblocks, nblocks, N, w_l1, w_ssim);
    if (threadIdx.x == 0) {
        scalars[4 * v] = mine.x; scalars[4 * v + 1] = mine.y; scalars[4 * v + 2] = mine.z; scalars[4 * v + 3] = mine.w;
        sum_w[v] = mine.w;
    }
}

// n_all > 0 (the LAST launch of a batched call): every view's scalar row is written by then (the fold launches come before),
// and thread 0 of block (0, 0, 0) writes the batch row from them next to its gradient work: the means of the first three
// columns of the float rows and the sum of the fourth, summed in view order in double.
__global__ void __launch_bounds__(LT * LT) ssim_backward_weighted_kernel(int W, int H, const float *__restrict__ x, WeightedChunk views,
                                                                          Window win, const float *__restrict__ D,
                                                                          const float *__restrict__ sum_w, float gw_l1, float gw_ssim,
                                                                          float *__restrict__ dL_dx, int n_all,
                                                                          const float *rows_all /* scalars row 0 */,
                                                                          float *batch_row /* scalars row n_all */)
{
    const size_t v = blockIdx.z, N = (size_t)W * H;
    ssim_backward_view<true>(W, H, x + v * N, views.gt[v], views.wt[v], sum_w[v], win, D + 3 * v * N, gw_l1, gw_ssim, dL_dx + v * N);
    if (n_all > 0 && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
        double l1 = 0.0, ssim = 0.0, loss = 0.0, sw = 0.0;
        for (int u = 0; u < n_all; ++u) {
            l1 += (double)rows_all[4 * u]; ssim += (double)rows_all[4 * u + 1]; loss += (double)rows_all[4 * u + 2];
            sw += (double)rows_all[4 * u + 3];
        }
        batch_row[0] = (float)(l1 / n_all); batch_row[1] = (float)(ssim / n_all); batch_row[2] = (float)(loss / n_all);
        batch_row[3] = (float)sw;
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

namespace {
// weighted scratch: the batched layout, then [V][blocks] per-block weight sums and the V folded weight sums
size_t weighted_scratch_floats(int V, int width, int height)
{
    return ssim_batch_partial_offset(V, width, height) + 3 * (size_t)V * ssim_blocks(width, height) + (size_t)V;
}

// the launches of both weighted entries; batch: the call also writes row V and divides the gradient's weights by V
int weighted_loss(const char *name, bool batch, int V, int width, int height, const float *imgs, const float *const *gts_host,
                  const float *const *weights_host, float w_l1, float w_ssim, float *dL_dimg, float *scratch, float *scalars,
                  void *stream)
{
    using namespace r2;
    const size_t N = (size_t)width * height, nb = ssim_blocks(width, height);
    const dim3 tiles((width + LT - 1) / LT, (height + LT - 1) / LT);
    if (tiles.y > 65535u || nb > 0x7fffffffu || (size_t)V * nb > 0x7fffffffu) {   // grid limits; block counts are ints on the device
        set_error("%s: %d views of %d x %d exceed the grid", name, V, width, height);
        return R2_ERR_INVALID;
    }
    float2 *partial = reinterpret_cast<float2 *>(scratch + ssim_batch_partial_offset(V, width, height));
    float *wpartial = reinterpret_cast<float *>(partial + (size_t)V * nb), *sum_w = wpartial + (size_t)V * nb;
    const Window win = make_ssim_window();
    const float gw_l1 = batch ? w_l1 / (float)V : w_l1, gw_ssim = batch ? w_ssim / (float)V : w_ssim;
    hipStream_t s = (hipStream_t)stream;
    for (int v0 = 0; v0 < V; v0 += R2_LOSS_BATCH_CHUNK) {
        const int nv = V - v0 < R2_LOSS_BATCH_CHUNK ? V - v0 : R2_LOSS_BATCH_CHUNK;
        WeightedChunk views;
        for (int k = 0; k < R2_LOSS_BATCH_CHUNK; ++k) {
            views.gt[k] = k < nv ? gts_host[v0 + k] : nullptr;
            views.wt[k] = k < nv && weights_host ? weights_host[v0 + k] : nullptr;
        }
        const dim3 grid(tiles.x, tiles.y, nv);
        const float *x = imgs + (size_t)v0 * N;
        float *D = scratch + 3 * (size_t)v0 * N;
        ssim_forward_weighted_kernel<<<grid, dim3(LT * LT), 0, s>>>(width, height, x, views, win, D, partial + (size_t)v0 * nb,
                                                                    wpartial + (size_t)v0 * nb);
        ssim_fold_weighted_kernel<<<dim3(nv), dim3(LT * LT), 0, s>>>(partial + (size_t)v0 * nb, wpartial + (size_t)v0 * nb, (int)nb, N,
                                                                     w_l1, w_ssim, scalars + 4 * (size_t)v0, sum_w + v0);
        ssim_backward_weighted_kernel<<<grid, dim3(LT * LT), 0, s>>>(width, height, x, views, win, D, sum_w + v0, gw_l1, gw_ssim,
                                                                     dL_dimg + (size_t)v0 * N, batch && v0 + nv == V ? V : 0,
                                                                     scalars, scalars + 4 * (size_t)V);
    }
    return 0;
}
}  // namespace

extern "C" size_t r2_loss_l1_ssim_weighted_scratch_floats(int width, int height)
{
    if (width <= 0 || height <= 0) return 0;
    return weighted_scratch_floats(1, width, height);
}

extern "C" int r2_loss_l1_ssim_weighted(int width, int height, const float *img, const float *gt, const float *weights,
                                        float w_l1, float w_ssim, float *dL_dimg, float *scratch, float *scalars, void *stream)
{
    using namespace r2;
    if (width <= 0 || height <= 0 || !img || !gt || !dL_dimg || !scratch || !scalars) {
        set_error("r2_loss_l1_ssim_weighted: invalid argument");
        return R2_ERR_INVALID;
    }
    const int rc = weighted_loss("r2_loss_l1_ssim_weighted", false, 1, width, height, img, &gt, &weights, w_l1, w_ssim, dL_dimg,
                                 scratch, scalars, stream);
    if (rc) return rc;
    R2_STAGE_CHECK(0, (hipStream_t)stream, "weighted l1 + ssim loss");
    return 0;
}

extern "C" size_t r2_loss_l1_ssim_weighted_batch_scratch_floats(int V, int width, int height)
{
    if (V < 1 || width <= 0 || height <= 0) return 0;
    return weighted_scratch_floats(V, width, height);
}

extern "C" int r2_loss_l1_ssim_weighted_batch(int V, int width, int height, const float *imgs, const float *const *gts_host,
                                              const float *const *weights_host, float w_l1, float w_ssim, float *dL_dimg,
                                              float *scratch, float *scalars, void *stream)
{
    using namespace r2;
    if (V < 1 || width <= 0 || height <= 0 || !imgs || !gts_host || !dL_dimg || !scratch || !scalars) {
        set_error("r2_loss_l1_ssim_weighted_batch: invalid argument");
        return R2_ERR_INVALID;
    }
    for (int v = 0; v < V; ++v)
        if (!gts_host[v]) {
            set_error("r2_loss_l1_ssim_weighted_batch: ground truth %d is NULL", v);
            return R2_ERR_INVALID;
        }
    const int rc = weighted_loss("r2_loss_l1_ssim_weighted_batch", true, V, width, height, imgs, gts_host, weights_host, w_l1,
                                 w_ssim, dL_dimg, scratch, scalars, stream);
    if (rc) return rc;
    R2_STAGE_CHECK(0, (hipStream_t)stream, "batched weighted l1 + ssim loss");
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
