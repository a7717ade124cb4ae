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
// With per-pixel weights w (r2_loss_l1_ssim_weighted*, the WEIGHTED instantiation of the same kernels plus a fold launch
// between the passes): y -> y' = w > 0 ? y : x (held constant), 1/N -> 1/sum w, D_i -> w D_i, sign -> w sign; include/r2hip.h.
//
// Every kernel takes its view from blockIdx.z; all four entries run one host loop (image_loss below), a single view being a
// chunk of one.
#include "block_fold.hpp"
#include "ssim_window.hpp"

namespace r2 {

namespace {

constexpr int LT = SSIM_LT, WIN = SSIM_WIN, HALO = SSIM_HALO, LR = SSIM_LR;
constexpr int NW = LT * LT / 64;   // waves per block of the image-loss kernels
using Window = SsimWindow;

__device__ __forceinline__ float load_or_zero(const float *__restrict__ p, int x, int y, int W, int H)
{
    return (x >= 0 && x < W && y >= 0 && y < H) ? p[(size_t)y * W + x] : 0.f;
}

// the weight of pixel o as the weighted loss counts it: negative, zero and NaN weights are 0; no array, or not WEIGHTED: 1.
// A product with a weight of exactly 1 is exact, which is what makes unit weights give the unweighted instantiation's bits.
template <bool WEIGHTED>
__device__ __forceinline__ float counted_weight(const float *__restrict__ wt, size_t o)
{
    if constexpr (WEIGHTED) {
        if (wt) {
            const float w = wt[o];
            return w > 0.f ? w : 0.f;
        }
    }
    return 1.f;
}

// pass 1 of ONE view, by the block (blockIdx.x, blockIdx.y) of its tile grid: SSIM map value + its three partial derivatives
// per pixel; per-block sums of S and |x - y|.
// WEIGHTED: wt [H][W] (nullptr = all ones) weighs every pixel.  The measurement is y' = y where the weight counts and the
// image's own value elsewhere, selected while the tile is staged (an unmeasured y may be NaN: it is loaded, never used); the
// derivative maps are stored times the weight, the sums become {sum w S, sum w |x - y'|} and, in wpartial, sum w.
template <bool WEIGHTED>
__device__ __forceinline__ void ssim_forward_view(int W, int H, const float *__restrict__ x, const float *__restrict__ y,
                                                  const float *__restrict__ wt, const Window &win,
                                                  float *__restrict__ D /* [3][H][W] */,
                                                  float2 *__restrict__ partial /* per block {sum S, sum |x-y|} */,
                                                  float *__restrict__ wpartial /* per block sum w */)
{
    __shared__ SsimTile tile;
    __shared__ Sums<float, WEIGHTED ? 3 : 2> red[NW];
    const SsimMoments m = ssim_tile_moments(tile, W, H, win, [&](int gx, int gy, bool inside) {
        float2 v = make_float2(0.f, 0.f);
        if (inside) {
            const size_t o = (size_t)gy * W + gx;
            v = make_float2(x[o], y[o]);
            if constexpr (WEIGHTED) v.y = (wt ? wt[o] : 1.f) > 0.f ? v.y : v.x;
        }
        return v;
    });
    const int tid = threadIdx.x, tx = tid % LT, ty = tid / LT;
    const int px = blockIdx.x * LT + tx, py = blockIdx.y * LT + ty;
    const float m1 = m.m1, m2 = m.m2;
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float s1 = m.e11 - m1 * m1, s2 = m.e22 - m2 * m2, s12 = m.e12 - m1 * m2;
    // sums of two products are spelled as the fmaf they are, so that no instantiation contracts them its own way
    const float A1 = 2.f * m1 * m2 + C1, A2 = 2.f * s12 + C2, B1 = fmaf(m2, m2, m1 * m1) + C1, B2 = s1 + s2 + C2;
    const float inv = 1.0f / (B1 * B2);
    const float S = A1 * A2 * inv;
    Sums<float, WEIGHTED ? 3 : 2> acc = {};   // {S, |x - y|, weight}, each times the weight
    if (px < W && py < H) {
        // m1 enters A1 (2 m2), B1 (2 m1), s1 (-2 m1 -> B2) and s12 (-m2 -> A2: -2 m2)
        const float d1 = fmaf(fmaf(2.f * m2, A2, -(2.f * m2 * A1)), inv, -(S * (2.f * m1 / B1 - 2.f * m1 / B2)));
        const float d2 = -S / B2;
        const float d3 = 2.f * A1 * inv;
        const size_t o = (size_t)py * W + px, N = (size_t)W * H;
        const float wq = counted_weight<WEIGHTED>(wt, o);
        D[o] = wq * d1; D[N + o] = wq * d2; D[2 * N + o] = wq * d3;
        acc.v[0] = wq * S;
        acc.v[1] = wq * fabsf(tile.x[ty + HALO][tx + HALO] - tile.y[ty + HALO][tx + HALO]);
        if constexpr (WEIGHTED) acc.v[2] = wq;
    }
    acc = block_fold<NW>(acc, red, FoldSum());
    if (tid == 0) {
        const int block = blockIdx.y * gridDim.x + blockIdx.x;
        partial[block] = make_float2(acc.v[0], acc.v[1]);
        if constexpr (WEIGHTED) wpartial[block] = acc.v[2];
    }
}

// pass 2 of ONE view: blur the three derivative maps (stored times the pixel weights), combine with x, y' -> dL/dx with the
// weights (w_l1, w_ssim).  inv: the reciprocal of what normalises the view, 1 / N or 1 / sum w (0 where no pixel is
// measured: a zero gradient).  The L1 term carries the pixel's own weight.
template <bool WEIGHTED>
__device__ __forceinline__ void ssim_backward_view(int W, int H, const float *__restrict__ x, const float *__restrict__ y,
                                                   const float *__restrict__ wt, float inv, const Window &win,
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
        const float xv = x[o], yl = y[o], wp = counted_weight<WEIGHTED>(wt, o);
        const float yv = wp > 0.f ? yl : xv, df = xv - yv;
        const float sgn = df > 0.f ? wp : (df < 0.f ? -wp : 0.f);
        const float g = fmaf(b3, yv, fmaf(b2, xv + xv, b1));
        const float s = (w_ssim * inv) * g;
        dL_dx[o] = fmaf(w_l1 * inv, sgn, -s);
    }
}

// fixed-order reduction of ONE view's per-block sums in double, by a whole block: deterministic scalars {l1 mean, ssim mean,
// loss}, returned to thread 0 (the other threads' return value is not meaningful).  A block that calls this more than once
// puts a __syncthreads() between the calls (the fold's slots are reused).
// WEIGHTED: the per-block weight sums wpartial are folded the same way and their sum takes the place of N: scalars {sum w
// |x - y'| / sum w, sum w S / sum w, loss} and, in .w, sum w rounded to float once; no measured pixel (sum w = 0): {0, 1, 0, 0}.
template <bool WEIGHTED>
__device__ __forceinline__ float4 ssim_fold_view(const float2 *__restrict__ partial, const float *__restrict__ wpartial,
                                                 int nblocks, size_t N, float w_l1, float w_ssim)
{
    __shared__ Sums<double, WEIGHTED ? 3 : 2> red[NW];
    Sums<double, WEIGHTED ? 3 : 2> s = {};   // {sum S, sum |x - y|, sum w}
    for (int i = threadIdx.x; i < nblocks; i += LT * LT) {
        const float2 q = partial[i];
        s.v[0] += q.x; s.v[1] += q.y;
        if constexpr (WEIGHTED) s.v[2] += wpartial[i];
    }
    s = block_fold<NW>(s, red, FoldSum());
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (threadIdx.x == 0) {
        double n = (double)N;
        if constexpr (WEIGHTED) n = s.v[2];
        const double l1 = n > 0.0 ? s.v[1] / n : 0.0, ssim = n > 0.0 ? s.v[0] / n : 1.0;
        out = make_float4((float)l1, (float)ssim, (float)((double)w_l1 * l1 + (double)w_ssim * (1.0 - ssim)), WEIGHTED ? (float)n : 0.f);
    }
    return out;
}

// ---- up to R2_LOSS_BATCH_CHUNK views per launch: the view is the third grid dimension, every block runs the view functions on
// its view.  The images, derivative maps, partial sums, gradients and scalar rows of a launch's views are contiguous; the
// ground truths and weights are not, so their pointers travel by value.  wt[v] == nullptr: view v has unit weights (and
// every view of an unweighted launch).
struct ViewChunk { const float *gt[R2_LOSS_BATCH_CHUNK]; const float *wt[R2_LOSS_BATCH_CHUNK]; };

template <bool WEIGHTED>
__global__ void __launch_bounds__(LT * LT) ssim_forward_kernel(int W, int H, const float *__restrict__ x, ViewChunk views, Window win,
                                                                float *__restrict__ D, float2 *__restrict__ partial,
                                                                float *__restrict__ wpartial /* WEIGHTED only */)
{
    const size_t v = blockIdx.z, N = (size_t)W * H, nblocks = (size_t)gridDim.x * gridDim.y;
    ssim_forward_view<WEIGHTED>(W, H, x + v * N, views.gt[v], views.wt[v], win, D + 3 * v * N, partial + v * nblocks,
                                wpartial + v * nblocks);
}

// the weighted loss's launch between the two passes, one block per view: the backward needs 1 / sum w in every block, and a
// fold by every block for itself would read all per-block sums once per block.  Block v: the scalar row {l1, ssim, loss,
// sum w} of the launch's view v, and its sum w again in sum_w[v] for the backward.
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

// (w_l1, w_ssim) weigh the scalars' loss, (gw_l1, gw_ssim) the gradient.  Unweighted: block (0, 0, v) also folds view v's
// partial sums into rows[v] = {l1, ssim, loss}; WEIGHTED: the fold launch has written the rows and the launch's sum_w.
// n_all > 0 (the LAST launch of a batched call, whose views complete the batch): block (0, 0, 0) also writes the batch row
// rows_all[n_all], the means over the views of the float rows (WEIGHTED: and the sum of their fourth column), summed in view
// order in double.  Unweighted, it folds every view of the batch again for that, from partial_all (view 0's partial sums).
template <bool WEIGHTED>
__global__ void __launch_bounds__(LT * LT) ssim_backward_kernel(int W, int H, const float *__restrict__ x, ViewChunk views, Window win,
                                                                 const float *__restrict__ D, const float2 *__restrict__ partial,
                                                                 const float *__restrict__ sum_w, float w_l1, float w_ssim,
                                                                 float gw_l1, float gw_ssim, float *__restrict__ dL_dx,
                                                                 float *__restrict__ rows, int n_all, const float2 *partial_all,
                                                                 float *rows_all)
{
    const size_t v = blockIdx.z, N = (size_t)W * H;
    float inv = 1.0f / (float)N;
    if constexpr (WEIGHTED) inv = sum_w[v] > 0.f ? 1.0f / sum_w[v] : 0.f;
    ssim_backward_view<WEIGHTED>(W, H, x + v * N, views.gt[v], views.wt[v], inv, win, D + 3 * v * N, gw_l1, gw_ssim, dL_dx + v * N);
    if (blockIdx.x != 0 || blockIdx.y != 0) return;
    constexpr int COLS = WEIGHTED ? 4 : 3;
    double sum[COLS] = {};
    if constexpr (WEIGHTED) {
        if (n_all == 0 || v != 0 || threadIdx.x != 0) return;
        for (int u = 0; u < n_all; ++u)
            for (int c = 0; c < COLS; ++c) sum[c] += (double)rows_all[COLS * u + c];
    } else {
        const int nblocks = gridDim.x * gridDim.y;
        const float4 mine = ssim_fold_view<false>(partial + v * nblocks, nullptr, nblocks, N, w_l1, w_ssim);
        if (threadIdx.x == 0) { rows[3 * v] = mine.x; rows[3 * v + 1] = mine.y; rows[3 * v + 2] = mine.z; }
        if (n_all == 0 || v != 0) return;
        for (int u = 0; u < n_all; ++u) {
            __syncthreads();
            const float4 r = ssim_fold_view<false>(partial_all + (size_t)u * nblocks, nullptr, nblocks, N, w_l1, w_ssim);
            sum[0] += (double)r.x; sum[1] += (double)r.y; sum[2] += (double)r.z;
        }
        if (threadIdx.x != 0) return;
    }
    float *batch_row = rows_all + COLS * (size_t)n_all;
    for (int c = 0; c < 3; ++c) batch_row[c] = (float)(sum[c] / n_all);
    if constexpr (WEIGHTED) batch_row[3] = (float)sum[3];
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
    sum = block_fold<4>(sum, red, FoldSum());
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// fixed-order fold of the per-block sums in double; cnt == 0 (no neighbour pairs) gives 0 / 0 = NaN like the reference
__global__ void __launch_bounds__(256) tv3d_finish_kernel(const float *__restrict__ partial, int nblocks, double cnt, float weight,
                                                          float *__restrict__ scalars)
{
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) s += partial[i];
    s = block_fold<4>(s, red, FoldSum());
    if (threadIdx.x == 0) {
        const double tv = s / cnt;
        scalars[0] = (float)tv;
        scalars[1] = (float)((double)weight * tv);
    }
}

}  // namespace
}  // namespace r2

namespace {
size_t ssim_blocks(int width, int height) { return (size_t)((width + r2::LT - 1) / r2::LT) * ((height + r2::LT - 1) / r2::LT); }

// scratch of V views, in floats: [V][3][H][W] derivative maps, then at partial (an even offset: 8-byte aligned for odd sizes)
// [V][blocks] float2 partial sums, then, weighted only, [V][blocks] per-block weight sums and the V folded weight sums
struct LossScratch { size_t partial, wpartial, sum_w, end; };

LossScratch loss_scratch(bool weighted, int V, int width, int height)
{
    const size_t vb = (size_t)V * ssim_blocks(width, height);
    LossScratch s;
    s.partial = (3 * (size_t)V * width * height + 1) & ~(size_t)1;
    s.wpartial = s.partial + 2 * vb;
    s.sum_w = s.wpartial + (weighted ? vb : 0);
    s.end = s.sum_w + (weighted ? (size_t)V : 0);
    return s;
}

// all four image-loss entries.  batch: gts_host (and weights_host) hold V pointers, the call also writes the batch row V and
// divides the gradient's weights by V; otherwise V == 1 and they point to the entry's own arguments.  weighted: three launches
// per chunk and four scalar columns, weights_host may be NULL; otherwise two launches, three columns and no weights_host.
int image_loss(const char *name, bool batch, bool weighted, int V, int width, int height, const float *imgs,
               const float *const *gts_host, const float *const *weights_host, float w_l1, float w_ssim, float *dL_dimg,
               float *scratch, float *scalars, void *stream)
{
    using namespace r2;
    if (V < 1 || width <= 0 || height <= 0 || !imgs || !gts_host || (!batch && !gts_host[0]) || !dL_dimg || !scratch || !scalars) {
        set_error("%s: invalid argument", name);
        return R2_ERR_INVALID;
    }
    for (int v = 0; v < V; ++v)
        if (!gts_host[v]) {
            set_error("%s: ground truth %d is NULL", name, v);
            return R2_ERR_INVALID;
        }
    const size_t N = (size_t)width * height, nb = ssim_blocks(width, height);
    const dim3 tiles((width + LT - 1) / LT, (height + LT - 1) / LT);
    if (tiles.y > 65535u || nb > 0x7fffffffu || (size_t)V * nb > 0x7fffffffu) {   // grid limits; block counts are ints on the device
        set_error("%s: %d views of %d x %d exceed the grid", name, V, width, height);
        return R2_ERR_INVALID;
    }
    const LossScratch at = loss_scratch(weighted, V, width, height);
    float2 *partial = reinterpret_cast<float2 *>(scratch + at.partial);
    float *wpartial = scratch + at.wpartial, *sum_w = scratch + at.sum_w;
    const int cols = weighted ? 4 : 3;
    const Window win = make_ssim_window();
    const float gw_l1 = batch ? w_l1 / (float)V : w_l1, gw_ssim = batch ? w_ssim / (float)V : w_ssim;
    hipStream_t s = (hipStream_t)stream;
    for (int v0 = 0; v0 < V; v0 += R2_LOSS_BATCH_CHUNK) {
        const int nv = V - v0 < R2_LOSS_BATCH_CHUNK ? V - v0 : R2_LOSS_BATCH_CHUNK;
        ViewChunk views;
        for (int k = 0; k < R2_LOSS_BATCH_CHUNK; ++k) {
            views.gt[k] = k < nv ? gts_host[v0 + k] : nullptr;
            views.wt[k] = k < nv && weights_host ? weights_host[v0 + k] : nullptr;
        }
        const dim3 grid(tiles.x, tiles.y, nv), block(LT * LT);
        const float *x = imgs + (size_t)v0 * N;
        float *D = scratch + 3 * (size_t)v0 * N, *rows = scalars + cols * (size_t)v0;
        float2 *p = partial + (size_t)v0 * nb;
        const int n_all = batch && v0 + nv == V ? V : 0;
        if (weighted) {
            float *wp = wpartial + (size_t)v0 * nb;
            ssim_forward_kernel<true><<<grid, block, 0, s>>>(width, height, x, views, win, D, p, wp);
            ssim_fold_weighted_kernel<<<dim3(nv), block, 0, s>>>(p, wp, (int)nb, N, w_l1, w_ssim, rows, sum_w + v0);
            ssim_backward_kernel<true><<<grid, block, 0, s>>>(width, height, x, views, win, D, p, sum_w + v0, w_l1, w_ssim, gw_l1,
                                                              gw_ssim, dL_dimg + (size_t)v0 * N, rows, n_all, partial, scalars);
        } else {
            ssim_forward_kernel<false><<<grid, block, 0, s>>>(width, height, x, views, win, D, p, nullptr);
            ssim_backward_kernel<false><<<grid, block, 0, s>>>(width, height, x, views, win, D, p, nullptr, w_l1, w_ssim, gw_l1,
                                                               gw_ssim, dL_dimg + (size_t)v0 * N, rows, n_all, partial, scalars);
        }
    }
    R2_STAGE_CHECK(0, s, batch ? (weighted ? "batched weighted l1 + ssim loss" : "batched l1 + ssim loss")
                               : (weighted ? "weighted l1 + ssim loss" : "l1 + ssim loss"));
    return 0;
}
}  // namespace

extern "C" size_t r2_loss_l1_ssim_scratch_floats(int width, int height) { return loss_scratch(false, 1, width, height).end; }

extern "C" int r2_loss_l1_ssim(int width, int height, const float *img, const float *gt, float w_l1, float w_ssim,
                               float *dL_dimg, float *scratch, float *scalars, void *stream)
{
    return image_loss("r2_loss_l1_ssim", false, false, 1, width, height, img, &gt, nullptr, w_l1, w_ssim, dL_dimg, scratch, scalars,
                      stream);
}

extern "C" size_t r2_loss_l1_ssim_batch_scratch_floats(int V, int width, int height)
{
    if (V < 1 || width <= 0 || height <= 0) return 0;
    return loss_scratch(false, V, width, height).end;
}

extern "C" int r2_loss_l1_ssim_batch(int V, int width, int height, const float *imgs, const float *const *gts_host, float w_l1,
                                     float w_ssim, float *dL_dimg, float *scratch, float *scalars, void *stream)
{
    return image_loss("r2_loss_l1_ssim_batch", true, false, V, width, height, imgs, gts_host, nullptr, w_l1, w_ssim, dL_dimg, scratch,
                      scalars, stream);
}

extern "C" size_t r2_loss_l1_ssim_weighted_scratch_floats(int width, int height)
{
    if (width <= 0 || height <= 0) return 0;
    return loss_scratch(true, 1, width, height).end;
}

extern "C" int r2_loss_l1_ssim_weighted(int width, int height, const float *img, const float *gt, const float *weights,
                                        float w_l1, float w_ssim, float *dL_dimg, float *scratch, float *scalars, void *stream)
{
    return image_loss("r2_loss_l1_ssim_weighted", false, true, 1, width, height, img, &gt, &weights, w_l1, w_ssim, dL_dimg, scratch,
                      scalars, stream);
}

extern "C" size_t r2_loss_l1_ssim_weighted_batch_scratch_floats(int V, int width, int height)
{
    if (V < 1 || width <= 0 || height <= 0) return 0;
    return loss_scratch(true, V, width, height).end;
}

extern "C" int r2_loss_l1_ssim_weighted_batch(int V, int width, int height, const float *imgs, const float *const *gts_host,
                                              const float *const *weights_host, float w_l1, float w_ssim, float *dL_dimg,
                                              float *scratch, float *scalars, void *stream)
{
    return image_loss("r2_loss_l1_ssim_weighted_batch", true, true, V, width, height, imgs, gts_host, weights_host, w_l1, w_ssim,
                      dL_dimg, scratch, scalars, stream);
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
