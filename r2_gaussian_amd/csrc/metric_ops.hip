// metric_ops.hip -- evaluation metrics of a reconstruction on the device: per-slice SSIM, SSE and maxima of the 2D slices taken
// along one axis of a C-contiguous float32 [n0,n1,n2] array, the building blocks of metric_vol / metric_proj
// (r2_gaussian/utils/image_utils.py:90-184, called by train.py:241-355 at every test iteration and by test.py:114-131).
//
// The reference loops over slices with five vendor conv2d calls and one host sync each; the vendor convolution reads past its
// 484-byte weight tensor on this stack (loss_ops.hip), so that loop can fault the device.  Here the SSIM of every slice of one
// axis is one launch of the loss's tile function (ssim_window.hpp: 16 x 16 output tile, 26 x 26 halo in LDS, horizontal then
// vertical 11-tap blur of the five moments) with the slice in blockIdx.z, followed by one small launch that folds the per-block
// partials of each slice in a fixed order in double: bit-reproducible, no atomics.
//
// Slice axes whose rows are contiguous in memory (axes 0 and 1) are read in place through a row and a slice stride.  Axis 2 is
// first transposed to [n2][n0][n1] into scratch through LDS tiles, then read the same way.  Without SSIM (PSNR only) the blur
// is skipped: a plain SSE / maximum pass with a wave along each row.  R2_METRIC_NORMALIZE (metric_proj) divides every slice of
// both inputs by its own maximum (multiplying by the reciprocal) before both metrics; the maxima come from a first such pass.
#include "block_fold.hpp"
#include "ssim_window.hpp"

namespace r2 {

namespace {

constexpr int LT = SSIM_LT, HALO = SSIM_HALO;
constexpr int NT = LT * LT;     // 256 threads = 4 waves in every kernel here
constexpr int SROWS = 16;       // rows per block of the SSE / maximum pass
constexpr int TT = 32;          // transpose tile

// one field per slice of per_slice: {mean of the SSIM map, sum (gt - pred)^2, max gt, max pred}
struct SliceGeom { int n, W, H; size_t rs, ss; };

SliceGeom slice_geom(int n0, int n1, int n2, int axis)
{
    if (axis == 0) return {n0, n2, n1, (size_t)n2, (size_t)n1 * n2};
    if (axis == 1) return {n1, n2, n0, (size_t)n1 * n2, (size_t)n2};
    return {n2, n1, n0, (size_t)n1, (size_t)n0 * n1};   // after the transpose to [n2][n0][n1]
}

size_t ssim_blocks(const SliceGeom &g) { return (size_t)((g.W + LT - 1) / LT) * ((g.H + LT - 1) / LT); }

// the fold of {sum, sum, max, max}
struct FoldSumSumMaxMax {
    __device__ __forceinline__ float4 operator()(float4 a, float4 b) const
    {
        return make_float4(a.x + b.x, a.y + b.y, fmaxf(a.z, b.z), fmaxf(a.w, b.w));
    }
};

// per-slice reciprocals of the maxima (normalisation), or 1
__device__ __forceinline__ float2 slice_scale(const float *__restrict__ norm, int s)
{
    return norm ? make_float2(1.0f / norm[4 * s + 2], 1.0f / norm[4 * s + 3]) : make_float2(1.f, 1.f);
}

// SSE and maxima of SROWS rows of slice blockIdx.y: each wave walks its rows with the lanes along the contiguous row
__global__ void __launch_bounds__(NT) metric_sse_max_kernel(int W, int H, size_t rs, size_t ss, const float *__restrict__ gt,
                                                            const float *__restrict__ pred, const float *__restrict__ norm,
                                                            float4 *__restrict__ partial)
{
    __shared__ float4 red[NT / 64];
    const int s = blockIdx.y, lane = threadIdx.x & 63;
    const float *g = gt + (size_t)s * ss, *p = pred + (size_t)s * ss;
    const float2 sc = slice_scale(norm, s);
    float4 acc = make_float4(0.f, 0.f, -INFINITY, -INFINITY);
    const int y1 = min(H, (int)(blockIdx.x + 1) * SROWS);
    for (int y = blockIdx.x * SROWS + (threadIdx.x >> 6); y < y1; y += NT / 64)
        for (int x = lane; x < W; x += 64) {
            const float u = g[(size_t)y * rs + x], v = p[(size_t)y * rs + x];
            float ua = u * sc.x, vb = v * sc.y;
            // both products rounded before the difference (no fma under -ffp-contract=fast): equal slices give exactly 0 and
            // PSNR inf, as the reference's two divisions do
            asm volatile("" : "+v"(ua), "+v"(vb));
            const float d = ua - vb;
            acc.y += d * d;
            acc.z = fmaxf(acc.z, u); acc.w = fmaxf(acc.w, v);
        }
    const float4 t = block_fold<NT / 64>(acc, red, FoldSumSumMaxMax());
    if (threadIdx.x == 0) partial[(size_t)s * gridDim.x + blockIdx.x] = t;
}

// the SSIM map of a 16 x 16 tile of slice blockIdx.z (the loss's forward pass without the derivative maps: the same
// ssim_tile_moments), with the tile's SSE and maxima; one partial per (block, slice)
__global__ void __launch_bounds__(NT) metric_ssim_kernel(int W, int H, size_t rs, size_t ss, const float *__restrict__ gt,
                                                         const float *__restrict__ pred, SsimWindow win,
                                                         const float *__restrict__ norm, float4 *__restrict__ partial)
{
    __shared__ SsimTile tile;
    __shared__ float4 red[NT / 64];
    const int tid = threadIdx.x, tx = tid % LT, ty = tid / LT, s = blockIdx.z;
    const float *g = gt + (size_t)s * ss, *p = pred + (size_t)s * ss;
    const float2 sc = slice_scale(norm, s);
    // zero padding AFTER the normalisation, as conv2d pads
    const SsimMoments m = ssim_tile_moments(tile, W, H, win, [&](int X, int Y, bool in) {
        return in ? make_float2(g[(size_t)Y * rs + X] * sc.x, p[(size_t)Y * rs + X] * sc.y) : make_float2(0.f, 0.f);
    });
    float4 acc = make_float4(0.f, 0.f, -INFINITY, -INFINITY);
    if (blockIdx.x * LT + tx < W && blockIdx.y * LT + ty < H) {
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f, m1 = m.m1, m2 = m.m2;
        const float s1 = m.e11 - m1 * m1, s2 = m.e22 - m2 * m2, s12 = m.e12 - m1 * m2;
        const float u = tile.x[ty + HALO][tx + HALO], v = tile.y[ty + HALO][tx + HALO], d = u - v;
        acc.x = (2.f * m1 * m2 + C1) * (2.f * s12 + C2) / ((m1 * m1 + m2 * m2 + C1) * (s1 + s2 + C2));
        acc.y = d * d;
        acc.z = u; acc.w = v;
    }
    float4 t = block_fold<NT / 64>(acc, red, FoldSumSumMaxMax());
    if (tid == 0) {
        if (norm) { t.z = norm[4 * s + 2]; t.w = norm[4 * s + 3]; }   // report the maxima of the inputs, not of the scaled slices
        partial[((size_t)s * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
    }
}

// per slice (blockIdx.x): fold its nb partials in a fixed order, the sums in double
struct SliceFold { double S, E; float gm, pm; };

__global__ void __launch_bounds__(NT) metric_finish_kernel(const float4 *__restrict__ partial, int nb, double inv_area, int ssim,
                                                           float *__restrict__ per_slice)
{
    __shared__ SliceFold red[NT / 64];
    const int s = blockIdx.x;
    const float4 *q = partial + (size_t)s * nb;
    SliceFold f = {0.0, 0.0, -INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < nb; i += NT) {
        const float4 v = q[i];
        f.S += v.x; f.E += v.y; f.gm = fmaxf(f.gm, v.z); f.pm = fmaxf(f.pm, v.w);
    }
    f = block_fold<NT / 64>(f, red, [](SliceFold a, SliceFold b) {
        return SliceFold{a.S + b.S, a.E + b.E, fmaxf(a.gm, b.gm), fmaxf(a.pm, b.pm)};
    });
    if (threadIdx.x == 0) {
        per_slice[4 * s + 0] = ssim ? (float)(f.S * inv_area) : NAN;
        per_slice[4 * s + 1] = (float)f.E;
        per_slice[4 * s + 2] = f.gm;
        per_slice[4 * s + 3] = f.pm;
    }
}

// out[c][r] = in[r][c] of an R x C matrix; blockIdx.z picks the array (ground truth / prediction)
__global__ void __launch_bounds__(NT) metric_transpose_kernel(long long R, int C, const float *__restrict__ a,
                                                              const float *__restrict__ b, float *__restrict__ ta,
                                                              float *__restrict__ tb)
{
    __shared__ float t[TT][TT + 1];
    const float *in = blockIdx.z ? b : a;
    float *out = blockIdx.z ? tb : ta;
    const long long r0 = (long long)blockIdx.x * TT;
    const int c0 = blockIdx.y * TT, tx = threadIdx.x % TT, ty = threadIdx.x / TT;
    for (int j = ty; j < TT; j += NT / TT)
        if (r0 + j < R && c0 + tx < C) t[j][tx] = in[(size_t)(r0 + j) * C + c0 + tx];
    __syncthreads();
    for (int j = ty; j < TT; j += NT / TT)
        if (r0 + tx < R && c0 + j < C) out[(size_t)(c0 + j) * R + r0 + tx] = t[tx][j];
}

}  // namespace
}  // namespace r2

extern "C" size_t r2_metric_slices_scratch_floats(int n0, int n1, int n2, int axis)
{
    using namespace r2;
    if (n0 <= 0 || n1 <= 0 || n2 <= 0 || axis < 0 || axis > 2) return 0;
    const SliceGeom g = slice_geom(n0, n1, n2, axis);
    return 4 * (size_t)g.n * ssim_blocks(g) + (axis == 2 ? 2 * (size_t)n0 * n1 * n2 : 0);
}

extern "C" int r2_metric_slices(int n0, int n1, int n2, int axis, const float *gt, const float *pred, int flags,
                                float *per_slice, float *scratch, void *stream)
{
    using namespace r2;
    if (n0 <= 0 || n1 <= 0 || n2 <= 0 || axis < 0 || axis > 2 || !gt || !pred || !per_slice || !scratch ||
        (flags & ~(R2_METRIC_SSIM | R2_METRIC_NORMALIZE)) != 0) {
        set_error("r2_metric_slices: invalid argument");
        return R2_ERR_INVALID;
    }
    const SliceGeom g = slice_geom(n0, n1, n2, axis);
    if (g.n > 65535 || (g.H + LT - 1) / LT > 65535) {   // grid y / z limits
        set_error("r2_metric_slices: %d slices of %d rows exceed the launch grid", g.n, g.H);
        return R2_ERR_INVALID;
    }
    const size_t nb = ssim_blocks(g);
    float4 *partial = reinterpret_cast<float4 *>(scratch);
    hipStream_t s = (hipStream_t)stream;
    if (axis == 2) {
        const long long R = (long long)n0 * n1;
        float *ta = scratch + 4 * (size_t)g.n * nb, *tb = ta + (size_t)R * n2;
        metric_transpose_kernel<<<dim3((unsigned)((R + TT - 1) / TT), (n2 + TT - 1) / TT, 2), dim3(NT), 0, s>>>(R, n2, gt, pred, ta, tb);
        gt = ta;
        pred = tb;
    }
    const double inv_area = 1.0 / ((double)g.W * g.H);
    const dim3 sse_grid((g.H + SROWS - 1) / SROWS, g.n);
    if (flags & R2_METRIC_NORMALIZE) {   // the maxima first: per_slice then holds them for the pass below
        metric_sse_max_kernel<<<sse_grid, dim3(NT), 0, s>>>(g.W, g.H, g.rs, g.ss, gt, pred, nullptr, partial);
        metric_finish_kernel<<<dim3(g.n), dim3(NT), 0, s>>>(partial, (int)sse_grid.x, inv_area, 0, per_slice);
    }
    const float *norm = (flags & R2_METRIC_NORMALIZE) ? per_slice : nullptr;
    if (flags & R2_METRIC_SSIM) {
        const dim3 grid((g.W + LT - 1) / LT, (g.H + LT - 1) / LT, g.n);
        metric_ssim_kernel<<<grid, dim3(NT), 0, s>>>(g.W, g.H, g.rs, g.ss, gt, pred, make_ssim_window(), norm, partial);
        metric_finish_kernel<<<dim3(g.n), dim3(NT), 0, s>>>(partial, (int)nb, inv_area, 1, per_slice);
    } else {
        metric_sse_max_kernel<<<sse_grid, dim3(NT), 0, s>>>(g.W, g.H, g.rs, g.ss, gt, pred, norm, partial);
        metric_finish_kernel<<<dim3(g.n), dim3(NT), 0, s>>>(partial, (int)sse_grid.x, inv_area, 0, per_slice);
    }
    R2_STAGE_CHECK(0, s, "metric slices");
    return 0;
}
