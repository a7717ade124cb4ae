// metric_ops.hip -- evaluation metrics of a reconstruction on the device: per-slice SSIM, SSE and maxima of the 2D slices taken
// along one axis of a C-contiguous float32 [n0,n1,n2] array, the building blocks of metric_vol / metric_proj
// (r2_gaussian/utils/image_utils.py:90-184, called by train.py:241-355 at every test iteration and by test.py:114-131).
//
// The reference loops over slices with five vendor conv2d calls and one host sync each; the vendor convolution reads past its
// 484-byte weight tensor on this stack (loss_ops.hip), so that loop can fault the device.  Here the SSIM of every slice of one
// axis is one launch of the tile scheme of ssim_forward_kernel (16 x 16 output tile, 26 x 26 halo in LDS, horizontal then
// vertical 11-tap blur of the five moments) with the slice in blockIdx.z, followed by one small launch that folds the per-block
// partials of each slice in a fixed order in double: bit-reproducible, no atomics.
//
// Slice axes whose rows are contiguous in memory (axes 0 and 1) are read in place through a row and a slice stride.  Axis 2 is
// first transposed to [n2][n0][n1] into scratch through LDS tiles, then read the same way.  Without SSIM (PSNR only) the blur
// is skipped: a plain SSE / maximum pass with a wave along each row.  R2_METRIC_NORMALIZE (metric_proj) divides every slice of
// both inputs by its own maximum (multiplying by the reciprocal) before both metrics; the maxima come from a first such pass.
#include "ssim_window.hpp"

namespace r2 {

namespace {

constexpr int LT = SSIM_LT, WIN = SSIM_WIN, HALO = SSIM_HALO, LR = SSIM_LR;
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

// {sum, sum, max, max} over the block in a fixed order; the result is valid in thread 0
__device__ __forceinline__ float4 block_reduce(float4 v, float4 *red)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        v.x += __shfl_xor(v.x, d); v.y += __shfl_xor(v.y, d);
        v.z = fmaxf(v.z, __shfl_xor(v.z, d)); v.w = fmaxf(v.w, __shfl_xor(v.w, d));
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float4 t = red[0];
    for (int w = 1; w < NT / 64; ++w) {
        t.x += red[w].x; t.y += red[w].y; t.z = fmaxf(t.z, red[w].z); t.w = fmaxf(t.w, red[w].w);
    }
    return t;
}

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
    const float4 t = block_reduce(acc, red);
    if (threadIdx.x == 0) partial[(size_t)s * gridDim.x + blockIdx.x] = t;
}

// the SSIM map of a 16 x 16 tile of slice blockIdx.z (ssim_forward_kernel without the derivative maps), with the tile's SSE and
// maxima; one partial per (block, slice)
__global__ void __launch_bounds__(NT) metric_ssim_kernel(int W, int H, size_t rs, size_t ss, const float *__restrict__ gt,
                                                         const float *__restrict__ pred, SsimWindow win,
                                                         const float *__restrict__ norm, float4 *__restrict__ partial)
{
    __shared__ float sx[LR][LR + 1], sy[LR][LR + 1];
    __shared__ float hb[5][LR][LT + 1];   // horizontally blurred x, y, x^2, y^2, xy
    __shared__ float4 red[NT / 64];
    const int tid = threadIdx.x, tx = tid % LT, ty = tid / LT, s = blockIdx.z;
    const int ox = blockIdx.x * LT, oy = blockIdx.y * LT;
    const float *g = gt + (size_t)s * ss, *p = pred + (size_t)s * ss;
    const float2 sc = slice_scale(norm, s);
    for (int i = tid; i < LR * LR; i += NT) {
        const int ry = i / LR, rx = i % LR, X = ox + rx - HALO, Y = oy + ry - HALO;
        const bool in = X >= 0 && X < W && Y >= 0 && Y < H;   // zero padding AFTER the normalisation, as conv2d pads
        sx[ry][rx] = in ? g[(size_t)Y * rs + X] * sc.x : 0.f;
        sy[ry][rx] = in ? p[(size_t)Y * rs + X] * sc.y : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < LR * LT; i += NT) {
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
    float4 acc = make_float4(0.f, 0.f, -INFINITY, -INFINITY);
    if (ox + tx < W && oy + ty < H) {
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
        const float s1 = e11 - m1 * m1, s2 = e22 - m2 * m2, s12 = e12 - m1 * m2;
        const float u = sx[ty + HALO][tx + HALO], v = sy[ty + HALO][tx + HALO], d = u - v;
        acc.x = (2.f * m1 * m2 + C1) * (2.f * s12 + C2) / ((m1 * m1 + m2 * m2 + C1) * (s1 + s2 + C2));
        acc.y = d * d;
        acc.z = u; acc.w = v;
    }
    float4 t = block_reduce(acc, red);
    if (tid == 0) {
        if (norm) { t.z = norm[4 * s + 2]; t.w = norm[4 * s + 3]; }   // report the maxima of the inputs, not of the scaled slices
        partial[((size_t)s * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
    }
}

// per slice (blockIdx.x): fold its nb partials in a fixed order, the sums in double
__global__ void __launch_bounds__(NT) metric_finish_kernel(const float4 *__restrict__ partial, int nb, double inv_area, int ssim,
                                                           float *__restrict__ per_slice)
{
    __shared__ double rs[NT / 64][2];
    __shared__ float rm[NT / 64][2];
    const int s = blockIdx.x, tid = threadIdx.x;
    const float4 *q = partial + (size_t)s * nb;
    double S = 0.0, E = 0.0;
    float gm = -INFINITY, pm = -INFINITY;
    for (int i = tid; i < nb; i += NT) {
        const float4 v = q[i];
        S += v.x; E += v.y; gm = fmaxf(gm, v.z); pm = fmaxf(pm, v.w);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        S += __shfl_xor(S, d); E += __shfl_xor(E, d);
        gm = fmaxf(gm, __shfl_xor(gm, d)); pm = fmaxf(pm, __shfl_xor(pm, d));
    }
    if ((tid & 63) == 0) { rs[tid >> 6][0] = S; rs[tid >> 6][1] = E; rm[tid >> 6][0] = gm; rm[tid >> 6][1] = pm; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NT / 64; ++w) {
            rs[0][0] += rs[w][0]; rs[0][1] += rs[w][1]; rm[0][0] = fmaxf(rm[0][0], rm[w][0]); rm[0][1] = fmaxf(rm[0][1], rm[w][1]);
        }
        per_slice[4 * s + 0] = ssim ? (float)(rs[0][0] * inv_area) : NAN;
        per_slice[4 * s + 1] = (float)rs[0][1];
        per_slice[4 * s + 2] = rm[0][0];
        per_slice[4 * s + 3] = rm[0][1];
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
