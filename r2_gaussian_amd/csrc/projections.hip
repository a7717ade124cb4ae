// projections.hip -- conditioning of measured projection stacks (projections.py: resize, median_filter, despeckle): the resize
// of the reference's real-data converter (cv2.resize with its row shift, lower clamp and crop, fused into one pass) and a
// k x k median filter against isolated outliers (zingers, hot pixels, NaN read-outs).  The contract -- the sampling rule, the
// weights, the order of every operation, the rank and the NaN rule -- is stated in include/r2hip.h (r2_proj_resize,
// r2_proj_median); tests/projections_ref.py restates it in float32 operation for operation, which is why this file is compiled
// without FMA contraction.
//
// Resize: one lane per cropped output pixel, neighbouring lanes on neighbouring output columns.  The bilinear kernel reads its
// two rows and two columns from tables that a first small launch computes in double; the box mean walks its fy x fx block row
// after row.  The shift and the clamp are applied as a pixel is read, so no prepared copy of the stack exists.
//
// Median: a workgroup of MED_TB lanes owns a tile of MED_TX x MED_TY pixels of one view.  It stages the tile and its halo of
// k / 2 in LDS through clamped indices (that is the replicated border) with a NaN turned into +inf, and every lane then selects
// the medians of MED_TY / 4 consecutive pixels of its column in registers.  A wave reads MED_TX = 64 consecutive floats of an LDS
// row at a time, so no access has a bank conflict, whatever the row stride.  3 x 3: every row's triple is sorted once with
// min3 / med3 / max3 and shared by the lane's pixels that use it, and a median is med3(max of the minima, med3 of the medians,
// min of the maxima): 8.5 three-input operations per pixel.  5 x 5: the forgetful selection -- the median of n values is never
// the minimum or the maximum of any n / 2 + 2 of them, so the network keeps 14 values, finds their minimum and maximum with
// min/max pairs, drops both, takes one more value in, and ends with three: 132 pairs, which makes this kernel VALU-bound.
#include "median_select.hpp"
#include "r2_common.hpp"
#include <math.h>

namespace r2 {

namespace {

constexpr int TB = 256;                              // resize and its tables: outputs per workgroup
constexpr int MED_TX = 64, MED_TY = 16;              // median: pixels of a tile
constexpr int MED_TB = 256;                          // median: lanes of a workgroup, MED_TX columns x 4 row groups
constexpr int MED_ROWS = MED_TY / (MED_TB / MED_TX); // median: pixels per lane

struct Prepared {
    const float *__restrict__ src;   // one view
    int H, W, sr, sc;
    float lo;
    // P(r, c) of r2hip.h
    __device__ __forceinline__ float operator()(int r, int c) const
    {
        const long long rr = (long long)r + sr, cc = (long long)c + sc;
        if (rr < 0 || rr >= H || cc < 0 || cc >= W) return 0.0f;
        return clamp(src[(size_t)rr * W + (size_t)cc]);
    }
    __device__ __forceinline__ float clamp(float x) const { return x < lo ? lo : x; }
};

// The bilinear tables in the workspace: int s[M], then float f[M], M = mh + mw, the rows' entries first.
__global__ void __launch_bounds__(TB) proj_resize_tables(int H, int W, int mh, int mw, double scale_y, double scale_x, int *s,
                                                         float *f)
{
    const int e = (int)(blockIdx.x * TB + threadIdx.x);
    if (e >= mh + mw) return;
    const bool row = e < mh;
    const int d = row ? e : e - mh, n = row ? H : W;
    const float fx = (float)(((double)d + 0.5) * (row ? scale_y : scale_x) - 0.5);
    const float fl = floorf(fx);
    int si = (int)fl;
    float fr = fx - fl;
    if (si < 0) {
        si = 0;
        fr = 0.0f;
    }
    if (si >= n - 1) {
        si = n - 1;
        fr = 0.0f;
    }
    s[e] = si;
    f[e] = fr;
}

struct Window {
    int mh, mw, r0, c0, oh, ow;
};

__global__ void __launch_bounds__(TB) proj_resize_linear(size_t total, Prepared p, Window w, const int *__restrict__ s,
                                                         const float *__restrict__ f, float *__restrict__ dst)
{
    const size_t o = (size_t)blockIdx.x * TB + threadIdx.x;
    if (o >= total) return;
    const size_t per = (size_t)w.oh * w.ow;
    const size_t v = o / per, q = o % per;
    const int y = w.r0 + (int)(q / (size_t)w.ow), x = w.mh + w.c0 + (int)(q % (size_t)w.ow);
    p.src += v * (size_t)p.H * p.W;
    const int ra = s[y], rb = min(ra + 1, p.H - 1), ca = s[x], cb = min(ca + 1, p.W - 1);
    const float b1 = f[y], b0 = 1.0f - b1, a1 = f[x], a0 = 1.0f - a1;
    const float h0 = p(ra, ca) * a0 + p(ra, cb) * a1;
    const float h1 = p(rb, ca) * a0 + p(rb, cb) * a1;
    dst[o] = h0 * b0 + h1 * b1;
}

// VEC4: fx = 4 and every block row starts on a 16-byte boundary (the entry checks it), so an inside block row is one load
template <bool VEC4>
__global__ void __launch_bounds__(TB) proj_resize_area(size_t total, Prepared p, Window w, int fy, int fx, float norm,
                                                       float *__restrict__ dst)
{
    const size_t o = (size_t)blockIdx.x * TB + threadIdx.x;
    if (o >= total) return;
    const size_t per = (size_t)w.oh * w.ow;
    const size_t v = o / per, q = o % per;
    const int y = (w.r0 + (int)(q / (size_t)w.ow)) * fy, x = (w.c0 + (int)(q % (size_t)w.ow)) * fx;
    p.src += v * (size_t)p.H * p.W;
    const long long rr = (long long)y + p.sr, cc = (long long)x + p.sc;
    float acc = 0.0f;
    if (rr >= 0 && rr + fy <= p.H && cc >= 0 && cc + fx <= p.W) {   // the whole block lies inside the image: no test per pixel
        const float *row = p.src + (size_t)rr * p.W + (size_t)cc;
        for (int i = 0; i < fy; ++i, row += p.W) {
            if constexpr (VEC4) {
                const float4 t = *reinterpret_cast<const float4 *>(row);
                const float t0 = p.clamp(t.x);
                acc = i == 0 ? t0 : acc + t0;
                acc = acc + p.clamp(t.y);
                acc = acc + p.clamp(t.z);
                acc = acc + p.clamp(t.w);
            } else {
                for (int j = 0; j < fx; ++j) {
                    const float t = p.clamp(row[j]);
                    acc = (i | j) == 0 ? t : acc + t;
                }
            }
        }
    } else {
        for (int i = 0; i < fy; ++i)
            for (int j = 0; j < fx; ++j) {
                const float t = p(y + i, x + j);
                acc = (i | j) == 0 ? t : acc + t;
            }
    }
    dst[o] = acc * norm;
}

template <int K>
__global__ void __launch_bounds__(MED_TB) proj_median(int V, int H, int W, const float *__restrict__ src, int conditional,
                                                      float threshold, float *__restrict__ dst,
                                                      unsigned char *__restrict__ flagged)
{
    constexpr int R = K / 2, LW = MED_TX + 2 * R, LH = MED_TY + 2 * R, KEEP = K * K / 2 + 2;
    __shared__ float tile[LH * LW];
    const int tiles_x = (W + MED_TX - 1) / MED_TX, tiles_y = (H + MED_TY - 1) / MED_TY;
    const unsigned per = (unsigned)tiles_x * (unsigned)tiles_y;
    const int v = (int)(blockIdx.x / per);
    const unsigned t = blockIdx.x % per;
    const int x0 = (int)(t % (unsigned)tiles_x) * MED_TX, y0 = (int)(t / (unsigned)tiles_x) * MED_TY;
    const size_t view = (size_t)v * H * W;
    // a lane's STAGE loads are issued together, before the first of them is used: one trip to memory per workgroup, not STAGE
    constexpr int STAGE = (LH * LW + MED_TB - 1) / MED_TB;
    float staged[STAGE];
#pragma unroll
    for (int i = 0; i < STAGE; ++i) {
        const int e = min((int)threadIdx.x + i * MED_TB, LH * LW - 1);
        const int ly = e / LW, lx = e % LW;
        const int gy = min(max(y0 + ly - R, 0), H - 1), gx = min(max(x0 + lx - R, 0), W - 1);
        staged[i] = src[view + (size_t)gy * W + gx];
    }
#pragma unroll
    for (int i = 0; i < STAGE; ++i) {
        const int e = (int)threadIdx.x + i * MED_TB;
        if (e < LH * LW) tile[e] = staged[i] != staged[i] ? INFINITY : staged[i];
    }
    __syncthreads();
    const int lx = (int)threadIdx.x % MED_TX, x = x0 + lx;
    const int ly0 = (int)threadIdx.x / MED_TX * MED_ROWS;   // the lane's pixels: MED_ROWS consecutive rows of its column
    if (x >= W || y0 + ly0 >= H) return;
    const float *col = tile + ly0 * LW + lx;                // pixel u's window: rows u .. u + K-1, columns 0 .. K-1 from here
    auto emit = [&](int u, float m) {
        const int y = y0 + ly0 + u;
        if (y >= H) return;
        const size_t o = view + (size_t)y * W + x;
        float c = col[(u + R) * LW + R];
        if (c == INFINITY) c = src[o];                      // +inf or a staged NaN: the pixel itself decides
        const bool replace = !(fabsf(c - m) <= threshold);
        dst[o] = conditional ? (replace ? m : c) : m;
        if (flagged) flagged[o] = replace ? 1 : 0;
    };
    if constexpr (K == 3) {
        // Each row's three values sorted once (min3, med3, max3) and shared by the three pixels of the column that use the
        // row; the median of nine is then the median of the largest minimum, the median of the medians and the smallest maximum.
        float lo[3], md[3], hi[3];
#pragma unroll
        for (int j = 0; j < MED_ROWS + 2; ++j) {
            const float a = col[j * LW], b = col[j * LW + 1], c = col[j * LW + 2];
            lo[j % 3] = fminf(fminf(a, b), c);
            md[j % 3] = __builtin_amdgcn_fmed3f(a, b, c);
            hi[j % 3] = fmaxf(fmaxf(a, b), c);
            if (j >= 2)
                emit(j - 2, __builtin_amdgcn_fmed3f(fmaxf(fmaxf(lo[0], lo[1]), lo[2]), __builtin_amdgcn_fmed3f(md[0], md[1], md[2]),
                                                    fminf(fminf(hi[0], hi[1]), hi[2])));
        }
    } else {
#pragma unroll 1
        for (int u = 0; u < MED_ROWS; ++u) {
            const float *win = col + u * LW;
            float a[KEEP];
#pragma unroll
            for (int i = 0; i < KEEP; ++i) a[i] = win[(i / K) * LW + i % K];
            int taken = KEEP;
            emit(u, select_median<KEEP>(a, [&]() {
                     const float nv = win[(taken / K) * LW + taken % K];
                     ++taken;
                     return nv;
                 }));
        }
    }
}

constexpr unsigned long long LIMIT_IMAGE = 0x80000000ULL, LIMIT_STACK = 1ULL << 38;

unsigned blocks_for(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

}  // namespace r2

extern "C" size_t r2_proj_resize_workspace_bytes(int mh, int mw)
{
    if (mh < 1 || mw < 1) return 0;
    return ((size_t)mh + mw) * (sizeof(int) + sizeof(float));
}

extern "C" int r2_proj_resize(int V, int H, int W, const float *src, int sr, int sc, float lo, int interp, int mh, int mw, int r0,
                              int c0, int oh, int ow, float *dst, void *ws, size_t ws_bytes, void *stream)
{
    using namespace r2;
    const bool dims = V >= 0 && H >= 1 && W >= 1 && mh >= 1 && mw >= 1 && oh >= 1 && ow >= 1 && r0 >= 0 && c0 >= 0 &&
                      (long long)r0 + oh <= mh && (long long)c0 + ow <= mw;
    const unsigned long long v = (unsigned long long)(V < 0 ? 0 : V);
    if (!dims || (unsigned long long)H * W >= LIMIT_IMAGE || (unsigned long long)mh * mw >= LIMIT_IMAGE ||
        v * H * W >= LIMIT_STACK || v * oh * ow >= LIMIT_STACK || sr > (1 << 30) || sr < -(1 << 30) || sc > (1 << 30) ||
        sc < -(1 << 30) || lo != lo || (interp != 0 && interp != 1) || (interp == 1 && (H % mh != 0 || W % mw != 0))) {
        set_error("r2_proj_resize: invalid argument (%d x %d x %d -> %d x %d, window %d, %d, %d x %d, shift %d, %d, interp %d)", V, H,
                  W, mh, mw, r0, c0, oh, ow, sr, sc, interp);
        return R2_ERR_INVALID;
    }
    if (V == 0) return 0;
    if (!src || !dst || (interp == 0 && !ws)) {
        set_error("r2_proj_resize: NULL pointer");
        return R2_ERR_INVALID;
    }
    if (interp == 0 && ws_bytes < r2_proj_resize_workspace_bytes(mh, mw)) {
        set_error("r2_proj_resize: workspace of %zu bytes, %zu needed", ws_bytes, r2_proj_resize_workspace_bytes(mh, mw));
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)V * oh * ow;
    const Prepared p{src, H, W, sr, sc, lo};
    const Window w{mh, mw, r0, c0, oh, ow};
    if (interp == 0) {
        const int M = mh + mw;
        int *ts = (int *)ws;
        float *tf = (float *)ws + M;
        const double inv_y = (double)mh / (double)H, inv_x = (double)mw / (double)W;
        proj_resize_tables<<<dim3(blocks_for((size_t)M, TB)), dim3(TB), 0, s>>>(H, W, mh, mw, 1.0 / inv_y, 1.0 / inv_x, ts, tf);
        proj_resize_linear<<<dim3(blocks_for(total, TB)), dim3(TB), 0, s>>>(total, p, w, ts, tf, dst);
    } else {
        const int fy = H / mh, fx = W / mw;
        const float norm = (float)(1.0 / ((double)fy * fx));
        if (fx == 4 && W % 4 == 0 && sc % 4 == 0 && (uintptr_t)src % 16 == 0)
            proj_resize_area<true><<<dim3(blocks_for(total, TB)), dim3(TB), 0, s>>>(total, p, w, fy, fx, norm, dst);
        else
            proj_resize_area<false><<<dim3(blocks_for(total, TB)), dim3(TB), 0, s>>>(total, p, w, fy, fx, norm, dst);
    }
    R2_STAGE_CHECK(0, s, "projection resize");
    return 0;
}

extern "C" int r2_proj_median(int V, int H, int W, const float *src, int k, int conditional, float threshold, float *dst,
                              unsigned char *flagged, void *stream)
{
    using namespace r2;
    const unsigned long long v = (unsigned long long)(V < 0 ? 0 : V);
    if (V < 0 || H < 1 || W < 1 || (unsigned long long)H * W >= LIMIT_IMAGE || v * H * W >= LIMIT_STACK || (k != 3 && k != 5) ||
        (conditional != 0 && conditional != 1) || threshold != threshold) {
        set_error("r2_proj_median: invalid argument (%d x %d x %d, k %d, conditional %d)", V, H, W, k, conditional);
        return R2_ERR_INVALID;
    }
    if (V == 0) return 0;
    if (!src || !dst) {
        set_error("r2_proj_median: NULL pointer");
        return R2_ERR_INVALID;
    }
    // V H W < 2^38 leaves fewer than 2^28 + V tiles
    const size_t tiles = (size_t)V * ((size_t)(W + MED_TX - 1) / MED_TX) * ((size_t)(H + MED_TY - 1) / MED_TY);
    if (tiles >= LIMIT_IMAGE) {
        set_error("r2_proj_median: %zu tiles, too many for one launch", tiles);
        return R2_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    if (k == 3)
        proj_median<3><<<dim3((unsigned)tiles), dim3(MED_TB), 0, s>>>(V, H, W, src, conditional, threshold, dst, flagged);
    else
        proj_median<5><<<dim3((unsigned)tiles), dim3(MED_TB), 0, s>>>(V, H, W, src, conditional, threshold, dst, flagged);
    R2_STAGE_CHECK(0, s, "projection median");
    return 0;
}
